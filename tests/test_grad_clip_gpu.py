"""Global gradient norm on the device (FusedAdam(clip_norm=...)): the deterministic sum of squares against fp64, FairSeq's
clip_grad_norm_ folded into Adam's gradient scale against an fp64 Adam, clip_norm=None / 0 against each other bit for bit,
the non-finite guard (a skipped update stores nothing and does not advance Adam's bias correction), the launcher's
--clip-norm / gnorm / clip / skipped_updates, and two ranks on one card."""
import math
import os
import struct
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(5,), (4096,), (4097,), (300, 41), (70000,)]     # test_fused_adam_multi_tensor_matches_per_tensor's: around the 4096 chunk


def _bits(t):
    return struct.pack("<f", float(t)).hex()


def _params(shapes, dtype, gen, mode, offset=0):
    """Parameters whose gradients sit as the optimiser will find them.  mode "multi": main_grad views packed into one
    arena from element `offset` on (the one-launch table walk); "single": the same views, optimiser built with
    multi_tensor=False (one launch per tensor); "mix": every other parameter has only p.grad."""
    init = [torch.randn(s, generator=gen) for s in shapes]
    ps = [torch.nn.Parameter(t.clone().cuda().to(dtype)) for t in init]
    arena = torch.zeros(sum(t.numel() for t in init) + offset + 8, device="cuda")
    o = offset
    for i, p in enumerate(ps):
        if mode == "mix" and i % 2 == 1:
            p.grad = torch.zeros(p.shape, device="cuda", dtype=dtype)         # a bf16 parameter's p.grad is bf16
        else:
            p.main_grad = arena[o:o + p.numel()].view(p.shape)
            o += p.numel()
    return init, ps, arena


def _set_grads(ps, grads):
    """→ the gradients as the optimiser will read them (a bf16 p.grad has rounded them), on the host."""
    seen = []
    for p, g in zip(ps, grads):
        dst = p.main_grad if hasattr(p, "main_grad") else p.grad
        dst.copy_(g.cuda())
        seen.append(dst.detach().float().cpu())
    return seen


@pytest.mark.parametrize("scaled", [False, True], ids=["noscale", "scale"])
@pytest.mark.parametrize("offset", [0, 1, 3])
@pytest.mark.parametrize("form", ["multi", "single"])
def test_gnorm_matches_fp64_and_is_deterministic(form, offset, scaled):
    """Each size alone and all together; views from element offsets 0, 1, 3 of the arena (16-byte aligned and not).
    Bound: 16 sequential fp32 adds + an 8-level fp32 tree per chunk, fp64 above: ~1.5e-6 relative; gate rtol 1e-5."""
    from multimodaldiscussiontransformer_amd.optim import FusedAdam
    gen = torch.Generator().manual_seed(7 + offset)
    s_in = 0.37
    scale = torch.tensor([s_in], device="cuda") if scaled else None
    for shapes in [[s] for s in SHAPES] + [SHAPES]:
        _, ps, arena = _params(shapes, torch.float32, gen, form, offset)
        assert ps[0].main_grad.data_ptr() % 16 == 4 * offset
        grads = _set_grads(ps, [torch.randn(p.shape, generator=gen) * 3.0 for p in ps])
        opt = FusedAdam(ps, lr=1e-3, clip_norm=0.0, multi_tensor=(form == "multi"))
        opt.step(grad_scale=scale)
        got = opt.last_gnorm.clone()
        want = math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads)) * (float(torch.tensor(s_in)) if scaled else 1.0)
        rel = abs(float(got) - want) / want
        print(f"gnorm {form} offset {offset} scaled {scaled} shapes {shapes}: got {float(got):.9g} fp64 {want:.9g} rel {rel:.2e}")
        assert rel <= 1e-5, (shapes, float(got), want)
        opt.step(grad_scale=scale)                 # the same gradients again: the same bits
        assert _bits(opt.last_gnorm) == _bits(got)
        assert int(opt.skipped) == 0 and int(opt.clipped) == 0 and int(opt.applied_steps) == 2
        if scaled:
            assert _bits(opt.grad_scale_used) == _bits(scale)      # max_norm 0: the incoming scale, bit for bit


def _adam64(ref, m, v, gd, t, lr=1e-2, wd=0.01):
    m = 0.9 * m + 0.1 * gd
    v = 0.999 * v + 0.001 * gd * gd
    ref = ref - wd * lr * ref
    ref = ref - lr * math.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t) * m / (v.sqrt() + 1e-8)
    return ref, m, v


CLIP_SHAPES = [(1000,), (4097,), (33, 7), (5000,)]


@pytest.mark.parametrize("mode", ["multi", "single", "mix"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_clipping_matches_fp64_reference(dtype, mode):
    """test_fused_adam_matches_reference_formula's fp64 Adam preceded by FairSeq's clip_grad_norm_ coefficient
    coef = min(1, max_norm / (|g * s| + 1e-6)), 5 steps with grad_scale 0.5; 10 328 standard-normal elements times the
    step's multiplier put |g * s| at about 51, 5.1, 102, 2.5 and 25 against max_norm 10, so steps 1, 3 and 5 clip and
    steps 2 and 4 do not."""
    from multimodaldiscussiontransformer_amd.optim import FusedAdam
    gen = torch.Generator().manual_seed(11)
    max_norm, mults = 10.0, [1.0, 0.1, 2.0, 0.05, 0.5]
    init, ps, _ = _params(CLIP_SHAPES, dtype, gen, mode)
    opt = FusedAdam(ps, lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, clip_norm=max_norm, multi_tensor=(mode != "single"))
    refs = [t.to(dtype).double() for t in init]           # bf16: the masters start from the rounded parameter
    ms = [torch.zeros_like(r) for r in refs]
    vs = [torch.zeros_like(r) for r in refs]
    scale = torch.tensor([0.5], device="cuda")
    want_clipped = 0
    for t, mult in enumerate(mults, 1):
        grads = _set_grads(ps, [torch.randn(p.shape, generator=gen) * mult for p in ps])
        opt.step(grad_scale=scale)
        gn = math.sqrt(sum(float(((g.double() * 0.5) ** 2).sum()) for g in grads))
        coef = min(1.0, max_norm / (gn + 1e-6))
        want_clipped += gn > max_norm
        assert abs(gn - max_norm) > 0.1 * max_norm          # four orders of magnitude beyond gnorm's fp32 error: the counter is exact
        assert abs(float(opt.last_gnorm) - gn) <= 1e-5 * gn
        for i, g in enumerate(grads):
            refs[i], ms[i], vs[i] = _adam64(refs[i], ms[i], vs[i], g.double() * 0.5 * coef, t)
    assert want_clipped == 3 and int(opt.clipped) == 3 and int(opt.skipped) == 0 and int(opt.applied_steps) == 5
    for p, r in zip(ps, refs):
        if dtype == torch.float32:
            torch.testing.assert_close(p.detach().cpu().double(), r, atol=1e-5, rtol=1e-5)
        else:
            master = opt.state[id(p)]["master"]
            torch.testing.assert_close(master.cpu().double(), r, atol=1e-5, rtol=1e-5)
            assert torch.equal(p.detach(), master.to(torch.bfloat16))


def _state(opt, ps):
    out = []
    for p in ps:
        st = opt.state[id(p)]
        out += [p.detach().clone(), st["m"].clone(), st["v"].clone()] + ([st["master"].clone()] if "master" in st else [])
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_clip_norm_zero_is_bit_identical_to_none_and_none_launches_nothing(dtype):
    from multimodaldiscussiontransformer_amd.optim import FusedAdam
    scale = torch.tensor([0.5], device="cuda")
    runs = {}
    for clip in (None, 0.0):
        gen = torch.Generator().manual_seed(13)
        _, ps, _ = _params(SHAPES, dtype, gen, "mix", offset=1)
        opt = FusedAdam(ps, lr=1e-2, clip_norm=clip)
        for step in range(4):
            _set_grads(ps, [torch.randn(p.shape, generator=gen) for p in ps])
            opt.step(grad_scale=scale if step != 2 else None)
        runs[clip] = (_state(opt, ps), opt)
    (a, off), (b, on) = runs[None], runs[0.0]
    assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))
    assert off.norm_launches == 0 and off._guard is None and off._partials is None     # no norm pass, no buffers
    with pytest.raises(RuntimeError, match="clip_norm"):
        off.last_gnorm
    # guarded: one table launch (3 main_grad tensors of one dtype) + 2 per-tensor launches + the finaliser, per step
    assert on.norm_launches == 4 * (1 + 2 + 1)
    assert int(on.applied_steps) == 4 and int(on.skipped) == 0 and int(on.clipped) == 0 and float(on.last_gnorm) > 0


@pytest.mark.parametrize("where", ["table", "rest"])
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), 1e30], ids=["nan", "inf", "overflow"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_non_finite_update_is_skipped_and_bias_correction_follows_applied(dtype, bad, where):
    """Update 1 finite, update 2 carries ONE bad element (NaN, Inf, or 1e30 whose square overflows the fp32 partial) in a
    tensor of the table walk or of the per-tensor path, update 3 finite.  Update 2 must store nothing; after update 3
    the weights equal an fp64 Adam that never saw update 2 (bias correction at t = 2, not 3).  The guard state and the
    partial sums are filled with NaN before the first step: nothing is read before it is written."""
    from multimodaldiscussiontransformer_amd.optim import FusedAdam
    gen = torch.Generator().manual_seed(17)
    init, ps, _ = _params(CLIP_SHAPES, dtype, gen, "mix", offset=3)
    opt = FusedAdam(ps, lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, clip_norm=0.0)
    guard, partials = opt.guard_buffers()
    guard.fill_(float("nan"))
    partials.fill_(float("nan"))
    refs = [t.to(dtype).double() for t in init]
    ms = [torch.zeros_like(r) for r in refs]
    vs = [torch.zeros_like(r) for r in refs]
    scale = torch.tensor([0.5], device="cuda")
    applied = 0
    for upd in (1, 2, 3):
        grads = [torch.randn(p.shape, generator=gen) for p in ps]
        if upd == 2:
            grads[2 if where == "table" else 3].view(-1)[17] = bad
            assert hasattr(ps[2], "main_grad") and not hasattr(ps[3], "main_grad")
        grads = _set_grads(ps, grads)
        before = _state(opt, ps)
        skipped_before = int(opt.skipped) if upd > 1 else 0
        opt.step(grad_scale=scale)
        if upd == 2:
            after = _state(opt, ps)
            assert all(torch.equal(x, y) for x, y in zip(before, after))
            assert int(opt.skipped) == skipped_before + 1 == 1 and not math.isfinite(float(opt.last_gnorm))
            continue
        applied += 1
        assert int(opt.skipped) == skipped_before and math.isfinite(float(opt.last_gnorm))
        for i, g in enumerate(grads):
            refs[i], ms[i], vs[i] = _adam64(refs[i], ms[i], vs[i], g.double() * 0.5, applied)
    assert opt.step_count == 3 and int(opt.applied_steps) == 2 and opt.applied_steps_host() == 2 and int(opt.clipped) == 0
    for p, r in zip(ps, refs):
        got = p.detach() if dtype == torch.float32 else opt.state[id(p)]["master"]
        torch.testing.assert_close(got.cpu().double(), r, atol=1e-5, rtol=1e-5)


def _launcher_argv(extra):
    """test_restore_file_resumes_training's small configuration."""
    return ["--task", "node_prediction", "--arch", "multi_graphormer_base", "--criterion", "node_cross_entropy",
            "--dataset-name", "synthetic", "--batch-size", "8", "--update-freq", "2", "--lr", "5e-4", "--end-learning-rate", "1e-5",
            "--warmup-updates", "3", "--total-num-update", "8", "--encoder-embed-dim", "128", "--encoder-ffn-embed-dim", "128",
            "--encoder-attention-heads", "2", "--num_fusion_layers", "0", "--num_bottleneck_tokens", "2",
            "--attention-dropout", "0", "--act-dropout", "0", "--dropout", "0", "--spatial-pos-max", "5", "--log-interval", "1",
            "--synthetic-nodes", "6", "--synthetic-seq-len", "12", "--synthetic-batches", "5", "--seed", "5",
            "--bert-config", '{"dim": 128, "layers": 2, "heads": 2, "intermediate": 128, "vocab": 512, "max_pos": 64}',
            "--vit-config", '{"dim": 128, "layers": 2, "heads": 2, "intermediate": 128, "image_size": 32, "patch": 16}'] + extra


def test_launcher_clip_norm_logs_gnorm_and_clips():
    """--clip-norm 0.05: the unclipped run of this configuration (--clip-norm 0) prints gnorm 0.284, 0.019, 0.712, 0.389,
    0.253, 0.052, 0.357, 0.453 for its 8 updates (docs/experiment_log.md), so all but the second clip at 0.05."""
    from multimodaldiscussiontransformer_amd import train
    hist = train.main(_launcher_argv(["--max-update", "8", "--no-save", "--clip-norm", "0.05"]))
    assert len(hist) == 8
    print("clip-norm 0.05:", [(h["num_updates"], h["gnorm"], h["clip"], h["loss"]) for h in hist])
    for h in hist:
        assert math.isfinite(h["gnorm"]) and math.isfinite(h["clip"]) and h["skipped_updates"] == 0 and math.isfinite(h["loss"])
    assert any(h["clip"] > 0 and h["gnorm"] > 0.05 for h in hist)
    opt = train.main.last_run["optimizer"]
    assert opt.clip_norm == 0.05 and opt.guard_host()["clipped"] == sum(h["clip"] > 0 for h in hist)


def test_launcher_clip_norm_zero_reproduces_the_unguarded_run(monkeypatch):
    """--clip-norm 0 (measure and guard, no clipping) against the same run with the optimiser the launcher built before it
    had a norm pass — FusedAdam(clip_norm=None): no norm launch, the unguarded kernels — in test_train_gpu's 1e-4
    relative gate.  (The optimiser arithmetic is bit-identical, test_clip_norm_zero_is_bit_identical_...; the two runs
    differ by the order of backward's fp32 atomic adds only.)"""
    from multimodaldiscussiontransformer_amd import optim, train
    argv = _launcher_argv(["--max-update", "8", "--no-save", "--clip-norm", "0"])
    hist = train.main(argv)
    assert train.main.last_run["optimizer"].norm_launches > 0

    class UnguardedAdam(optim.FusedAdam):
        def __init__(self, params, **kw):
            kw["clip_norm"] = None
            super().__init__(params, **kw)

        def guard_log_vector(self):          # the log line's fields, for a run that measures nothing
            return torch.zeros(4, dtype=torch.float64, device="cuda")

    monkeypatch.setattr(optim, "FusedAdam", UnguardedAdam)
    want = train.main(argv)
    plain = train.main.last_run["optimizer"]
    assert isinstance(plain, UnguardedAdam) and plain.clip_norm is None and plain.norm_launches == 0
    print("clip-norm 0:", [(h["num_updates"], h["gnorm"], h["loss"]) for h in hist], "unguarded:", [h["loss"] for h in want])
    assert [h["num_updates"] for h in hist] == list(range(1, 9)) == [h["num_updates"] for h in want]
    for h, w in zip(hist, want):
        assert abs(h["loss"] - w["loss"]) <= 1e-4 * max(1.0, abs(w["loss"])), (h, w)
        assert h["gnorm"] > 0 and h["clip"] == 0 and h["skipped_updates"] == 0


def test_launcher_checkpoint_keeps_adams_step(tmp_path):
    from multimodaldiscussiontransformer_amd import train
    d = tmp_path / "ck"
    train.main(_launcher_argv(["--max-update", "4", "--save-dir", str(d), "--clip-norm", "0.05"]))
    ck = d / "checkpoint_last.pt"
    st = torch.load(ck, weights_only=False)
    steps = {int(e["step"]) for e in st["last_optimizer_state"]["state"].values()}
    assert steps == {4} and st["optimizer_history"][-1]["num_updates"] == 4
    second = train.main(_launcher_argv(["--max-update", "6", "--restore-file", str(ck), "--no-save", "--clip-norm", "0.05"]))
    assert [h["num_updates"] for h in second] == [5, 6] and all(h["skipped_updates"] == 0 for h in second)
    opt = train.main.last_run["optimizer"]
    assert opt.step_count == 6 and opt.applied_steps_host() == 6 and int(opt.applied_steps) == 6


def test_launcher_raises_on_a_non_finite_update_unless_fp16(monkeypatch):
    """A NaN planted in the gradient arena of update 2: --bf16 stops with FloatingPointError at the next log line, the
    weights untouched by that update; --fp16 skips it, counts it and trains on."""
    from multimodaldiscussiontransformer_amd import train
    from multimodaldiscussiontransformer_amd.ddp import DataParallel
    real = DataParallel.finish_backward
    calls = {"n": 0}

    def poisoned(self, *a, **k):
        out = real(self, *a, **k)
        calls["n"] += 1
        if calls["n"] == 2:
            next(p for p in self.model.parameters() if hasattr(p, "main_grad") and p.numel() > 100).main_grad.view(-1)[5] = float("nan")
        return out

    monkeypatch.setattr(DataParallel, "finish_backward", poisoned)
    with pytest.raises(FloatingPointError, match="between 2 and 2"):
        train.main(_launcher_argv(["--max-update", "4", "--no-save", "--bf16"]))
    calls["n"] = 0
    hist = train.main(_launcher_argv(["--max-update", "4", "--no-save", "--fp16"]))
    assert [h["skipped_updates"] for h in hist] == [0, 1, 1, 1] and not math.isfinite(hist[1]["gnorm"])
    assert all(math.isfinite(h["loss"]) for h in hist) and math.isfinite(hist[-1]["gnorm"])
    opt = train.main.last_run["optimizer"]
    assert opt.step_count == 4 and opt.applied_steps_host() == 3
    assert all(bool(torch.isfinite(p).all()) for p in opt.params)


@pytest.mark.skipif(os.environ.get("MDT_SKIP_MULTIPROC") == "1", reason="MDT_SKIP_MULTIPROC=1")
def test_two_ranks_agree_on_gnorm_bits():
    """tests/test_ddp_gpu.py's pattern: two fresh child processes (gloo, both on cuda:0) under a hard time limit."""
    import signal
    env = dict(os.environ, MDT_SINGLE_DEVICE="1", HSA_ENABLE_IPC_MODE_LEGACY="0", GPU_MAX_HW_QUEUES="4")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29537", os.path.join(ROOT, "tests", "grad_clip_gpu_worker.py")]
    proc = subprocess.Popen(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True)
    try:
        out, err = proc.communicate(timeout=300)
    except subprocess.TimeoutExpired:
        os.killpg(proc.pid, signal.SIGKILL)          # exactly the process group started above
        out, err = proc.communicate()
        pytest.fail("two-rank worker did not finish in 300 s:\n" + out[-2000:] + err[-2000:])
    print(out[-2000:])
    assert proc.returncode == 0, out[-3000:] + err[-3000:]
    assert "GRAD_CLIP_DDP_OK" in out, out[-3000:]
