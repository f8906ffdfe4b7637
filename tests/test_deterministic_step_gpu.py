"""Deterministic (ordered) mode at the level of a training step: the Tiny model of oracle.cases.tiny_hparams("A") (text and
images, D = 768) with dropout on, in fp32 and bf16.  With engine.set_deterministic(True) the loss and every element of the
fp32 gradient arena are bit-for-bit functions of weights, batch and seeds — across repetitions and with another stream
keeping the device busy — no launch of the step accumulates with float atomics, and the results still pass the oracle
gate of tests/test_model_gpu.py.  The switch leaves nothing behind; the launcher's --deterministic reproduces a run."""
import numpy as np
import pytest
import torch

from oracle import cases
from oracle import mdt_ref_cpu as R
from oracle import structure as S
from tests.util_model import fill_hash_weights, model_args, named_canonical_params, split_qkv_grad

pytestmark = pytest.mark.gpu

P_DROP = 0.1


@pytest.fixture
def engine():
    from multimodaldiscussiontransformer_amd import engine as E
    from multimodaldiscussiontransformer_amd import fp8
    was = E.deterministic()
    yield E
    fp8.ACTIVE = None
    E.set_deterministic(was)


def _model(dtype, dropout=P_DROP):
    from multimodaldiscussiontransformer_amd.criterions import GraphPredictionNodeCrossEntropy
    from multimodaldiscussiontransformer_amd.data.packer import pack_batch
    from multimodaldiscussiontransformer_amd.models import GraphormerModel
    hp = cases.tiny_hparams("A")
    trees = cases.tiny_trees("A", hp)
    model = GraphormerModel.build_model(model_args(hp, dropout=dropout, attention_dropout=dropout, act_dropout=dropout), task=None)
    model = fill_hash_weights(model).cuda().to(dtype).train()
    model.prepare_main_grads()
    pb = pack_batch(trees, 5)
    assert pb.I > 0, "the fixture has images"
    crit = GraphPredictionNodeCrossEntropy(None, positive_weight=hp.pos_weight, negative_weight=hp.neg_weight)
    sample = {"nsamples": len(trees), "net_input": {"batched_data": pb.batched_data}}
    return hp, trees, model, crit, sample


def _step(model, crit, sample, seed=1234):
    """forward + backward from zeroed gradients and one dropout seed → (loss, gradient arena), copies"""
    torch.manual_seed(seed)
    model.zero_main_grads()
    loss, _, _ = crit(model, sample)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), model.main_grad_flat.clone()


def _same(a, b):
    return torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a.view(torch.int16),
                       b.view(torch.int32) if b.dtype == torch.float32 else b.view(torch.int16))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_ordered_step_is_bit_reproducible(engine, dtype):
    from multimodaldiscussiontransformer_amd import ops
    _, _, model, crit, sample = _model(dtype)
    engine.set_deterministic(True)
    ops.float_atomic_launches(reset=True)
    loss0, grad0 = _step(model, crit, sample)
    assert ops.float_atomic_launches() == 0, "an ordered step launched a float-atomic kernel"
    assert bool(torch.isfinite(grad0).all()) and float(grad0.abs().max()) > 0
    for rep in range(1, 4):
        loss, grad = _step(model, crit, sample)
        assert _same(loss, loss0), f"repetition {rep}: loss bits differ"
        assert _same(grad, grad0), f"repetition {rep}: {int((grad != grad0).sum())} gradient elements differ"
    # the same while another stream keeps the device busy with an unrelated large GEMM
    noise = torch.cuda.Stream()
    a = torch.randn(4096, 4096, device="cuda", dtype=torch.bfloat16)
    for rep in range(2):
        with torch.cuda.stream(noise):
            for _ in range(40):
                a @ a
        loss, grad = _step(model, crit, sample)
        assert _same(loss, loss0) and _same(grad, grad0), f"with a busy second stream, repetition {rep}: bits differ"
    noise.synchronize()
    assert ops.float_atomic_launches() == 0
    # another seed is another step: the comparison above is not vacuous
    _, other = _step(model, crit, sample, seed=99)
    assert not _same(other, grad0)
    # the default step does use them
    engine.set_deterministic(False)
    _step(model, crit, sample)
    assert ops.float_atomic_launches(reset=True) > 0


def test_ordered_step_passes_the_oracle_gate(engine):
    """tests/test_model_gpu.py's gate for this fixture (fp32, no dropout): logits and every parameter gradient within 1e-3
    of the oracle on the same seeded inputs."""
    hp, trees, model, crit, sample = _model(torch.float32, dropout=0.0)
    engine.set_deterministic(True)
    _step(model, crit, sample)
    with torch.no_grad():
        logits, _ = model(sample["net_input"]["batched_data"])
    ref_b = S.collate(trees, 5)
    W = R.make_weights(hp)
    batch = R.to_torch_batch(ref_b)
    lo, _ = R.model_forward(W, hp, batch)
    ol, _ = R.node_cross_entropy(lo, batch["y"], batch["y_mask"], hp)
    ol.backward()
    np.testing.assert_allclose(logits.cpu().numpy(), lo.detach().numpy(), atol=1e-3)
    grads = {n: getattr(p, "main_grad", None) for n, p in named_canonical_params(model).items()}
    checked = 0
    for name in W:
        if W[name].grad is None:
            continue
        gr = split_qkv_grad(name, grads)
        assert gr is not None, name
        ref = W[name].grad
        assert float((gr.float().cpu() - ref).abs().max()) <= 1e-3 * max(1.0, float(ref.abs().max())), name
        checked += 1
    assert checked >= 90, checked


def test_switch_leaves_no_state_behind(engine):
    """The default mode before and after a deterministic step is the default mode: same loss bits (the forward has no
    atomics), the same number of float-atomic launches, gradients equal up to the order of the fp32 atomics
    (the tolerance tests/test_model_gpu.py grants two default runs of this model)."""
    from multimodaldiscussiontransformer_amd import ops
    _, _, model, crit, sample = _model(torch.float32)
    assert not engine.deterministic()
    ops.float_atomic_launches(reset=True)
    loss_a, grad_a = _step(model, crit, sample)
    n_a = ops.float_atomic_launches(reset=True)
    engine.set_deterministic(True)
    assert engine.deterministic()
    loss_d, grad_d = _step(model, crit, sample)
    assert ops.float_atomic_launches(reset=True) == 0
    engine.set_deterministic(False)
    assert not engine.deterministic()
    loss_b, grad_b = _step(model, crit, sample)
    assert ops.float_atomic_launches(reset=True) == n_a > 0
    assert _same(loss_a, loss_b) and _same(loss_a, loss_d)
    scale = max(1.0, float(grad_a.abs().max()))
    torch.testing.assert_close(grad_b, grad_a, atol=2e-5 * scale, rtol=1e-4)
    torch.testing.assert_close(grad_d, grad_a, atol=2e-5 * scale, rtol=1e-4)       # the two modes differ by summation order only


def test_environment_sets_the_default():
    import subprocess
    import sys
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for val, want in (("1", "True"), ("0", "False")):
        r = subprocess.run([sys.executable, "-c", "from multimodaldiscussiontransformer_amd import engine; print(engine.deterministic())"],
                           cwd=root, env=dict(os.environ, MDT_DETERMINISTIC=val), capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip() == want, (r.stdout, r.stderr[-300:])


def test_fp8_and_deterministic_refuse_each_other(engine):
    _, _, model, _, _ = _model(torch.bfloat16)
    engine.set_deterministic(True)
    with pytest.raises(NotImplementedError, match="deterministic"):
        model.enable_fp8()
    engine.set_deterministic(False)
    model.enable_fp8()
    try:
        with pytest.raises(NotImplementedError, match="fp8"):
            engine.set_deterministic(True)
        assert not engine.deterministic()
    finally:
        model.enable_fp8(False)


def test_structural_bias_past_272_tokens_is_refused(engine):
    """The key-chunked long path has its bias gradient with float atomics only: ordered mode says so instead of using it."""
    E = engine
    nseq, Sq, H, D, ns = 1, 300, 2, 32, 7
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(nseq * Sq, D, generator=g) * 0.5).cuda().requires_grad_(True)
    qkv_w = torch.nn.Parameter((torch.randn(3 * D, D, generator=g) * 0.1).cuda())
    o_w = torch.nn.Parameter((torch.randn(D, D, generator=g) * 0.1).cuda())
    table = torch.nn.Parameter((torch.randn(ns, H, generator=g) * 0.1).cuda())
    virt = torch.nn.Parameter((torch.randn(1, H, generator=g) * 0.1).cuda())
    spec = E.AttnSpec(nseq=nseq, S=Sq, H=H, attn_bias=torch.zeros(nseq, Sq, Sq, device="cuda"),
                      spatial_pos=torch.randint(0, ns, (nseq, Sq - 1, Sq - 1), generator=g).to(torch.int32).cuda(),
                      sp_table=table, virt=virt)

    def run(tape, xv):
        return (E.attention_layer(tape, xv, qkv_w, None, o_w, None, spec),)

    E.set_deterministic(True)
    (out,) = E.run_tape(run, [x], [qkv_w, o_w, table, virt])
    with pytest.raises(NotImplementedError, match="272"):
        out.sum().backward()
    E.set_deterministic(False)
    (out,) = E.run_tape(run, [x], [qkv_w, o_w, table, virt])
    out.sum().backward()                    # the default mode takes the long path as before
    assert table.grad is not None and bool(torch.isfinite(table.grad).all())


def _launcher_argv(save_dir):
    return ["--task", "node_prediction", "--arch", "multi_graphormer_base", "--criterion", "node_cross_entropy",
            "--dataset-name", "synthetic", "--batch-size", "8", "--update-freq", "2", "--lr", "5e-4", "--end-learning-rate", "1e-5",
            "--warmup-updates", "3", "--total-num-update", "8", "--encoder-embed-dim", "128", "--encoder-ffn-embed-dim", "128",
            "--encoder-attention-heads", "2", "--num_fusion_layers", "1", "--num_bottleneck_tokens", "2",
            "--attention-dropout", "0.1", "--act-dropout", "0.1", "--dropout", "0.1", "--spatial-pos-max", "5", "--log-interval", "1",
            "--synthetic-nodes", "6", "--synthetic-seq-len", "12", "--synthetic-batches", "5", "--synthetic-image-frac", "0.5", "--seed", "5",
            "--bert-config", '{"dim": 128, "layers": 2, "heads": 2, "intermediate": 128, "vocab": 512, "max_pos": 64}',
            "--vit-config", '{"dim": 128, "layers": 2, "heads": 2, "intermediate": 128, "image_size": 32, "patch": 16}',
            "--deterministic", "--max-update", "3", "--save-dir", str(save_dir)]


def test_launcher_deterministic_flag_reproduces_a_run(engine, tmp_path, capsys):
    from multimodaldiscussiontransformer_amd import ops, train
    runs = []
    for i in range(2):
        ops.float_atomic_launches(reset=True)
        hist = train.main(_launcher_argv(tmp_path / f"run{i}"))
        assert ops.float_atomic_launches() == 0
        assert not engine.deterministic(), "the launcher left the process-wide switch on"
        sd = torch.load(tmp_path / f"run{i}" / "checkpoint_last.pt", weights_only=False)["model"]
        runs.append(([h["loss"] for h in hist], sd))
    assert "--deterministic" in capsys.readouterr().err
    (l0, s0), (l1, s1) = runs
    assert len(l0) == 3 and l0 == l1, (l0, l1)
    assert set(s0) == set(s1)
    for k in s0:
        assert _same(s0[k], s1[k]) if s0[k].dtype in (torch.float32, torch.bfloat16) else torch.equal(s0[k], s1[k]), k
    with pytest.raises(SystemExit):
        train.main(_launcher_argv(tmp_path / "x") + ["--deterministik"])          # unknown flags are still refused
    with pytest.raises(SystemExit):
        train.main(_launcher_argv(tmp_path / "y") + ["--fp8"])
    assert not engine.deterministic()
