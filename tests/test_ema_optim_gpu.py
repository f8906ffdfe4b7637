"""FusedAdam's weight average (ema_decay=...) on the Tiny model of oracle.cases.tiny_hparams("A"): the launches of an optimiser
without it are today's, the arena follows the host fp64 recurrence over snapshots of the masters (copy before the start update,
plain launches between the update counts, a skipped update), ema_weights() swaps the average in and every bit back out, and the
state dict round-trips under the model's keys."""
import pytest
import torch

import tests.ema_reference as E
from tests.test_deterministic_step_gpu import _model, _same

pytestmark = pytest.mark.gpu


@pytest.fixture
def engine():
    from multimodaldiscussiontransformer_amd import engine as EN
    from multimodaldiscussiontransformer_amd import fp8
    was = EN.deterministic()
    EN.set_deterministic(True)
    yield EN
    fp8.ACTIVE = None
    EN.set_deterministic(was)


class CountingLib:
    """optim.lib with the names of the entry points called, in order."""

    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("mdt_"):
            return fn

        def call(*a):
            self.calls.append(name)
            return fn(*a)
        return call


def _opt(model, **kw):
    from multimodaldiscussiontransformer_amd.optim import FusedAdam
    return FusedAdam([p for p in model.parameters() if hasattr(p, "main_grad")], lr=1e-3, **kw)


def _backward(model, crit, sample, seed):
    torch.manual_seed(seed)
    model.zero_main_grads()
    loss, _, _ = crit(model, sample)
    loss.backward()


def _weights(opt):
    """The fp32 weights the average follows (masters, or the fp32 parameters), one flat host tensor in parameter order."""
    return torch.cat([(opt.state[id(p)]["master"] if "master" in opt.state[id(p)] else p.detach()).reshape(-1) for p in opt.params])


def _ema(opt):
    return torch.cat([opt.state[id(p)]["ema"].reshape(-1) for p in opt.params])


@pytest.mark.parametrize("clip_norm", [None, 0.0], ids=["unguarded", "guarded"])
def test_no_decay_issues_todays_launches(engine, monkeypatch, clip_norm):
    """ema_decay=None: nothing allocated, only the entry points that existed before the average, and after 3 deterministic steps the
    bits of an optimiser that DOES keep an average (whose Adam arithmetic must not notice it)."""
    from multimodaldiscussiontransformer_amd import optim
    _, _, model, crit, sample = _model(torch.bfloat16, dropout=0.0)
    twin = _model(torch.bfloat16, dropout=0.0)[2]
    lib = CountingLib(optim.lib)
    monkeypatch.setattr(optim, "lib", lib)
    plain, avg = _opt(model, clip_norm=clip_norm), _opt(twin, clip_norm=clip_norm, ema_decay=0.9, ema_update_freq=2)
    assert plain.ema_arena is None and plain.ema_decay is None and all("ema" not in st for st in plain.state.values())
    for k in range(3):
        _backward(model, crit, sample, 100 + k)
        mark = len(lib.calls)
        plain.step()
        names = set(lib.calls[mark:])
        assert names and not any("ema" in n for n in names), names
        assert names <= {"mdt_adam_step_multi", "mdt_adam_step", "mdt_adam_step_multi_guarded", "mdt_adam_step_guarded",
                         "mdt_grad_sumsq_multi", "mdt_grad_sumsq", "mdt_grad_norm_finalize"}, names
        _backward(twin, crit, sample, 100 + k)
        mark = len(lib.calls)
        avg.step()
        names = set(lib.calls[mark:])
        assert any(n.startswith("mdt_adam_step_multi_ema") for n in names) == (k == 1), (k, names)      # update counts 1, 2, 3: only 2 % 2 == 0
    torch.cuda.synchronize()
    for p, q in zip(plain.params, avg.params):
        assert _same(p.data, q.data) and _same(plain.state[id(p)]["master"], avg.state[id(q)]["master"])
        assert _same(plain.state[id(p)]["m"], avg.state[id(q)]["m"]) and _same(plain.state[id(p)]["v"], avg.state[id(q)]["v"])
    with pytest.raises(RuntimeError, match="ema_decay"):
        plain.ema_state_dict(model)
    with pytest.raises(RuntimeError, match="ema_decay"):
        with plain.ema_weights():
            pass


@pytest.mark.parametrize("start,freq", [(2, 2), (3, 1)], ids=["start2_freq2", "start3_freq1"])
def test_recurrence(engine, start, freq):
    """6 steps, the masters snapshotted after each; update 4 has a NaN planted in its gradient and is skipped on the device.  The
    schedule follows the count INCLUDING the update (FairSeq hands EMA.step the new num_updates): start 2 / freq 2 updates at counts
    2, 4 (skipped), 6 with the decay; start 3 / freq 1 copies at counts 1 and 2 and averages from 3 on."""
    _, _, model, crit, sample = _model(torch.bfloat16, dropout=0.0)
    opt = _opt(model, clip_norm=0.0, ema_decay=0.9, ema_start_update=start, ema_update_freq=freq)
    e0 = _ema(opt)
    assert torch.equal(e0, _weights(opt)), "the average is seeded from the masters"
    snaps, decays = [], []
    for k in range(1, 7):
        _backward(model, crit, sample, 200 + k)
        if k == 4:
            next(p for p in opt.params if p.numel() > 100).main_grad.view(-1)[5] = float("nan")
        before = _ema(opt)
        opt.step()
        snaps.append(_weights(opt))
        d = None if k % freq else (0.0 if k < start else 0.9)
        if k == 4:
            d = None
            assert torch.equal(snaps[-1], snaps[-2]) and _same(_ema(opt), before), "a skipped update moved the weights or the average"
        decays.append(d)
        if d is None:
            assert _same(_ema(opt), before), f"update {k}: a plain launch moved the average"
        elif d == 0.0:
            assert _same(_ema(opt), snaps[-1]), f"update {k}: before the start update the average is a copy"
    assert opt.guard_host()["skipped"] == 1
    assert sum(d == 0.9 for d in decays) >= 2
    E.check(_ema(opt).cpu(), E.reference_recurrence(e0.cpu(), [s.cpu() for s in snaps], decays), f"start {start} freq {freq}")
    assert not torch.equal(_ema(opt), snaps[-1])


def _logits(model, sample):
    with torch.no_grad():
        out, _ = model(sample["net_input"]["batched_data"])
    return out.detach().float().cpu().clone()


@pytest.mark.parametrize("fp8_on", [False, True], ids=["bf16", "fp8"])
def test_ema_weights_context(engine, fp8_on):
    from multimodaldiscussiontransformer_amd import fp8
    if fp8_on:
        engine.set_deterministic(False)                     # the fp8 path has no ordered reductions
    _, _, model, crit, sample = _model(torch.bfloat16, dropout=0.0)
    state = model.enable_fp8() if fp8_on else None
    opt = _opt(model, ema_decay=0.5)
    for k in range(2):
        _backward(model, crit, sample, 300 + k)
        opt.step()
    model.eval()
    raw = _logits(model, sample)
    bits0 = [p.data.clone() for p in opt.params]
    masters0 = [opt.state[id(p)]["master"].clone() for p in opt.params]
    ema0 = _ema(opt)
    # a copy of the model with the averaged weights loaded through its own state dict
    want = None
    if not fp8_on:
        twin = _model(torch.bfloat16, dropout=0.0)[2]
        sd = twin.state_dict()
        sd.update({k: v.to(sd[k].dtype) for k, v in opt.ema_state_dict(model).items()})
        twin.load_state_dict(sd)
        engine.weights_changed()
        want = _logits(twin.eval(), sample)
    epoch, version = engine.WEIGHT_EPOCH, (state.weights_version if fp8_on else None)
    with opt.ema_weights():
        assert engine.WEIGHT_EPOCH > epoch and (not fp8_on or state.weights_version > version)
        epoch, version = engine.WEIGHT_EPOCH, (state.weights_version if fp8_on else None)
        for p in opt.params:
            assert _same(p.data, opt.state[id(p)]["ema"].to(p.dtype)), "inside: the parameter is not T(ema)"
        inside = _logits(model, sample)
        if want is not None:
            assert torch.equal(inside, want), "inside: not the logits of a model holding the averaged weights"
        assert not torch.equal(inside, raw)
        with pytest.raises(RuntimeError, match="nest"):
            with opt.ema_weights():
                pass
        with pytest.raises(RuntimeError, match="inside ema_weights"):
            opt.step()
    assert engine.WEIGHT_EPOCH > epoch and (not fp8_on or state.weights_version > version)
    torch.cuda.synchronize()
    for p, b, m in zip(opt.params, bits0, masters0):
        assert _same(p.data, b) and _same(opt.state[id(p)]["master"], m), "after: a parameter or master did not get its bits back"
    assert _same(_ema(opt), ema0)
    assert torch.equal(_logits(model, sample), raw)
    # an exception inside still restores
    with pytest.raises(KeyError):
        with opt.ema_weights():
            raise KeyError("x")
    assert all(_same(p.data, b) for p, b in zip(opt.params, bits0))
    model.train()
    _backward(model, crit, sample, 310)
    opt.step()                                              # and the optimiser steps again


def test_fp32_model_exchanges_and_restores(engine):
    """No masters: the swap trades parameter and average, and trades them back."""
    _, _, model, crit, sample = _model(torch.float32, dropout=0.0)
    opt = _opt(model, ema_decay=0.5)
    _backward(model, crit, sample, 400)
    opt.step()
    p0, e0 = _weights(opt), _ema(opt)
    assert not torch.equal(p0, e0)
    with opt.ema_weights():
        assert _same(_weights(opt), e0) and _same(_ema(opt), p0)
    assert _same(_weights(opt), p0) and _same(_ema(opt), e0)


def test_state_dict_round_trip(engine):
    _, _, model, crit, sample = _model(torch.bfloat16, dropout=0.0)
    opt = _opt(model, ema_decay=0.5)
    _backward(model, crit, sample, 500)
    opt.step()
    sd = opt.ema_state_dict(model)
    spans = [(p.data.data_ptr(), p.data.data_ptr() + p.numel() * p.element_size()) for p in opt.params]
    trainable = [k for k, v in model.state_dict().items() if any(b <= v.data_ptr() < e for b, e in spans)]
    assert list(sd) == trainable and len(sd) > len(opt.params), "the model's trainable state-dict keys, q/k/v split"
    assert any(".q_proj." in k or ".query." in k for k in sd)
    assert all(v.dtype == torch.float32 and v.device.type == "cpu" and tuple(v.shape) == tuple(model.state_dict()[k].shape) for k, v in sd.items())
    assert sum(v.numel() for k, v in sd.items()) >= sum(p.numel() for p in opt.params)
    ema0 = _ema(opt)
    opt.ema_arena.fill_(7.0)
    opt.load_ema_state_dict(model, sd)
    assert _same(_ema(opt), ema0)
    again = opt.ema_state_dict(model)
    assert all(_same(again[k], sd[k]) for k in sd)
    short = dict(sd)
    gone = short.pop(next(iter(short)))
    with pytest.raises(RuntimeError, match="missing keys"):
        opt.load_ema_state_dict(model, short)
    with pytest.raises(RuntimeError, match="unexpected keys"):
        opt.load_ema_state_dict(model, dict(sd, not_a_key=gone))


@pytest.mark.parametrize("clip_norm", [None, 0.0], ids=["unguarded", "guarded"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_parameters_outside_the_table_take_the_single_tensor_form(dtype, clip_norm):
    """tests/test_grad_clip_gpu.py's stand-alone parameters: all in the table ("multi"), one launch per tensor ("single"), every
    other one with only p.grad ("mix": those take the per-tensor launches of step(), the single-tensor `_ema` entry points).  The three optimisers
    end with the same bits in parameters and averages, and ema_weights() covers the parameters outside the table too."""
    from multimodaldiscussiontransformer_amd.optim import FusedAdam
    from tests.test_grad_clip_gpu import CLIP_SHAPES, _params, _set_grads
    grads = [[(torch.randn(s, generator=torch.Generator().manual_seed(31 + 7 * k + i)) * 0.1).bfloat16().float() for i, s in enumerate(CLIP_SHAPES)]
             for k in range(3)]                                   # bf16 numbers: a bf16 p.grad holds what an fp32 main_grad holds
    out = {}
    for mode in ("multi", "single", "mix"):
        _, ps, _ = _params(CLIP_SHAPES, dtype, torch.Generator().manual_seed(5), mode)
        opt = FusedAdam(ps, lr=1e-2, clip_norm=clip_norm, multi_tensor=(mode != "single"), ema_decay=0.9, ema_start_update=2)
        for g in grads:
            _set_grads(ps, g)
            opt.step()
        out[mode] = (opt, [p.data.clone() for p in ps], [opt.state[id(p)]["ema"].clone() for p in ps])
    for mode in ("single", "mix"):
        for a, b in zip(out[mode][1] + out[mode][2], out["multi"][1] + out["multi"][2]):
            assert _same(a, b), f"{mode}: not the bits of the table form"
    opt, params, emas = out["mix"]
    assert not any(_same(e, (opt.state[id(p)]["master"] if dtype == torch.bfloat16 else p.data)) for p, e in zip(opt.params, emas))
    with opt.ema_weights():
        for p, e in zip(opt.params, emas):
            assert _same(p.data, e.to(dtype)), "inside: a parameter outside the table was not swapped"
    for p, b, e in zip(opt.params, params, emas):
        assert _same(p.data, b) and _same(opt.state[id(p)]["ema"], e)
