"""tests/node_objective_reference.py proves itself without a GPU, and the Python layers above mdt_node_objective are checked as
far as they go without one.

The reference's VALUES are the fp64 autograd of torch's own expressions: F.cross_entropy(weight, label_smoothing, "sum") at
gamma = 0, an explicit (1 - q)^gamma focal expression elsewhere, reference_node_ce_f32 with both knobs at 0.  Its BOUNDS accept
an fp32 emulation of the kernel's stated arithmetic at every case of the GPU matrix (tests/test_node_objective_gpu.py) and
reject each named mutant of it at the cases where the mutant can differ at all (the cases that apply are counted and must
exist).  Then: the launcher's derived flags, the criterion's choice between ops.node_ce and ops.node_objective (ops
monkeypatched: no device), and compute_metrics with and without nll_loss."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tests.loss_optim_reference as LR
import tests.node_objective_reference as R
from tests.node_objective_reference import bf16, f32, f64

WN, WP = R.WEIGHTS


def rejected(fn):
    """A mutant's err / bound does not belong in the worst-error table the GPU files report from."""
    worst = dict(LR.WORST)
    try:
        fn()
    except AssertionError:
        return True
    finally:
        LR.WORST.clear()
        LR.WORST.update(worst)
    return False


# ------------------------------------------------------------------------------------------------ values against autograd
def _autograd(l, rows, y, eps, gamma, fp16_loss, gs, explicit):
    """(out [2], d logits [M, 2]) in fp64 from torch's autograd; ``explicit``: the (1 - q)^gamma expression, otherwise
    F.cross_entropy (gamma must be 0)."""
    lf = l.float()
    w = torch.tensor([WN, WP], dtype=f32)
    if fp16_loss:
        lf, w = lf.half().float(), w.half().float()
    x = lf.double().clone().requires_grad_(True)
    w = w.double()
    eps, gamma = float(np.float32(eps)), float(np.float32(gamma))
    lr_, yy = x[rows.long()], y.long()
    if explicit:
        lp = torch.log_softmax(lr_, 1)
        lpy = lp.gather(1, yy[:, None])[:, 0]
        # 1 - q with q = exp(lp_y), written -expm1(lp_y): in fp64 `1 - exp(lp_y)` is 0 for the saturated rows (q = 1 - 9e-27) and
        # autograd then multiplies 0^(gamma - 1) = inf by 0
        one_minus_q = -torch.expm1(lpy)
        nll = -w[yy] * lpy
        smooth = -(lp * w[None, :]).sum(1)
        loss = ((1.0 - eps) * one_minus_q ** gamma * nll + eps / 2 * smooth).sum()
    else:
        assert gamma == 0.0
        loss = F.cross_entropy(lr_, yy, weight=w, label_smoothing=eps, reduction="sum")
        nll = -w[yy] * torch.log_softmax(lr_, 1).gather(1, yy[:, None])[:, 0]
    (g,) = torch.autograd.grad(loss, x)
    return torch.stack([loss.detach(), nll.sum().detach()]), g * float(np.float32(gs))


def _close(got, want, what):
    # fp64 against fp64: two ways of writing one expression.  (1 - q)^gamma cancels where q is near 1 (relative error up to
    # 2^-53 / (1 - q)), which is why the kernel does not write it that way; the saturated rows are compared through the
    # absolute term.
    tol = 1e-9 * want.abs() + 1e-12
    assert bool(((got - want).abs() <= tol).all()), f"{what}: worst {float(((got - want).abs() - tol).max()):.3e} over"


@pytest.mark.parametrize("fp16_loss", [0, 1])
@pytest.mark.parametrize("dtype", [f32, bf16], ids=["f32", "bf16"])
def test_values_are_fp64_autograd_of_torchs_expressions(dtype, fp16_loss):
    for nlab in (1, 257):
        l, rows, y = R.inputs(nlab, dtype)
        # the saturated rows at +-15 here: at +-30 the fp64 log-softmax of the target is exactly 0, 1 - q is 0 and autograd's
        # derivative of 0^gamma is inf times 0 for gamma < 1 (the emulation test below keeps them at +-30)
        l = l.clamp(-15.0, 15.0)
        for (eps, gamma) in R.SETTINGS:
            for gs in R.SCALES:
                ref = R.reference_node_objective(l, rows, y, WN, WP, eps, gamma, fp16_loss, gs)
                forms = [True] + ([False] if gamma == 0.0 else [])
                for explicit in forms:
                    out, g = _autograd(l, rows, y, eps, gamma, fp16_loss, gs, explicit)
                    what = f"nlab{nlab} eps{eps} gamma{gamma} explicit{explicit}"
                    _close(ref["out"][0], out, what + " out")
                    _close(ref["dlogits"][0], g, what + " dlogits")


def test_plain_setting_is_reference_node_ce_f32():
    for nlab in (1, 257, 1031):
        for dtype in (f32, bf16):
            l, rows, y = R.inputs(nlab, dtype)
            for gs in R.SCALES:
                ref = R.reference_node_objective(l, rows, y, WN, WP, 0.0, 0.0, 0, gs)
                old = LR.reference_node_ce_f32(l, rows, y, WN, WP, gs)
                _close(ref["out"][0][0:1], old["loss"][0], "loss")
                _close(ref["out"][0][1:2], old["loss"][0], "nll")
                _close(ref["dlogits"][0], old["dlogits"][0], "dlogits")
                assert ref["counters"] == old["counters"]
                # the same arithmetic up to the exact products by 1 - eps = 1 and f = 1: the bounds are of one size
                assert bool((ref["out"][1][0] <= 2.0 * old["loss"][1] + 1e-30).all()) and bool((old["loss"][1] <= 2.0 * ref["out"][1][0] + 1e-30).all())


# ------------------------------------------------------------------------------------------------ the emulation and its mutants
MUTANTS = ("f_detached", "smoothing_eps", "focal_on_smoothing", "no_grad_scale", "weights_swapped")


def emulate(l, rows, y, w_neg, w_pos, fp16_loss, eps, gamma, gs, dl0, mutant=None):
    """node_objective_kernel in fp32 torch, operation by operation → (out fp32 [2], counters, d logits of the logits' type)."""
    T = l.dtype
    rr, yy = rows.long(), y.long()
    n = int(yy.numel())
    t32 = lambda v: torch.tensor(v, dtype=f32)      # noqa: E731
    lf = l.float()[rr]
    wn, wp = t32(w_neg), t32(w_pos)
    if mutant == "weights_swapped":
        wn, wp = wp, wn
    if fp16_loss:
        lf, wn, wp = lf.half().float(), wn.half().float(), wp.half().float()
    eps, gamma, gs = t32(eps), t32(gamma), t32(1.0 if mutant == "no_grad_scale" else gs)
    ome, he, sw = t32(1.0) - eps, (eps if mutant == "smoothing_eps" else eps * t32(0.5)), wn + wp
    m = lf.max(1, keepdim=True).values
    a = lf - m
    e = torch.exp(a)
    S = e[:, :1] + e[:, 1:]
    lp = a - torch.log(S)
    if fp16_loss:
        hp = (e * (1.0 / S)).half()
        pred = (hp[:, 1] > hp[:, 0]).long()
    else:
        pred = (lf[:, 1] > lf[:, 0]).long()
    lpy, lpo = lp.gather(1, yy[:, None])[:, 0], lp.gather(1, (1 - yy)[:, None])[:, 0]
    wy, wo = torch.where(yy == 1, wp, wn), torch.where(yy == 1, wn, wp)
    nll = -(wy * lpy)
    f = torch.exp(gamma * lpo)
    smooth0 = nll - wo * lpo
    smooth = f * smooth0 if mutant == "focal_on_smoothing" else smooth0
    li = ome * (f * nll) + he * smooth

    def total(v):
        parts = []
        for t in range(256):
            acc = torch.zeros((), dtype=f32)
            for x in v[t::256]:
                acc = acc + x
            parts.append(acc)
        tot = torch.zeros((), dtype=f32)
        for p in parts:
            tot = tot + p
        return tot

    out = torch.stack([total(li), total(nll)])
    q, r = torch.exp(lpy), torch.exp(lpo)
    inner = r if mutant == "f_detached" else r - (gamma * q) * lpy
    A = ome * (wy * (f * inner))
    so, sy = sw * r - wo, sw * q - wy
    if mutant == "focal_on_smoothing":
        # the gradient of that mutant loss, f smooth0: f d smooth0 + smooth0 df with df / dl_o = gamma f q = -df / dl_y
        so, sy = f * so + smooth0 * (gamma * f * q), f * sy - smooth0 * (gamma * f * q)
    go, gy = A + he * so, -A + he * sy
    g = torch.zeros(n, 2, dtype=f32)
    if n:
        g.scatter_(1, yy[:, None], gy[:, None]).scatter_(1, (1 - yy)[:, None], go[:, None])
    dl = torch.zeros_like(dl0)
    dl[rr] = (g * gs).to(T)
    counters = [int((pred == yy).sum()), int(((pred == yy) & (pred == 1)).sum()), int((yy == 1).sum()), int((pred == 1).sum())]
    return out, counters, dl


def check_all(got, ref, what):
    out, counters, dl = got
    R.check("node_objective out", out, ref["out"], what)
    R.check("node_objective dlogits", dl, ref["dlogits"], what)
    assert counters == ref["counters"], f"{what}: counters {counters} against {ref['counters']}"


def _applies(mut, nlab, eps, gamma, gs):
    if nlab < 255:                     # one random row: a mutant may hide inside the bound there
        return False
    return {"f_detached": gamma > 0, "smoothing_eps": eps > 0, "focal_on_smoothing": eps > 0 and gamma > 0,
            "no_grad_scale": gs != 1.0, "weights_swapped": True}[mut]


def test_emulation_accepted_and_mutants_rejected():
    hits = {}
    for nlab, dtype, fp16_loss, (eps, gamma), gs in R.matrix():
        l, rows, y = R.inputs(nlab, dtype)
        what = f"nlab{nlab} {dtype} fp16_loss{fp16_loss} eps{eps} gamma{gamma} gs{gs:.3f}"
        nan0 = torch.full(l.shape, float("nan"), dtype=dtype)
        ref = R.reference_node_objective(l, rows, y, WN, WP, eps, gamma, fp16_loss, gs)
        check_all(emulate(l, rows, y, WN, WP, fp16_loss, eps, gamma, gs, nan0), ref, what)
        for mut in MUTANTS:
            if not _applies(mut, nlab, eps, gamma, gs):
                continue
            hits[mut] = hits.get(mut, 0) + 1
            got = emulate(l, rows, y, WN, WP, fp16_loss, eps, gamma, gs, nan0, mutant=mut)
            assert rejected(lambda: check_all(got, ref, what)), f"{what}: mutant {mut} accepted"
    assert set(hits) == set(MUTANTS) and min(hits.values()) >= 8, hits


def test_denormal_floor_and_the_unmeasured_range():
    """(30, -30) with the target on the large logit: lp_o = -60, f = expf(-60 gamma) underflows at gamma = 2 and 5 — the
    reference's f carries the 2^-149 floor and the kernel's 0 is inside it; an argument in [-104, -64) is refused."""
    l = torch.tensor([[30.0, -30.0]])
    rows, y = torch.tensor([0], dtype=torch.int32), torch.tensor([0], dtype=torch.int32)
    for gamma in (2.0, 5.0):
        ref = R.reference_node_objective(l, rows, y, WN, WP, 0.0, gamma)
        assert 0.0 <= float(ref["out"][0][0]) < R.DENORM
        check_all(emulate(l, rows, y, WN, WP, 0, 0.0, gamma, 1.0, torch.zeros(1, 2)), ref, f"gamma {gamma}")
    with pytest.raises(AssertionError, match="outside the range EXPF_REL was measured on"):
        R.reference_node_objective(l, rows, y, WN, WP, 0.0, 1.5)          # -90


# ------------------------------------------------------------------------------------------------ the Python layers
def test_launcher_knows_both_flags():
    from multimodaldiscussiontransformer_amd import train
    from multimodaldiscussiontransformer_amd.criterions.hatespeech_loss import GraphPredictionNodeCrossEntropyConfig as Cfg
    assert Cfg().label_smoothing == 0.0 and Cfg().focal_gamma == 0.0
    a = train.build_parser().parse_args(["--label-smoothing", "0.1", "--focal-gamma", "2"])
    assert a.label_smoothing == 0.1 and a.focal_gamma == 2.0
    b = train.build_parser().parse_args([])
    assert b.label_smoothing is None and b.focal_gamma is None      # not given: main() keeps them out of the checkpoint cfg
    assert b.positive_weight == 1.0 and b.negative_weight == 1.0


def test_criterion_refuses_values_outside_the_ranges():
    from multimodaldiscussiontransformer_amd.criterions import GraphPredictionNodeCrossEntropy as Crit
    for kw in (dict(label_smoothing=1.0), dict(label_smoothing=-0.1), dict(label_smoothing=float("nan")), dict(focal_gamma=-1.0),
               dict(focal_gamma=float("inf")), dict(focal_gamma=float("nan"))):
        with pytest.raises(ValueError):
            Crit(None, 1.5, 1.0, **kw)
    c = Crit(None, 1.5, 1.0, True, label_smoothing=0.1, focal_gamma=2.0)
    assert (c.positive_weight, c.negative_weight, c.label_smoothing, c.focal_gamma) == (1.5, 1.0, 0.1, 2.0)
    built = Crit.build_criterion(types.SimpleNamespace(positive_weight=1.5, negative_weight=1.0, label_smoothing=0.25, focal_gamma=0.5), None)
    assert (built.label_smoothing, built.focal_gamma) == (0.25, 0.5)
    assert Crit.build_criterion(types.SimpleNamespace(positive_weight=1.5), None).label_smoothing == 0.0


class _Stub(torch.nn.Module):
    def __init__(self, logits):
        super().__init__()
        self.logits = torch.nn.Parameter(logits)

    def forward(self, batched_data=None, **kw):
        return self.logits, None


def _patched(monkeypatch, calls):
    from multimodaldiscussiontransformer_amd import ops
    from multimodaldiscussiontransformer_amd.criterions import hatespeech_loss as H

    def node_ce(logits, rows, targets, w_neg, w_pos, *, fp16_loss=True, grad_scale=1.0, want_grad=True):
        calls.append(("node_ce", w_neg, w_pos, fp16_loss))
        return torch.tensor([3.0]), torch.tensor([4, 1, 2, 3], dtype=torch.int32), torch.full_like(logits, 0.5)

    def node_objective(logits, rows, targets, w_neg, w_pos, *, label_smoothing=0.0, focal_gamma=0.0, fp16_loss=True, grad_scale=1.0,
                       want_grad=True):
        calls.append(("node_objective", w_neg, w_pos, fp16_loss, label_smoothing, focal_gamma))
        return torch.tensor([5.0, 7.0]), torch.tensor([4, 1, 2, 3], dtype=torch.int32), torch.full_like(logits, 0.25)

    monkeypatch.setattr(ops, "node_ce", node_ce)
    monkeypatch.setattr(ops, "node_objective", node_objective)
    pb = types.SimpleNamespace(label_rows=torch.tensor([0, 2], dtype=torch.int32), targets=torch.tensor([0, 1], dtype=torch.int32), n_labels=2)
    monkeypatch.setattr(H, "packed_from_batched_data", lambda bd: pb)
    return {"net_input": {"batched_data": {"x": torch.zeros(1, 3, 1)}}}


def test_criterion_with_defaults_calls_node_ce(monkeypatch):
    from multimodaldiscussiontransformer_amd.criterions import GraphPredictionNodeCrossEntropy as Crit
    calls = []
    sample = _patched(monkeypatch, calls)
    model = _Stub(torch.zeros(3, 2))
    loss, n, log = Crit(None, 1.5, 1.0, False)(model, sample)
    assert calls == [("node_ce", 1.0, 1.5, False)]
    assert list(log) == ["loss", "sample_size", "nsentences", "ntokens", "ncorrect", "num_positive_correct", "total_positive",
                         "num_pred_positive"]
    assert float(loss.detach()) == 3.0 and n == 2
    (2.0 * loss).backward()
    assert torch.equal(model.logits.grad, torch.full((3, 2), 1.0))


def test_criterion_with_the_objective_calls_node_objective(monkeypatch):
    from multimodaldiscussiontransformer_amd.criterions import GraphPredictionNodeCrossEntropy as Crit
    for kw in (dict(label_smoothing=0.1), dict(focal_gamma=2.0), dict(label_smoothing=0.1, focal_gamma=2.0)):
        calls = []
        sample = _patched(monkeypatch, calls)
        model = _Stub(torch.zeros(3, 2))
        crit = Crit(None, 1.5, 1.0, **kw)
        loss, n, log = crit(model, sample)
        assert calls == [("node_objective", 1.0, 1.5, True, kw.get("label_smoothing", 0.0), kw.get("focal_gamma", 0.0))]
        assert list(log)[-1] == "nll_loss" and len(log) == 9
        assert float(loss.detach()) == 5.0 and float(log["nll_loss"]) == 7.0 and float(log["loss"]) == 5.0 and n == 2
        assert not log["nll_loss"].requires_grad and loss.requires_grad
        (2.0 * loss).backward()
        assert torch.equal(model.logits.grad, torch.full((3, 2), 0.5))          # dlogits * gloss
        with pytest.raises(NotImplementedError):
            crit(model, sample, reduce=False)


def test_compute_metrics_with_and_without_nll_loss():
    from multimodaldiscussiontransformer_amd.criterions import GraphPredictionNodeCrossEntropy as Crit
    base = dict(sample_size=4, ncorrect=3, num_positive_correct=1, total_positive=2, num_pred_positive=1)
    plain = Crit.compute_metrics([dict(base, loss=2.0), dict(base, loss=6.0)])
    assert list(plain) == ["loss", "accuracy", "recall", "precision", "f1"] and plain["loss"] == 1.0
    m = Crit.compute_metrics([dict(base, loss=2.0, nll_loss=4.0), dict(base, loss=6.0, nll_loss=8.0)])
    assert list(m) == ["loss", "nll_loss", "accuracy", "recall", "precision", "f1"]
    assert m["loss"] == 1.0 and m["nll_loss"] == 1.5 and {k: m[k] for k in plain} == plain
    assert Crit.compute_metrics([dict(loss=0.0, nll_loss=0.0, sample_size=0)])["nll_loss"] == 0.0
    Crit.reduce_metrics([dict(base, loss=2.0, nll_loss=4.0)])
    assert Crit.last_metrics["nll_loss"] == 1.0
