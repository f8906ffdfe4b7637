"""mdt_node_objective (csrc/node_objective.hip) on the GPU against tests/node_objective_reference.py, whose bounds
tests/test_node_objective_reference_cpu.py proves at the same cases, and the criterion above it.

The C ABI is called directly, every output carved out of a sentinel-filled allocation (tests/test_loss_optim_gpu.py Carve).  The
kernel walks the labelled rows with one 256-thread workgroup, thread t taking rows t, t + 256, ...: nlab 255 / 256 / 257 are the
boundaries of that walk, 1031 a ragged multi-chunk case, 0 and 1 the degenerate ones; M = nlab + 5 leaves unlabelled rows.  For
fp16_loss = 1 the judge of the counters is mdt_node_ce on the same logits (equal integers); for fp16_loss = 0 the reference's as
well."""
import math

import pytest
import torch

import tests.node_objective_reference as R
import tests.test_loss_optim_gpu as G
from multimodaldiscussiontransformer_amd import _lib as L
from tests.node_objective_reference import bf16, f32

pytestmark = pytest.mark.gpu

DEV = "cuda"
WN, WP = R.WEIGHTS


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available(), "GPU tests need a device"


def _bits(t):
    return t.view(torch.int32 if t.dtype == f32 else torch.int16)


def _objective(l, rows, y, fp16_loss, eps, gamma, gs, with_grad=True):
    M, nlab = l.shape[0], int(y.numel())
    ld = l.to(DEV)
    rd = rows.to(DEV) if nlab else None
    yd = y.to(DEV) if nlab else None
    out, cnt, dl = G.Carve([2], f32), G.Carve([4], torch.int32), G.Carve([M * 2], l.dtype)
    dl.view(0).fill_(float("nan"))
    rc = L.lib.mdt_node_objective(L.stream(), 0 if l.dtype == f32 else 1, M, nlab, L.ptr(ld), L.ptr(rd), L.ptr(yd), WN, WP, fp16_loss,
                                  eps, gamma, gs, L.ptr(out.view(0)), L.ptr(cnt.view(0)), L.ptr(dl.view(0)) if with_grad else None)
    torch.cuda.synchronize()
    assert rc == 0, G.status(rc)
    assert out.untouched() and cnt.untouched() and dl.untouched(), "a sentinel around an output was overwritten"
    if not with_grad:
        assert bool(torch.isnan(dl.view(0).float()).all()), "dlogits = NULL: the buffer that was not passed was written"
    return out.view(0).cpu(), cnt.view(0).cpu().tolist(), dl.view(0).cpu().view(M, 2) if with_grad else None


@pytest.mark.parametrize("dtype", [f32, bf16], ids=["f32", "bf16"])
@pytest.mark.parametrize("nlab", R.NLAB)
def test_kernel_against_the_reference(nlab, dtype):
    cases = [c for c in R.matrix() if c[0] == nlab and c[1] == dtype]
    assert len(cases) == 2 * len(R.SETTINGS)
    l, rows, y = R.inputs(nlab, dtype)
    mask = torch.ones(l.shape[0], dtype=torch.bool)
    mask[rows.long()] = False
    assert int(mask.sum()) == 5
    for _, _, fp16_loss, (eps, gamma), gs in cases:
        what = f"nlab{nlab} {dtype} fp16_loss{fp16_loss} eps{eps} gamma{gamma} gs{gs:.3f}"
        ref = R.reference_node_objective(l, rows, y, WN, WP, eps, gamma, fp16_loss, gs)
        out, c, dl = _objective(l, rows, y, fp16_loss, eps, gamma, gs)
        print(f"{what}: out {out.tolist()} ref {ref['out'][0].tolist()} bound {ref['out'][1].tolist()}")
        R.check("node_objective out", out, ref["out"], what)
        R.check("node_objective dlogits", dl, ref["dlogits"], what)
        assert bool((_bits(dl)[mask] == 0).all()), f"{what}: d logits of an unlabelled row is not 0"
        _, c_ce, _ = G._node_ce(l, rows, y, WN, WP, fp16_loss, gs, with_grad=False)
        assert c == c_ce, f"{what}: counters {c}, mdt_node_ce's {c_ce}"
        if not fp16_loss:
            assert c == ref["counters"], f"{what}: counters {c} against {ref['counters']}"
        out2, c2, dl2 = _objective(l, rows, y, fp16_loss, eps, gamma, gs)
        assert torch.equal(_bits(out), _bits(out2)) and c == c2 and torch.equal(_bits(dl), _bits(dl2)), f"{what}: two calls differ"
        out3, c3, _ = _objective(l, rows, y, fp16_loss, eps, gamma, gs, with_grad=False)
        assert torch.equal(_bits(out), _bits(out3)) and c == c3, f"{what}: dlogits = NULL changes the result"
        if nlab == 0:
            assert out.tolist() == [0.0, 0.0] and c == [0, 0, 0, 0]


def test_refusals_write_nothing():
    l = torch.zeros(4, 2, device=DEV)
    rows = torch.tensor([0, 2], dtype=torch.int32, device=DEV)
    yd = torch.zeros(2, dtype=torch.int32, device=DEV)
    nan, inf = float("nan"), float("inf")
    good = dict(dtype=0, logits=l, rows=rows, targets=yd, eps=0.1, gamma=2.0, out=True, cnt=True)
    bad = [("null logits", dict(logits=None)), ("null rows", dict(rows=None)), ("null targets", dict(targets=None)),
           ("null out", dict(out=False)), ("null counters", dict(cnt=False)), ("eps 1", dict(eps=1.0)), ("eps < 0", dict(eps=-0.1)),
           ("eps nan", dict(eps=nan)), ("eps inf", dict(eps=inf)), ("gamma < 0", dict(gamma=-1.0)), ("gamma inf", dict(gamma=inf)),
           ("gamma nan", dict(gamma=nan)), ("dtype 2", dict(dtype=2)), ("dtype -1", dict(dtype=-1))]
    for what, change in bad:
        a = dict(good, **change)
        out, cnt, dl = G.Carve([2], f32), G.Carve([4], torch.int32), G.Carve([8], f32)
        rc = L.lib.mdt_node_objective(L.stream(), a["dtype"], 4, 2, L.ptr(a["logits"]), L.ptr(a["rows"]), L.ptr(a["targets"]), 1.0, 1.5, 1,
                                      a["eps"], a["gamma"], 1.0, L.ptr(out.view(0)) if a["out"] else None,
                                      L.ptr(cnt.view(0)) if a["cnt"] else None, L.ptr(dl.view(0)))
        msg = L.lib.mdt_last_error_string().decode()
        torch.cuda.synchronize()
        assert rc != 0, what
        assert "node_objective" in msg, (what, msg)
        for c in (out, cnt, dl):
            assert bool((c.buf.view(c.itype) == c.bits).all()), f"{what}: an output was written by a refused call"
    # the same operands unchanged are accepted
    out, cnt, dl = G.Carve([2], f32), G.Carve([4], torch.int32), G.Carve([8], f32)
    rc = L.lib.mdt_node_objective(L.stream(), 0, 4, 2, L.ptr(l), L.ptr(rows), L.ptr(yd), 1.0, 1.5, 1, 0.1, 2.0, 1.0, L.ptr(out.view(0)),
                                  L.ptr(cnt.view(0)), L.ptr(dl.view(0)))
    torch.cuda.synchronize()
    assert rc == 0, G.status(rc)
    assert cnt.view(0).cpu().tolist() == [2, 0, 0, 0] and out.untouched() and cnt.untouched() and dl.untouched()


# ------------------------------------------------------------------------------------------------ the criterion
class _Stub(torch.nn.Module):
    def __init__(self, logits):
        super().__init__()
        self.logits = torch.nn.Parameter(logits)

    def forward(self, batched_data=None, **kw):
        return self.logits, None


@pytest.fixture(scope="module")
def tiny():
    """The Tiny model without dropout, by tests/test_deterministic_step_gpu.py's builder: (model, sample, its logits)."""
    from tests.test_deterministic_step_gpu import _model
    _, _, model, _, sample = _model(torch.float32, dropout=0.0)
    with torch.no_grad():
        logits, _ = model(**sample["net_input"])
    return model, sample, logits.detach().clone()


def _crit(**kw):
    from multimodaldiscussiontransformer_amd.criterions import GraphPredictionNodeCrossEntropy
    return GraphPredictionNodeCrossEntropy(None, WP, WN, **kw)


@pytest.mark.parametrize("fp16_loss", [False, True])
def test_criterion_on_fixed_logits(tiny, fp16_loss):
    """A stub model returning fixed logits: loss and nll_loss are out[0] and out[1], loss.backward() delivers dlogits * gloss, and
    with fp16_loss = False nll_loss is the default criterion's loss on the same logits within the reference's bound."""
    from multimodaldiscussiontransformer_amd import ops
    from multimodaldiscussiontransformer_amd.data.packer import packed_from_batched_data
    _, sample, logits = tiny
    pb = packed_from_batched_data(sample["net_input"]["batched_data"])
    assert pb.n_labels > 0
    gen = torch.Generator().manual_seed(R.SEED)
    fixed = (torch.rand(logits.shape, generator=gen) * 8 - 4).to(DEV)
    eps, gamma = 0.1, 2.0
    stub = _Stub(fixed.clone())
    loss, n, log = _crit(fp16_loss=fp16_loss, label_smoothing=eps, focal_gamma=gamma)(stub, sample)
    assert n == pb.n_labels and list(log)[-1] == "nll_loss" and log["nll_loss"].dim() == 0 and loss.dim() == 0
    out, counters, dl = ops.node_objective(fixed, pb.label_rows, pb.targets, WN, WP, label_smoothing=eps, focal_gamma=gamma,
                                           fp16_loss=fp16_loss)
    assert torch.equal(loss.detach(), out[0]) and torch.equal(log["nll_loss"], out[1]) and torch.equal(log["loss"], out[0])
    assert [int(log[k]) for k in ("ncorrect", "num_positive_correct", "total_positive", "num_pred_positive")] == counters.tolist()
    (loss * 0.375).backward()
    assert torch.equal(stub.logits.grad, dl * 0.375) and float(dl.abs().max()) > 0
    ref = R.reference_node_objective(fixed.cpu(), pb.label_rows.cpu(), pb.targets.cpu(), WN, WP, eps, gamma, int(fp16_loss))
    R.check("criterion out", out.cpu(), ref["out"], "stub")
    R.check("criterion dlogits", dl.cpu(), ref["dlogits"], "stub")
    # the default criterion on the same logits: ops.node_ce, today's keys
    plain_loss, _, plain_log = _crit(fp16_loss=fp16_loss)(_Stub(fixed.clone()), sample)
    assert "nll_loss" not in plain_log and len(plain_log) == 8
    if not fp16_loss:
        R.check("nll_loss against the default loss", plain_loss.detach().view(1).cpu(), (ref["out"][0][1:2], ref["out"][1][1:2]), "stub")
        R.check("nll_loss", log["nll_loss"].view(1).cpu(), (ref["out"][0][1:2], ref["out"][1][1:2]), "stub")


def test_criterion_on_the_tiny_model(tiny):
    from multimodaldiscussiontransformer_amd.data.packer import packed_from_batched_data
    model, sample, _ = tiny
    pb = packed_from_batched_data(sample["net_input"]["batched_data"])
    eps, gamma = 0.25, 0.5

    class Record(torch.nn.Module):          # the logits the criterion saw (each reference is of the forward it judges)
        def forward(self, **kw):
            out = model(**kw)
            self.seen = out[0].detach().clone()
            return out

    rec = Record()
    model.zero_main_grads()
    loss, n, log = _crit(fp16_loss=False, label_smoothing=eps, focal_gamma=gamma)(rec, sample)
    ref = R.reference_node_objective(rec.seen.cpu(), pb.label_rows.cpu(), pb.targets.cpu(), WN, WP, eps, gamma, 0)
    got = torch.stack([loss.detach(), log["nll_loss"]]).cpu()
    R.check("criterion out (Tiny)", got, ref["out"], "tiny")
    with torch.no_grad():
        plain_loss, _, plain_log = _crit(fp16_loss=False)(rec, sample)
    ref0 = R.reference_node_objective(rec.seen.cpu(), pb.label_rows.cpu(), pb.targets.cpu(), WN, WP, 0.0, 0.0, 0)
    R.check("nll_loss against the default loss (Tiny)", plain_loss.view(1).cpu(), (ref0["out"][0][1:2], ref0["out"][1][1:2]), "tiny")
    assert [int(log[k]) for k in list(plain_log)[4:]] == [int(plain_log[k]) for k in list(plain_log)[4:]] == ref0["counters"]
    loss.backward()
    torch.cuda.synchronize()
    g = model.main_grad_flat
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 and math.isfinite(float(loss.detach()))
