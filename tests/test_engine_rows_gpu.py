"""The engine's row helpers on a bare Tape, forward and adjoint: expand_sequences, expand_rows, take_rows, rows_mix,
scatter_rows, graph_node_features, classifier_head and Tape.add_grad (multimodaldiscussiontransformer_amd/engine.py).

The reference is the same row maps written with torch indexing on fp64 CPU leaves and autograd.  Forward results and
adjoints that only copy must be bit-equal to it; adjoints that add are checked within the bounds of
tests/rowops_reference.py from the operands the kernel read; parameter gradients (the learned front rows, the degree
tables, the graph token), fp32 sums over sequences, are compared with the fp64 sums under the any-order bound, which
must not be vacuous.  classifier_head records what its GEMMs and tanh kernels read and wrote: every GEMM output is
checked with tests/gemm_reference.py, every tanh with the tanh references, and the row traffic around them exactly.

Shapes: D = 256 in fp32 and 520 in bf16 (a second sweep of the 64-lane column loop), five sequences of 3, 1, 4, 2 and 5
tokens, nb = 4 bottleneck rows.  Every upstream gradient differs from row to row, so a row permutation in an adjoint
changes the result."""
import pytest
import torch

import tests.gemm_reference as GR
import tests.rowops_reference as RR
from tests.rowops_reference import bf16, f32

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEED = 2468
LENS = (3, 1, 4, 2, 5)
NB = 4
CASES = [(f32, 256), (bf16, 520)]
IDS = ["f32-D256", "bf16-D520"]


@pytest.fixture(scope="module")
def E():
    from multimodaldiscussiontransformer_amd import engine
    assert torch.cuda.is_available(), "GPU tests need a device"
    return engine


def val(rows, D, k, dtype, scale=1.0):
    return RR.values((rows, D), SEED + 31 * k, scale, dtype)


def dev(t):
    return t.to(DEV).contiguous()


def leaf(t):
    return t.double().clone().requires_grad_()


def same(got, want64, what):
    """Bit equality with the fp64 reference rounded to the stored type (the reference value is representable: a copy)."""
    want = want64.detach().to(got.dtype)
    assert want.double().equal(want64.detach()), f"{what}: the reference is not representable, this is no copy"
    g = got.cpu()
    assert g.shape == want.shape and bool((g == want).all()), f"{what}: {int((g != want).sum())} elements differ from the copy"


def check_sum(name, got, terms64, dterms=None, what=""):
    """An fp32 parameter gradient against Σ over dim 0 of terms64 [n, ...] (each term known to within dterms)."""
    d = torch.zeros_like(terms64) if dterms is None else dterms
    v = terms64.sum(0)
    dl = RR._sum_err(terms64, d, 0)
    RR.check(name, got.cpu().view(v.shape), (v, dl, dl == 0), what=what, dtype=f32, nonvacuous=True)


def ragged_geometry():
    """pre2fus / bn_rows_all / bn0 / cls of the ragged text layout for LENS, as the encoder builds them."""
    lens = torch.tensor(LENS)
    M = len(LENS)
    off = torch.zeros(M + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(lens, 0)
    comment = torch.repeat_interleave(torch.arange(M), lens)
    rows_pre = int(off[-1])
    pre2fus = torch.arange(rows_pre) + (comment + 1) * NB
    bn0 = off[:M] + torch.arange(M) * NB
    bn_all = (bn0[:, None] + torch.arange(NB)[None]).reshape(-1)
    return dict(M=M, rows_pre=rows_pre, rows_fus=rows_pre + M * NB, pre2fus=pre2fus, bn0=bn0, cls=bn0 + NB, bn_all=bn_all)


def i32(t):
    return t.to(torch.int32).to(DEV).contiguous()


# ------------------------------------------------------------------------------------------------ expand_sequences
@pytest.mark.parametrize("with_front", (True, False), ids=["front", "zeros"])
@pytest.mark.parametrize("dtype,D", CASES, ids=IDS)
def test_expand_sequences(E, dtype, D, with_front):
    nseq, s_in, S = 5, 3, 3 + NB
    x, front, G = val(nseq * s_in, D, 1, dtype), val(NB, D, 2, dtype), val(nseq * S, D, 3, dtype)
    tape = E.Tape()
    xv = E.Var(dev(x))
    fp = torch.nn.Parameter(dev(front)) if with_front else None
    o = E.expand_sequences(tape, xv, nseq, s_in, NB, fp)
    X, F = leaf(x), leaf(front)
    head = F[None].expand(nseq, NB, D) if with_front else torch.zeros(nseq, NB, D, dtype=torch.float64)
    ref = torch.cat([head, X.view(nseq, s_in, D)], 1).reshape(nseq * S, D)
    same(o.data, ref, "expand_sequences forward")
    o.grad = dev(G)
    tape.backward()
    (ref * G.double()).sum().backward()
    same(xv.grad, X.grad, "expand_sequences dx")
    if with_front:
        terms = G.double().view(nseq, S, D)[:, :NB]
        assert torch.allclose(terms.sum(0), F.grad, rtol=1e-13, atol=1e-13), "the terms summed here are not autograd's"
        check_sum("front grad", tape.tmp_grads[id(fp)], terms, what="expand_sequences front")


# ------------------------------------------------------------------------------------------------ expand_rows + take_rows
@pytest.mark.parametrize("dtype,D", CASES, ids=IDS)
def test_expand_rows_then_take_rows(E, dtype, D):
    """The ragged text layout: body rows to pre2fus, learned rows to bn_rows_all, then the bottleneck rows read back.
    Backward: take_rows accumulates its gradient onto a non-zero gradient of the expanded buffer (one add per element),
    expand_rows gathers dx from it and sums the front rows over the comments."""
    g = ragged_geometry()
    M, rows_pre, rows_fus = g["M"], g["rows_pre"], g["rows_fus"]
    x, front = val(rows_pre, D, 1, dtype), val(NB, D, 2, dtype)
    G0, G1 = val(rows_fus, D, 3, dtype), val(M * NB, D, 4, dtype)
    tape = E.Tape()
    xv, fp = E.Var(dev(x)), torch.nn.Parameter(dev(front))
    pre2fus, bn_all = i32(g["pre2fus"]), i32(g["bn_all"])
    o = E.expand_rows(tape, xv, rows_fus, pre2fus, bn_all, NB, fp)
    bn = E.take_rows(tape, o, M * NB, s_idx=bn_all)
    X, F = leaf(x), leaf(front)
    ref = torch.zeros(rows_fus, D, dtype=torch.float64)
    ref = ref.index_copy(0, g["pre2fus"], X).index_copy(0, g["bn_all"], F.repeat(M, 1))
    ref_bn = ref[g["bn_all"]]
    same(o.data, ref, "expand_rows forward")
    same(bn.data, ref_bn, "take_rows forward")
    o.grad, bn.grad = dev(G0), dev(G1)
    stored = o.grad                                              # take_rows adds into this very buffer
    tape.backward()
    ((ref * G0.double()).sum() + (ref_bn * G1.double()).sum()).backward()
    acc = RR.reference_row_axpby(G0, M * NB, d=(g["bn_all"], 1, 1, 0), a=G1, accumulate=True)
    RR.check("take_rows adjoint", stored.cpu(), acc, what="g[bn_rows_all] += g_bn")
    same(xv.grad, X.grad, "expand_rows dx")                      # the body rows were not added to: G0 at pre2fus
    bound = RR.bound(acc[0], acc[1], dtype)[g["bn_all"]].view(M, NB * D)
    terms = (G0.double()[g["bn_all"]] + G1.double()).view(M, NB * D)
    assert torch.allclose(terms.sum(0).view(NB, D), F.grad, rtol=1e-13, atol=1e-13), "the terms summed here are not autograd's"
    check_sum("front grad", tape.tmp_grads[id(fp)], terms, bound, what="expand_rows front")
    check_sum("front grad", tape.tmp_grads[id(fp)], stored.cpu().double()[g["bn_all"]].view(M, NB * D), what="expand_rows front, stored terms")


# ------------------------------------------------------------------------------------------------ take_rows / scatter_rows
@pytest.mark.parametrize("dtype,D", CASES, ids=IDS)
def test_take_rows_with_a_two_level_map(E, dtype, D):
    """s_map = (inner 3, stride 7, offset 4): rows 4, 5, 6, 11, 12, 13, ...; the adjoint adds onto a non-zero gradient."""
    n, s_map = 15, (3, 7, 4)
    src, G, Gs0 = val(5 * 7, D, 1, dtype), val(n, D, 2, dtype), val(5 * 7, D, 3, dtype)
    rows = RR.row_index(torch.arange(n), None, *s_map)
    tape = E.Tape()
    sv = E.Var(dev(src))
    o = E.take_rows(tape, sv, n, s_map=s_map)
    S = leaf(src)
    ref = S[rows]
    same(o.data, ref, "take_rows forward")
    o.grad, sv.grad = dev(G), dev(Gs0)
    tape.backward()
    RR.check("take_rows adjoint", sv.grad.cpu(), RR.reference_row_axpby(Gs0, n, d=(None,) + s_map, a=G, accumulate=True), what="take_rows(s_map) adjoint")
    ((ref * G.double()).sum() + (S * Gs0.double()).sum()).backward()
    RR.assert_within(sv.grad.cpu(), S.grad, RR.bound(S.grad, RR.U32 * S.grad.abs(), dtype), what="take_rows adjoint against autograd", dtype=dtype)
    # a zero start: the adjoint is a copy
    tape = E.Tape()
    sv = E.Var(dev(src))
    o = E.take_rows(tape, sv, n, s_map=s_map)
    o.grad = dev(G)
    tape.backward()
    same(sv.grad, torch.zeros(5 * 7, D, dtype=torch.float64).index_copy(0, rows, G.double()), "take_rows adjoint from zero")


@pytest.mark.parametrize("dtype,D", CASES, ids=IDS)
def test_scatter_rows(E, dtype, D):
    """The ragged rows back into the padded [M L, D] shape: out[comment L + pos] = text[pre2fus]."""
    g = ragged_geometry()
    Lq = max(LENS)
    comment = torch.repeat_interleave(torch.arange(g["M"]), torch.tensor(LENS))
    pos = torch.cat([torch.arange(n) for n in LENS])
    dense = comment * Lq + pos
    src, G = val(g["rows_fus"], D, 1, dtype), val(g["M"] * Lq, D, 2, dtype)
    tape = E.Tape()
    sv = E.Var(dev(src))
    o = E.scatter_rows(tape, sv, g["M"] * Lq, i32(dense), i32(g["pre2fus"]))
    S = leaf(src)
    ref = torch.zeros(g["M"] * Lq, D, dtype=torch.float64).index_copy(0, dense, S[g["pre2fus"]])
    same(o.data, ref, "scatter_rows forward")
    o.grad = dev(G)
    tape.backward()
    (ref * G.double()).sum().backward()
    same(sv.grad, S.grad, "scatter_rows adjoint")


# ------------------------------------------------------------------------------------------------ rows_mix
@pytest.mark.parametrize("dtype,D", CASES, ids=IDS)
def test_rows_mix_assignment_with_index_vectors(E, dtype, D):
    """(alpha, beta) = (1, 0): dst[d_idx] = src[s_idx] in place; adjoint g_src[s_idx] += g_dst[d_idx], g_dst[d_idx] = 0."""
    n, Rd, Rs = 6, 11, 9
    d_idx, s_idx = RR._distinct(n, Rd, SEED, "cpu").long(), RR._distinct(n, Rs, SEED + 1, "cpu").long()
    dst, src, Gd, Gs0 = val(Rd, D, 1, dtype), val(Rs, D, 2, dtype), val(Rd, D, 3, dtype), val(Rs, D, 4, dtype)
    tape = E.Tape()
    dv, sv = E.Var(dev(dst)), E.Var(dev(src))
    E.rows_mix(tape, dv, sv, n, alpha=1.0, beta=0.0, d_idx=i32(d_idx), s_idx=i32(s_idx))
    Dl, Sl = leaf(dst), leaf(src)
    ref = Dl.index_copy(0, d_idx, Sl[s_idx])
    same(dv.data, ref, "rows_mix(1, 0) forward")
    dv.grad, sv.grad = dev(Gd), dev(Gs0)
    tape.backward()
    ((ref * Gd.double()).sum() + (Sl * Gs0.double()).sum()).backward()
    same(dv.grad, Dl.grad, "rows_mix(1, 0) g_dst")
    RR.check("rows_mix adjoint", sv.grad.cpu(), RR.reference_row_axpby(Gs0, n, d=(s_idx, 1, 1, 0), a=Gd, am=(d_idx, 1, 1, 0), accumulate=True),
             what="g_src[s_idx] += g_dst[d_idx]")
    RR.assert_within(sv.grad.cpu(), Sl.grad, RR.bound(Sl.grad, RR.U32 * Sl.grad.abs(), dtype), what="rows_mix g_src against autograd", dtype=dtype)


@pytest.mark.parametrize("dtype,D", CASES, ids=IDS)
def test_rows_mix_assignment_with_a_destination_map(E, dtype, D):
    """(1, 0) with d_map = (nb, S, 0): the nb front rows of every sequence take consecutive source rows."""
    nseq, S = 5, NB + 3
    n = nseq * NB
    d_map = (NB, S, 0)
    rows = RR.row_index(torch.arange(n), None, *d_map)
    dst, src, Gd = val(nseq * S, D, 1, dtype), val(n, D, 2, dtype), val(nseq * S, D, 3, dtype)
    tape = E.Tape()
    dv, sv = E.Var(dev(dst)), E.Var(dev(src))
    E.rows_mix(tape, dv, sv, n, alpha=1.0, beta=0.0, d_map=d_map)
    Dl, Sl = leaf(dst), leaf(src)
    ref = Dl.index_copy(0, rows, Sl)
    same(dv.data, ref, "rows_mix(d_map) forward")
    dv.grad = dev(Gd)
    tape.backward()
    (ref * Gd.double()).sum().backward()
    same(dv.grad, Dl.grad, "rows_mix(d_map) g_dst")
    same(sv.grad, Sl.grad, "rows_mix(d_map) g_src")


@pytest.mark.parametrize("dtype,D", CASES, ids=IDS)
def test_rows_mix_average(E, dtype, D):
    """(0.5, 0.5) with d_idx only: dst[d_idx[r]] = 0.5 src[r] + 0.5 dst[d_idx[r]], b aliasing dst in place; the adjoint
    scales g_dst in place (a aliasing dst) and adds 0.5 g_dst[d_idx] onto a non-zero g_src."""
    n, Rd = 6, 11
    d_idx = RR._distinct(n, Rd, SEED, "cpu").long()
    dst, src, Gd, Gs0 = val(Rd, D, 1, dtype), val(n, D, 2, dtype), val(Rd, D, 3, dtype), val(n, D, 4, dtype)
    tape = E.Tape()
    dv, sv = E.Var(dev(dst)), E.Var(dev(src))
    E.rows_mix(tape, dv, sv, n, alpha=0.5, beta=0.5, d_idx=i32(d_idx))
    RR.check("rows_mix forward", dv.data.cpu(), RR.reference_row_axpby(dst, n, d=(d_idx, 1, 1, 0), a=src, alpha=0.5, b=dst, bm=(d_idx, 1, 1, 0), beta=0.5),
             what="rows_mix(0.5, 0.5) forward")
    Dl, Sl = leaf(dst), leaf(src)
    ref = Dl.index_copy(0, d_idx, 0.5 * Sl + 0.5 * Dl[d_idx])
    dv.grad, sv.grad = dev(Gd), dev(Gs0)
    tape.backward()
    ((ref * Gd.double()).sum() + (Sl * Gs0.double()).sum()).backward()
    same(dv.grad, Dl.grad, "rows_mix(0.5, 0.5) g_dst")            # halving is exact
    RR.check("rows_mix adjoint", sv.grad.cpu(), RR.reference_row_axpby(Gs0, n, a=Gd, am=(d_idx, 1, 1, 0), alpha=0.5, accumulate=True),
             what="g_src += 0.5 g_dst[d_idx]")
    RR.assert_within(sv.grad.cpu(), Sl.grad, RR.bound(Sl.grad, RR.U32 * Sl.grad.abs(), dtype), what="rows_mix g_src against autograd", dtype=dtype)


# ------------------------------------------------------------------------------------------------ graph node features
@pytest.mark.parametrize("dtype,D", CASES, ids=IDS)
def test_graph_node_features(E, dtype, D):
    """Two trees of 3 and 1 comments on a [2, 4] grid (two padding nodes): forward within the two-add bound, the text
    gradient a copy onto the comments' bottleneck rows, the degree-table and graph-token gradients fp32 sums."""
    B, T = 2, 4
    N = T - 1
    g = ragged_geometry()
    node_row = torch.tensor([0, 1, 2, 3, -1, -1])                # comment of node (b, n); M = 4 of the 5 text comments
    M = 4
    deg_in = torch.tensor([1, 3, 3, 2, 0, 0])
    deg_out = torch.tensor([2, 2, 1, 5, 0, 0])
    text_row = torch.where(node_row >= 0, g["bn0"][node_row.clamp(min=0)], node_row)
    graph_row = torch.tensor([1, 2, 3, 5])                       # b T + 1 + n of comment m
    pad_row = torch.ones(B, T, dtype=torch.bool)
    pad_row[:, 0] = False
    in_sc = torch.full((B, T), -1, dtype=torch.int64)
    out_sc = torch.full((B, T), -1, dtype=torch.int64)
    in_sc[:, 1:] = torch.where(deg_in > 0, deg_in, torch.full_like(deg_in, -1)).view(B, N)
    out_sc[:, 1:] = torch.where(deg_out > 0, deg_out, torch.full_like(deg_out, -1)).view(B, N)
    text, in_emb, out_emb, token = val(g["rows_fus"], D, 1, dtype), val(6, D, 2, dtype), val(6, D, 3, dtype), val(1, D, 4, dtype)
    G = val(B * T, D, 5, dtype)
    tape = E.Tape()
    tv = E.Var(dev(text))
    pi, po, pk = (torch.nn.Parameter(dev(t)) for t in (in_emb, out_emb, token))
    o = E.graph_node_features(tape, tv, i32(text_row), i32(deg_in), i32(deg_out), pi, po, pk, B, T, i32(g["bn0"][:M]), i32(graph_row), M,
                              i32(in_sc.view(-1)), i32(out_sc.view(-1)))
    ref = RR.reference_node_feature(torch.zeros(B * T, D, dtype=dtype), text, text_row, deg_in, deg_out, in_emb, out_emb, token.view(-1), B, T)
    RR.check("graph_node_features forward", o.data.cpu(), ref, what="graph_node_features forward")
    o.grad = dev(G)
    tape.backward()
    Gd = G.double()
    want_text = torch.zeros(g["rows_fus"], D, dtype=torch.float64).index_copy(0, g["bn0"][:M], Gd[graph_row])
    same(tv.grad, want_text, "graph_node_features text gradient")
    node_g = Gd.view(B, T, D)[:, 1:].reshape(B * N, D)
    for name, p, deg in (("in_degree grad", pi, deg_in), ("out_degree grad", po, deg_out)):
        got = tape.tmp_grads[id(p)].cpu()
        assert float(got[0].abs().max()) == 0.0, f"{name}: the padding row of the table received a gradient"
        for k in range(1, 6):
            terms = node_g[deg == k]
            if terms.shape[0]:
                check_sum(name, got[k], terms, what=f"{name} row {k}")
            else:
                assert float(got[k].abs().max()) == 0.0
    check_sum("graph_token grad", tape.tmp_grads[id(pk)], Gd.view(B, T, D)[:, 0], what="graph token")


# ------------------------------------------------------------------------------------------------ classifier head
class Recorder:
    """Wraps ops.gemm / tanh_fwd / tanh_bwd: the real kernels run, what they read and wrote is kept (host copies)."""

    def __init__(self, ops, monkeypatch):
        self.gemms, self.tanh_f, self.tanh_b = [], [], []
        real_gemm, real_tf, real_tb = ops.gemm, ops.tanh_fwd, ops.tanh_bwd

        def gemm(a, b, **kw):
            c_old = kw["out"].detach().cpu().clone() if kw.get("out") is not None else None
            out = real_gemm(a, b, **kw)
            torch.cuda.synchronize()
            self.gemms.append(dict(a=a.cpu(), b=b.detach().cpu(), out=out.cpu().clone(), c_old=c_old,
                                   kw={k: (v.detach().cpu().clone() if torch.is_tensor(v) else v) for k, v in kw.items() if k != "out"}))
            return out

        def tanh_fwd(x):
            y = real_tf(x)
            self.tanh_f.append((x.cpu(), y.cpu()))
            return y

        def tanh_bwd(y, dy):
            dx = real_tb(y, dy)
            self.tanh_b.append((y.cpu(), dy.cpu(), dx.cpu()))
            return dx

        monkeypatch.setattr(ops, "gemm", gemm)
        monkeypatch.setattr(ops, "tanh_fwd", tanh_fwd)
        monkeypatch.setattr(ops, "tanh_bwd", tanh_bwd)


def check_gemm(rec, what, asum0=None):
    """One recorded ops.gemm call against tests/gemm_reference.py from the operands it read."""
    kw = rec["kw"]
    ep = int(kw.get("epilogue", 0)) | (GR.EPI_BIAS if kw.get("bias") is not None else 0) | (GR.EPI_ASUM if kw.get("asum") is not None else 0)
    ref = GR.reference(rec["a"], rec["b"], trans_a=kw.get("trans_a", False), trans_b=kw.get("trans_b", False), epilogue=ep, bias=kw.get("bias"),
                       c_old=rec["c_old"], colsum0=asum0, split_k=kw.get("split_k", 1))
    GR.check({"out": rec["out"]}, ref, {"out": rec["out"].dtype}, what=what)
    return ref


@pytest.mark.parametrize("dtype,D", CASES, ids=IDS)
def test_classifier_head(E, dtype, D, monkeypatch):
    """p_drop = 0.  Forward: the [CLS] and bottleneck-0 rows gathered exactly, pooler GEMM, tanh, classifier GEMM, the mean of
    the two halves of the [2M, 2] logits (the scalar kernel) correctly rounded.  Backward: 0.5 g copied to both halves,
    the GEMMs, tanh', and the two halves of the row gradient copied onto the [CLS] and bottleneck rows of a zero buffer."""
    from multimodaldiscussiontransformer_amd import ops
    g = ragged_geometry()
    M = g["M"]
    text = val(g["rows_fus"], D, 1, dtype)
    pool_w, pool_b = val(D, D, 2, dtype, 2.0 * D ** -0.5), val(1, D, 3, dtype).view(-1)
    cls_w, cls_b = val(2, D, 4, dtype, 2.0 * D ** -0.5), val(1, 2, 5, dtype).view(-1)
    G = val(M, 2, 6, dtype)
    P = [torch.nn.Parameter(dev(t)) for t in (pool_w, pool_b, cls_w, cls_b)]
    rec = Recorder(ops, monkeypatch)
    tape = E.Tape()
    tv = E.Var(dev(text))
    o = E.classifier_head(tape, tv, M, i32(g["cls"]), i32(g["bn0"]), *P, p_drop=0.0)
    torch.cuda.synchronize()
    rows = torch.cat([text[g["cls"]], text[g["bn0"]]])
    pre_g, l2_g = rec.gemms
    assert torch.equal(pre_g["a"], rows), "classifier_head: the gathered [CLS] / bottleneck rows are no copies"
    check_gemm(pre_g, "pooler GEMM")
    (x_t, y_t), = rec.tanh_f
    assert torch.equal(x_t, pre_g["out"])
    RR.check("tanh_fwd", y_t, RR.reference_tanh_fwd(x_t), what="pooler tanh")
    assert torch.equal(l2_g["a"], y_t)
    check_gemm(l2_g, "classifier GEMM")
    l2 = l2_g["out"]
    RR.check("logits mean", o.data.cpu(), RR.reference_row_axpby(torch.zeros(M, 2, dtype=dtype), M, a=l2, alpha=0.5, b=l2, bm=(None, 1, 1, M), beta=0.5),
             what="logits = 0.5 l2[:M] + 0.5 l2[M:]")
    # backward
    o.grad = dev(G)
    tape.backward()
    torch.cuda.synchronize()
    wg_cls, dpooled_g, wg_pool, drows_g = rec.gemms[2:]
    half = (0.5 * G.double()).to(dtype)
    assert torch.equal(wg_cls["a"], torch.cat([half, half])), "dl2 is not 0.5 g in both halves"
    check_gemm(dpooled_g, "d pooled GEMM")
    (y_b, dy_b, dx_b), = rec.tanh_b
    assert torch.equal(y_b, y_t) and torch.equal(dy_b, dpooled_g["out"])
    RR.check("tanh_bwd", dx_b, RR.reference_tanh_bwd(y_b, dy_b), what="pooler tanh'")
    assert torch.equal(drows_g["a"], dx_b) and torch.equal(wg_pool["a"], dx_b) and torch.equal(wg_pool["b"], rows)
    check_gemm(drows_g, "d rows GEMM")
    drows = drows_g["out"].double()
    want = torch.zeros(g["rows_fus"], D, dtype=torch.float64).index_copy(0, g["cls"], drows[:M]).index_copy(0, g["bn0"], drows[M:])
    same(tv.grad, want, "classifier_head text gradient")
    # parameter gradients: the weight GEMMs from what they read, the bias sums against fp64
    zeros = {n: torch.zeros(n) for n in (2, D)}
    for r, name, n in ((wg_cls, "classifier", 2), (wg_pool, "pooler", D)):
        check_gemm(r, f"{name} weight gradient", asum0=zeros[n] if r["kw"].get("asum") is not None else None)
    check_sum("bias grad", tape.tmp_grads[id(P[3])], wg_cls["a"].double(), what="classifier bias gradient")
    check_sum("bias grad", tape.tmp_grads[id(P[1])], dx_b.double(), what="pooler bias gradient")
    assert torch.equal(tape.tmp_grads[id(P[2])].cpu(), wg_cls["out"]) and torch.equal(tape.tmp_grads[id(P[0])].cpu(), wg_pool["out"])


# ------------------------------------------------------------------------------------------------ Tape.add_grad
@pytest.mark.parametrize("dtype,D", CASES, ids=IDS)
def test_add_grad_accumulates_twice(E, dtype, D):
    """The first gradient is taken over as it is, the second and the third are added to it, one rounded add each."""
    rows = 7
    g1, g2, g3 = val(rows, D, 1, dtype), val(rows, D, 2, dtype), val(rows, D, 3, dtype)
    tape = E.Tape()
    v = E.Var(torch.zeros(rows, D, dtype=dtype, device=DEV))
    first = dev(g1)
    tape.add_grad(v, first)
    assert v.grad is first
    tape.add_grad(v, dev(g2))
    torch.cuda.synchronize()
    after2 = v.grad.cpu().clone()
    RR.check("add_grad", after2, RR.reference_row_axpby(g1, rows, a=g2, accumulate=True), what="g1 + g2")
    tape.add_grad(v, dev(g3))
    torch.cuda.synchronize()
    RR.check("add_grad", v.grad.cpu(), RR.reference_row_axpby(after2, rows, a=g3, accumulate=True), what="(g1 + g2) + g3")
    frozen = E.Var(torch.zeros(1, D, dtype=dtype, device=DEV), needs_grad=False)
    tape.add_grad(frozen, dev(g1[:1]))
    assert frozen.grad is None


def test_report_worst_error_over_bound():
    """Not a check of its own: prints the worst err / bound each helper reached in this run (pytest -s, or the log)."""
    print("\nengine rows worst err/bound: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(RR.WORST.items())))
    assert all(v <= 1.0 for v in RR.WORST.values())
