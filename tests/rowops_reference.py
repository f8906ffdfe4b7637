"""fp64 reference and per-element error bounds for the row movers of csrc/rowops.hip (mdt_row_axpby, mdt_row_scatter_add_f32,
mdt_bert_embed_sum / _rows, mdt_vit_patchify, mdt_vit_assemble, mdt_graph_node_feature, mdt_tanh_fwd / _bwd; include/mdt_hip.h),
pure torch: no device, no native library.

Every reference_*() computes the documented result from the exact stored operands and returns, per element of the WHOLE output
buffer (the rows a call must leave alone included), the triple (fp64 value, δ, exact): δ bounds the fp32 arithmetic error a
kernel may make before its one rounding to the output type T, and ``exact`` marks the elements with δ = 0 whose bits are
determined — the stored result must equal value.to(T).  check() turns (value, δ) into a tolerance with
tests/gemm_reference.py (bound(): half an ulp of T plus δ; unit roundoff 2^-24 for fp32, 2^-8 for bf16), demands equality
on the exact elements, refuses a vacuous bound for sums and keeps the worst err / bound per entry point.
Equality is by value: a copied -0 arrives as +0 (the kernels compute 0 + alpha a), which == accepts.

The error model, u = 2^-24 (unit roundoff of fp32), γ_n = n u / (1 - n u).

Row addressing.  row_index() is the twin of pick_row: an index vector wins over the affine map (whose inner / stride /
offset are then ignored), otherwise row = (r / inner) stride + r % inner + off (inner <= 1: r stride + off).  A negative
destination row skips r, a negative source row contributes nothing (not even its 0: the term is absent, no add happens).

mdt_row_axpby, one element: v = 0; v += alpha a; v += beta b; v += dst (each only when present); dst = T(v).
    product p = c x     exact in fp32 when c x is an fp32 number (c = 1, c = 0.5, ...), else δp = u |p|
    the first term      0 + p = p: no rounding
    every later add     δ' = δ + δterm + u (|v'| + δ + δterm), nothing where nothing came in and v' is an fp32 number
With FMA contraction (the build uses -ffp-contract=off, the bound does not depend on it) an add that follows a product is
one rounding of p_exact + v instead of two: its error u |v'| is below what the line above allows, so the same δ holds.
Hence the bit-equal cases: a pure copy or gather (alpha = 1, one source), the zero fill, the rows of skipped destinations and
everything the call does not address, and — fp32 output — ONE add of exact terms (alpha = beta = 0.5, or alpha = 1 with
accumulate): only the add rounds, T is fp32, so the result is the correctly rounded sum, value.to(float32).  In bf16 the
same add is followed by the rounding to bf16 (two roundings): δ = u |v| unless the sum is an fp32 number.

mdt_tanh_fwd: y = T(tanhf(x)).  The accuracy of the device tanhf is stated neither by the HIP headers nor by this
project's kernel guides, so it was measured: tools/probes/tanh_probe.hip compares tanhf with fp64 tanh for every bf16
value in [-12, 12] and for 2^20 evenly spaced fp32 values there.  Worst relative error on an MI355X: 9.795e-8 = 1.643 u over
the bf16 values, 1.404e-7 = 2.356 u over the fp32 grid (TANH_MEASURED; docs/experiment_log.md); the model allows twice the
worst and never less than u: δ = ε_tanh |tanh x|.
mdt_tanh_bwd: dx = T(dy (1 - t t)) from the stored t:
    q = t t          δq = u t² (0 where t² is an fp32 number)
    s = 1 - q        δs = δq + u (|s| + δq): an ABSOLUTE error of the order u t² that does not shrink with s — near |t| = 1
                     the difference cancels and a relative bound on s would be wrong by the factor t² / s
    dx = dy s        δ = |dy| δs + u |dy| (|s| + δs)
mdt_vit_patchify: one rounding of an fp32 pixel, bit-equal to .to(T).  mdt_vit_assemble: one add (the fp32 rule above).
mdt_graph_node_feature: (in_emb + out_emb) + src, two adds in that order; without a source row one add; the graph-token
row is a copy.  mdt_bert_embed_sum / _rows: (word + type) + position, tests/layernorm_reference.py reference_embed_sum.
mdt_row_scatter_add_f32: table[t] += Σ src rows with idx = t, fp32 atomics in any order: the bound of a sum of n exact
terms plus the starting value taken in any order, γ_{n+1} (|start| + Σ |terms|) (_sum_err of the LayerNorm reference),
0 where all of them sit on one power-of-two granule g with (|start| + Σ |terms|) / g < 2^24 — every partial sum in every
order is then an fp32 number and the bits are determined.  A table row nothing is added to keeps its bits.

Engine-level references (tests/test_engine_embeddings_gpu.py).  reference_type_split: the two-row token-type gradient of
engine._type_emb_grad, two any-order column sums (all rows; the rows weighted by their type) and the row_axpby rule above for
row 1 = one + old and row 0 = (tot - one) + old.  reference_patch_embed: mdt_vit_patch_embed, the fp64 value of the projection,
bias and position add on the stored operands before its ONE rounding; δ = γ_K |A| |B| for the accumulation in any order plus one
rounding of a partial sum for each of the two adds, in either order.

Row geometry (tests/test_rowops_reference_cpu.py).  reference_text_rows / reference_prune_rows: the encoder's index vectors as
plain loops over the comments, tokens and images of the host trees, with no formula taken from data/geometry.py.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Optional, Tuple

import numpy as np
import torch

import tests.layernorm_reference as LR
from tests.layernorm_reference import Guarded, assert_within, bound, gen, gen_int, reference_embed_sum, ulp  # noqa: F401

U32 = LR.U32
TANH_MEASURED = 1.405e-7              # 2.356 * 2^-24 (fp32 grid; 1.643 * 2^-24 over the bf16 values)
TANH_REL = max(2.0 * TANH_MEASURED, U32)
bf16, f32 = torch.bfloat16, torch.float32

_rounded, _sum_err, _rep32 = LR._rounded, LR._sum_err, LR._rep32


# ------------------------------------------------------------------------------------------------ addressing
def row_index(r, idx, inner=1, stride=1, off=0):
    """pick_row: the row that loop index ``r`` (int or int64 tensor) addresses."""
    if idx is not None:
        return idx.long()[r]
    if inner <= 1:
        return r * stride + off
    q = torch.div(r, inner, rounding_mode="floor") if torch.is_tensor(r) else r // inner
    return q * stride + (r - q * inner) + off


Map = Tuple[Optional[torch.Tensor], int, int, int]          # (idx, inner, stride, off)
PLAIN: Map = (None, 1, 1, 0)


# ------------------------------------------------------------------------------------------------ references
def _whole(dst0):
    v = dst0.double().clone()
    return v, torch.zeros_like(v), torch.ones_like(v, dtype=torch.bool)


def reference_row_axpby(dst0, nrows, d: Map = PLAIN, a=None, am: Map = PLAIN, alpha=1.0, b=None, bm: Map = PLAIN, beta=1.0,
                        accumulate=False):
    """(value, δ, exact) [rows of dst0, D] after mdt_row_axpby on the buffer ``dst0``; ``a`` / ``b`` as stored BEFORE the call
    (pass dst0 itself for an operand that aliases dst)."""
    T, dev = dst0.dtype, dst0.device
    D = dst0.shape[1]
    r = torch.arange(nrows, device=dev)
    dr = row_index(r, *d)
    live = dr >= 0
    assert int(dr[live].unique().numel()) == int(live.sum()), "row_axpby reference: a destination row appears twice"
    assert not live.any() or int(dr[live].max()) < dst0.shape[0], "row_axpby reference: destination row out of range"
    v = torch.zeros(nrows, D, dtype=torch.float64, device=dev)
    dl = torch.zeros_like(v)
    nterm = torch.zeros(nrows, dtype=torch.int64, device=dev)
    clean = torch.ones_like(v, dtype=torch.bool)             # every product so far is an fp32 number

    def add(v, dl, nterm, t, dt, have):
        first = (nterm == 0)[:, None]
        vn, dn = v + t, dl + dt
        dn = torch.where(first, dn, _rounded(dn, vn, vn.abs() + dn))
        h = have[:, None]
        return torch.where(h, vn, v), torch.where(h, dn, dl), nterm + have.long()

    for src, m, coef in ((a, am, alpha), (b, bm, beta)):
        if src is None:
            continue
        sr = row_index(r, *m)
        have = sr >= 0
        assert not have.any() or int(sr[have].max()) < src.shape[0], "row_axpby reference: source row out of range"
        t = float(np.float32(coef)) * src.double()[sr.clamp(min=0)]
        dt = torch.where(_rep32(t), torch.zeros_like(t), U32 * t.abs())
        clean &= (dt == 0) | ~have[:, None]
        v, dl, nterm = add(v, dl, nterm, t, dt, have)
    if accumulate:
        t = dst0.double()[dr.clamp(min=0)]
        v, dl, nterm = add(v, dl, nterm, t, torch.zeros_like(t), torch.ones_like(live))
    if T == f32:                                             # one add of exact terms into fp32: the correctly rounded sum
        dl = torch.where(clean & (nterm <= 2)[:, None], torch.zeros_like(dl), dl)
    V, DL, EX = _whole(dst0)
    V[dr[live]], DL[dr[live]], EX[dr[live]] = v[live], dl[live], (dl == 0)[live]
    return V, DL, EX


def reference_scatter_add(table0, idx, src, nrows, s_stride=1, s_off=0):
    """table after mdt_row_scatter_add_f32: row t gains the rows r * s_stride + s_off of ``src`` with idx[r] = t."""
    V, DL, EX = _whole(table0)
    r = torch.arange(nrows, device=idx.device)
    rows = src.double()[r * s_stride + s_off]
    ix = idx.long()[:nrows]
    for t in ix[ix >= 0].unique().tolist():
        terms = rows[ix == t]
        c0 = table0.double()[t]
        V[t] = c0 + terms.sum(0)
        DL[t] = _sum_err(terms, torch.zeros_like(terms), 0, c0)
        EX[t] = DL[t] == 0
    return V, DL, EX


def reference_embed(out0, word, pos, typ, ids, types, pos_ids, out_rows):
    """out0 with row out_rows[r] = (word[ids[r]] + typ[types[r]]) + pos[pos_ids[r]]."""
    V, DL, EX = _whole(out0)
    v, d = reference_embed_sum(word, pos, typ, ids.view(-1), types.view(-1), pos_ids.view(-1))
    V[out_rows], DL[out_rows], EX[out_rows] = v, d, d == 0
    return V, DL, EX


def reference_type_split(table0, types, src):
    """The two-row token-type table after engine._type_emb_grad on the rows ``src`` (``types`` 0 / 1 per row): two fp32 column
    sums in any order, tot = Σ src and one = Σ types src (the products by 0 / 1 are exact; the zero terms are added too), then
    row 1 = one + table[1] (one add) and row 0 = (tot - one) + table[0] (the row_axpby rule: 1 tot is the first term, the add
    of -1 one rounds, the add of the old value rounds)."""
    V, DL, EX = _whole(table0)
    assert table0.shape[0] == 2, "the token-type split is written for two types"
    G = src.double()
    w = types.double().view(-1, 1)
    assert G.shape[0] == w.shape[0] and bool(((w == 0) | (w == 1)).all())
    zero = torch.zeros_like(G)
    tot, d_tot = G.sum(0), _sum_err(G, zero, 0)
    one, d_one = (G * w).sum(0), _sum_err(G * w, zero, 0)
    t0 = table0.double()
    v1 = one + t0[1]
    V[1], DL[1] = v1, _rounded(d_one, v1, v1.abs() + d_one)
    diff = tot - one
    d_diff = _rounded(d_tot + d_one, diff, diff.abs() + d_tot + d_one)
    v0 = diff + t0[0]
    V[0], DL[0] = v0, _rounded(d_diff, v0, v0.abs() + d_diff)
    return V, DL, DL == 0


def reference_patch_embed(img, p, wmat, bias, cls, pos):
    """tokens [I (np + 1), D] of mdt_vit_patch_embed: the fp64 value of Conv2d + bias + position (and [CLS] + position) on the
    stored operands (pixels rounded to the weight's type, as the A loader rounds them) before its ONE rounding to T.  δ: the
    K-term fp32 accumulation in any order, γ_K (|A| |B|), and the two adds (bias, position) in either order, each rounding a
    partial sum of magnitude at most |A| |B| + |bias| + |pos| (+ what it carries); the [CLS] row is one add of stored values."""
    I, C, HW, _ = img.shape
    T = wmat.dtype
    gw = HW // p
    npatch, K, D = gw * gw, C * p * p, wmat.shape[0]
    cols = reference_patchify(torch.zeros(I * npatch, K, dtype=T), img, p)[0]
    W, b, P = wmat.double().view(D, K), bias.double().view(1, D), pos.double().view(npatch + 1, D)
    S = cols.abs() @ W.abs().t()
    g = LR._gamma(K)
    body = P[1:].repeat(I, 1)
    v = cols @ W.t() + b + body
    d = g * S + 2.0 * U32 * (1.0 + g) * (S + b.abs() + body.abs())
    vc, dc = _one_add(cls.double().view(1, D), P[:1], T)
    v = torch.cat([vc.expand(I, 1, D), v.view(I, npatch, D)], 1).reshape(I * (npatch + 1), D)
    d = torch.cat([dc.expand(I, 1, D), d.view(I, npatch, D)], 1).reshape(I * (npatch + 1), D)
    return v, d, d == 0


def reference_patchify(cols0, img, p):
    """cols0 [I * gw * gw, >= K] with its first K columns = the gathered pixels (exact: one rounding to T)."""
    I, C, HW, _ = img.shape
    gw = HW // p
    V, DL, EX = _whole(cols0)
    g = img.view(I, C, gw, p, gw, p).permute(0, 2, 4, 1, 3, 5).reshape(I * gw * gw, C * p * p)
    V[:, :C * p * p] = g.to(cols0.dtype).double()            # the rounding IS the operation
    return V, DL, EX


def _one_add(x, y, T):
    v = x + y
    d = _rounded(torch.zeros_like(v), v, v.abs())
    return v, (torch.zeros_like(d) if T == f32 else d)


def reference_assemble(tokens0, patches, cls, pos, I, npatch, seq_stride, off):
    V, DL, EX = _whole(tokens0)
    P = pos.double()
    for i in range(I):
        s = torch.cat([cls.double().view(1, -1), patches.double()[i * npatch:(i + 1) * npatch]])
        v, d = _one_add(s, P[:npatch + 1], tokens0.dtype)
        lo = i * seq_stride + off
        V[lo:lo + npatch + 1], DL[lo:lo + npatch + 1], EX[lo:lo + npatch + 1] = v, d, d == 0
    return V, DL, EX


def reference_node_feature(x0, src, node_row, in_degree, out_degree, in_emb, out_emb, graph_token, B, Tn):
    V, DL, EX = _whole(x0)
    T = x0.dtype
    nr = node_row.long().view(-1)
    v, d = _one_add(in_emb.double()[in_degree.long().view(-1)], out_emb.double()[out_degree.long().view(-1)], T)
    if src is not None:
        have = (nr >= 0)[:, None]
        s = src.double()[nr.clamp(min=0)]
        d1 = _rounded(torch.zeros_like(v), v, v.abs())       # the first add as an intermediate: rounded in fp32 for every T
        v2 = v + s
        d2 = _rounded(d1, v2, v2.abs() + d1)
        v, d = torch.where(have, v2, v), torch.where(have, d2, d)
    else:
        assert bool((nr < 0).all()), "graph_node_feature without src: every node_row must be negative"
    rows = (torch.arange(B, device=x0.device)[:, None] * Tn + 1 + torch.arange(Tn - 1, device=x0.device)[None]).view(-1)
    V[rows], DL[rows], EX[rows] = v, d, d == 0
    V[torch.arange(B, device=x0.device) * Tn] = graph_token.double().view(1, -1)
    return V, DL, EX


def reference_tanh_fwd(x):
    v = torch.tanh(x.double())
    d = TANH_REL * v.abs()
    return v, d, d == 0


def reference_tanh_bwd(y, dy):
    t, g = y.double(), dy.double()
    q = t * t
    dq = _rounded(torch.zeros_like(q), q, q)
    s = 1.0 - q
    ds = _rounded(dq, s, s.abs() + dq)
    v = g * s
    d = g.abs() * ds
    d = _rounded(d, v, g.abs() * (s.abs() + ds))
    return v, d, d == 0


# ------------------------------------------------------------------------------------------------ the check
WORST = {}        # entry point -> worst err / bound seen by check() (the GPU files report it)


def check(name, got, ref, what="", dtype=None, nonvacuous=False):
    """``got`` (the whole output buffer) against ``ref`` = (value, δ, exact): every element within bound(value, δ, T), the
    exact ones equal to value.to(T); ``nonvacuous``: median bound / |ref| <= 2^-7 (sums).  Keeps the worst err / bound."""
    v, d, exact = ref
    dt = dtype or got.dtype
    assert tuple(got.shape) == tuple(v.shape), f"{what}: shape {tuple(got.shape)} against {tuple(v.shape)}"
    bnd = bound(v, d, dt)
    fin = torch.isfinite(v)
    ratio = torch.where(fin, (got.double() - v).abs() / bnd.clamp(min=1e-300), torch.zeros_like(v))
    if ratio.numel():
        r = float(ratio.max())
        WORST[name] = max(WORST.get(name, 0.0), r if r == r else float("inf"))
    assert_within(got, v, bnd, what=f"{what} {name}", dtype=dt, median_limit=2.0 ** -7 if nonvacuous else None)
    bad = exact & (got != v.to(dt))
    n = int(bad.sum())
    if n:
        at = tuple(int(i) for i in np.unravel_index(int(torch.argmax(bad.view(-1).to(torch.uint8))), tuple(v.shape)))
        raise AssertionError(f"{what} {name}: {n} of {int(exact.sum())} bit-determined elements differ; first at {at}: "
                             f"out {float(got[at])!r} want {float(v.to(dt)[at])!r}")


# ------------------------------------------------------------------------------------------------ the matrix
# widths of tests/test_rowops_gpu.py; tests/test_rowops_reference_cpu.py proves the bounds at each.  A wave sweeps 64 lanes x VN
# elements: one full sweep exactly (256 / 512), a second sweep with one lane (260 / 520), 3 (bf16: 1.5) and 4 (2) sweeps.
VEC_DIMS = {f32: (4, 256, 260, 768, 1024), bf16: (8, 512, 520, 768, 1024)}
SCALAR_DIMS = (2, 3, 65, 130)
ROWS = (1, 3, 4, 5)
BIG_ROWS = 4099                       # 1025 workgroups of 4 rows, the last with 3
BIG_DIMS = (128, 768)
S_IN, N_FRONT = 3, 2                  # sequence geometry of the two-level maps: S = 5 rows per sequence, 2 in front
S_SEQ = S_IN + N_FRONT


def vn(dtype, D):
    """Elements per 16-byte vector, 1 when D cannot be swept in vectors (the scalar kernel)."""
    n = 8 if dtype == bf16 else 4
    return n if D % n == 0 else 1


@dataclass
class Axpby:
    """One mdt_row_axpby call: the start content of dst, the operands (``a_is_dst`` / ``b_is_dst``: the operand IS the
    destination buffer, in place) and the row maps."""
    form: str
    nrows: int
    dst0: torch.Tensor
    d: Map = PLAIN
    a: Optional[torch.Tensor] = None
    am: Map = PLAIN
    alpha: float = 1.0
    b: Optional[torch.Tensor] = None
    bm: Map = PLAIN
    beta: float = 1.0
    accumulate: bool = False
    a_is_dst: bool = False
    b_is_dst: bool = False
    note: str = field(default="", compare=False)

    def reference(self):
        return reference_row_axpby(self.dst0, self.nrows, self.d, self.dst0 if self.a_is_dst else self.a, self.am, self.alpha,
                                   self.dst0 if self.b_is_dst else self.b, self.bm, self.beta, self.accumulate)


def _distinct(n, total, seed, device, lo=0):
    """n distinct rows of [lo, total) in random order, int32."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randperm(total - lo, generator=g)[:n] + lo).to(torch.int32).to(device)


def _span(nrows, inner, stride, off):
    """Rows a two-level map reaches over nrows loop indices, plus one that must stay untouched."""
    return int(row_index(nrows - 1, None, inner, stride, off)) + 2


# form -> the engine call it stands for (multimodaldiscussiontransformer_amd/engine.py)
AXPBY_FORMS = {
    "idx_dst": "expand_rows forward: di = pre2fus",
    "idx_src": "expand_rows adjoint: ai = pre2fus / bn_rows_all",
    "idx_both": "scatter_rows, rows_mix(1, 0) with index vectors",
    "idx_wins": "an index vector with a non-trivial map beside it: the map is ignored",
    "inner_dst": "expand_sequences forward: d_inner = s_in, d_stride = S, d_off = n_front",
    "inner_src": "expand_sequences adjoint, take_rows(s_map), the ViT gradient: a_inner = s_in, a_stride = S, a_off = n_front",
    "broadcast": "expand_sequences / expand_rows: the learned bottleneck rows, a_inner = n_front, a_stride = 0",
    "offset": "classifier_head: the second half of the pooled rows, d_off = M",
    "b_off": "classifier_head: logits = 0.5 l2[:M] + 0.5 l2[M:], b_off = M",
    "zero_fill": "expand_sequences(front=None): neither a nor b",
    "b_is_dst": "rows_mix(0.5, 0.5): b aliases dst in place",
    "a_is_dst": "rows_mix adjoint: g_dst[dr] *= beta, a aliases dst in place",
    "accumulate": "take_rows / scatter_rows / classifier_head adjoints, Tape.add_grad: accumulate on a non-zero start",
    "general": "alpha, beta no powers of two, both sources and accumulate: the bounded case",
    "negative": "negative entries in di (row skipped) and ai (nothing contributed)",
}


def values(shape, seed, scale=1.0, dtype=f32, device="cpu"):
    """Products of two uniform numbers, rounded to ``dtype``: unlike gen(), whose fp32 values all sit on the grid 2^-23 scale
    of torch.rand (their sums and halves never round in fp32), these use the whole significand at every exponent."""
    return (gen(shape, seed, 1.0, f32, device) * gen(shape, seed + 7919, scale, f32, device)).to(dtype)


def axpby_case(form, nrows, D, dtype, seed, device="cpu") -> Axpby:
    """The operands of ``form`` at ``nrows`` loop indices, from values()."""
    n = nrows

    def val(rows, k):
        return values((rows, D), seed + 17 * k, 1.0, dtype, device)

    if form == "idx_dst":
        return Axpby(form, n, val(n + 3, 1), d=(_distinct(n, n + 3, seed, device), 1, 1, 0), a=val(n, 2))
    if form == "idx_src":
        return Axpby(form, n, val(n + 1, 1), a=val(n + 3, 2), am=(_distinct(n, n + 3, seed, device), 1, 1, 0))
    if form == "idx_both":
        return Axpby(form, n, val(n + 3, 1), d=(_distinct(n, n + 3, seed, device), 1, 1, 0), a=val(n + 2, 2),
                     am=(_distinct(n, n + 2, seed + 1, device), 1, 1, 0))
    if form == "idx_wins":
        return Axpby(form, n, val(n + 3, 1), d=(_distinct(n, n + 3, seed, device), 3, 7, 2), a=val(n + 2, 2),
                     am=(_distinct(n, n + 2, seed + 1, device), 2, 5, 1))
    if form == "inner_dst":
        return Axpby(form, n, val(_span(n, S_IN, S_SEQ, N_FRONT), 1), d=(None, S_IN, S_SEQ, N_FRONT), a=val(n, 2))
    if form == "inner_src":
        return Axpby(form, n, val(n + 1, 1), a=val(_span(n, S_IN, S_SEQ, N_FRONT), 2), am=(None, S_IN, S_SEQ, N_FRONT))
    if form == "broadcast":          # rows past n_front exist (and differ) so that a stride read as 1 reads something else
        return Axpby(form, n, val(_span(n, N_FRONT, S_SEQ, 0), 1), d=(None, N_FRONT, S_SEQ, 0), a=val(N_FRONT + n, 2),
                     am=(None, N_FRONT, 0, 0))
    if form == "offset":
        return Axpby(form, n, val(2 * n + 1, 1), d=(None, 1, 1, n), a=val(n, 2))
    if form == "b_off":
        return Axpby(form, n, val(n + 1, 1), a=val(n, 2), alpha=0.5, b=val(2 * n + 1, 3), bm=(None, 1, 1, n), beta=0.5)
    if form == "zero_fill":
        return Axpby(form, n, val(_span(n, N_FRONT, S_SEQ, 0), 1), d=(None, N_FRONT, S_SEQ, 0))
    if form == "b_is_dst":
        di = _distinct(n, n + 3, seed, device)
        return Axpby(form, n, val(n + 3, 1), d=(di, 1, 1, 0), a=val(n + 2, 2), am=(_distinct(n, n + 2, seed + 1, device), 1, 1, 0),
                     alpha=0.5, bm=(di, 1, 1, 0), beta=0.5, b_is_dst=True)
    if form == "a_is_dst":
        di = _distinct(n, n + 3, seed, device)
        return Axpby(form, n, val(n + 3, 1), d=(di, 1, 1, 0), am=(di, 1, 1, 0), alpha=0.5, a_is_dst=True)
    if form == "accumulate":
        return Axpby(form, n, val(n + 3, 1), d=(_distinct(n, n + 3, seed, device), 1, 1, 0), a=val(n, 2), accumulate=True)
    if form == "general":
        return Axpby(form, n, val(n + 3, 1), d=(_distinct(n, n + 3, seed, device), 1, 1, 0), a=val(n + 2, 2),
                     am=(_distinct(n, n + 2, seed + 1, device), 1, 1, 0), alpha=0.3, b=val(n, 3), beta=-1.7, accumulate=True)
    if form == "negative":           # row 0 of dst and of a is nobody's, so a negative index read as 0 shows
        di = _distinct(n, n + 3, seed, device, lo=1)
        ai = _distinct(n, n + 3, seed + 1, device, lo=1)
        r = torch.arange(n, device=device)
        di = torch.where(r % 4 == 1, torch.full_like(di, -1), di)
        ai = torch.where(r % 3 == 0, torch.full_like(ai, -3), ai)
        return Axpby(form, n, val(n + 3, 1), d=(di, 1, 1, 0), a=val(n + 3, 2), am=(ai, 1, 1, 0), b=val(n, 3), beta=1.0)
    raise KeyError(form)


def granule_rows(rows, D, seed, dtype, device="cpu", r=16):
    """Values k / 16, |k| <= r: sums of up to 2^24 / r of them are exact in fp32 in every order."""
    return (gen_int((rows, D), seed, r, f32, device) / 16.0).to(dtype)


def tanh_inputs(n, dtype, seed, device="cpu"):
    """n arguments in (-4, 4), with 0, ±tiny, ±9.5 and values whose tanh is within 2^-8 of ±1 at the front."""
    x = values((n,), seed, 4.0, f32, device)
    special = torch.tensor([0.0, 2.0 ** -100, -2.0 ** -100, 9.5, -9.5, 3.2, -3.2, 4.5, -4.5, 3.0, -3.0], device=device)
    k = min(n, special.numel())
    x[:k] = special[:k]
    return x.to(dtype)


def near_one(n, dtype, seed, device="cpu"):
    """n stored tanh values for the backward in (-1, 1), the front ones 0, ±1 and |t| within 2^-8 of 1."""
    t = torch.tanh(values((n,), seed, 4.0, f32, device))
    if dtype == bf16:
        special = torch.tensor([0.0, 1.0, -1.0, 1.0 - 2.0 ** -8, -(1.0 - 2.0 ** -8), 1.0 - 2.0 ** -7, 2.0 ** -100], device=device)
    else:
        special = torch.tensor([0.0, 1.0, -1.0, 1.0 - 2.0 ** -24, -(1.0 - 2.0 ** -24), 1.0 - 2.0 ** -9, -(1.0 - 2.0 ** -12),
                                0.99999, 2.0 ** -100], device=device)
    k = min(n, special.numel())
    t[:k] = special[:k]
    return t.to(dtype)


# ------------------------------------------------------------------------------------------------ operands of the other entry points
def embed_operands(M, L, D, dtype, seed, device="cpu"):
    """Tables and ids of one embedding case; the position table has M * L rows so that a position taken from r exists."""
    V = 37
    word, pos, typ = values((V, D), seed + 1, 1.0, dtype, device), values((M * L, D), seed + 2, 0.5, dtype, device), \
        values((2, D), seed + 3, 0.25, dtype, device)
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, V, (M, L), generator=g, dtype=torch.int32).to(device)
    types = torch.randint(0, 2, (M, L), generator=g, dtype=torch.int32).to(device)
    return word, pos, typ, ids, types


TEXT_V, TEXT_P, TEXT_M, TEXT_L = 97, 40, 9, 24
TEXT_LENS = (24, 1, 24, 17, 24, 9, 24, 24, 24)        # 171 valid tokens of the 216 padded rows


def text_case(seed=77):
    """The token layout of the engine's embedding suites (tests/test_engine_embeddings_gpu.py and its CPU companion): a padded
    [M, L] id matrix whose padding is id 0, and the ragged view of its valid tokens (their flat rows m L + l and pos_ids l).
    Id 0 sits on 130 of the valid tokens as well (the ragged form still has a segment of more than two 64-row chunks and a
    heavily contended table row; 175 rows in the padded form), ids 1..12 occur exactly once, the other 29 valid tokens draw
    from ids 13..59 and the table rows 60..96 are never referenced; token type 1 on the rows with r % 5 in (1, 3)."""
    M, L = TEXT_M, TEXT_L
    g = torch.Generator().manual_seed(seed)
    lens = torch.tensor(TEXT_LENS)
    l = torch.arange(L)[None].expand(M, L)
    valid = (l < lens[:, None]).reshape(-1)
    rows = torch.nonzero(valid).view(-1)
    n = int(rows.numel())
    perm = rows[torch.randperm(n, generator=g)]
    ids = torch.zeros(M * L, dtype=torch.int64)
    ids[perm[130:142]] = torch.arange(1, 13)
    ids[perm[142:]] = torch.randint(13, 60, (n - 142,), generator=g)
    r = torch.arange(M * L)
    types = ((r % 5 == 1) | (r % 5 == 3)).long()
    return dict(M=M, L=L, ids=ids.view(M, L).to(torch.int32), types=types.view(M, L).to(torch.int32), rows=rows,
                pos_padded=(r % L).to(torch.int32), ids_rows=ids[rows].to(torch.int32), types_rows=types[rows].to(torch.int32),
                pos_rows=(rows % L).to(torch.int32))


def embed_rows(M, L, seq_stride, off, device="cpu"):
    """(output row, position id) of loop index r = m L + l."""
    r = torch.arange(M * L, device=device)
    m, l = torch.div(r, L, rounding_mode="floor"), r % L
    return m * seq_stride + off + l, l


def node_operands(B, Tn, D, dtype, seed, device="cpu", with_src=True):
    """Degree tables, graph token, source rows and the node -> source row map (every third node is padding: -1, degree 0)."""
    n = B * (Tn - 1)
    g = torch.Generator().manual_seed(seed)
    ind = torch.randint(0, 6, (n,), generator=g, dtype=torch.int32)
    outd = torch.randint(0, 6, (n,), generator=g, dtype=torch.int32)
    node_row = (torch.randperm(n + 2, generator=g)[:n]).to(torch.int32)
    pad = torch.arange(n) % 3 == 2
    node_row[pad], ind[pad], outd[pad] = -1, 0, 0
    if not with_src:
        node_row[:] = -1
    o = dict(in_emb=values((6, D), seed + 1, 1.0, dtype, device), out_emb=values((6, D), seed + 2, 1.0, dtype, device),
             token=values((D,), seed + 3, 1.0, dtype, device), src=values((n + 2, D), seed + 4, 1.0, dtype, device) if with_src else None,
             node_row=node_row.to(device), ind=ind.to(device), outd=outd.to(device))
    return o


def scatter_operands(n, D, dtype, seed, granule, device="cpu", s_stride=2, s_off=1, table_rows=5):
    rows = n * s_stride + s_off
    if granule:
        src = granule_rows(rows, D, seed + 1, dtype, device)
        table0 = granule_rows(table_rows + 1, D, seed + 2, f32, device, r=144)
    else:
        src, table0 = values((rows, D), seed + 1, 1.0, dtype, device), values((table_rows + 1, D), seed + 2, 3.0, f32, device)
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, table_rows, (n,), generator=g, dtype=torch.int32)
    idx[torch.arange(n) % 7 == 3] = -1                            # skipped rows
    return table0, idx.to(device), src


# ------------------------------------------------------------------------------------------------ row geometry of a batch
def _i32(v):
    return torch.tensor(v, dtype=torch.int32).reshape(-1)


def batch_layout(trees):
    """What the loop references below read, taken from the host trees themselves with plain loops: ``mask`` (per comment, its
    attention mask as a list of 0 / 1), ``node_comment`` (per padded node (b, n), its comment number or -1) and
    ``img_comment`` (the comments that carry an image, in order)."""
    N = max(len(t["parent"]) for t in trees)
    mask, node_comment, img_comment = [], [], []
    for t in trees:
        n = len(t["parent"])
        for k in range(N):
            if k < n:
                node_comment.append(len(mask))
                if bool(t["image_index"][k]):
                    img_comment.append(len(mask))
                mask.append([int(v != 0) for v in t["attention_mask"][k]])
            else:
                node_comment.append(-1)
    return mask, node_comment, img_comment


def _first_rows(nb, mask, ragged):
    """(first fused row of every comment, token count of every comment in this layout, rows of the fused buffer): comment m
    starts where the running sum of nb + tokens stands."""
    first, ntok, row = [], [], 0
    for mk in mask:
        first.append(row)
        ntok.append(sum(mk) if ragged else len(mk))
        row += nb + ntok[-1]
    return first, ntok, row


def _reference_bins(ntok, extra, cap=64):
    """RaggedText.length_bins with its default cap: the comments of at most ``cap - extra`` tokens, shortest first, and the
    rest, each with the key length it runs at; None unless both bins exist."""
    top = max(ntok) + extra
    order = sorted(range(len(ntok)), key=lambda m: ntok[m])           # stable: ties keep the comment order
    short = [m for m in order if ntok[m] + extra <= cap]
    rest = [m for m in order if ntok[m] + extra > cap]
    if cap >= top or not short or not rest:
        return None
    return [(_i32(short), cap), (_i32(rest), top)]


def reference_text_rows(nb, Sv, mask, node_comment, img_comment, ragged, length_bins=True):
    """The index vectors of MultiGraphormerGraphEncoder._indices, row by row: comment m starts at the running sum of
    nb + tokens; bottleneck token k sits at first + k, [CLS] at first + nb, token t at first + nb + t (ragged: t counts the
    valid tokens; padded: every position owns a row); image i owns Sv rows from i Sv, bottleneck tokens first."""
    M, L = len(mask), len(mask[0])
    first, ntok, rows_fus = _first_rows(nb, mask, ragged)
    pre2fus, bn_all, off_pre = [], [], [0]
    for m in range(M):
        for k in range(nb):
            bn_all.append(first[m] + k)
        for t in range(ntok[m]):
            pre2fus.append(first[m] + nb + t)
        off_pre.append(off_pre[-1] + ntok[m])
    img_text, vit = [], []
    for i, c in enumerate(img_comment):
        for k in range(nb):
            img_text.append(first[c] + k)
            vit.append(i * Sv + k)
    if ragged:
        spec_pre = dict(S=max(ntok), seq_offsets=_i32(off_pre), bins=_reference_bins(ntok, 0) if length_bins else None)
        spec_fus = dict(S=max(ntok) + nb, seq_offsets=_i32(first + [rows_fus]), bins=_reference_bins(ntok, nb) if length_bins else None)
    else:
        spec_pre = dict(S=L, key_mask=torch.tensor(mask, dtype=torch.uint8))
        spec_fus = dict(S=nb + L, key_mask=torch.tensor([[1] * nb + mk for mk in mask], dtype=torch.uint8))
    return dict(ragged=ragged, Sv=Sv, P=Sv - nb, rows_pre=len(pre2fus), rows_fus=rows_fus, spec_pre=spec_pre, spec_fus=spec_fus,
                pre2fus=_i32(pre2fus), bn0_rows=_i32(first), cls_rows=_i32([f + nb for f in first]), bn_rows_all=_i32(bn_all),
                text_row_of_node=_i32([first[c] if c >= 0 else -1 for c in node_comment]), img_text_bn_rows=_i32(img_text),
                vit_bn_rows=_i32(vit))


def reference_prune_rows(nb, Sv, mask, img_comment, ragged):
    """(prune, rows) of MultiGraphormerGraphEncoder._prune_indices: the last fusion layer keeps bottleneck token 0 and [CLS]
    of every comment and bottleneck token 0 (row i Sv) of every image; comment m lands on rows 2m and 2m + 1 of its output."""
    first, _, _ = _first_rows(nb, mask, ragged)
    keep, bn0, cls = [], [], []
    for m, f in enumerate(first):
        keep += [f, f + nb]
        bn0.append(2 * m)
        cls.append(2 * m + 1)
    prune = dict(text_keep=_i32(keep), vit_keep=_i32([i * Sv for i in range(len(img_comment))]),
                 img_bn0_compact=_i32([2 * c for c in img_comment]))
    return prune, dict(bn0_rows=_i32(bn0), cls_rows=_i32(cls))
