"""fp64 reference and per-element error bounds for the LayerNorm family (mdt_layernorm_fwd, mdt_layernorm_fwd_q8,
mdt_bert_embed_ln_rows, mdt_layernorm_bwd; include/mdt_hip.h), pure torch: no device, no native library.

reference_fwd() / reference_bwd() / reference_embed_sum() compute the documented result from the exact stored operands
and, next to every value, a bound δ on the fp32 arithmetic error a kernel may make.  tests/gemm_reference.py turns
(value, δ) into a tolerance (bound(): half an ulp of the storage type plus δ) and checks it (assert_within());
check() below adds the refusal of a vacuous bound for the three column sums and keeps the worst err / bound per output.

The error model, u = 2^-24 (unit roundoff of fp32), γ_n = n u / (1 - n u).

Sums.  A sum of n fp32 terms added with round-to-nearest in ANY order (a lane's vectors, the DPP tree over the wave,
the four waves of a workgroup, float atomics across workgroups) errs by at most γ_n Σ|terms| (Higham, "Accuracy and
Stability of Numerical Algorithms", Thm 4.2 and the remark that the constant holds for every ordering); terms that
carry an error d of their own add Σ d and enter the magnitude as |term| + d.  A sum is exact (δ = 0) where all terms
are exact multiples of one power of two g and (Σ|terms|) / g < 2^24: every partial sum, in any order, is then an fp32
number.  That is what makes a constant row, an integer-valued row and the integer-dy dbeta exact.
Single operations.  Each further fp32 operation (the kernels are built with -ffp-contract=off: no fused multiply-add)
adds u times the magnitude it rounds, nothing where its exact result is an fp32 number and its inputs are exact; a
product a b with errors δa, δb carries |a| δb + δa (|b| + δb).

Forward, row of D elements x, eps as the fp32 number the ABI receives:
    s = Σ x                    δs = sum rule                        mean = s / D       δmean = δs / D + u |mean|
    d = x - mean               δd = δmean + u |d|
    q = Σ d²                   per term 2 |d| δd + δd² + u (|d| + δd)², then the sum rule
    var = q / D, w = var + eps δw = δq / D + u var + u w
    rstd = w^-1/2              δrstd = ((w - δw)^-1/2 - w^-1/2) + ε_rsqrt (w - δw)^-1/2
    y = ((d rstd) gamma) + beta, one rounding per operation as above.
The function x -> x^-1/2 is decreasing and convex, so the first term of δrstd is the exact supremum of the carried
error over [w - δw, w + δw]; to first order it is ½ rstd³ δw.  A row with δw > w / 2 is refused (AssertionError): the
model does not bound it, and a bound that says nothing must not pass for a test.
ε_rsqrt: neither the HIP headers nor the kernel guides of this project state an accuracy for the device rsqrtf, so it
was measured: tools/probes/rsqrt_probe.hip compares rsqrtf with 1 / sqrt in fp64 for every fp32 mantissa of three pairs
of binades (the error pattern repeats every two binades), around 2^-40, 1 and 2^110, which cover eps = 1e-12 and the
variances of every case of tests/test_layernorm_routes_gpu.py.  Worst relative error on an MI355X: 9.398e-8 = 1.577 u in each range
(RSQRT_MEASURED; docs/experiment_log.md); the model allows twice that.

Backward, from the STORED mean / rstd (fp32, exact operands here: the forward statistics are checked on their own):
    a = x - mean, xh = a rstd, gg = dy gamma (exact for bf16 operands), p = gg xh
    m1 = (Σ gg) / D, m2 = (Σ p) / D                                       sum rule, one division each
    v = rstd ((gg - m1) - xh m2) [+ add]                                  one rounding per operation
    dx = T(v)
    dxd = T(dx_stored * scale)     the STORED dx (the kernel re-reads its rounded output), scale = 0 or fp32(1/(1-p)) of
                                   dropout counter row * D + col, whatever the row strides
    colsum += Σ_rows dxd_stored    (dx_stored when nothing is dropped): exact terms, sum rule over rows + 1 terms
    dbeta  += Σ_rows dy            exact terms; integer dy with Σ|dy| < 2^24 makes it exact
    dgamma += Σ_rows dy xh         each term |dy| δxh + u |dy xh|, then the sum rule
The reference rounds where the kernel rounds: dxd and colsum are computed from the tensors the kernel stored (dx_stored,
dxd_stored), each of which is checked against its own bound first.

Embedding front end: xs = T((word[id] + type[t]) + pos[p]), two fp32 additions in that order, then LayerNorm of the
stored xs.
"""
from __future__ import annotations

import numpy as np
import torch

import tests.gemm_reference as R
from tests.gemm_reference import Guarded, assert_within, bound, drop_scale, gen, gen_int, ulp  # noqa: F401  (one import site for the tests)

U32 = R.U32
RSQRT_MEASURED = 9.4e-8               # 1.577 * 2^-24, the same in all three ranges
RSQRT_REL = 2.0 * RSQRT_MEASURED
SUMS = ("dgamma", "dbeta", "colsum")

_gamma, _rep32, F24 = R._gamma, R._rep32, R.F24


def _rounded(d, value, magnitude):
    """δ after one fp32 operation whose exact result is ``value``: unchanged where nothing came in and nothing rounds."""
    return torch.where((d == 0) & _rep32(value), d, d + U32 * magnitude)


def _sum_err(terms, d, dim, c0=None):
    """Error bound of (c0 +) Σ terms along ``dim`` in fp32 in any order, each term carrying error d (module docstring)."""
    n = terms.shape[dim] + (0 if c0 is None else 1)
    a = terms.abs()
    tot = a.sum(dim)
    c = torch.zeros_like(tot) if c0 is None else c0.abs()
    general = d.sum(dim) + _gamma(n) * (c + (a + d).sum(dim))
    clean = (d == 0).all(dim) & torch.isfinite(terms).all(dim)
    exact = torch.zeros_like(clean)
    for q in range(0, 9):                              # g = 2^-q
        g = 2.0 ** q
        exact |= ((terms * g) == torch.round(terms * g)).all(dim) & ((c * g) == torch.round(c * g)) & ((tot + c) * g < F24)
    return torch.where(exact & clean, torch.zeros_like(general), general)


def reference_fwd(x, gamma, beta, eps):
    """{y, mean, rstd}: (fp64 value, δ) each, of LayerNorm over the last axis of the stored x [rows, D]."""
    u = U32
    X, G, B = x.double(), gamma.double()[None, :], beta.double()[None, :]
    D = X.shape[1]
    e = float(np.float32(eps))
    zero = torch.zeros_like(X)
    mu = X.sum(1) / D
    d_mu = _sum_err(X, zero, 1) / D
    d_mu = _rounded(d_mu, mu, mu.abs() + d_mu)
    d = X - mu[:, None]
    d_d = _rounded(d_mu[:, None] + zero, d, d.abs() + d_mu[:, None])
    sq = d * d
    d_sq = 2 * d.abs() * d_d + d_d * d_d
    d_sq = _rounded(d_sq, sq, (d.abs() + d_d) ** 2)
    var = sq.sum(1) / D
    d_var = _sum_err(sq, d_sq, 1) / D
    d_var = _rounded(d_var, var, var + d_var)
    w = var + e
    d_w = _rounded(d_var, w, w + d_var)
    assert bool((d_w <= 0.5 * w).all()), "layernorm reference: a row's variance is not bounded by the error model (δw > w / 2)"
    rs = w.pow(-0.5)
    rs_hi = (w - d_w).pow(-0.5)
    d_rs = (rs_hi - rs) + RSQRT_REL * rs_hi
    rsb, d_rsb = rs[:, None], d_rs[:, None]
    t1 = d * rsb
    d_t1 = d.abs() * d_rsb + (rsb + d_rsb) * d_d
    d_t1 = torch.where((d == 0) & (d_d == 0), zero, d_t1 + u * (d.abs() + d_d) * (rsb + d_rsb))
    t2 = t1 * G
    d_t2 = d_t1 * G.abs()
    d_t2 = torch.where((t1 == 0) & (d_t1 == 0), zero, d_t2 + u * (t1.abs() + d_t1) * G.abs())
    y = t2 + B
    d_y = _rounded(d_t2, y, y.abs() + d_t2)
    return {"y": (y, d_y), "mean": (mu, d_mu), "rstd": (rs, d_rs)}


def reference_embed_sum(word, pos, typ, ids, types, pos_ids):
    """xs = (word[ids] + typ[types]) + pos[pos_ids] before its rounding to the table type: (value, δ)."""
    w, t, p = word.double()[ids.long()], typ.double()[types.long()], pos.double()[pos_ids.long()]
    a = w + t
    d = _rounded(torch.zeros_like(a), a, a.abs())
    v = a + p
    return v, _rounded(d, v, v.abs() + d)


def reference_bwd(dy, x, gamma, mean, rstd, add=None, drop_p=0.0, drop_seed=0, dgamma0=None, dbeta0=None, colsum0=None,
                  want_dropped=False, want_colsum=False, dx_stored=None, dxd_stored=None, counter_ld=None):
    """{dx, dxd, dgamma, dbeta, colsum}: (fp64 value, δ) each.  ``mean`` / ``rstd``: what the forward stored.
    ``dx_stored`` / ``dxd_stored``: the tensors the kernel wrote, needed by dxd (want_dropped) and colsum (want_colsum),
    which the kernel computes from its rounded outputs.  ``counter_ld`` replaces D in the dropout counter (mutant tests)."""
    u = U32
    GY, X, G = dy.double(), x.double(), gamma.double()[None, :]
    rows, D = X.shape
    mu, rs = mean.double()[:, None], rstd.double()[:, None]
    zero = torch.zeros_like(X)
    a = X - mu
    d_a = _rounded(zero, a, a.abs())
    xh = a * rs
    d_xh = rs * d_a
    d_xh = _rounded(d_xh, xh, (a.abs() + d_a) * rs)
    gg = GY * G
    d_gg = _rounded(zero, gg, gg.abs())
    p = gg * xh
    d_p = gg.abs() * d_xh + d_gg * (xh.abs() + d_xh)
    d_p = _rounded(d_p, p, (gg.abs() + d_gg) * (xh.abs() + d_xh))
    m1 = gg.sum(1) / D
    d_m1 = _sum_err(gg, d_gg, 1) / D
    d_m1 = _rounded(d_m1, m1, m1.abs() + d_m1)[:, None]
    m2 = p.sum(1) / D
    d_m2 = _sum_err(p, d_p, 1) / D
    d_m2 = _rounded(d_m2, m2, m2.abs() + d_m2)[:, None]
    m1, m2 = m1[:, None], m2[:, None]
    tb = gg - m1
    d_tb = d_gg + d_m1
    d_tb = _rounded(d_tb, tb, tb.abs() + d_tb)
    tc = xh * m2
    d_tc = xh.abs() * d_m2 + d_xh * (m2.abs() + d_m2)
    d_tc = _rounded(d_tc, tc, (xh.abs() + d_xh) * (m2.abs() + d_m2))
    td = tb - tc
    d_td = d_tb + d_tc
    d_td = _rounded(d_td, td, td.abs() + d_td)
    v = rs * td
    d_v = rs * d_td
    d_v = _rounded(d_v, v, rs * (td.abs() + d_td))
    if add is not None:
        v = v + add.double()
        d_v = _rounded(d_v, v, v.abs() + d_v)
    out = {"dx": (v, d_v)}
    if want_dropped:
        assert dx_stored is not None, "dxd is computed from the stored dx"
        s = drop_scale(rows, D, drop_p, drop_seed, device=X.device, counter_ld=counter_ld)
        vd = dx_stored.double() * s
        out["dxd"] = (vd, _rounded(zero, vd, vd.abs()))
    if want_colsum:
        src = dxd_stored if want_dropped else dx_stored
        assert src is not None, "colsum sums the stored tail output"
        c0 = colsum0.double() if colsum0 is not None else torch.zeros(D, dtype=torch.float64, device=X.device)
        t = src.double()
        out["colsum"] = (c0 + t.sum(0), _sum_err(t, zero, 0, c0))
    b0 = dbeta0.double() if dbeta0 is not None else torch.zeros(D, dtype=torch.float64, device=X.device)
    out["dbeta"] = (b0 + GY.sum(0), _sum_err(GY, zero, 0, b0))
    g0 = dgamma0.double() if dgamma0 is not None else torch.zeros(D, dtype=torch.float64, device=X.device)
    t = GY * xh
    d_t = GY.abs() * d_xh
    d_t = _rounded(d_t, t, GY.abs() * (xh.abs() + d_xh))
    out["dgamma"] = (g0 + t.sum(0), _sum_err(t, d_t, 0, g0))
    return out


WORST = {}        # output name -> worst err / bound seen by check() (the GPU matrix reports it)


def check(got: dict, ref: dict, dtypes: dict, what: str = "", sums=SUMS):
    """assert_within for every entry of ``got`` against its (value, δ) in ``ref``.  The fp32 column sums named in
    ``sums`` (dgamma, dbeta, colsum) must also have a bound that is not vacuous: median bound / |ref| <= 2^-7, as
    gemm_reference.check asks of the GEMM column sums.  Keeps the worst err / bound of every output in WORST."""
    for name, t in got.items():
        v, d = ref[name]
        dt = dtypes.get(name, t.dtype)
        bnd = bound(v, d, dt)
        fin = torch.isfinite(v)
        ratio = torch.where(fin, (t.double() - v).abs() / bnd.clamp(min=1e-300), torch.zeros_like(v))
        if ratio.numel():
            r = float(ratio.max())
            WORST[name] = max(WORST.get(name, 0.0), r if r == r else float("inf"))
        assert_within(t, v, bnd, what=f"{what} {name}", dtype=dt, median_limit=2.0 ** -7 if name in sums else None)


# ------------------------------------------------------------------------------------------------ the matrix
# (dtype, D) of tests/test_layernorm_routes_gpu.py; tests/test_layernorm_reference_cpu.py proves the bounds at each
FWD_DIMS = {torch.bfloat16: (8, 72, 128, 520, 768, 776, 1024, 3072, 4096), torch.float32: (4, 132, 768, 1024, 1536, 2048)}
BWD_DIMS = {torch.bfloat16: (128, 256, 512, 768, 776, 1024, 3072, 4096), torch.float32: (128, 768, 1536, 2048)}
FORMS = tuple(range(8))      # bit 2: the dropped copy, bit 1: the column sums, bit 0: the residual gradient
P_DROP = 0.4


def vector_width(dtype, D):
    """Elements per vector a lane holds (csrc/layernorm.hip ln_row_layout): 8-byte vectors for bf16 rows of 768."""
    return 4 if (dtype == torch.float32 or D == 768) else 8


def operands(rows, D, dtype, seed, device="cpu", int_dy=False, x_scale=2.0):
    """x, gamma, beta, dy, add and the starting dgamma / dbeta / colsum of one case, from the generator of gemm_reference."""
    o = {"x": gen((rows, D), seed + 1, x_scale, dtype, device),
         "gamma": (1.0 + 0.25 * gen((D,), seed + 2, 1.0, torch.float32, device)).to(dtype),
         "beta": gen((D,), seed + 3, 0.5, dtype, device),
         "dy": gen_int((rows, D), seed + 4, 3, dtype, device) if int_dy else gen((rows, D), seed + 4, 1.0, dtype, device),
         "add": gen((rows, D), seed + 5, 1.0, dtype, device)}
    for i, n in enumerate(SUMS):
        o[n + "0"] = gen_int((D,), seed + 6 + i, 9, torch.float32, device) if int_dy else gen((D,), seed + 6 + i, 3.0, torch.float32, device)
    return o


def far_mean_row(D, dtype, seed, device="cpu"):
    """A row of mean 1000 and spread 1, as far as ``dtype`` can hold one, on a granule that keeps its fp32 sums exact:
    fp32 1000 + k / 16 with k in [-16, 16]; bf16, whose spacing at 1000 is 4, 1000 + 4 k with k in [-1, 1]."""
    if dtype == torch.float32:
        return 1000.0 + gen_int((D,), seed + 50, 16, torch.float32, device) / 16.0
    return (1000.0 + 4.0 * gen_int((D,), seed + 50, 1, torch.float32, device)).to(dtype)


def largest_scale(D):
    """The largest power of two S such that rows of |x| <= 2 S keep Σ (x - mean)² <= D (4 S)² below 2^128 in any order."""
    s = 0
    while D * 16.0 * 4.0 ** (s + 1) < 2.0 ** 128:
        s += 1
    return 2.0 ** s
