"""fp64 reference and per-output error bounds for mdt_node_objective (csrc/node_objective.hip; include/mdt_hip.h), the
label-smoothed / focal objective of the two-class node classifier, in the conventions of tests/loss_optim_reference.py: operands
AS STORED, hyper-parameters as the fp32 numbers the ABI receives, (fp64 value, δ) per output element with δ the bound of the fp32
arithmetic error before the one rounding to the storage type (check() adds half an ulp of |value| + δ).  Pure torch.

Arithmetic of one labelled row (the kernel's stated order; y the target, o = 1 - y; eps, gamma, w the fp32 numbers):
    fp16_loss = 1: l_0, l_1, w_0, w_1 are rounded to fp16 first — an exact operation the reference repeats, everything after it
    is fp32 for either setting (no half rounding in between, no half cascade)
    m = max(l);  a_c = l_c - m;  e_c = expf(a_c);  ls = logf(e_0 + e_1);  lp_c = a_c - ls
    q = expf(lp_y);  r = expf(lp_o);  nll = -(w_y lp_y);  f = expf(gamma lp_o)
    loss = (1 - eps) (f nll) + (eps / 2) (nll - w_o lp_o)              1 - eps is one fp32 subtraction, eps / 2 is exact
    A = (1 - eps) (w_y (f (r - (gamma q) lp_y)));  sw = w_0 + w_1
    g_o = A + (eps / 2) (sw r - w_o);  g_y = -A + (eps / 2) (sw q - w_y);  d logits = T(g grad_scale)
    out[0] = Σ loss, out[1] = Σ nll: thread t adds its rows t, t + 256, ... in turn, thread 0 adds the 256 partial sums in turn.

Error model: that of tests/loss_optim_reference.py (u = 2^-24, one rounding per fp32 operation through _rounded, a power-of-two
or absent grad_scale exact through _mul_scale, γ_depth for the two sums with depth = ceil(n / 256) + 256), with its measured
constants EXPF_REL and LOGF_REL.  An exponential of an argument x that carries the absolute error d is off by
exp(x) expm1(d) + EXPF_REL exp(x + d).  The log-softmax part is derived as reference_node_ce_f32 derives it.  Products by 0
(eps = 0, gamma = 0) are exact zeros and carry nothing: at gamma = 0 the argument of f is 0 and expf(0) = 1 exactly
(tools/probes/libm_probe.hip), so f = 1 with δ = 0.

The denormal floor.  f = expf(gamma lp_o) is the one exponential whose argument is not bounded by the logits alone: it goes down
to gamma lp_o (-300 for logits (30, -30) at gamma = 5).  Below about -87.3 the result is a denormal or 0 and a relative bound
means nothing: δ(f) carries an ABSOLUTE floor of one fp32 denormal step, 2^-149 (DENORM), whenever gamma != 0 — the kernel's
result there is 0 or a denormal within one step of the exact value, whether the device flushes or not.  EXPF_REL was measured
on (-64, 0] (docs/experiment_log.md); the reference refuses a case in which an exponential's argument lies in [-104, -64), where
the result is a number the measurement did not reach and the floor does not cover (no constant was added for it; no case of the
matrix needs one).  Below -104 the exact value is under half a denormal step and the floor alone is the bound.

Counters: for fp16_loss = 0 they are exact where the margin min |l_1 - l_0| is positive (pred = l_1 > l_0).  For fp16_loss = 1
the prediction compares half-rounded softmax values (ties to index 0); the reference emulates that in fp32, which a knife-edge
rounding can move, so the GPU test takes mdt_node_ce's counters on the same logits as the judge (they must be equal integers).
"""
from __future__ import annotations

import numpy as np
import torch

from tests.loss_optim_reference import EXPF_REL, LOGF_REL, U32, _gamma, _mul_scale, _rounded, check, f32v  # noqa: F401

bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64
DENORM = 2.0 ** -149                  # one fp32 denormal step
EXP_MEASURED_FROM = -64.0             # EXPF_REL holds on (-64, 0]
EXP_ZERO_BELOW = -104.0               # exp(x) < 2^-150 for x < -103.98: 0 or one denormal step


def _exp(x, d, floor=False):
    """(exp(x), δ) for an argument carrying the absolute error d; expf(0) = 1 exactly where nothing came in."""
    lo = x - d
    assert not bool(((lo < EXP_MEASURED_FROM) & (x + d >= EXP_ZERO_BELOW)).any()), \
        "node objective reference: an expf argument in [-104, -64), outside the range EXPF_REL was measured on"
    v = torch.exp(x)
    dv = v * torch.expm1(d) + EXPF_REL * torch.exp(x + d)
    dv = torch.where((x == 0) & (d == 0), torch.zeros_like(dv), dv)
    if floor:
        dv = dv + DENORM
    return v, dv


def _mul(a, da, b, db=None):
    """(a b, δ) after one fp32 multiplication; b exact where db is None."""
    v = a * b
    if db is None:
        d = da * b.abs()
    else:
        d = a.abs() * db + b.abs() * da + da * db
    exact_zero = ((a == 0) & (da == 0)) | ((b == 0) & (db is None or (db == 0)))
    return v, torch.where(exact_zero, torch.zeros_like(d), _rounded(d, v, v.abs() + d))


def _add(a, da, b, db):
    v = a + b
    d = da + db
    return v, _rounded(d, v, v.abs() + d)


def reference_node_objective(logits, rows, targets, w_neg, w_pos, label_smoothing, focal_gamma, fp16_loss=0, grad_scale=1.0):
    """{"out": (value [2], δ): objective and plain weighted NLL, "dlogits": (value [M, 2], δ), "counters": [4], "margin":
    min |l1 - l0| over the labelled rows (of the logits as the kernel uses them)} from the stored logits [M, 2] (fp32 or bf16)."""
    M = logits.shape[0]
    rr, y = rows.long(), targets.long()
    n = int(y.numel())
    lf = logits.float()
    wn, wp = np.float32(w_neg), np.float32(w_pos)
    if fp16_loss:
        lf = lf.half().float()
        wn, wp = np.float32(np.float16(wn)), np.float32(np.float16(wp))
    wn, wp = float(wn), float(wp)
    eps32, gam = np.float32(label_smoothing), float(np.float32(focal_gamma))
    ome, he = 1.0 - float(eps32), float(eps32) * 0.5          # the kernel's 1.0f - eps is one rounding away from 1 - eps
    dome = 0.0 if float(np.float32(1.0) - eps32) == ome else U32 * ome
    l = lf.double()[rr]
    zero = torch.zeros_like(l)
    z1 = zero[:, 0]
    # ---- log-softmax (as reference_node_ce_f32)
    mx = l.max(1, keepdim=True).values
    a = l - mx
    da = _rounded(zero, a, a.abs())
    e, de = _exp(a, da)
    S = e.sum(1, keepdim=True)
    dS = de.sum(1, keepdim=True)
    dS = dS + U32 * (S + dS)
    ls = torch.log(S)
    dls = dS / (S - dS) + LOGF_REL * ls.abs()
    lp = a - ls
    dlp = da + dls
    dlp = dlp + U32 * (lp.abs() + dlp)
    yi, oi = y[:, None], (1 - y)[:, None]
    lpy, dlpy = lp.gather(1, yi)[:, 0], dlp.gather(1, yi)[:, 0]
    lpo, dlpo = lp.gather(1, oi)[:, 0], dlp.gather(1, oi)[:, 0]
    wy = torch.where(y == 1, torch.full_like(z1, wp), torch.full_like(z1, wn))
    wo = torch.where(y == 1, torch.full_like(z1, wn), torch.full_like(z1, wp))
    gam_t, ome_t, he_t = torch.full_like(z1, gam), torch.full_like(z1, ome), torch.full_like(z1, he)
    dome_t = torch.full_like(z1, dome)
    # ---- row terms
    ty, dty = _mul(lpy, dlpy, wy)                         # w_y lp_y; nll = -ty
    nll, dnll = -ty, dty
    arg, darg = _mul(lpo, dlpo, gam_t)
    f, df = _exp(arg, darg, floor=gam != 0.0)
    h1, dh1 = _mul(f, df, nll, dnll)
    h2, dh2 = _mul(h1, dh1, ome_t, dome_t)
    to, dto = _mul(lpo, dlpo, wo)
    s, ds = _add(nll, dnll, -to, dto)
    sm, dsm = _mul(s, ds, he_t)
    li, dli = _add(h2, dh2, sm, dsm)
    depth = (n + 255) // 256 + 256

    def total(v, d):
        if not n:
            return torch.zeros((), dtype=f64), torch.zeros((), dtype=f64)
        return v.sum(), d.sum() + _gamma(depth) * (v.abs() + d).sum()

    L, dL = total(li, dli)
    N, dN = total(nll, dnll)
    out = (torch.stack([L, N]), torch.stack([dL, dN]))
    # ---- gradient
    q, dq = _exp(lpy, dlpy)
    r, dr = _exp(lpo, dlpo)
    g1, dg1 = _mul(q, dq, gam_t)
    g2, dg2 = _mul(g1, dg1, lpy, dlpy)
    g3, dg3 = _add(r, dr, -g2, dg2)
    g4, dg4 = _mul(f, df, g3, dg3)
    g5, dg5 = _mul(g4, dg4, wy)
    A, dA = _mul(g5, dg5, ome_t, dome_t)
    sw = torch.full_like(z1, wn + wp)
    dsw = torch.zeros_like(z1) if float(np.float32(wn + wp)) == wn + wp else U32 * sw

    def smooth(p, dp, w):
        u, du = _mul(p, dp, sw, dsw)
        v, dv = _add(u, du, -w, torch.zeros_like(w))
        return _mul(v, dv, he_t)

    so, dso = smooth(r, dr, wo)
    sy, dsy = smooth(q, dq, wy)
    go, dgo = _add(A, dA, so, dso)
    gy, dgy = _add(-A, dA, sy, dsy)
    gs = f32v(grad_scale)
    go, dgo = _mul_scale(go, dgo, None if gs == 1.0 else gs)
    gy, dgy = _mul_scale(gy, dgy, None if gs == 1.0 else gs)
    g, dg = torch.zeros(n, 2, dtype=f64), torch.zeros(n, 2, dtype=f64)
    if n:
        g.scatter_(1, yi, gy[:, None]).scatter_(1, oi, go[:, None])
        dg.scatter_(1, yi, dgy[:, None]).scatter_(1, oi, dgo[:, None])
    V, D = torch.zeros(M, 2, dtype=f64), torch.zeros(M, 2, dtype=f64)
    V[rr], D[rr] = g, dg
    # ---- counters
    if fp16_loss:
        l32 = lf[rr]
        e32 = torch.exp(l32 - l32.max(1, keepdim=True).values)
        inv = 1.0 / (e32[:, :1] + e32[:, 1:])
        hp = (e32 * inv).half()
        pred = (hp[:, 1] > hp[:, 0]).long()
    else:
        pred = (l[:, 1] > l[:, 0]).long()
    counters = [int((pred == y).sum()), int(((pred == y) & (pred == 1)).sum()), int((y == 1).sum()), int((pred == 1).sum())]
    margin = float((l[:, 1] - l[:, 0]).abs().min()) if n else float("inf")
    return {"out": out, "dlogits": (V, D), "counters": counters, "margin": margin}


# ------------------------------------------------------------------------------------------------ the matrix
SEED = 9931
SETTINGS = ((0.0, 0.0), (0.1, 0.0), (0.0, 2.0), (0.1, 2.0), (0.25, 0.5), (0.0, 5.0))      # (label_smoothing, focal_gamma)
SCALES = (1.0, 1.0 / 7.0)
WEIGHTS = (1.0, 1.5)                                                                    # (negative, positive)
NLAB = (0, 1, 255, 256, 257, 1031)      # the chunk boundaries of the kernel's 256-thread walk and one ragged multi-chunk case
FIXED_ROWS = ((30.0, -30.0), (-30.0, 30.0), (0.0, 0.0), (1.25, 1.25), (-2.5, -2.5), (0.5, 0.5 + 2.0 ** -7))


def inputs(nlab, dtype, seed=SEED):
    """(logits [nlab + 5, 2] of ``dtype`` drawn in +-4, rows int32 [nlab]: a shuffled subset, targets int32 [nlab]).  From
    nlab = 255 on, the first labelled rows hold FIXED_ROWS twice over, once per target: saturated rows both ways round, exact
    ties and a near-tie (2^-7: a number of every storage type, and of fp16)."""
    gen = torch.Generator().manual_seed(seed + nlab)
    M = nlab + 5
    l = (torch.rand(M, 2, generator=gen) * 8 - 4)
    rows = torch.randperm(M, generator=gen)[:nlab].to(torch.int32)
    y = (torch.rand(nlab, generator=gen) < 0.4).to(torch.int32)
    if nlab >= 2 * len(FIXED_ROWS):
        for k, fr in enumerate(FIXED_ROWS + FIXED_ROWS):
            l[int(rows[k])] = torch.tensor(fr)
            y[k] = k // len(FIXED_ROWS)
    return l.to(dtype), rows, y


def matrix():
    """(nlab, dtype, fp16_loss, (eps, gamma), grad_scale): every size, type and fp16_loss with every setting, the two scales
    alternating so that each setting meets both."""
    k = 0
    for nlab in NLAB:
        for dtype in (f32, bf16):
            for fp16_loss in (0, 1):
                for j, st in enumerate(SETTINGS):
                    yield nlab, dtype, fp16_loss, st, SCALES[(j + k) % 2]
                k += 1
