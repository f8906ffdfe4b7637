"""fp64 references and per-element error bounds for the epilogue forms of the adapter up-projection (include/mdt_hip.h:
mdt_lora_up_add_drop, mdt_lora_up_add_mul, mdt_lora_up_act) and the adapter pipelines of the three dense sites of a block
(attention output projection, fc1, fc2).  Pure torch: no device, no native library.  Builds on tests/lora_reference.py (same
conventions: every function returns (value, δ), δ bounding the fp32 arithmetic error before the one rounding to the stored type)
and tests/activation_reference.py (the five activation kinds and their measured constants).

Error model (lora_reference's).  p = Σ_k t w over n terms in fp32: |p̂ - p| <= γ_n S, S = Σ|t||w|.  Each further fp32 operation
adds u = 2^-24 times what it rounds:
  up_add_drop   Y + fl(alpha s) p̂   the product alpha s is rounded (u |alpha s p|), the FMA with Y rounds once (u (|v| + δ)).
                A dropped element (s = 0) is not written: exact, the old bits.
  up_add_mul    Y + fl(alpha p̂) aux  the product alpha p̂ is rounded (u |alpha p aux|), then the FMA.
  up_act        v = fl(pre + alpha p̂) (an FMA: u (|v| + δ)), not stored.  h = act(v) s and u = act'(v) s then carry
                  (a) activation_reference's own arithmetic bound for the kind, evaluated at v, and
                  (b) the error δ_v of v carried through the function: at most L1 δ_v s for h and L2 δ_v s for u, with
                      L1 = sup |act'| and L2 = sup |act''| of the kind (mean value theorem; LIPSCHITZ computes both suprema on a
                      fine fp64 grid and adds 1 %).  ReLU's derivative jumps at 0: where |v| <= δ_v either value (0 or s) is
                      right, so δ_u = s there and 0 elsewhere; LINEAR's u = s is exact.
With integer operands, a power-of-two alpha and p = 0.5 (scale 2) every operation of the two add forms is exact and δ = 0.
"""
from __future__ import annotations

import numpy as np
import torch

import tests.activation_reference as AR
import tests.gemm_reference as GR
from tests.lora_reference import F24, U32, Guarded, _gamma, _integral, _pow2, assert_within, bound, gen, gen_int, stored, up_add  # noqa: F401
from tests.lora_reference import down, wgrad
from tests.rowops_reference import TANH_REL

KINDS = ("gelu", "relu", "gelu_accurate", "tanh", "linear")


def scale_of(keep: torch.Tensor, p: float, R: int, N: int) -> torch.Tensor:
    """fp64 [R, N] dropout scale from the keep bytes of counters 0 ... R N - 1 (ops.dropout_mask, or GR.keep_bits on the CPU):
    0 or fp32(1 / (1 - p)); all ones at p = 0."""
    if p == 0.0:
        return torch.ones(R, N, dtype=torch.float64)
    return keep.reshape(R, N).cpu().double() * GR.drop_params(p)[1]


def cpu_scale(R: int, N: int, p: float, seed: int) -> torch.Tensor:
    return AR.drop_scale(R, N, p, seed)


def _lipschitz():
    x = torch.linspace(-12.0, 12.0, 480_001, dtype=torch.float64)
    out = {}
    for k in KINDS:
        d1 = AR.act_grad(k, x)
        d2 = (d1[1:] - d1[:-1]) / (x[1] - x[0])
        out[k] = (1.01 * float(d1.abs().max()), 1.01 * float(d2.abs().max()) if k not in ("relu", "linear") else 0.0)
    return out


LIPSCHITZ = _lipschitz()     # {kind: (sup |act'|, sup |act''|) + 1 %}; relu's second entry is unused (its jump is handled apart)


def _products(t, w):
    T, W = t.double(), w.double()
    return T @ W, T.abs() @ W.abs(), T.shape[1]


def up_add_drop(t, w, y_old, alpha, scale):
    """mdt_lora_up_add_drop: Y = Y_old + (alpha s) (T W) where s != 0, Y_old (its bits) where s = 0.  ``scale``: fp64 [R, N]."""
    acc, S, n = _products(t, w)
    Y = y_old.double()
    al = float(np.float32(alpha))
    keep = scale != 0
    v = torch.where(keep, Y + al * scale * acc, Y)
    smax = float(scale.max()) if scale.numel() else 1.0
    exact = (_integral(t.double()) and _integral(w.double()) and _integral(Y) and _pow2(al) and _pow2(smax if smax else 1.0)
             and float((abs(al) * scale * S + Y.abs()).max()) / min(abs(al), 1.0) < F24)
    if exact:
        return v, torch.zeros_like(v)
    d = _gamma(n) * abs(al) * scale * S + U32 * (al * scale * acc).abs()
    d = d + U32 * (v.abs() + d)
    return v, torch.where(keep, d, torch.zeros_like(d))


def up_add_mul(t, w, y_old, aux, alpha):
    """mdt_lora_up_add_mul: Y = Y_old + (alpha (T W)) aux."""
    acc, S, n = _products(t, w)
    Y, A = y_old.double(), aux.double()
    al = float(np.float32(alpha))
    v = Y + al * acc * A
    exact = (_integral(t.double()) and _integral(w.double()) and _integral(Y) and _integral(A) and _pow2(al)
             and float((abs(al) * S * A.abs() + Y.abs()).max()) / min(abs(al), 1.0) < F24)
    if exact:
        return v, torch.zeros_like(v)
    d = _gamma(n) * abs(al) * S * A.abs() + U32 * (al * acc * A).abs()
    return v, d + U32 * (v.abs() + d)


def pre_sum(t, w, pre, alpha):
    """v = pre + alpha (T W) of mdt_lora_up_act and the bound δ_v of its fp32 value."""
    acc, S, n = _products(t, w)
    al = float(np.float32(alpha))
    v = pre.double() + al * acc
    d = _gamma(n) * abs(al) * S
    return v, d + U32 * (v.abs() + d)


def up_act(kind, t, w, pre, alpha, scale):
    """mdt_lora_up_act: {"h": (value, δ), "u": (value, δ)} with v = pre + alpha (T W), h = act(v) s, u = act'(v) s."""
    kind = AR.canonical(kind)
    v, dv = pre_sum(t, w, pre, alpha)
    s = scale
    h, u = AR.act(kind, v) * s, AR.act_grad(kind, v) * s
    l1, l2 = LIPSCHITZ[kind]
    if kind == "linear":
        dh, du = dv * s + U32 * (h.abs() + dv * s), torch.zeros_like(u)
    elif kind == "relu":
        dh = dv * s + U32 * (h.abs() + dv * s)
        du = torch.where(v.abs() <= dv, s, torch.zeros_like(s))
    elif kind == "tanh":
        tt = torch.tanh(v)
        q = tt * tt
        dh = (TANH_REL + U32) * tt.abs() * s
        dq = 2.0 * TANH_REL * q + U32 * q
        du = (dq + U32 * (1.0 - q).abs()) * s + U32 * u.abs()
    else:
        sh, su = AR.sensitivity(kind, v, s)
        k = AR.K_GELU if kind == "gelu" else AR.K_GELU_ACCURATE
        dh, du = k * U32 * sh, k * U32 * su
    if kind not in ("linear", "relu"):
        dh, du = dh + l1 * dv * s * (1.0 + 2.0 * U32), du + l2 * dv * s * (1.0 + 2.0 * U32)
    return {"h": (h, dh), "u": (u, du)}


# ------------------------------------------------------------------------------------------------ the three sites
def dense_site(x, W, b, A, Bt, s, res, scale, g, dtype=torch.float64, u=None, slab=1024):
    """An adapted dense layer with a fused dropout + residual epilogue (the attention output projection, fc2) as the engine
    composes it, in fp64 with roundings to ``dtype`` exactly where the engine stores: the GEMM outputs, t and dt.
        forward   t = x A^T;  y = [res + m (x W^T + b)] + (s m) (t Bt)            (m = ``scale``, the hidden-dropout scale)
        backward  gd = g m;  dBt = s t^T gd;  dt = s gd Bt^T;  dA = dt^T x;  dx = gd W + dt A
    ``u`` (fc2): the input gradient is never materialised, dx = (gd W) u + (dt A) u — the gradient of fc1's pre-activation.
    x [R, K], W [N, K], b [N], A [r, K], Bt [r, N], res, scale, g [R, N].  → dict of fp64 tensors."""
    X, Wd = x.double(), W.double()
    s = float(np.float32(s))
    t = stored(down(x, A)[0], dtype)
    base = stored(res.double() + scale * (X @ Wd.t() + b.double()), dtype)
    y = stored(up_add_drop(t, Bt, base, s, scale)[0], dtype)
    gd = stored(g.double() * scale, dtype)
    dBt = wgrad(t, gd, torch.zeros_like(Bt, dtype=torch.float64), s, slab)[0]
    dt = stored(down(gd, Bt, s)[0], dtype)
    dA = wgrad(dt, X, torch.zeros_like(A, dtype=torch.float64), 1.0, slab)[0]
    if u is None:
        dx = up_add(dt, A, stored(gd @ Wd, dtype), 1.0)[0]
    else:
        dx = up_add_mul(dt, A, stored((gd @ Wd) * u.double(), dtype), u, 1.0)[0]
    return {"t": t, "y": y, "gd": gd, "dBt": dBt, "dt": dt, "dA": dA, "dx": stored(dx, dtype), "dW": gd.t() @ X, "db": gd.sum(0)}


def fc1_site(kind, x, W, b, A, Bt, s, scale, dtype=torch.float64, slab=1024):
    """The adapted fc1, forward: pre = x W^T + b (stored), t = x A^T (stored), v = pre + s t Bt, h = act(v) m, u = act'(v) m
    (m = ``scale``, the activation-dropout scale).  → dict; fc1_site_bwd takes it on."""
    pre = stored(x.double() @ W.double().t() + b.double(), dtype)
    t = stored(down(x, A)[0], dtype)
    r = up_act(kind, t, Bt, pre, float(np.float32(s)), scale)
    return {"pre": pre, "t": t, "h": stored(r["h"][0], dtype), "u": stored(r["u"][0], dtype)}


def fc1_site_bwd(fwd, x, W, A, Bt, s, du, dtype=torch.float64, slab=1024):
    """... and backward from du, the gradient of the pre-activation sum v: dBt = s t^T du, dt = s du Bt^T, dA = dt^T x,
    dx = du W + dt A."""
    s = float(np.float32(s))
    D = du.double()
    dBt = wgrad(fwd["t"], D, torch.zeros_like(Bt, dtype=torch.float64), s, slab)[0]
    dt = stored(down(D, Bt, s)[0], dtype)
    dA = wgrad(dt, x.double(), torch.zeros_like(A, dtype=torch.float64), 1.0, slab)[0]
    dx = up_add(dt, A, stored(D @ W.double(), dtype), 1.0)[0]
    return {"dBt": dBt, "dt": dt, "dA": dA, "dx": stored(dx, dtype), "dW": D.t() @ x.double(), "db": D.sum(0)}


def pipeline(kind, x, P, s, m_act, m_hid, g, dtype=torch.float64):
    """The adapted FFN y = x + m_hid (fc2(h) + s (h A2^T) Bt2), h = act(fc1(x) + s (x A1^T) Bt1) m_act, forward and backward from
    g = dL/dy, composed of fc1_site and dense_site.  ``P``: dict with W1 [F, D], b1, A1 [r, D], Bt1 [r, F], W2 [D, F], b2,
    A2 [r, F], Bt2 [r, D].  → {"fc1": ..., "fc2": ..., "y", "dx"} (dx includes the residual's share)."""
    f1 = fc1_site(kind, x, P["W1"], P["b1"], P["A1"], P["Bt1"], s, m_act, dtype)
    f2 = dense_site(f1["h"], P["W2"], P["b2"], P["A2"], P["Bt2"], s, x, m_hid, g, dtype, u=f1["u"])
    b1 = fc1_site_bwd(f1, x, P["W1"], P["A1"], P["Bt1"], s, f2["dx"], dtype)
    return {"fc1": {**f1, **b1}, "fc2": f2, "y": f2["y"], "dx": g.double() + b1["dx"]}
