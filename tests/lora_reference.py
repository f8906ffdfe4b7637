"""fp64 reference and per-element error bounds for the low-rank adapter kernels (include/mdt_hip.h "low-rank adapters":
mdt_lora_down, mdt_lora_up_add, mdt_lora_wgrad), pure torch: no device, no native library.  Modelled on tests/gemm_reference.py,
whose ulp() / bound() / assert_within() / Guarded it reuses.

Every function returns (value, δ): the documented result in fp64 from the exact operand values, and a bound δ on the fp32
arithmetic error before the one rounding to the stored type; gemm_reference.bound() adds half an ulp of that type.

The error model (gemm_reference's).  Products of bf16 numbers are exact in fp32; a sum of K terms in fp32 in any order errs by at
most γ_K Σ|a||b|, γ_K = K u / (1 - K u), u = 2^-24 (fp32 operands: the same γ_K covers the rounded products).  The factor
alpha joins by one more fp32 operation (a product in down and wgrad, the FMA with Y in up_add): u times what it rounds.
mdt_lora_wgrad adds ceil(R / SLAB) slab partials and the old dW one after the other: one rounding of the running total per add.

Exact operands.  With integer operands whose Σ|a||b| (plus |old value|) stays below 2^24 and a power-of-two alpha every fp32
operation is exact in any order and δ = 0: the wgrad cases use such operands (int_operands), so a missing 16-row step or a missing
slab cannot hide inside a bound.

Where the pipeline rounds in the middle (t and dt are stored in the working type) the reference takes the STORED tensor as the
next stage's input instead of widening the bound: pipeline() rounds at those two places and nowhere else.
"""
from __future__ import annotations

import numpy as np
import torch

from tests.gemm_reference import F24, U32, Guarded, assert_within, bound, gen, gen_int, ulp  # noqa: F401

TARGET_INDEX = {"q": 0, "k": 1, "v": 2}


def _gamma(n):
    return n * U32 / (1.0 - n * U32)


def _integral(x):
    return bool((x == torch.round(x)).all())


def _pow2(a: float) -> bool:
    m, _ = np.frexp(abs(float(a)))
    return a != 0 and m == 0.5


def _exact(a, b, S, alpha, extra=None):
    """Integer operands, power-of-two alpha, every partial sum (and the old value joining it) below 2^24 in magnitude."""
    if not (_integral(a) and _integral(b) and _pow2(alpha)):
        return False
    tot = abs(alpha) * S if extra is None else abs(alpha) * S + extra.abs()
    if extra is not None and not _integral(extra / min(abs(alpha), 1.0)):
        return False
    return (not S.numel()) or float(tot.max()) / min(abs(alpha), 1.0) < F24


def int_operands(R, n, N, seed=0, dtype=torch.bfloat16, device="cpu"):
    """(t [R, n], x [R, N]) integer-valued in [-2, 2] / [-4, 4]: Σ_r |t||x| <= 8 R stays below 2^24 up to R = 2^21 rows."""
    return gen_int((R, n), 300 + seed, 2, dtype, device), gen_int((R, N), 400 + seed, 4, dtype, device)


def down(x, w, alpha=1.0):
    """mdt_lora_down: T[R, n] = alpha * X[R, K] W[n, K]^T."""
    X, W = x.double(), w.double()
    K = X.shape[1]
    al = float(np.float32(alpha))
    acc = X @ W.t()
    S = X.abs() @ W.abs().t()
    v = al * acc
    if _exact(X, W, S, al):
        return v, torch.zeros_like(v)
    return v, _gamma(K) * abs(al) * S + U32 * abs(al) * (acc.abs() + _gamma(K) * S)


def up_add(t, w, y_old, alpha=1.0):
    """mdt_lora_up_add: Y[R, N] = Y_old + alpha * T[R, n] W[n, N], one rounding of the sum."""
    T, W, Y = t.double(), w.double(), y_old.double()
    n = T.shape[1]
    al = float(np.float32(alpha))
    acc = T @ W
    S = T.abs() @ W.abs()
    v = Y + al * acc
    if _exact(T, W, S, al, Y):
        return v, torch.zeros_like(v)
    d = _gamma(n) * abs(al) * S
    return v, d + U32 * (v.abs() + d)


def wgrad(t, x, dw_old, alpha=1.0, slab=1024):
    """mdt_lora_wgrad: dW[n, N] = dW_old + alpha * T[R, n]^T X[R, N] (fp32), slabs of ``slab`` token rows added in ascending order,
    the old value last."""
    T, X, D0 = t.double(), x.double(), dw_old.double()
    R = T.shape[0]
    al = float(np.float32(alpha))
    acc = T.t() @ X
    S = T.abs().t() @ X.abs()
    v = D0 + al * acc
    if _exact(T, X, S, al, D0):
        return v, torch.zeros_like(v)
    slabs = max((R + slab - 1) // slab, 1)
    d = _gamma(min(R, slab)) * abs(al) * S + U32 * abs(al) * S          # inside the slabs, and alpha times each partial
    d = d + (slabs + 1) * U32 * (abs(al) * S + D0.abs() + d)            # the running total of the slab adds, the old value last
    return v, d


def stored(v, dtype):
    """What the kernel leaves in memory for the fp64 value v (round to nearest even), widened back to fp64."""
    return v.to(dtype).double()


def pipeline(src, A, Bt, s, targets, qkv, dqkv, dx, dtype=torch.float64, slab=1024, dA0=None, dBt0=None):
    """The adapter's forward and its four backward products as the engine composes them from the three entry points, in fp64 with
    the two intermediate roundings to ``dtype`` (t, dt) and no other.  src [R, D]; A, Bt [|J| r, D] target-major; qkv, dqkv
    [R, 3 D]; dx [R, D] (the output of the base projection's input gradient).  Returns a dict of fp64 tensors: t, qkv, dBt, dt,
    dA, dx."""
    D = src.shape[1]
    r = A.shape[0] // len(targets)
    s = float(np.float32(s))
    t = stored(down(src, A)[0], dtype)
    out_qkv = qkv.double().clone()
    dBt = torch.zeros_like(Bt, dtype=torch.float64) if dBt0 is None else dBt0.double().clone()
    dA = torch.zeros_like(A, dtype=torch.float64) if dA0 is None else dA0.double().clone()
    dt = torch.zeros_like(t)
    for j, name in enumerate(targets):
        c = TARGET_INDEX[name] * D
        rows = slice(j * r, (j + 1) * r)
        out_qkv[:, c:c + D] = up_add(t[:, rows], Bt[rows], out_qkv[:, c:c + D], s)[0]
        dBt[rows] = wgrad(t[:, rows], dqkv[:, c:c + D], dBt[rows], s, slab)[0]
        dt[:, rows] = stored(down(dqkv[:, c:c + D], Bt[rows], s)[0], dtype)
    dA = wgrad(dt, src, dA, 1.0, slab)[0]
    out_dx = up_add(dt, A, dx, 1.0)[0]
    return {"t": t, "qkv": out_qkv, "dBt": dBt, "dt": dt, "dA": dA, "dx": out_dx}
