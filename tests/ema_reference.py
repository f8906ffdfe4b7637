"""fp64 reference and per-element error bound of the weight average the `_ema` forms of the Adam step keep (csrc/optim.hip,
include/mdt_hip.h: mdt_adam_step_ema and its three siblings), and the inputs of tests/test_ema_gpu.py.  Pure torch: no device,
no native library.  The Adam arithmetic itself is tests/loss_optim_reference.py's reference_adam(); nothing of it is restated.

One update of one element, as the kernel does it after the fresh parameter value p (the value stored to the master, or to the
fp32 parameter where there is no master) is final:

    e' = d e + (1.0f - d) p        d = the float the ABI receives, 1.0f - d ONE fp32 subtraction in the kernel

The reference takes its operands AS STORED: e and p as fp32 tensors, d as f32v(d), ``1.0f - d`` as the fp32 difference omd (exact
for d >= 0.5 by Sterbenz' lemma, one rounding below; either way it is the number the kernel multiplies with, so it carries no δ —
a host that formed 1 - d in double and rounded that would multiply with ANOTHER number, which the CPU test shows at d = 0.9999).
It returns (fp64 value, δ): δ bounds the fp32 arithmetic error before the one rounding to fp32 that tests/gemm_reference.py
bound() adds (half an ulp of |value| + δ).

The error model, u = 2^-24 (tests/loss_optim_reference.py).  The build uses -ffp-contract=off, but no bound here may depend on it, so
δ is the union of the evaluation orders a compiler may choose around the fp64 value d e + omd p:

    two products, one sum      rn(rn(d e) + rn(omd p))            δ = u |d e| + u |omd p|   (a product that is an fp32 number adds 0)
    fma(d, e, rn(omd p))       one product rounded, one fused     δ = u |omd p|
    fma(omd, p, rn(d e))       the other one                      δ = u |d e|

The first contains the other two, so δ = δ1 + δ2 with δ1 = u |d e| (0 where d e is an fp32 number, e.g. e = 0) and δ2 likewise: the
union, written out, not an ulp count.  An incoming error dp of p (reference_adam's δ, where p is not taken from the stored master)
enters as omd dp.

Exact cases:
    d = 0            e' = p bit for bit: the kernel stores p itself (0 * e + 1 * p would turn p = -0 into +0 and a non-finite e into NaN)
    skipped update   (guard skip) nothing is stored: e' = e bit for bit
    p == e           value = (d + omd) e, which is e where omd is exact: e is met within the bound of one update, no more
"""
from __future__ import annotations

import numpy as np
import torch

import tests.loss_optim_reference as R
from tests.loss_optim_reference import U32, _rounded, bound, f32, f32v, f64  # noqa: F401


def one_minus(d):
    """``1.0f - d`` as the kernel forms it: one fp32 subtraction of the float the ABI receives."""
    return float(np.float32(1.0) - np.float32(d))


def reference_ema(e, p, d, dp=None, skip=False):
    """(fp64 value, δ) of the stored average after one update of the stored fp32 ``e`` with the stored fp32 ``p`` (or an fp64 value
    ``p`` with error ``dp``) and decay ``d``; ``skip``: the update was skipped by the guard."""
    E, P = e.double(), p.double()
    zero = torch.zeros_like(E)
    dp = zero if dp is None else dp
    if skip:
        return E, zero
    d32, omd = f32v(d), one_minus(d)
    if d32 == 0.0:
        return P, dp
    t1 = d32 * E
    d1 = _rounded(zero, t1, t1.abs())
    t2 = omd * P
    d2 = _rounded(omd * dp, t2, t2.abs() + omd * dp)
    unfused, fma_first, fma_second = d1 + d2, d2, d1
    return t1 + t2, torch.maximum(unfused, torch.maximum(fma_first, fma_second))


def reference_adam_ema(p0, grad, m0, v0, e0, hyp, step, d, gs=None, guard=None):
    """The Adam reference of tests/loss_optim_reference.py chained into the average: {"m", "v", "p", "ema"} of (value, δ)."""
    ref = R.reference_adam(p0, grad, m0, v0, hyp["lr"], hyp["beta1"], hyp["beta2"], hyp["eps"], hyp["wd"], step, gs, guard)
    skip = bool(guard is not None and guard["skip"])
    pv, pd = ref["p"]
    # the kernel feeds the average the STORED p: its storage rounding is part of what comes in
    ref["ema"] = reference_ema(e0, pv, d, dp=None if skip else bound(pv, pd, f32), skip=skip)
    return ref


def reference_recurrence(e0, snapshots, decays):
    """The average after a run: ``snapshots[k]`` the stored fp32 weights after update k, ``decays[k]`` the decay update k ran its
    `_ema` launch with, or None where the average was left alone (a plain launch, or a skipped update).  (fp64 value, δ): the
    storage rounding of every update but the last has become incoming error of the next."""
    E = e0.double()
    dE = torch.zeros_like(E)
    delta = torch.zeros_like(E)
    for p, d in zip(snapshots, decays):
        if d is None:
            continue
        P = p.double()
        d32, omd = f32v(d), one_minus(d)
        if d32 == 0.0:
            E, dE, delta = P, torch.zeros_like(P), torch.zeros_like(P)
            continue
        t1 = d32 * E
        d1 = _rounded(d32 * dE, t1, t1.abs() + d32 * dE)
        t2 = omd * P
        d2 = _rounded(torch.zeros_like(P), t2, t2.abs())
        E, delta = t1 + t2, d1 + d2
        dE = bound(E, delta, f32)
    return E, delta


def check_not_vacuous(e, p, ref, what=""):
    """The bound must tell e' apart from both of its inputs' neighbourhood: it is narrower than the distance between e and p at
    every element (inputs with e == p somewhere are for the p == e case alone and do not come here)."""
    v, dl = ref
    b = bound(v, dl, f32)
    dist = (e.double() - p.double()).abs()
    bad = int((b >= dist).sum())
    assert bad == 0, f"{what}: vacuous — the bound is at least |e - p| at {bad} of {b.numel()} elements"


def check(got, ref, what=""):
    R.check("ema", got, ref, what, dtype=f32)


# ------------------------------------------------------------------------------------------------ the matrix
SEED = 9173
EMA_NUMELS = (1, 4095, 4096, 4097, 3 * 4096 + 5)        # one table: the binary search over five tensors and the chunk tails
EMA_NULL = 2                                            # the tensor of the table whose EMA entry is NULL
EMA_OFFSET = 3                                          # the tensor whose EMA view starts 4 bytes past a 16-byte boundary
EMA_DECAYS = (0.9, 0.9999, 0.3, 0.0)                    # 0.3: 1.0f - d rounds; 0.9999: double and float 1 - d differ; 0: the copy
EMA_BIG_TENSORS = 65540                                 # one-element tensors: more chunks than the launch's grid of 65 536


def ema_inputs(n, seed):
    """(p0, grad, m0, v0, e0) fp32 [n]: adam_inputs of tests/loss_optim_reference.py and an average that is p0 moved by 5 % to 45 %
    either way — never equal to p0 or to the updated p — with exact zeros (d e is then exact, and e' = omd p shows what omd was)
    every 11th element and a value 2^-20 of p0 every 13th."""
    p0, grad, m0, v0 = R.adam_inputs(n, seed)
    gen = torch.Generator().manual_seed(seed + 77)
    r = (torch.rand(n, generator=gen) * 0.4 + 0.05) * R._signs(n, gen)
    e0 = p0 * (1.0 + r)
    i = torch.arange(n)
    e0[i % 13 == 6] = p0[i % 13 == 6] * 2.0 ** -20
    e0[i % 11 == 5] = 0.0
    return p0, grad, m0, v0, e0
