"""fp64 reference and per-element error bounds for mdt_act_fwd (csrc/activation.hip, include/mdt_hip.h), and the oracle's
Graphormer layer with its activation line parametrised.  Pure torch: no device, no native library.

mdt_act_fwd: h = T(act(x) s), u = T(act'(x) s) from the STORED x (fp32 or bf16), s the dropout scale of the element (0 or
fp32(1 / (1 - p)), counter r N + c of the site — tests/gemm_reference.py drop_scale restates the generator), 1 at p = 0.
reference(kind, x, p, seed) returns {"h": (value, δ, exact), "u": (value, δ, exact)}: the fp64 value, a bound δ on the fp32
arithmetic error before the one rounding to T (tests/gemm_reference.py bound(): ½ ulp_T(|value| + δ) + δ, so bf16 adds half
an ulp of the stored value) and ``exact``, the elements whose bits are determined.

The error model, u32 = 2^-24:
  RELU, LINEAR   act / act' are a copy, a zero or a one, and the scale is ONE fp32 multiply, so the stored result is the
                 correctly rounded product: exact everywhere (at p = 0 a copy, a 0 / 1 mask or zeros).
  TANH           t = tanhf(x) with the measured relative bound of tests/rowops_reference.py (TANH_REL, used for mdt_tanh_fwd):
                     h = t s            δ = (ε_t |t| + u32 |t|) s
                     u = (1 - t t) s    δ(t t) = 2 |t| ε_t |t| + u32 t²;  δ(1 - t t) = δ(t t) + u32 |1 - t²|;  times s: + u32 |u|
                 (absolute in t², as for mdt_tanh_bwd: near |t| = 1 the difference cancels).
  GELU, GELU_ACCURATE   the error of the device's erff, tanhf and __expf is stated nowhere, so the bound is composed
                 through the formula as K u32 S(x): S(x) adds up the magnitudes of the formula's terms, each weighted by how an
                 error of that term reaches the result, and K is one constant per function, 4 x the worst err / (u32 S) seen
                 on an MI355X over fp32 inputs (GELU_MEASURED / GELU_ACCURATE_MEASURED; docs/experiment_log.md).
      GELU            h = 0.5 x (1 + e) s, e = erff(x / sqrt 2): an ABSOLUTE error in e reaches h as 0.5 |x| (in the negative tail
                      1 + e cancels), the roundings of the products as |h|:          S_h = (0.5 |x| + |h|) s
                      u = (cdf + x pdf) s, cdf = 0.5 (1 + e), pdf = φ(0) __expf(-x²/2); the exponential's argument is rounded
                      before it is used, a relative error of pdf that grows as x²/2:  S_u = (0.5 + cdf + |x| pdf (1 + x²/2)) s
      GELU_ACCURATE   a = k (x + c x³), t = tanhf(a); an error of a reaches t as (1 - t²) |a| relative to a, tanhf adds |t|:
                      τ = (1 - t²) |a| + |t|.   h = 0.5 x (1 + t) s:               S_h = (0.5 |x| τ + |h|) s
                      u = (0.5 (1 + t) + g (1 - t²)) s, g = 0.5 x k (1 + 3 c x²):  S_u = (0.5 τ + 0.5 |1 + t| + |g| (2 |t| τ + (1 - t²))) s
Non-finite results (x = ±inf, NaN; inf times a dropped element's 0) are not bounded: they must be the same NaN / ±inf.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

import tests.gemm_reference as GR
from tests.gemm_reference import U32, bound  # noqa: F401
from tests.rowops_reference import TANH_REL

KINDS = {"gelu": 0, "relu": 1, "gelu_accurate": 2, "tanh": 3, "linear": 4}
ALIASES = {"gelu_fast": "gelu_accurate"}
K_TANH = math.sqrt(2.0 / math.pi)
C_TANH = 0.044715
PHI0 = 1.0 / math.sqrt(2.0 * math.pi)

# worst err / (u32 S) of an fp32 mdt_act_fwd against fp64 on an MI355X (tests/test_activation_gpu.py prints them; both outputs,
# with and without dropout, every shape of the kernel test), and the constants of the bound: 4 x that
GELU_MEASURED = 1.4084
GELU_ACCURATE_MEASURED = 1.8823
K_GELU = 4.0 * GELU_MEASURED
K_GELU_ACCURATE = 4.0 * GELU_ACCURATE_MEASURED


def canonical(name: str) -> str:
    name = ALIASES.get(name, name)
    if name not in KINDS:
        raise KeyError(name)
    return name


# ------------------------------------------------------------------------------------------------ the functions, any float type
def act(kind: str, x: torch.Tensor) -> torch.Tensor:
    kind = canonical(kind)
    if kind == "gelu":
        return 0.5 * x * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0))))
    if kind == "relu":
        return torch.where(x > 0, x, torch.where(torch.isnan(x), x, torch.zeros_like(x)))
    if kind == "gelu_accurate":
        return 0.5 * x * (1.0 + torch.tanh(K_TANH * (x + C_TANH * (x * x * x))))
    if kind == "tanh":
        return torch.tanh(x)
    return x.clone()


def act_grad(kind: str, x: torch.Tensor) -> torch.Tensor:
    kind = canonical(kind)
    if kind == "gelu":
        return 0.5 * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0)))) + x * (PHI0 * torch.exp(-0.5 * x * x))
    if kind == "relu":
        return (x > 0).to(x.dtype)
    if kind == "gelu_accurate":
        x2 = x * x
        t = torch.tanh(K_TANH * (x + C_TANH * (x2 * x)))
        return 0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * (K_TANH * (1.0 + 3.0 * C_TANH * x2))
    if kind == "tanh":
        t = torch.tanh(x)
        return 1.0 - t * t
    return torch.ones_like(x)


def drop_scale(rows: int, N: int, p: float, seed: int) -> torch.Tensor:
    """fp64 [rows, N]: the scale mdt_act_fwd applies to element (r, c) — 1 at p = 0."""
    if p == 0.0:
        return torch.ones(rows, N, dtype=torch.float64)
    return GR.drop_scale(rows, N, p, seed)


def sensitivity(kind: str, x: torch.Tensor, s: torch.Tensor):
    """(S_h, S_u) of the docstring for the two GELU kinds, fp64."""
    kind = canonical(kind)
    ax = x.abs()
    if kind == "gelu":
        cdf = 0.5 * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0))))
        pdf = PHI0 * torch.exp(-0.5 * x * x)
        return (0.5 * ax + (x * cdf).abs()) * s, (0.5 + cdf + ax * pdf * (1.0 + 0.5 * x * x)) * s
    assert kind == "gelu_accurate"
    x2 = x * x
    a = K_TANH * (x + C_TANH * (x2 * x))
    t = torch.tanh(a)
    omt2 = 1.0 - t * t
    tau = omt2 * a.abs() + t.abs()
    g = 0.5 * x * K_TANH * (1.0 + 3.0 * C_TANH * x2)
    h = 0.5 * x * (1.0 + t)
    return (0.5 * ax * tau + h.abs()) * s, (0.5 * tau + 0.5 * (1.0 + t).abs() + g.abs() * (2.0 * t.abs() * tau + omt2)) * s


def reference(kind: str, x: torch.Tensor, p: float = 0.0, seed: int = 0):
    """{"h": (value, δ, exact), "u": (value, δ, exact)} of mdt_act_fwd on the stored [rows, N] pre-activation ``x``."""
    kind = canonical(kind)
    rows, N = x.shape
    s = drop_scale(rows, N, p, seed)
    if kind in ("relu", "linear"):
        # one fp32 multiply of exact operands: the fp32 product IS the kernel's value before its rounding to T
        x32, s32 = x.float(), s.float()
        a32 = act(kind, x32)
        h = (a32 * s32).double()
        u = (act_grad(kind, x32) * s32).double()
        z = torch.zeros_like(h)
        return {"h": (h, z, torch.ones_like(h, dtype=torch.bool)), "u": (u, z, torch.ones_like(u, dtype=torch.bool))}
    xd = x.double()
    h, u = act(kind, xd) * s, act_grad(kind, xd) * s
    if kind == "tanh":
        t = torch.tanh(xd)
        dh = (TANH_REL + U32) * t.abs() * s
        q = t * t
        dq = 2.0 * TANH_REL * q + U32 * q
        du = (dq + U32 * (1.0 - q).abs()) * s + U32 * u.abs()
    else:
        sh, su = sensitivity(kind, xd, s)
        k = K_GELU if kind == "gelu" else K_GELU_ACCURATE
        dh, du = k * U32 * sh, k * U32 * su
    no = torch.zeros_like(h, dtype=torch.bool)
    return {"h": (h, dh, no), "u": (u, du, no)}


def compare(got: torch.Tensor, ref, dtype=None, what: str = ""):
    """``got`` against one entry (value, δ, exact) of reference(): finite values within bound(value, δ, T), exact ones equal to
    value.to(T), a NaN where the reference has one, the same infinity where it has one.  → worst err / bound over the bounded
    elements."""
    v, d, exact = ref
    dt = dtype or got.dtype
    assert tuple(got.shape) == tuple(v.shape), f"{what}: shape {tuple(got.shape)} against {tuple(v.shape)}"
    g = got.detach().cpu()
    vt = v.to(dt)                                   # what the value becomes in T (RNE)
    nan = torch.isnan(v)
    inf = torch.isinf(vt.double()) & ~nan
    assert bool(torch.isnan(g)[nan].all()), f"{what}: a NaN of the reference is not a NaN"
    assert not bool(torch.isnan(g)[~nan].any()), f"{what}: NaN where the reference is a number"
    assert bool((g[inf] == vt[inf]).all()), f"{what}: an infinity of the reference is not that infinity"
    fin = ~nan & ~inf
    ex = fin & exact
    assert bool((g[ex] == vt[ex]).all()), f"{what}: {int((g[ex] != vt[ex]).sum())} of the exactly determined elements differ"
    bd = fin & ~exact
    if not bool(bd.any()):
        return 0.0
    err = (g.double() - v)[bd].abs()
    bnd = bound(v[bd], d[bd], dt)
    ratio = err / bnd
    worst = float(ratio.max())
    assert worst <= 1.0, f"{what}: {int((ratio > 1).sum())} of {int(bd.sum())} elements over their bound, worst err / bound {worst:.3g}"
    return worst


def measured_constant(kind: str, x: torch.Tensor, h: torch.Tensor, u, p: float = 0.0, seed: int = 0) -> float:
    """worst err / (u32 S) of an fp32 result against fp64 over the finite elements with S > 0: what GELU_MEASURED /
    GELU_ACCURATE_MEASURED record."""
    assert h.dtype == torch.float32
    xd = x.double().cpu()
    s = drop_scale(x.shape[0], x.shape[1], p, seed)
    sh, su = sensitivity(kind, xd, s)
    worst = 0.0
    for got, val, sens in ((h, act(kind, xd) * s, sh), (u, act_grad(kind, xd) * s, su)):
        if got is None:
            continue
        ok = torch.isfinite(val) & torch.isfinite(sens) & (sens > 0)
        # bound() adds the half ulp of the fp32 store on top of δ = K u32 S, so it is taken out of what K has to carry
        err = ((got.detach().cpu().double() - val).abs() - 0.5 * GR.ulp(val, torch.float32)).clamp(min=0.0)
        if bool(ok.any()):
            worst = max(worst, float((err[ok] / (U32 * sens[ok])).max()))
    return worst


# ------------------------------------------------------------------------------------------------ the layer
def graph_layer(x, W, p, nheads, bias, key_padding_mask, pre_ln=False, activation="gelu", act_scale=None):
    """oracle.mdt_ref_cpu.graph_layer with the activation line parametrised (and, for the activation-dropout test, the
    mask ``act_scale`` behind it); everything else is that function, statement for statement.  The activation runs in
    fp32 as there (``.float()``), except on fp64 operands, which stay fp64: that is the restatement the fp32 product path is
    held against."""
    from oracle import mdt_ref_cpu as R
    D = x.shape[-1]

    def ln(t, n):
        return F.layer_norm(t, (D,), W[f"{p}.{n}.weight"], W[f"{p}.{n}.bias"], 1e-5)

    r = x
    if pre_ln:
        x = ln(x, "self_attn_layer_norm")
    x = r + R.graph_mha(x, W, p + ".self_attn", nheads, bias, key_padding_mask)
    if not pre_ln:
        x = ln(x, "self_attn_layer_norm")
    r = x
    if pre_ln:
        x = ln(x, "final_layer_norm")
    pre = F.linear(x, W[p + ".fc1.weight"], W[p + ".fc1.bias"])
    if pre.dtype != torch.float64:
        pre = pre.float()
    x = (F.gelu(pre) if canonical(activation) == "gelu" else act(activation, pre)).type_as(x)
    if act_scale is not None:
        x = x * act_scale
    x = r + F.linear(x, W[p + ".fc2.weight"], W[p + ".fc2.bias"])
    if not pre_ln:
        x = ln(x, "final_layer_norm")
    return x


def patched_graph_layer(activation):
    """What to monkeypatch oracle.mdt_ref_cpu.graph_layer with (graph_stack looks it up at call time)."""
    def layer(x, W, p, nheads, bias, key_padding_mask, pre_ln=False):
        return graph_layer(x, W, p, nheads, bias, key_padding_mask, pre_ln, activation=activation)
    return layer
