"""fp64 reference and per-element error bounds for mdt_gemm (include/mdt_hip.h), pure torch: no device, no native library.

reference() computes the documented result of one mdt_gemm call from the exact operand values and, next to every value, a
bound δ on the fp32 arithmetic error the kernels may make.  bound() turns (value, δ) into a tolerance for the stored
output: half an ulp of the output type for its final rounding plus δ.  assert_within() checks an output against it.

The error model.  bf16 x bf16 products are exact in fp32; a dot product of K terms summed in fp32 with round-to-nearest
adds, in any order (MFMA blocks, 32-deep K steps, split-K slabs), errs by at most γ_K · Σ_k |a_k| |b_k| with
γ_K = K u / (1 - K u), u = 2^-24 (Higham, "Accuracy and Stability of Numerical Algorithms", Thm 3.1; fp32 operands:
the same γ_K covers the rounded products too).  So δ_acc = c K u (|alpha| |op(A)| |op(B)|)[m, n] with c = 1 / (1 - K u),
i.e. c = 1 + O(K u): a worst-case bound, not a √K estimate, and the only freedom it leaves is the summation order.
Each fp32 operation of the epilogue (alpha / bias FMA, activation, dropout scale, saved-derivative product, residual,
accumulate) adds at most u times the magnitude it rounds, and an operation f carries the incoming δ over with its
Lipschitz factor (sup |GELU'| = 1.129, sup |GELU''| = 0.798, |aux|, the dropout scale).  The approximations the code
documents enter as ε: the bf16 epilogues' erf (Abramowitz-Stegun 7.1.26, |err| <= 1.5e-7, half of it in Φ) with
approximate exp2 / reciprocal, taken as 2e-7 per unit of |x| (GELU) and 2e-7 (1 + |x|) (GELU').

Exact operands.  Where every fp32 operation is provably exact the bound says so (δ = 0): an accumulation whose
operands are integers with Σ_k |a_k| |b_k| < 2^24 (every partial sum, in any order, is an integer below 2^24), an
epilogue step whose inputs are exact and whose exact result is an fp32 number, and a column / row sum of integers whose
Σ |terms| stays below 2^24.  The column-sum checks use such operands (int_operands): a worst-case bound for an
M-term fp32 sum of random values would be a large fraction of the sum itself at the token counts of the persistent
routes, too wide to see a missing 16-row slice.

Where a kernel rounds in the middle of the epilogue the reference rounds at the same place instead of widening the
bound: GELU with a saved pre-activation (no MDT_EPI_AUX_GRAD) activates at the bf16 value it stored, so the reference
takes that stored tensor (checked on its own against its bound) as the activation's input.

Dropout keep-bits come from an independent port of the counter hash (csrc/common.hpp make_drop / drop_mix), never from
the library's own mask kernel.
"""
from __future__ import annotations

import math

import numpy as np
import torch

U32 = 2.0 ** -24                      # unit roundoff of fp32
GELU_D1 = 1.1290                      # sup |GELU'(x)|, at x = sqrt(2)
GELU_D2 = 0.7979                      # sup |GELU''(x)| = 2 φ(0)
EPS_ERF = 2e-7                        # documented erf approximation (1.5e-7) plus approximate exp2 / rcp, per unit of |x|

EPI_BIAS, EPI_GELU, EPI_RESIDUAL, EPI_DGELU, EPI_ACCUM, EPI_ATOMIC, EPI_DROPOUT = 1, 2, 4, 8, 16, 32, 64
EPI_COLSUM, EPI_AUX_GRAD, EPI_MULAUX, EPI_ASUM = 128, 256, 512, 1024

_M32 = 0xFFFFFFFF
_M64 = 0xFFFFFFFFFFFFFFFF


# ------------------------------------------------------------------------------------------------ operands
def gen(shape, seed, scale=1.0, dtype=torch.bfloat16, device="cpu"):
    """Uniform(-scale, scale) rounded to ``dtype``: the operand generator of the CPU mutant tests and the GPU matrix."""
    g = torch.Generator(device=device).manual_seed(seed)
    return ((torch.rand(*shape, generator=g, device=device, dtype=torch.float32) * 2 - 1) * scale).to(dtype)


def gen_int(shape, seed, r, dtype=torch.bfloat16, device="cpu"):
    """Integers uniform in [-r, r] (exact in bf16 for r <= 256)."""
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.randint(-r, r + 1, tuple(shape), generator=g, device=device, dtype=torch.int32).to(dtype)


# integer operand ranges of the column-sum cases: A in [-4, 4], B in [-8, 8], the saved derivative in [-1, 1], so that at
# K <= 1088 and M ~ 22 000 the column sums of |C| stay below 2^24 (exact fp32 sums in any order) while most |C| exceed 256
# (bf16 rounds them, so a sum of the rounded outputs differs from the documented sum of the fp32 results)
INT_A, INT_B, INT_AUX, INT_CS = 4, 8, 1, 50


def int_operands(M, N, K, trans_a=False, trans_b=False, seed=0, dtype=torch.bfloat16, device="cpu"):
    """(a, b) stored as mdt_gemm expects them, integer-valued: the operands of the column-sum cases (with alpha
    a power of two the column sums of |C| stay below 2^24 at K <= 1088 and M ~ 22 000)."""
    a = gen_int((K, M) if trans_a else (M, K), 100 + seed, INT_A, dtype, device)
    b = gen_int((K, N) if trans_b else (N, K), 200 + seed, INT_B, dtype, device)
    return a, b


def b_scale(K):
    """Scale of B: op(A) @ op(B) then has a standard deviation of about 2/3, the range where GELU bends."""
    return 2.0 / math.sqrt(max(K, 1))


# ------------------------------------------------------------------------------------------------ dropout port
def drop_key(seed: int) -> int:
    """make_drop: splitmix64 finaliser of the 64-bit site seed, folded to 32 bits."""
    z = (int(seed) + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    z ^= z >> 31
    return (z ^ (z >> 32)) & _M32


def drop_params(p: float):
    """(16-bit threshold, fp32 keep scale) exactly as make_drop computes them from the fp32 p."""
    p32 = np.float32(p)
    thresh = int(np.float32(p32 * np.float32(65536.0)) + np.float32(0.5))
    inv_keep = float(np.float32(1.0) / (np.float32(1.0) - p32))
    return thresh, inv_keep


def _drop_mix(x: torch.Tensor) -> torch.Tensor:
    """drop_mix on int64 tensors holding uint32 values (__umul24 = low 32 bits of the 24 x 24-bit product)."""
    def rotl(v, r):
        return ((v << r) | (v >> (32 - r))) & _M32
    x = (((x & 0xFFFFFF) * 0x95F24D) + rotl(x, 15)) & _M32
    x = x ^ (x >> 15)
    x = (((x & 0xFFFFFF) * 0xC2B2AE) + rotl(x, 13)) & _M32
    x = x ^ (x >> 13)
    x = (((x & 0xFFFFFF) * 0x85EBCB) + rotl(x, 17)) & _M32
    x = x ^ (x >> 16)
    return x


def keep_bits(counters: torch.Tensor, p: float, seed: int) -> torch.Tensor:
    """True where counter i of site ``seed`` is kept (drop_scale: 16 random bits per counter, two counters per word)."""
    c = counters.to(torch.int64)
    h = _drop_mix((c >> 1) ^ drop_key(seed))
    bits = torch.where((c & 1) == 1, h >> 16, h & 0xFFFF)
    return bits >= drop_params(p)[0]


def drop_scale(M: int, N: int, p: float, seed: int, device="cpu", counter_ld=None) -> torch.Tensor:
    """fp64 [M, N]: 0 or fp32(1 / (1 - p)) per element, counter m * N + n (``counter_ld`` replaces N: mutant tests only)."""
    ld = N if counter_ld is None else counter_ld
    m = torch.arange(M, device=device, dtype=torch.int64)[:, None]
    n = torch.arange(N, device=device, dtype=torch.int64)[None, :]
    keep = keep_bits(m * ld + n, p, seed)
    return keep.double() * drop_params(p)[1]


# ------------------------------------------------------------------------------------------------ reference
def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0))))


def gelu_grad(x):
    return 0.5 * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0)))) + x * torch.exp(-0.5 * x * x) * (1.0 / math.sqrt(2.0 * math.pi))


def _op_a(a, trans_a):
    """op(A) [M, K]: A stored [M, K], or [K, M] with trans_a."""
    a = a.double()
    return a.t() if trans_a else a


def _op_b(b, trans_b):
    """op(B) [K, N]: B stored [N, K] (an nn.Linear weight), or [K, N] with trans_b."""
    b = b.double()
    return b if trans_b else b.t()


def _gamma(n):
    return n * U32 / (1.0 - n * U32)


F24 = 2.0 ** 24


def _rep32(x):
    """x (fp64) is an fp32 number."""
    return x.float().double() == x


def _integral(x, dim=None):
    ok = x == torch.round(x)
    return bool(ok.all()) if dim is None else ok.all(dim)


def _sum_bound(terms, d, c0, n, dim):
    """Error bound of c0 + Σ terms (along ``dim``) summed in fp32 in any order, each term carrying error d: 0 where all
    terms and c0 are exact multiples of one power of two g with (Σ|terms| + |c0|) / g < 2^24 (every partial sum is then
    an fp32 number), else Σ d + γ_{n+1} (|c0| + Σ (|terms| + d))."""
    general = d.sum(dim) + _gamma(n + 1) * (c0.abs() + (terms.abs() + d).sum(dim))
    fin = bool(torch.isfinite(terms).all())
    for q in range(0, 9):                             # g = 2^-q, the coarsest granule the terms sit on
        if fin and _integral(terms * 2.0 ** q) and _integral(c0 * 2.0 ** q):
            exact = (d == 0).all(dim) & ((terms.abs().sum(dim) + c0.abs()) * 2.0 ** q < F24)
            return torch.where(exact, torch.zeros_like(general), general)
    return general


def reference(a, b, *, trans_a=False, trans_b=False, alpha=1.0, epilogue=0, bias=None, residual=None, aux=None, c_old=None,
              colsum0=None, drop_p=0.0, drop_seed=0, split_k=1):
    """The documented result of mdt_gemm in fp64 with its error bound: {name: (value, δ)} for "out" (C after the call,
    the accumulated old C included), "aux" (what a GELU epilogue saves), "colsum" (MDT_EPI_COLSUM) and "asum"
    (MDT_EPI_ASUM).  ``aux``: the input of MDT_EPI_MULAUX / DGELU; for MDT_EPI_GELU without AUX_GRAD the tensor the
    kernel STORED (it activates at that rounded value); for GELU | AUX_GRAD only whether it is given matters.
    ``c_old``: C before the call (ACCUM / ATOMIC); ``colsum0``: the colsum buffer before the call.
    Rows of op(A) / columns of op(B) holding a NaN or Inf give non-finite outputs (rows / columns), as IEEE says."""
    ep = int(epilogue)
    A, B = _op_a(a, trans_a), _op_b(b, trans_b)
    M, K = A.shape
    N = B.shape[1]
    bad_r = ~torch.isfinite(A).all(1)
    bad_c = ~torch.isfinite(B).all(0)
    A0 = torch.where(torch.isfinite(A), A, torch.zeros_like(A))
    B0 = torch.where(torch.isfinite(B), B, torch.zeros_like(B))
    acc = A0 @ B0
    S = A0.abs() @ B0.abs()
    if bad_r.any() or bad_c.any():
        acc = acc.clone()
        acc[bad_r, :] = float("nan")
        acc[:, bad_c] = float("nan")
    al = float(np.float32(alpha))
    u = U32
    exact_acc = _integral(A0) and _integral(B0) and float(S.max()) < F24 if S.numel() else True
    d = torch.zeros_like(S) if exact_acc else _gamma(K) * abs(al) * S
    va = al * acc
    v = va
    rnd = abs(al) * S
    if ep & EPI_BIAS:
        bv = bias.double()[None, :]
        v = va + bv
        rnd = rnd + bv.abs()
    d = torch.where((d == 0) & _rep32(va) & _rep32(v), d, d + u * rnd)      # alpha / bias: exact when nothing rounds
    out = {}
    s = None
    if ep & EPI_DROPOUT:
        s = drop_scale(M, N, drop_p, drop_seed, device=acc.device)
    if (ep & EPI_GELU) and (ep & EPI_AUX_GRAD):
        sc = s if s is not None else 1.0
        g1 = gelu_grad(v) * sc
        if aux is not None:
            out["aux"] = (g1, (GELU_D2 * d + EPS_ERF * (1 + v.abs())) * sc + 2 * u * g1.abs())
        y = gelu(v) * sc
        d = (GELU_D1 * d + EPS_ERF * v.abs()) * sc + 3 * u * y.abs()
        v = y
    else:
        if ep & EPI_GELU:
            if aux is not None:
                out["aux"] = (v, d)
                x = aux.double()                        # the kernel's stored bf16 pre-activation, exact
                v = gelu(x)
                d = EPS_ERF * x.abs() + 2 * u * v.abs()
            else:
                y = gelu(v)
                d = GELU_D1 * d + EPS_ERF * v.abs() + 2 * u * y.abs()
                v = y
        if ep & EPI_DROPOUT:
            v = v * s
            d = d * s + u * v.abs()
    if ep & EPI_MULAUX:
        x = aux.double()
        v = v * x
        d = d * x.abs()
        d = torch.where((d == 0) & _rep32(v), d, d + u * v.abs())
    if ep & EPI_DGELU:
        x = aux.double()
        g1 = gelu_grad(x)
        d = d * g1.abs() + v.abs() * EPS_ERF * (1 + x.abs())
        v = v * g1
        d = d + u * v.abs()
    if ep & EPI_RESIDUAL:
        r = residual.double()
        d = torch.where((d == 0) & _rep32(v + r), d, d + u * (v.abs() + r.abs() + d))
        v = v + r
    if ep & EPI_COLSUM:
        c0 = colsum0.double() if colsum0 is not None else torch.zeros(N, dtype=torch.float64, device=acc.device)
        out["colsum"] = (c0 + v.sum(0), _sum_bound(v, d, c0, M, 0))
    if ep & (EPI_ACCUM | EPI_ATOMIC):
        c = c_old.double()
        n_adds = max(int(split_k), 1) if ep & EPI_ATOMIC else 1
        # every partial result added (a split-K slab's, or the whole one) and every running total is bounded by
        # |c| + |alpha| S + d: one rounding of that size per add
        part = abs(al) * S + v.abs()
        d = torch.where((d == 0) & _rep32(v + c) & (n_adds == 1), d, d + n_adds * u * (part + d + c.abs()))
        v = v + c
    out["out"] = (v, d)
    if ep & EPI_ASUM:
        c0 = colsum0.double()
        out["asum"] = (c0 + A.sum(1), _sum_bound(A, torch.zeros_like(A), c0, K, 1))
    return out


# ------------------------------------------------------------------------------------------------ bounds
def _mant_bits(dtype):
    if dtype == torch.bfloat16:
        return 8
    if dtype == torch.float32:
        return 24
    if dtype == torch.float64:
        return 53
    raise ValueError(f"no ulp for {dtype}")


def ulp(x: torch.Tensor, dtype) -> torch.Tensor:
    """ulp of ``dtype`` at magnitude |x| (normal range; below it the smallest normal's)."""
    ax = x.abs().double().clamp(min=2.0 ** -126)
    _, e = torch.frexp(ax)                        # ax = m 2^e, m in [0.5, 1): ulp = 2^(e - mantissa bits)
    k = torch.where(torch.isfinite(ax), e.to(torch.int64) - _mant_bits(dtype), torch.zeros_like(e, dtype=torch.int64))
    return ((k + 1023) << 52).view(torch.float64)   # the power of two built from its bits: exact (ldexp / pow need not be)


def bound(value: torch.Tensor, delta: torch.Tensor, dtype) -> torch.Tensor:
    """Per-element tolerance of a result stored as ``dtype``: ½ ulp(|value| + δ) + δ."""
    return 0.5 * ulp(value.abs() + delta, dtype) + delta


def assert_within(out: torch.Tensor, ref: torch.Tensor, bnd: torch.Tensor, what: str = "", dtype=None, median_limit=None):
    """Every finite reference element is met within its bound and every non-finite one is non-finite in ``out``; bf16
    results additionally are (a) not biased — over >= 1e5 non-zero elements |mean((out - ref) sign(ref) / ulp)| <= 0.05
    (round-to-nearest-even ~ 0, truncation ~ -0.5) — and (b) checked against a bound that is not vacuous: the median of
    bound / |ref| over the non-zero elements is at most 2^-7 (``median_limit`` sets that limit for other types too)."""
    dtype = dtype or out.dtype
    o = out.double()
    r = ref.double()
    fin = torch.isfinite(r)
    pattern = int((fin != torch.isfinite(o)).sum())
    assert pattern == 0, f"{what}: {pattern} elements differ in finiteness from the reference"
    err = (o - r).abs()
    ok = (err <= bnd) | ~fin
    n_over = int((~ok).sum())
    if n_over:
        ratio = torch.where(fin, err / bnd.clamp(min=1e-300), torch.zeros_like(err))
        ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
        flat = int(torch.argmax(ratio))
        idx = np.unravel_index(flat, tuple(r.shape))
        raise AssertionError(f"{what}: {n_over} of {r.numel()} elements over their bound; worst at {tuple(int(i) for i in idx)}: "
                             f"out {float(o.reshape(-1)[flat])!r} ref {float(r.reshape(-1)[flat])!r} "
                             f"bound {float(bnd.reshape(-1)[flat]):.3e} err/bound {float(ratio.reshape(-1)[flat]):.3g}")
    if dtype == torch.bfloat16:
        nz = fin & (r != 0)
        if int(nz.sum()) >= 100_000:
            bias = float(((o - r) * torch.sign(r) / ulp(r, torch.bfloat16))[nz].mean())
            assert abs(bias) <= 0.05, f"{what}: rounding bias {bias:+.3f} ulp (round-to-nearest-even gives ~0)"
        median_limit = 2.0 ** -7 if median_limit is None else median_limit
    if median_limit is not None:
        nz = fin & (r != 0)
        if int(nz.sum()):
            med = float((bnd / r.abs())[nz].median())
            assert med <= median_limit, f"{what}: vacuous bound, median bound/|ref| = {med:.3e} > {median_limit:.3e}"


def check(got: dict, ref: dict, dtypes: dict, what: str = ""):
    """assert_within for every entry of ``got`` ({name: tensor}) against reference() output ``ref``; ``dtypes``: the
    storage type of each entry (colsum / asum are fp32).  The fp32 column / row sums must also have a bound that is not
    vacuous: median bound / |ref| <= 2^-7, as for bf16 outputs."""
    for name, t in got.items():
        v, d = ref[name]
        dt = dtypes.get(name, t.dtype)
        lim = 2.0 ** -7 if name in ("colsum", "asum") else None
        assert_within(t, v, bound(v, d, dt), what=f"{what} {name}", dtype=dt, median_limit=lim)


# ------------------------------------------------------------------------------------------------ guard bands
_SENTINEL = {torch.bfloat16: (torch.int16, 0x7FA5), torch.float32: (torch.int32, 0x7FA5A5A5)}


class Guarded:
    """A [rows, cols] view with row stride ``ld`` >= cols inside a buffer with ``pre`` rows before and ``post`` rows after
    it; everything is filled with a sentinel bit pattern (a NaN) first.  ``untouched()``: every byte outside the view
    still holds it."""

    def __init__(self, rows, cols, dtype, device, ld=None, pre=2, post=3, init=None):
        self.rows, self.cols, self.pre = rows, cols, pre
        self.ld = ld or cols
        self.itype, self.bits = _SENTINEL[dtype]
        self.buf = torch.empty(pre + rows + post, self.ld, dtype=dtype, device=device)
        self.buf.view(self.itype).fill_(self.bits)
        self.view = self.buf[pre:pre + rows, :cols]
        if init is not None:
            self.view.copy_(init)

    def untouched(self) -> bool:
        b = self.buf.view(self.itype)
        parts = [b[:self.pre], b[self.pre + self.rows:], b[self.pre:self.pre + self.rows, self.cols:]]
        return all(bool((p == self.bits).all()) for p in parts if p.numel())
