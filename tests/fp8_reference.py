"""fp64 reference and per-element error bounds for the 8-bit path: mdt_fp8_quantize, mdt_gemm_fp8 and mdt_gemm_fp8_q8
(include/mdt_hip.h), pure torch: no device, no native library, and no torch.float8 type (the CPU tests compare this module with
those types; nothing here is built from them).

Formats (OCP 8-bit floating point).  e4m3fn: 1 sign, 4 exponent (bias 7), 3 mantissa bits; no infinities; S.1111.111 is the only
NaN; largest finite value 1.75 * 2^8 = 448; subnormals m * 2^-9.  e5m2: 1 sign, 5 exponent (bias 15), 2 mantissa bits; IEEE-like:
exponent 31 is infinity (mantissa 0) or NaN; largest finite value 1.75 * 2^15 = 57344; subnormals m * 2^-16.  decode() reads a
256-entry table built from these definitions.

The quantiser is determined bit for bit, so its check is equality (quantize_reference / assert_bytes):
  v = fp32(x) * fp32(scale), one fp32 rounding; a NaN becomes a NaN code (any byte that decodes to NaN is accepted where x is NaN);
  everything else is clamped to +-FMAX (so +-Inf gives +-FMAX) and rounded to nearest-even on the format's grid, subnormals
  included; the sign of a zero is kept.  Every finite fp32 value is an fp64 number and so is every grid point: the rounding is
  done in fp64 without error.  amax = max(amax0, max |fp32(x)|) over the UNSCALED source, +inf as soon as one element is NaN / Inf,
  unchanged for an all-zero tensor.

The GEMM.  All finite e4m3 / e5m2 values are bf16 numbers, so tests/gemm_reference.py applies to the decoded operands unchanged:
reference_gemm_fp8() decodes, calls gemm_reference.reference with alpha = fp32(inv_a * inv_b) (both kernels form that product in
fp32 once: gemm_f8.hip `p.alpha = *alpha_dev * *alpha_dev2`, gemm.hip likewise) and widens delta by one more term:

  The MFMA term.  gemm_reference's delta_acc = gamma_K |alpha| sum_k |a_k| |b_k| assumes exact products added in fp32 with
  round-to-nearest.  The 8-bit MFMAs do not do that inside one instruction: v_mfma_f32_16x16x128_f8f6f4 (route f8_w4, 128 k per
  instruction) and v_mfma_f32_16x16x32_{fp8,bf8}_fp8 (route f8_pp256p, 32 k) align an instruction's products to the largest one
  and keep a limited number of bits below it.  No guide states that number, so it is measured (tools/probes/mfma_f8_probe.hip,
  against the probe's own fp64 sums, 524 288 instructions per line; docs/experiment_log.md has the full output):

      worst |D - fp64| / max_k |a_k b_k|              16x16x128 e4m3 / e5m2       16x16x32 e4m3 / e5m2
      operands at the test matrix's distribution      1.83e-4 / 1.58e-4           1.66e-4 / 1.21e-4
      ... with a running accumulator going in         2.06e-4 / 1.56e-4           1.57e-4 / 1.37e-4   (fp32 accumulate rounding taken off)
      bytes uniform over every finite code            6.11e-4 / 4.24e-4           5.00e-4 / 4.31e-4
      staircase (equal-signed products 2^-s below)    7.51e-4 / 7.48e-4           7.51e-4 / 7.48e-4
      quarter-integer operands                        0 (absolute)

  Model: delta_mfma = c |alpha| sum over instructions of max_k |a_k b_k| (k over the instruction's 128 or 32), with
  c = 2 x the worst ratio seen — the margin rule of TANH_REL in tests/rowops_reference.py, for operand patterns the probe did
  not draw: MFMA_WORST_128 = MFMA_WORST_32 = 7.5102e-4, C_MFMA_128 = C_MFMA_32 = 1.50204e-3.  The term enters at the accumulator
  and is carried through the epilogue with the same Lipschitz factors gemm_reference uses for delta_acc (1 for alpha / bias /
  residual, the dropout scale, sup |GELU'| and sup |GELU''|, |aux|, |GELU'(aux)|), times (1 + 8 u) for the roundings on the way.
  delta_mfma = 0 where gemm_reference proves the accumulation exact (integer operands with sum |a||b| < 2^24): every product and
  every partial sum of an instruction is then an integer of at most 13 bits, far inside what the instruction keeps — the probe's
  quarter-integer line (worst absolute error 0) is the evidence.

The fused fp8 copy (mdt_gemm_fp8_q8) is defined on the STORED bf16 output: q8 = quantize_reference(stored, scale, fmt) and
amax = max(amax0, max |stored|) exactly.  The test hands in the tensor the kernel wrote after that tensor has passed its own bound,
as the GELU-with-saved-aux reference of gemm_reference takes the stored pre-activation.

Operand families.  "random": gemm_reference.gen operands with b_scale(K), quantised with the tensor-max scale by
quantize_reference — the distribution the bounds and the median condition (tests/test_fp8_reference_cpu.py) are checked at.
"integer": gemm_reference.int_operands ([-4, 4] x [-8, 8], exact in e5m2 / e4m3), encoded to bytes, with power-of-two inverse
scales: every bit of the result is determined, delta = 0, and the column sums are exact.
"""
from __future__ import annotations

import numpy as np
import torch

import tests.gemm_reference as R

E4M3, E5M2 = 0, 1
FMAX = {E4M3: 448.0, E5M2: 57344.0}
_EBITS = {E4M3: 4, E5M2: 5}
_MBITS = {E4M3: 3, E5M2: 2}
_BIAS = {E4M3: 7, E5M2: 15}

# tools/probes/mfma_f8_probe.hip on MI355X: worst |D - fp64| / max_k |a_k b_k| of one instruction over all operand patterns
MFMA_WORST_128 = 7.5102e-4            # v_mfma_f32_16x16x128_f8f6f4, A e4m3 or e5m2 (the staircase pattern; random operands 2.1e-4)
MFMA_WORST_32 = 7.5102e-4             # v_mfma_f32_16x16x32_{fp8,bf8}_fp8
C_MFMA_128 = 2.0 * MFMA_WORST_128
C_MFMA_32 = 2.0 * MFMA_WORST_32
ROUTE_BLOCK = {"f8_w4": (128, C_MFMA_128), "f8_pp256p": (32, C_MFMA_32)}     # route: (k per instruction, c)

NAN_CODE = 0x7F                       # a NaN in both formats (e4m3fn: the only one; e5m2: exponent 31, mantissa 3)


# ------------------------------------------------------------------------------------------------ formats
def _table(fmt: int) -> torch.Tensor:
    """fp64[256]: the value of every byte, from the format definition."""
    eb, mb, bias = _EBITS[fmt], _MBITS[fmt], _BIAS[fmt]
    out = []
    for v in range(256):
        s = -1.0 if v >> 7 else 1.0
        e = (v >> mb) & ((1 << eb) - 1)
        m = v & ((1 << mb) - 1)
        if fmt == E5M2 and e == 31:
            x = float("inf") if m == 0 else float("nan")
        elif fmt == E4M3 and e == 15 and m == 7:
            x = float("nan")
        elif e == 0:
            x = m * 2.0 ** (1 - bias - mb)
        else:
            x = (1.0 + m * 2.0 ** -mb) * 2.0 ** (e - bias)
        out.append(s * x)
    return torch.tensor(out, dtype=torch.float64)


_TABLES = {}


def decode(u8: torch.Tensor, fmt: int) -> torch.Tensor:
    """fp64 value of every byte of ``u8`` read as e4m3fn (fmt 0) or e5m2 (fmt 1)."""
    key = (fmt, str(u8.device))
    if key not in _TABLES:
        _TABLES[key] = _table(fmt).to(u8.device)
    return _TABLES[key][u8.to(torch.int64)]


def _pow2(k: torch.Tensor) -> torch.Tensor:
    """2^k (int64 k in the normal fp64 range) built from its bits: exact."""
    return ((k + 1023) << 52).view(torch.float64)


def quantize_reference(x: torch.Tensor, scale, fmt: int, amax0: float = 0.0):
    """(bytes u8 of x.shape, running maximum as a Python float): what mdt_fp8_quantize must write for source ``x`` (bf16 / fp32),
    ``scale`` (fp32 value or 1-element tensor) and a maximum slot that held ``amax0``.  Where x is NaN the byte is NAN_CODE with
    x's sign; assert_bytes accepts any NaN code there."""
    mb, bias, fmax = _MBITS[fmt], _BIAS[fmt], FMAX[fmt]
    x32 = x.to(torch.float32)
    sc = float(np.float32(float(scale)))
    v32 = x32 * torch.tensor(sc, dtype=torch.float32, device=x.device)     # one fp32 rounding
    nan = torch.isnan(v32)
    v = v32.double()
    sign = torch.signbit(v32)
    a = torch.where(nan, torch.zeros_like(v), v.abs()).clamp(max=fmax)    # +-Inf saturates
    emin = 1 - bias
    _, e = torch.frexp(a.clamp(min=2.0 ** -200))                          # a = m 2^e, m in [0.5, 1): floor(log2 a) = e - 1
    ex = (e.to(torch.int64) - 1).clamp(min=emin)
    q = _pow2(ex - mb)                                                    # grid spacing at a (the subnormal spacing below 2^emin)
    r = torch.round(a / q) * q                                            # torch.round: half to even; a / q and the product are exact
    # encode r: below 2^emin the code is the subnormal mantissa (2^mb itself is the first normal: the same integer formula)
    _, e2 = torch.frexp(r.clamp(min=2.0 ** -200))
    ex2 = (e2.to(torch.int64) - 1).clamp(min=emin)
    frac = r / _pow2(ex2)                                                 # [1, 2) for normals, [0, 1) for subnormals
    normal = r >= 2.0 ** emin
    code = torch.where(normal, ((ex2 + bias) << mb) + ((frac - 1.0) * 2 ** mb).to(torch.int64), (r / 2.0 ** (emin - mb)).to(torch.int64))
    code = torch.where(nan, torch.full_like(code, NAN_CODE), code)
    code = code | (sign.to(torch.int64) << 7)
    ax = x32.abs()
    if x32.numel() == 0:
        amax = float(amax0)
    elif not bool(torch.isfinite(x32).all()):
        amax = float("inf")
    else:
        amax = max(float(amax0), float(ax.max()))
    return code.to(torch.uint8), amax


def assert_bytes(got: torch.Tensor, want: torch.Tensor, src: torch.Tensor, fmt: int, what: str = ""):
    """Equality of the fp8 bytes; where the source is NaN any byte that decodes to NaN is accepted."""
    nan = torch.isnan(src.float())
    if bool(nan.any()):
        bad_nan = int((~torch.isnan(decode(got, fmt)) & nan).sum())
        assert bad_nan == 0, f"{what}: {bad_nan} NaN sources did not become a NaN code"
    diff = (got != want) & ~nan
    n = int(diff.sum())
    if n:
        idx = tuple(int(i) for i in torch.nonzero(diff)[0])
        raise AssertionError(f"{what}: {n} of {got.numel()} fp8 bytes differ; first at {idx}: got 0x{int(got[idx]):02x} "
                             f"want 0x{int(want[idx]):02x} source {float(src[idx].float())!r}")


# ------------------------------------------------------------------------------------------------ the GEMM
def mfma_term(A: torch.Tensor, B: torch.Tensor, block: int) -> torch.Tensor:
    """fp64 [M, N]: sum over the K / block instructions of max_k |A[m, k] B[n, k]| (A [M, K], B [N, K], finite parts only).
    Computed in fp32 and scaled up by 1 + 2^-20, so it never undershoots."""
    A = torch.where(torch.isfinite(A), A, torch.zeros_like(A)).abs().float()
    B = torch.where(torch.isfinite(B), B, torch.zeros_like(B)).abs().float()
    M, K = A.shape
    N = B.shape[0]
    total = torch.zeros(M, N, dtype=torch.float32, device=A.device)
    cur = torch.empty_like(total)
    tmp = torch.empty_like(total)
    for k0 in range(0, K, block):
        cur.zero_()
        for k in range(k0, min(k0 + block, K)):
            torch.mul(A[:, k:k + 1], B[None, :, k], out=tmp)
            torch.maximum(cur, tmp, out=cur)
        total += cur
    return total.double() * (1.0 + 2.0 ** -20 + K / block * 2.0 ** -23)


def reference_gemm_fp8(a8, b8, inv_a, inv_b, a_format, *, route="f8_w4", epilogue=0, bias=None, residual=None, aux=None, drop_p=0.0,
                       drop_seed=0, colsum0=None, q8=None):
    """The documented result of mdt_gemm_fp8 / mdt_gemm_fp8_q8 with its error bound, as gemm_reference.reference returns it
    ({"out" / "aux" / "colsum": (fp64 value, delta)}), delta widened by the MFMA term of ``route`` (module docstring).
    ``q8`` = (format, scale, amax0, stored bf16 output): adds "q8" (the expected bytes) and "q8_amax" (the expected running
    maximum, a float), both from the STORED output."""
    A, B = decode(a8, a_format), decode(b8, E4M3)
    alpha = float(np.float32(np.float32(float(inv_a)) * np.float32(float(inv_b))))
    ep = int(epilogue)
    ref = R.reference(A, B, alpha=alpha, epilogue=ep, bias=bias, residual=residual, aux=aux, drop_p=drop_p, drop_seed=drop_seed,
                      colsum0=colsum0)
    A0 = torch.where(torch.isfinite(A), A, torch.zeros_like(A))
    B0 = torch.where(torch.isfinite(B), B, torch.zeros_like(B))
    S_max = float((A0.abs().sum(1).max() * B0.abs().max())) if A.numel() else 0.0     # >= max sum_k |a||b|
    exact = R._integral(A0) and R._integral(B0) and (S_max < R.F24 or float((A0.abs() @ B0.abs().t()).max()) < R.F24)
    if not exact:
        block, c = ROUTE_BLOCK[route]
        dm = c * abs(alpha) * mfma_term(A, B, block) * (1.0 + 8 * R.U32)
        M, N = dm.shape
        s = R.drop_scale(M, N, drop_p, drop_seed, device=dm.device) if ep & R.EPI_DROPOUT else 1.0
        d_out = dm
        if (ep & R.EPI_GELU) and (ep & R.EPI_AUX_GRAD):
            if "aux" in ref:
                ref["aux"] = (ref["aux"][0], ref["aux"][1] + R.GELU_D2 * dm * s)
            d_out = R.GELU_D1 * dm * s
        else:
            if ep & R.EPI_GELU:
                if "aux" in ref:
                    ref["aux"] = (ref["aux"][0], ref["aux"][1] + dm)
                    d_out = torch.zeros_like(dm)          # activated at the stored value
                else:
                    d_out = R.GELU_D1 * dm
            if ep & R.EPI_DROPOUT:
                d_out = d_out * s
        if ep & R.EPI_MULAUX:
            d_out = d_out * aux.double().abs()
        if ep & R.EPI_DGELU:
            d_out = d_out * R.gelu_grad(aux.double()).abs()
        if "colsum" in ref:
            ref["colsum"] = (ref["colsum"][0], ref["colsum"][1] + d_out.sum(0) * (1.0 + R._gamma(M + 1)))
        ref["out"] = (ref["out"][0], ref["out"][1] + d_out)
    if q8 is not None:
        fmt, scale, amax0, stored = q8
        ref["q8"], ref["q8_amax"] = quantize_reference(stored, scale, fmt, amax0)
    return ref


# ------------------------------------------------------------------------------------------------ operands
def scale_for(x: torch.Tensor, fmt: int) -> float:
    """The tensor-max scale FMAX / max |x| as the fp32 number the library holds."""
    return float(np.float32(FMAX[fmt]) / np.float32(float(x.float().abs().max())))


def inv32(scale: float) -> float:
    return float(np.float32(1.0) / np.float32(scale))


def random_operands(M, N, K, a_format, seed=0, device="cpu"):
    """(a8 [M, K], b8 [N, K], inv_a, inv_b): gemm_reference.gen operands (A uniform(-1, 1), B at b_scale(K)) quantised with the
    tensor-max scale: the operands of the random family."""
    a = R.gen((M, K), 100 + seed, device=device)
    b = R.gen((N, K), 200 + seed, scale=R.b_scale(K), device=device)
    sa, sb = scale_for(a, a_format), scale_for(b, E4M3)
    return quantize_reference(a, sa, a_format)[0], quantize_reference(b, sb, E4M3)[0], inv32(sa), inv32(sb)


def integer_operands(M, N, K, a_format, seed=0, device="cpu"):
    """(a8, b8): gemm_reference.int_operands ([-4, 4] x [-8, 8]) encoded exactly; use power-of-two inverse scales with them."""
    a, b = R.int_operands(M, N, K, seed=seed, device=device)
    a8, b8 = quantize_reference(a, 1.0, a_format)[0], quantize_reference(b, 1.0, E4M3)[0]
    assert torch.equal(decode(a8, a_format), a.double()) and torch.equal(decode(b8, E4M3), b.double())
    return a8, b8


# the median condition (gemm_reference.assert_within: median bound / |ref| <= 2^-7 for a bf16 output) with the measured c decides
# which cells of the GPU matrix run with random operands; a cell over the limit runs with integer operands only
def random_allowed(route, kind, K):
    if kind == "fc1":
        return False                                  # 0.0103 at K = 640 already (0.0076 at K = 768 before the MFMA term)
    if route == "f8_w4":
        return K <= 1280
    if kind in ("dense", "res", "gelu_aux"):
        return K <= 768
    return K <= 320 or (K <= 576 and kind in ("plain", "bias"))


# ------------------------------------------------------------------------------------------------ guard bands
SENTINEL8 = 0x7F          # a NaN code in both formats: no finite output's copy holds it, so a view left unwritten is seen too


class Guarded8:
    """gemm_reference.Guarded for uint8: a [rows, cols] view with row stride ``ld`` >= cols inside a buffer with ``pre`` rows
    before and ``post`` rows after it, everything filled with SENTINEL8 first (``init``: the view's content)."""

    def __init__(self, rows, cols, device, ld=None, pre=2, post=3, init=None):
        self.rows, self.cols, self.pre = rows, cols, pre
        self.ld = ld or cols
        self.buf = torch.full((pre + rows + post, self.ld), SENTINEL8, dtype=torch.uint8, device=device)
        self.view = self.buf[pre:pre + rows, :cols]
        if init is not None:
            self.view.copy_(init)

    def untouched(self) -> bool:
        b = self.buf
        parts = [b[:self.pre], b[self.pre + self.rows:], b[self.pre:self.pre + self.rows, self.cols:]]
        return all(bool((p == SENTINEL8).all()) for p in parts if p.numel())


def pristine(g) -> bool:
    """A Guarded / Guarded8 buffer built without ``init`` still holds nothing but its sentinel, the view included."""
    if isinstance(g, Guarded8):
        return bool((g.buf == SENTINEL8).all())
    return bool((g.buf.view(g.itype) == g.bits).all())
