"""tests/fp8_reference.py can fail: its decoder and quantiser equal torch's float8 types bit for bit, a CPU emulation of the 8-bit
kernels' arithmetic (fp32 sums per 128- or 32-deep instruction block, fp32 epilogue in the kernels' order, round-to-nearest-even
to bf16, the fp8 copy made from the stored bf16) passes its bounds in both operand families, and each listed mutant of it — a
subtly wrong kernel — is rejected, at the operand scales of the GPU matrix (tests/test_fp8_routes_gpu.py) and its smallest K."""
import numpy as np
import pytest
import torch

import tests.fp8_reference as F
import tests.gemm_reference as R

bf16, f32 = torch.bfloat16, torch.float32
TORCH8 = {F.E4M3: torch.float8_e4m3fn, F.E5M2: torch.float8_e5m2}
M, N = 2 * 256 + 37, 256          # two full 256-row tiles and a ragged third
P, SEED = 0.4, 4321
E = R
EPIS = {
    "plain": 0, "bias": E.EPI_BIAS, "dense": E.EPI_BIAS | E.EPI_RESIDUAL | E.EPI_DROPOUT,
    "fc1": E.EPI_BIAS | E.EPI_GELU | E.EPI_AUX_GRAD, "res": E.EPI_RESIDUAL, "mulaux_colsum": E.EPI_MULAUX | E.EPI_COLSUM,
    "dgelu_drop": E.EPI_DGELU | E.EPI_DROPOUT, "gelu_aux": E.EPI_BIAS | E.EPI_GELU,
}
A_FMT = {"plain": F.E5M2, "res": F.E5M2, "mulaux_colsum": F.E5M2, "bias": F.E4M3, "dense": F.E4M3, "fc1": F.E4M3,
         "dgelu_drop": F.E5M2, "gelu_aux": F.E4M3}
K_MIN = {"f8_w4": 640, "f8_pp256p": 256}


# ------------------------------------------------------------------------------------------------ decode / quantiser
@pytest.mark.parametrize("fmt", [F.E4M3, F.E5M2])
def test_decode_equals_torch_float8_on_all_256_bytes(fmt):
    u = torch.arange(256, dtype=torch.uint8)
    d, t = F.decode(u, fmt), u.view(TORCH8[fmt]).double()
    assert torch.equal(torch.isnan(d), torch.isnan(t)) and torch.equal(torch.isinf(d), torch.isinf(t))
    fin = torch.isfinite(t)
    assert torch.equal(d[fin], t[fin]) and torch.equal(torch.signbit(d[fin]), torch.signbit(t[fin]))
    assert int(torch.isnan(d).sum()) == (2 if fmt == F.E4M3 else 6) and int(torch.isinf(d).sum()) == (0 if fmt == F.E4M3 else 2)
    assert float(d[fin].max()) == F.FMAX[fmt]


def _torch_quantize(x, scale, fmt):
    v = x.float() * torch.tensor(float(np.float32(scale)), dtype=f32)
    v = torch.where(torch.isnan(v), v, v.clamp(-F.FMAX[fmt], F.FMAX[fmt]))
    return v.to(TORCH8[fmt]).view(torch.uint8)


@pytest.mark.parametrize("fmt", [F.E4M3, F.E5M2])
@pytest.mark.parametrize("scale", [1.0, 0.37, 3.0e4, 2.0 ** -12])      # 3e4 saturates most of the range, 2^-12 reaches the subnormals
def test_quantize_reference_equals_torch_cast_on_every_bf16_bit_pattern(fmt, scale):
    x = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(bf16)
    q, amax = F.quantize_reference(x, scale, fmt)
    F.assert_bytes(_torch_quantize(x, scale, fmt), q, x, fmt, what=f"fmt {fmt} scale {scale}")
    assert amax == float("inf")                                       # the patterns hold NaNs and infinities
    fin = torch.isfinite(x.float())
    assert F.quantize_reference(x[fin], scale, fmt, 1e-3)[1] == float(x[fin].float().abs().max())


def test_quantize_reference_ties_signs_and_specials():
    # e4m3: spacing 2 in [16, 32): 17 -> 16 (even), 19 -> 20; subnormal spacing 2^-9: 1.5 * 2^-9 -> 2 * 2^-9, 0.5 * 2^-9 -> 0, 2.5 * 2^-9 -> 2 * 2^-9
    x = torch.tensor([17.0, 19.0, -17.0, 1.5 * 2 ** -9, 0.5 * 2 ** -9, 2.5 * 2 ** -9, 7.5 * 2 ** -9, 464.0, 1e9, 0.0, -0.0], dtype=f32)
    q, _ = F.quantize_reference(x, 1.0, F.E4M3)
    assert F.decode(q, F.E4M3).tolist() == [16.0, 20.0, -16.0, 2 * 2 ** -9, 0.0, 2 * 2 ** -9, 2 ** -6, 448.0, 448.0, 0.0, -0.0]
    assert q[-2:].tolist() == [0x00, 0x80]                            # the sign of a zero is kept
    # e5m2: spacing 4 in [16, 32): 18 -> 16, 22 -> 24; subnormal spacing 2^-16
    x = torch.tensor([18.0, 22.0, -22.0, 1.5 * 2 ** -16, 0.5 * 2 ** -16, 3.5 * 2 ** -16, 61440.0, float("inf"), float("-inf")], dtype=f32)
    q, amax = F.quantize_reference(x, 1.0, F.E5M2)
    assert F.decode(q, F.E5M2).tolist() == [16.0, 24.0, -24.0, 2 * 2 ** -16, 0.0, 2 ** -14, 57344.0, 57344.0, -57344.0]
    assert amax == float("inf")
    q, amax = F.quantize_reference(torch.tensor([float("nan"), 1.0]), 1.0, F.E4M3, 0.5)
    assert bool(torch.isnan(F.decode(q, F.E4M3))[0]) and amax == float("inf")
    q, amax = F.quantize_reference(torch.zeros(8), 2.0, F.E5M2, 0.25)
    assert amax == 0.25 and not bool(q.any())
    assert F.quantize_reference(torch.tensor([3.0, -5.0]), 100.0, F.E4M3, 7.0)[1] == 7.0      # a maximum above the tensor's stays
    assert F.quantize_reference(torch.tensor([3.0, -5.0]), 100.0, F.E4M3, 1.0)[1] == 5.0      # the UNSCALED source


def test_assert_bytes_and_guard_band_can_fail():
    x = torch.tensor([1.0, float("nan"), 2.0])
    want, _ = F.quantize_reference(x, 1.0, F.E4M3)
    got = want.clone(); got[1] = 0xFF                                  # another NaN code: accepted
    F.assert_bytes(got, want, x, F.E4M3)
    got[1] = 0x7E
    with pytest.raises(AssertionError, match="NaN"):
        F.assert_bytes(got, want, x, F.E4M3)
    got = want.clone(); got[2] ^= 1
    with pytest.raises(AssertionError, match="differ"):
        F.assert_bytes(got, want, x, F.E4M3)
    g = F.Guarded8(5, 8, "cpu", ld=16)
    assert F.pristine(g)
    g.view.fill_(1)
    assert g.untouched() and not F.pristine(g)
    g.buf[3, 8] = 0
    assert not g.untouched()


# ------------------------------------------------------------------------------------------------ emulation
def _gelu_parts32(x):
    cdf = (0.5 * (1.0 + torch.erf(x * 0.70710678118654752))).to(f32)
    pdf = (0.3989422804014327 * torch.exp(-0.5 * x * x)).to(f32)
    return cdf, pdf


def _trunc_bf16(x):
    return (x.contiguous().view(torch.int32) & ~0xFFFF).view(f32).to(bf16)


def emulate(a8, b8, inv_a, inv_b, a_fmt, block, *, epilogue=0, bias=None, residual=None, aux=None, colsum0=None, q8=None, mutant=None):
    """One mdt_gemm_fp8(_q8) call as the kernels compute it: 256-row tiles, an fp32 sum per ``block``-deep instruction added to
    an fp32 accumulator, alpha = fp32(inv_a * inv_b), the epilogue of gemm_epilogue.hpp, RNE to bf16, the copy from the bf16."""
    ep = epilogue
    fa = (1 - a_fmt) if mutant == "wrong_format" else a_fmt
    A = F.decode(a8, fa).to(f32)
    Bt = F.decode(b8, F.E4M3).to(f32).t().contiguous()
    Mx, K = A.shape
    N = b8.shape[0]
    acc = torch.zeros(Mx, N, dtype=f32)
    for k0 in range(0, K, block):
        part = (A[:, k0:k0 + block] @ Bt[k0:k0 + block]).to(f32)
        if mutant == "drop_stage" and k0 == block:                     # one 16 x 16 block misses one 64-k stage (32-k form: one instruction)
            w = min(64, block)
            part[272:288, 32:48] -= (A[272:288, k0:k0 + w] @ Bt[k0:k0 + w, 32:48]).to(f32)
        acc = (acc + part).to(f32)
        if mutant == "step_twice" and k0 == 2 * block:
            acc[272:288, 32:48] += part[272:288, 32:48]
    if mutant == "block_from_neighbour":
        acc[256 + 16:256 + 32] = acc[16:32]                            # a 16-row block of tile 1 holds tile 0's
    if mutant == "pending_from_previous":
        acc[256 + 128:512] = acc[128:256]                              # the pending half of a workgroup's second tile is its first tile's
    al = np.float32(inv_a) if mutant == "inv_a_only" else np.float32(inv_a) * np.float32(inv_b)
    v = (acc * float(al)).to(f32)
    if ep & E.EPI_BIAS and mutant != "bias_after_gelu":
        v = (v + bias.to(f32)[None, :]).to(f32)                        # (the kernel's FMA rounds once: within the bound's u |v|)
    got = {}
    s = torch.ones(Mx, N, dtype=f32)
    if ep & E.EPI_DROPOUT:
        s = R.drop_scale(Mx + 1, N, P, SEED).to(f32)
        s = s[1:] if mutant == "drop_row_shift" else s[:Mx]
    if (ep & E.EPI_GELU) and (ep & E.EPI_AUX_GRAD):
        cdf, pdf = _gelu_parts32(v)
        got["aux"] = ((v * pdf + cdf).to(f32) * s).to(bf16)
        v = ((v * cdf).to(f32) * s).to(f32)
        if mutant == "bias_after_gelu":
            v = (v + bias.to(f32)[None, :]).to(f32)
    else:
        if ep & E.EPI_GELU:
            u = v.to(bf16)
            got["aux"] = u
            x = u.to(f32)
            v = (x * _gelu_parts32(x)[0]).to(f32)
        if ep & E.EPI_DROPOUT:
            v = (v * s).to(f32)
    if ep & E.EPI_MULAUX:
        v = (v * aux.to(f32)).to(f32)
    if ep & E.EPI_DGELU:
        x = aux.to(f32)
        cdf, pdf = _gelu_parts32(x)
        v = (v * (x * pdf + cdf).to(f32)).to(f32)
    if ep & E.EPI_RESIDUAL:
        v = (v + residual.to(f32)).to(f32)
    o = _trunc_bf16(v) if mutant == "truncate" else v.to(bf16)
    if ep & E.EPI_COLSUM:
        terms = o.to(f32) if mutant == "colsum_rounded" else v
        keep = torch.ones(Mx, 1, dtype=f32)
        if mutant == "colsum_slice_dropped":
            keep[256 + 64:256 + 80] = 0
        cs = colsum0.to(f32).clone()
        for r0 in range(0, Mx, 16):
            cs = (cs + (terms[r0:r0 + 16] * keep[r0:r0 + 16]).sum(0, dtype=f32)).to(f32)
        got["colsum"] = cs
    got["out"] = o
    if q8 is not None:
        fmt, scale, amax0 = q8
        src = v if mutant == "q8_from_fp32" else o
        got["q8"], amax = F.quantize_reference(src, scale, fmt, amax0)
        if mutant == "q8_amax_scaled":
            amax = max(amax0, float((o.float() * float(np.float32(scale))).abs().max()))
        got["q8_amax"] = amax
    return got


def operands(kind, family, route, seed=0, K=None, rows=M, N=N):
    K = K or K_MIN[route]
    fmt = A_FMT[kind]
    ep = EPIS[kind]
    if family == "integer":
        a8, b8 = F.integer_operands(rows, N, K, fmt, seed=seed)
        inv_a, inv_b = (1.0, 0.5) if ep & E.EPI_COLSUM else (2.0 ** -4, 2.0 ** -4)
    else:
        a8, b8, inv_a, inv_b = F.random_operands(rows, N, K, fmt, seed=seed)
    kw = {}
    if ep & E.EPI_BIAS:
        kw["bias"] = R.gen((N,), 400 + seed, 0.5)
    if ep & E.EPI_RESIDUAL:
        kw["residual"] = R.gen((rows, N), 500 + seed)
    if ep & E.EPI_MULAUX:
        kw["aux"] = R.gen_int((rows, N), 600 + seed, R.INT_AUX) if family == "integer" else R.gen((rows, N), 600 + seed, 1.1)
    if ep & E.EPI_DGELU:
        kw["aux"] = R.gen((rows, N), 600 + seed, 3.0)
    if ep & E.EPI_COLSUM:
        kw["colsum0"] = R.gen_int((N,), 700 + seed, R.INT_CS, dtype=f32)
    return a8, b8, inv_a, inv_b, fmt, ep, kw


def run(kind, family, route, mutant=None, q8=None, K=None):
    a8, b8, inv_a, inv_b, fmt, ep, kw = operands(kind, family, route, K=K)
    block = F.ROUTE_BLOCK[route][0]
    got = emulate(a8, b8, inv_a, inv_b, fmt, block, epilogue=ep, q8=q8, mutant=mutant, **kw)
    ref_kw = dict(kw)
    if ep & E.EPI_GELU:
        ref_kw["aux"] = got["aux"]
    if ep & E.EPI_DROPOUT:
        ref_kw.update(drop_p=P, drop_seed=SEED)
    ref = F.reference_gemm_fp8(a8, b8, inv_a, inv_b, fmt, route=route, epilogue=ep,
                               q8=None if q8 is None else (*q8, got["out"]), **ref_kw)
    tensors = {k: v for k, v in got.items() if k in ("out", "aux", "colsum")}
    if family == "random":
        tensors.pop("colsum", None)                                   # column sums: integer family only (exact)
    elif "colsum" in tensors:
        assert bool((ref["colsum"][1] == 0).all()), "integer column sums must be provably exact"
    R.check(tensors, ref, {"out": bf16, "aux": bf16, "colsum": f32}, what=f"{kind}/{family}/{route}/{mutant}")
    if q8 is not None:
        F.assert_bytes(got["q8"], ref["q8"], got["out"], q8[0], what=f"{kind} fp8 copy")
        assert got["q8_amax"] == ref["q8_amax"], f"fp8 copy running maximum {got['q8_amax']!r}, expected {ref['q8_amax']!r}"
    return got, ref


random_allowed = F.random_allowed

FAITHFUL = [(k, f, r) for k in ("plain", "bias", "dense", "fc1", "res", "mulaux_colsum") for f in ("integer", "random")
            for r in ("f8_w4", "f8_pp256p") if f == "integer" or random_allowed(r, k, K_MIN[r])]
FAITHFUL += [(k, f, "f8_pp256p") for k in ("dgelu_drop", "gelu_aux") for f in ("integer", "random")]


@pytest.mark.parametrize("kind,family,route", FAITHFUL)
def test_faithful_emulation_is_accepted(kind, family, route):
    run(kind, family, route)


def _saturating_scale(kind, family, fmt):
    """Three times the tensor-max scale of the call's own output: part of the copy saturates."""
    out = run(kind, family, "f8_w4")[0]["out"]
    return float(np.float32(3.0 * F.FMAX[fmt] / float(out.float().abs().max())))


# (fc1 has no random cell: the median condition fails with the measured c, see random_allowed)
@pytest.mark.parametrize("kind,fmt,family", [("fc1", F.E4M3, "integer"), ("mulaux_colsum", F.E5M2, "integer"), ("mulaux_colsum", F.E5M2, "random")])
def test_faithful_fp8_copy_is_accepted(kind, fmt, family):
    scale = _saturating_scale(kind, family, fmt)
    for amax0 in (1e-3, 1e9):                         # below the tensor's maximum, and above it (must not change)
        got, ref = run(kind, family, "f8_w4", q8=(fmt, scale, amax0))
        assert ref["q8_amax"] == max(amax0, float(got["out"].float().abs().max()))
        assert int((F.decode(got["q8"], fmt).abs() == F.FMAX[fmt]).sum()) > 100      # the scale saturates part of the tensor


MUTANTS = [
    ("dense", "random", "f8_w4", "drop_stage"), ("dense", "random", "f8_pp256p", "drop_stage"), ("dense", "integer", "f8_w4", "drop_stage"),
    ("dense", "random", "f8_w4", "step_twice"), ("res", "random", "f8_pp256p", "step_twice"),
    ("res", "random", "f8_w4", "wrong_format"), ("bias", "random", "f8_w4", "wrong_format"), ("res", "integer", "f8_w4", "wrong_format"),
    ("bias", "random", "f8_w4", "inv_a_only"), ("plain", "integer", "f8_w4", "inv_a_only"),
    ("dense", "random", "f8_w4", "block_from_neighbour"), ("dense", "integer", "f8_w4", "block_from_neighbour"),
    ("dense", "random", "f8_w4", "pending_from_previous"), ("mulaux_colsum", "integer", "f8_w4", "pending_from_previous"),
    ("bias", "random", "f8_w4", "truncate"), ("plain", "integer", "f8_w4", "truncate"), ("res", "random", "f8_pp256p", "truncate"),
    ("fc1", "integer", "f8_w4", "bias_after_gelu"),
    ("dense", "random", "f8_w4", "drop_row_shift"), ("dense", "integer", "f8_pp256p", "drop_row_shift"),
    ("mulaux_colsum", "integer", "f8_w4", "colsum_rounded"), ("mulaux_colsum", "integer", "f8_w4", "colsum_slice_dropped"),
]


@pytest.mark.parametrize("kind,family,route,mutant", MUTANTS)
def test_mutant_is_rejected(kind, family, route, mutant):
    with pytest.raises(AssertionError):
        run(kind, family, route, mutant)


@pytest.mark.parametrize("kind,fmt,family,mutant", [(k, f, fam, m) for m in ("q8_from_fp32", "q8_amax_scaled")
                                                    for k, f, fam in (("fc1", F.E4M3, "integer"), ("mulaux_colsum", F.E5M2, "random"))])
def test_fp8_copy_mutant_is_rejected(kind, fmt, family, mutant):
    with pytest.raises(AssertionError, match="fp8"):
        run(kind, family, "f8_w4", mutant, q8=(fmt, _saturating_scale(kind, family, fmt), 1e-3))


def test_truncation_is_caught_by_the_bias_statistic_alone():
    a8, b8, inv_a, inv_b, fmt, ep, kw = operands("plain", "random", "f8_w4")
    ref = F.reference_gemm_fp8(a8, b8, inv_a, inv_b, fmt, route="f8_w4")
    v, d = ref["out"]
    wide = R.bound(v, d, bf16) * 2.0
    with pytest.raises(AssertionError, match="rounding bias"):
        R.assert_within(emulate(a8, b8, inv_a, inv_b, fmt, 128, mutant="truncate")["out"], v, wide, dtype=bf16, median_limit=1.0)
    R.assert_within(emulate(a8, b8, inv_a, inv_b, fmt, 128)["out"], v, wide, dtype=bf16, median_limit=1.0)


# ---- column sums at the token count of the persistent GPU case (22 053 x 768 x 768, integer operands); 64 columns show it
def test_integer_colsum_at_the_persistent_token_count_is_exact_and_a_missing_slice_is_rejected():
    GM, GK = 86 * 256 + 37, 768
    a8, b8, inv_a, inv_b, fmt, ep, kw = operands("mulaux_colsum", "integer", "f8_w4", seed=5, K=GK, rows=GM, N=64)
    S = F.decode(a8, fmt).abs() @ F.decode(b8, F.E4M3).abs().t()
    assert float(S.max()) < 16384, float(S.max())                      # sum |a||b| per element (about 8 500), far below 2^24
    ref = F.reference_gemm_fp8(a8, b8, inv_a, inv_b, fmt, epilogue=ep, **kw)
    assert bool((ref["colsum"][1] == 0).all()) and bool((ref["out"][1] == 0).all())
    got = emulate(a8, b8, inv_a, inv_b, fmt, 128, epilogue=ep, **kw)
    R.check({"out": got["out"], "colsum": got["colsum"]}, ref, {"out": bf16, "colsum": f32}, what="integer colsum at M = 22053")
    bad = emulate(a8, b8, inv_a, inv_b, fmt, 128, epilogue=ep, mutant="colsum_slice_dropped", **kw)
    with pytest.raises(AssertionError, match="colsum"):
        R.check({"colsum": bad["colsum"]}, ref, {"colsum": f32}, what="integer colsum at M = 22053")


# ---- the median condition with the measured c: the table that decides the operand family of every GPU cell
TABLE = [(r, k, K) for r, Ks in (("f8_w4", (640, 768, 896, 1280)), ("f8_pp256p", (256, 320, 576, 768)))
         for K in Ks for k in ("plain", "bias", "dense", "fc1", "res", "mulaux_colsum", "dgelu_drop", "gelu_aux")]


@pytest.mark.parametrize("route,kind,K", TABLE, ids=[f"{r}-{k}-K{K}" for r, k, K in TABLE])
def test_median_condition_decides_the_operand_family(route, kind, K):
    """median bound / |ref| of the bf16 output with random operands and delta_mfma included: at most 2^-7 wherever
    random_allowed() lets the GPU matrix use random operands, and over it (or within 2 % of it: no cell sits on the limit)
    wherever it does not — those cells run with integer operands only, never with a relaxed limit."""
    rows = 192
    a8, b8, inv_a, inv_b, fmt, ep, kw = operands(kind, "random", route, seed=1, K=K, rows=rows)
    kw.pop("colsum0", None)
    ep &= ~E.EPI_COLSUM
    if ep & E.EPI_DROPOUT:
        kw.update(drop_p=P, drop_seed=SEED)
    if kind == "gelu_aux":
        pre = F.reference_gemm_fp8(a8, b8, inv_a, inv_b, fmt, route=route, epilogue=ep, aux=torch.zeros(rows, N), **kw)
        kw["aux"] = pre["aux"][0].to(bf16)
    v, d = F.reference_gemm_fp8(a8, b8, inv_a, inv_b, fmt, route=route, epilogue=ep, **kw)["out"]
    nz = v != 0
    med = float((R.bound(v, d, bf16) / v.abs())[nz].median())
    print(f"median bound/|ref| {route} {kind} K={K}: {med:.4f}")
    if random_allowed(route, kind, K):
        assert med <= 2.0 ** -7 * 0.99, med
    else:
        assert med > 2.0 ** -7 * 0.98, med
