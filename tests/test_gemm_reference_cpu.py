"""The bounds of tests/gemm_reference.py can fail: a CPU emulation of the kernels' arithmetic (fp32 accumulation in 32-deep
K steps, fp32 epilogue in the kernels' order, round-to-nearest-even to bf16) passes assert_within, and each listed
mutant of it — a subtly wrong kernel — is rejected.  The shapes have the structure of the GPU matrix
(tests/test_gemm_routes_gpu.py): a ragged last row tile, a partial last K step, row strides wider than N; the operands
come from the same generator at the same scales."""
import numpy as np
import pytest
import torch

import tests.gemm_reference as R

BM = 32          # row tile of the emulated kernel (the ragged tail: rows 320..336 of M = 337)
M, N, K = 337, 320, 80
LDC = N + 8
P, SEED = 0.4, 1234
ALPHA = 0.75
f32 = torch.float32


def _rne_bf16(x):
    return x.to(torch.bfloat16)


def _trunc_bf16(x):
    bits = x.contiguous().view(torch.int32) & ~0xFFFF
    return bits.view(f32).to(torch.bfloat16)


def _gelu32(x):
    return (0.5 * x * (1.0 + torch.erf(x * 0.70710678118654752))).to(f32)


def _gelu_grad32(x):
    cdf = 0.5 * (1.0 + torch.erf(x * 0.70710678118654752))
    return (cdf + x * 0.3989422804014327 * torch.exp(-0.5 * x * x)).to(f32)


def emulate(a, b, *, trans_a=False, epilogue=0, alpha=1.0, bias=None, residual=None, aux=None, c_old=None, colsum0=None,
            out_dtype=torch.bfloat16, mutant=None):
    """One mdt_gemm call as the kernels compute it (op(B) = b^T, b stored [N, K]); returns the outputs the call writes,
    C as a [M, LDC] buffer so that its padding columns can be inspected."""
    ep = epilogue
    A = (a.t() if trans_a else a).to(f32)
    Bt = b.t().to(f32)
    Mx, Kx = A.shape
    acc = torch.zeros(Mx, N, dtype=f32)
    nsteps = (Kx + 31) // 32
    for s in range(nsteps):
        k0, k1 = 32 * s, min(32 * s + 32, Kx)
        if mutant == "drop_partial_k" and k1 - k0 < 32:
            continue
        part = (A[:, k0:k1] @ Bt[k0:k1, :]).to(f32)
        if mutant == "drop_kstep" and s == 1:
            part[16:32, 16:32] = 0                  # one 16 x 16 sub-tile misses one 32-deep step
        acc = (acc + part).to(f32)
    if mutant == "wrong_tail_row":
        acc[Mx - 3] = acc[Mx - 4]                   # a row of the ragged tail taken from its neighbour
    al = 1.0 if mutant == "alpha_ignored" else float(np.float32(alpha))
    v = (acc * al).to(f32)
    if ep & R.EPI_BIAS and mutant != "bias_omitted":
        v = (v + bias.to(f32)[None, :]).to(f32)
        if mutant == "bias_twice":
            v = (v + bias.to(f32)[None, :]).to(f32)
    got = {}
    s = torch.ones(Mx, N, dtype=f32)
    if ep & R.EPI_DROPOUT:
        ld = LDC if mutant == "drop_counter_ldc" else None
        s = R.drop_scale(Mx, N, P, SEED, counter_ld=ld).to(f32)
    if (ep & R.EPI_GELU) and (ep & R.EPI_AUX_GRAD):
        sa = torch.ones_like(s) * (s != 0) if mutant == "aux_grad_unscaled" else s
        got["aux"] = _rne_bf16((_gelu_grad32(v) * sa).to(f32))
        v = (_gelu32(v) * s).to(f32)
    else:
        if ep & R.EPI_GELU:
            u = _rne_bf16(v)
            got["aux"] = u
            v = _gelu32(u.to(f32))
        if ep & R.EPI_DROPOUT:
            v = (v * s).to(f32)
    if ep & R.EPI_MULAUX:
        v = (v * aux.to(f32)).to(f32)
    if ep & R.EPI_DGELU:
        v = (v * _gelu_grad32(aux.to(f32))).to(f32)
    if ep & R.EPI_RESIDUAL:
        v = (v + residual.to(f32)).to(f32)
    if ep & R.EPI_COLSUM:
        rows = v[: (Mx // BM) * BM] if mutant == "colsum_missing_last_tile" else v
        got["colsum"] = (colsum0.to(f32) + rows.sum(0, dtype=torch.float64).to(f32)).to(f32)
    if ep & (R.EPI_ACCUM | R.EPI_ATOMIC):
        v = (v + c_old.to(f32)).to(f32)
    if ep & R.EPI_ASUM:
        rs = A.sum(1, dtype=torch.float64).to(f32)
        got["asum"] = (colsum0.to(f32) + (rs * float(np.float32(alpha)) if mutant == "asum_scaled" else rs)).to(f32)
    cbuf = torch.full((Mx, LDC), float("nan"), dtype=out_dtype)
    cbuf[:, :N] = _trunc_bf16(v) if (mutant == "truncate" and out_dtype == torch.bfloat16) else v.to(out_dtype)
    got["out"] = cbuf[:, :N]
    return got


def case(kind):
    a = R.gen((M, K), 1)
    b = R.gen((N, K), 2, scale=R.b_scale(K))
    kw = {}
    if kind == "dense":            # o-proj / fc2 forward: bias, dropout, residual
        kw = dict(epilogue=R.EPI_BIAS | R.EPI_DROPOUT | R.EPI_RESIDUAL, bias=R.gen((N,), 3, 0.5), residual=R.gen((M, N), 4))
    elif kind == "fc1":            # bias, GELU, saved derivative, dropout
        kw = dict(epilogue=R.EPI_BIAS | R.EPI_GELU | R.EPI_AUX_GRAD | R.EPI_DROPOUT, bias=R.gen((N,), 3, 0.5))
    elif kind == "gelu_aux":
        kw = dict(epilogue=R.EPI_BIAS | R.EPI_GELU, bias=R.gen((N,), 3, 0.5))
    elif kind == "mulaux_colsum":  # d fc1: saved-derivative multiply, bias-gradient column sums
        kw = dict(epilogue=R.EPI_MULAUX | R.EPI_COLSUM, aux=R.gen((M, N), 5, 1.1), colsum0=R.gen((N,), 6, dtype=f32))
    elif kind == "accum_colsum_f32":
        kw = dict(epilogue=R.EPI_ACCUM | R.EPI_COLSUM, c_old=R.gen((M, N), 7, dtype=f32), colsum0=R.gen((N,), 6, dtype=f32),
                  out_dtype=f32)
    elif kind == "dgelu_drop":
        kw = dict(epilogue=R.EPI_DGELU | R.EPI_DROPOUT, aux=R.gen((M, N), 8, 3.0))
    kw.setdefault("epilogue", 0)
    kw.setdefault("out_dtype", torch.bfloat16)
    return a, b, kw


def run(kind, mutant=None):
    a, b, kw = case(kind)
    out_dtype = kw.pop("out_dtype")
    got = emulate(a, b, alpha=ALPHA, out_dtype=out_dtype, mutant=mutant, **kw)
    ref_kw = {k: v for k, v in kw.items() if k in ("epilogue", "bias", "residual", "c_old", "colsum0")}
    aux = kw.get("aux")
    if kw["epilogue"] & R.EPI_GELU:
        aux = got["aux"]                            # the reference activates at the stored value, as the kernel does
    ref = R.reference(a, b, alpha=ALPHA, aux=aux, drop_p=P, drop_seed=SEED, **ref_kw)
    R.check(got, ref, {"out": out_dtype, "colsum": f32}, what=f"{kind}/{mutant}")


def run_asum(mutant=None):
    dy = R.gen((K, 256), 11)                        # stored [K, M]: the weight-gradient layout (trans_a)
    x = R.gen((N, K), 12, scale=R.b_scale(K))
    c0 = R.gen((256, N), 13, dtype=f32)
    cs0 = R.gen((256,), 14, dtype=f32)
    ep = R.EPI_ATOMIC | R.EPI_ASUM
    got = emulate(dy, x, trans_a=True, epilogue=ep, alpha=ALPHA, c_old=c0, colsum0=cs0, out_dtype=f32, mutant=mutant)
    ref = R.reference(dy, x, trans_a=True, alpha=ALPHA, epilogue=ep, c_old=c0, colsum0=cs0, split_k=1)
    R.check(got, ref, {"out": f32, "asum": f32}, what=f"asum/{mutant}")


FAITHFUL = ["plain", "dense", "fc1", "gelu_aux", "mulaux_colsum", "accum_colsum_f32", "dgelu_drop"]


@pytest.mark.parametrize("kind", FAITHFUL)
def test_faithful_emulation_is_accepted(kind):
    run(kind)


def test_faithful_asum_is_accepted():
    run_asum()


MUTANTS = [
    ("dense", "truncate"),
    ("dense", "drop_kstep"),
    ("dense", "drop_partial_k"),
    ("dense", "wrong_tail_row"),
    ("dense", "bias_omitted"),
    ("dense", "bias_twice"),
    ("dense", "alpha_ignored"),
    ("dense", "drop_counter_ldc"),
    ("plain", "truncate"),
    ("fc1", "aux_grad_unscaled"),
    ("mulaux_colsum", "colsum_missing_last_tile"),
    ("accum_colsum_f32", "drop_kstep"),
]


@pytest.mark.parametrize("kind,mutant", MUTANTS)
def test_mutant_is_rejected(kind, mutant):
    with pytest.raises(AssertionError):
        run(kind, mutant)


def test_asum_scaled_by_alpha_is_rejected():
    with pytest.raises(AssertionError):
        run_asum("asum_scaled")


def test_truncation_is_caught_by_the_bias_check_alone():
    """Truncation must fail the rounding-bias statistic even with a bound wide enough to let every element through."""
    a, b, _ = case("plain")
    got = emulate(a, b, alpha=ALPHA, mutant="truncate")["out"]
    v, d = R.reference(a, b, alpha=ALPHA)["out"]
    wide = R.bound(v, d, torch.bfloat16) * 2.0
    with pytest.raises(AssertionError, match="rounding bias"):
        R.assert_within(got, v, wide, dtype=torch.bfloat16)
    R.assert_within(emulate(a, b, alpha=ALPHA)["out"], v, wide, dtype=torch.bfloat16)


def test_dropout_port_matches_the_documented_hash():
    """Fixed points of the port: threshold and scale from the fp32 p, and the 2-counters-per-word split."""
    assert R.drop_params(0.4) == (26214, float(np.float32(1) / np.float32(0.6)))
    assert R.drop_params(0.0)[0] == 0
    c = torch.arange(0, 4096, dtype=torch.int64)
    keep = R.keep_bits(c, 0.4, 77)
    assert abs(float(keep.double().mean()) - 0.6) < 0.03
    assert bool(R.keep_bits(c, 0.0, 77).all())
    h = R._drop_mix(torch.tensor([0], dtype=torch.int64) ^ R.drop_key(77))
    assert bool(keep[0] == ((h & 0xFFFF) >= 26214).item()) and bool(keep[1] == ((h >> 16) >= 26214).item())


def test_guard_band_sees_a_stray_write():
    g = R.Guarded(5, 7, torch.bfloat16, "cpu", ld=16)
    g.view.fill_(1.0)
    assert g.untouched()
    g.buf[2, 7] = 0.0                               # one element past the last column of the first row
    assert not g.untouched()


# ---- column sums at the token count of the persistent GPU routes (tests/test_gemm_routes_gpu.py, route pp256p: M = 22053,
# K = 576, integer operands from the same generator); 64 columns are enough to show that every mutant is seen
GM, GN, GK = 86 * 256 + 37, 64, 576


def emulate_colsum(mutant=None):
    """MULAUX | COLSUM as the kernels compute it: fp32 accumulation in 32-deep steps, fp32 product with the saved
    derivative, fp32 column sums of the unrounded results (in row tiles of 16, added in turn), bf16 output."""
    a, b = R.int_operands(GM, GN, GK, seed=5)
    aux = R.gen_int((GM, GN), 6, R.INT_AUX)
    cs0 = R.gen_int((GN,), 7, R.INT_CS, dtype=f32)
    A, Bt = a.to(f32), b.t().to(f32)
    acc = torch.zeros(GM, GN, dtype=f32)
    for k0 in range(0, GK, 32):
        acc = (acc + (A[:, k0:k0 + 32] @ Bt[k0:k0 + 32, :]).to(f32)).to(f32)
    v = (acc * aux.to(f32)).to(f32)
    terms = v
    if mutant == "rounded_terms":
        terms = v.to(torch.bfloat16).to(f32)              # summed after the rounding to C's type
    keep = torch.ones(GM, dtype=torch.bool)
    if mutant == "ragged_tail_dropped":
        keep[GM - 37:] = False                            # the 37 rows past the last full 256-row tile
    if mutant == "row_slice_dropped":
        keep[4096:4096 + 16] = False                      # one 16-row group of one tile
    cs = cs0.clone()
    for r0 in range(0, GM, 16):
        part = (terms[r0:r0 + 16] * keep[r0:r0 + 16, None]).sum(0, dtype=f32)
        cs = (cs + part).to(f32)
    got = {"out": v.to(torch.bfloat16), "colsum": cs}
    ref = R.reference(a, b, epilogue=R.EPI_MULAUX | R.EPI_COLSUM, aux=aux, colsum0=cs0)
    return got, ref


def test_colsum_at_gpu_token_count_is_exact_and_accepted():
    got, ref = emulate_colsum()
    assert bool((ref["colsum"][1] == 0).all())            # provably exact: the check is bit for bit
    R.check(got, ref, {"out": torch.bfloat16, "colsum": f32}, what="colsum at M = 22053")


@pytest.mark.parametrize("mutant", ["ragged_tail_dropped", "row_slice_dropped", "rounded_terms"])
def test_colsum_mutant_at_gpu_token_count_is_rejected(mutant):
    got, ref = emulate_colsum(mutant)
    with pytest.raises(AssertionError, match="colsum"):
        R.check(got, ref, {"out": torch.bfloat16, "colsum": f32}, what="colsum at M = 22053")


def test_fp32_sums_with_a_vacuous_bound_are_refused():
    """The worst-case bound of a 22053-term sum of random values is a large fraction of the sum: the non-vacuity check
    of the column sums refuses to call that a test."""
    a = R.gen((GM, GK), 8)
    b = R.gen((GN, GK), 9, scale=R.b_scale(GK))
    aux = R.gen((GM, GN), 10, 1.1)
    ref = R.reference(a, b, epilogue=R.EPI_MULAUX | R.EPI_COLSUM, aux=aux, colsum0=torch.zeros(GN, dtype=torch.float64))
    v, d = ref["colsum"]
    with pytest.raises(AssertionError, match="vacuous"):
        R.assert_within(v.float(), v, R.bound(v, d, f32), dtype=f32, median_limit=2.0 ** -7)
