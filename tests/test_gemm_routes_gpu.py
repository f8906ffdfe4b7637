"""Every GEMM route x the epilogue flag sets a training step launches x the shapes where kernels break, against the fp64
reference of tests/gemm_reference.py with per-element bounds.

Routes are forced with the library's switches (MDT_GEMM_ROUTE, MDT_GEMM_DYNAMIC) and every case asserts the route that ran
(mdt_last_route: a forced route whose preconditions fail runs the default one); each case writes C, the saved
aux tensor, the column sums and the row sums (MDT_EPI_ASUM) into views of larger sentinel-filled buffers whose row strides
exceed N, and every sentinel byte must survive the call.  Operands come from the generator and scales the CPU mutant
tests (tests/test_gemm_reference_cpu.py) prove the bounds against."""
import pytest
import torch

import tests.gemm_reference as R
from multimodaldiscussiontransformer_amd import _lib as L

pytestmark = pytest.mark.gpu

bf16, f32 = torch.bfloat16, torch.float32
P_DROP = 0.4
P256_M = 86 * 256 + 37        # 87 row tiles x 3 column tiles (N = 768) = 261 tiles: the last persistent round is partial

ROUTE_ENV = ("MDT_GEMM_ROUTE", "MDT_GEMM_DYNAMIC")

# route: (switches, the route that runs, dtype of A / B, M, N, K, trans_a, row-stride padding of C / residual / aux)
ROUTES = {
    "generic_f32": ({}, "generic", f32, 101, 70, 45, False, 3),
    "generic_bf16": ({}, "generic", bf16, 77, 130, 100, False, 3),                     # N % 128 != 0
    "generic_head": ({}, "generic", bf16, 300, 2, 768, False, 3),                      # the classifier head's N = 2, unaligned rows
    "tile128": ({"MDT_GEMM_ROUTE": "tile128"}, "tile128", bf16, 128 + 37, 256, 128, False, 8),
    "tile128_m13": ({"MDT_GEMM_ROUTE": "tile128"}, "tile128", bf16, 13, 256, 64, False, 8),             # M < 16, one K tile
    "tile128_kmajor": ({"MDT_GEMM_ROUTE": "tile128"}, "tile128", bf16, 256, 256, 200, True, 8),         # partial last 64-deep k-major tile
    "tile256x128": ({"MDT_GEMM_ROUTE": "tile256x128"}, "tile256x128", bf16, 256 + 255, 256, 192, False, 8),
    "pp256": ({"MDT_GEMM_ROUTE": "pp256"}, "pp256", bf16, 512 + 13, 512, 320, False, 8),
    "pp256_255tiles": ({}, "pp256", bf16, 85 * 256 - 1, 768, 576, False, 8),          # default choice, one tile short of persistence
    "pp256p": ({"MDT_GEMM_ROUTE": "pp256p"}, "pp256p", bf16, P256_M, 768, 576, False, 8),
    "pp256p_dynamic": ({"MDT_GEMM_ROUTE": "pp256p", "MDT_GEMM_DYNAMIC": "1"}, "pp256p", bf16, P256_M, 768, 640, False, 8),
    "w4p": ({"MDT_GEMM_ROUTE": "w4p"}, "w4p", bf16, P256_M, 768, 640, False, 8),
    # the 4-wave kernel forced, but K = 576 is 18 32-deep steps, fewer than its 18 explicit steps + 2: stays on pp256p
    "w4p_forced_8wave": ({"MDT_GEMM_ROUTE": "w4p"}, "pp256p", bf16, P256_M, 768, 576, False, 8),
    "w4p_default": ({}, "w4p", bf16, P256_M, 768, 768, False, 8),
    "splitk_pp256": ({"MDT_GEMM_ROUTE": "pp256"}, "pp256", bf16, 512, 512, 2013, True, 8),
    "splitk_w4s": ({"MDT_GEMM_ROUTE": "w4s"}, "w4s", bf16, 512, 512, 2013, True, 8),
    "asum_fallback": ({"MDT_GEMM_ROUTE": "tile128"}, "tile128", bf16, 512, 512, 2013, True, 8),
    # 1 x 3 tiles, more column than row tiles: split-K walks them column-major (group_n = 1); slabs of 512 / 512 / 512 / 477 k
    "splitk_pp256_colmajor": ({"MDT_GEMM_ROUTE": "pp256"}, "pp256", bf16, 256, 768, 2013, True, 8),
    "splitk_w4s_colmajor": ({"MDT_GEMM_ROUTE": "w4s"}, "w4s", bf16, 256, 768, 2013, True, 8),
    # the halved order (group_n = tiles_n / 2), the smallest shape that gets it on 256 CUs: B panels 12 x 256 x 768 x 2 = 4.7 MB
    # > 3.5 MB, one half 2.36 MB <= 2.5 MB, 86 x 12 = 1032 tiles >= 4 x 256
    "pp_halves": ({}, "w4p", bf16, 86 * 256, 3072, 768, False, 8),
    "pp_halves_8wave": ({"MDT_GEMM_ROUTE": "pp256p"}, "pp256p", bf16, 86 * 256, 3072, 768, False, 8),
}

E = R                         # the flag constants
EPIS = {   # name: (flags, B stored [K, N] — the input-gradient layout)
    "plain": (0, True),
    "bias": (E.EPI_BIAS, False),                                                     # qkv
    "dense": (E.EPI_BIAS | E.EPI_RESIDUAL | E.EPI_DROPOUT, False),                   # o-proj, fc2
    "fc1": (E.EPI_BIAS | E.EPI_GELU | E.EPI_AUX_GRAD | E.EPI_DROPOUT, False),
    "fc1_nodrop": (E.EPI_BIAS | E.EPI_GELU | E.EPI_AUX_GRAD, False),                 # HF blocks: no activation dropout
    "gelu_aux": (E.EPI_BIAS | E.EPI_GELU, False),
    "mulaux_colsum": (E.EPI_MULAUX | E.EPI_COLSUM, True),                            # d fc1
    "res": (E.EPI_RESIDUAL, True),                                                   # dgrad
    "dgelu_drop": (E.EPI_DGELU | E.EPI_DROPOUT, True),
    "accum": (E.EPI_ACCUM, False),
    "accum_colsum": (E.EPI_ACCUM | E.EPI_COLSUM, False),
    "atomic": (E.EPI_ATOMIC, True),
    "atomic_asum": (E.EPI_ATOMIC | E.EPI_ASUM, True),
}
ALL = ["plain", "bias", "dense", "fc1", "gelu_aux", "mulaux_colsum", "res", "dgelu_drop", "accum", "accum_colsum"]

# (route, epilogue, output dtype, K override, split_k)
MATRIX = (
    [("generic_f32", e, f32, None, 1) for e in ALL] + [("generic_f32", "atomic", f32, None, 3)]
    + [("generic_bf16", e, bf16, None, 1) for e in ALL] + [("generic_bf16", "accum_colsum", f32, None, 1)]
    + [("generic_head", e, f32, None, 1) for e in ("plain", "bias", "accum_colsum")] + [("generic_head", "plain", bf16, None, 1),
                                                                                          ("generic_head", "atomic", f32, None, 2)]
    + [("tile128", e, bf16, None, 1) for e in ALL]
    + [("tile128", e, f32, None, 1) for e in ("accum", "dgelu_drop", "accum_colsum")] + [("tile128", "atomic", f32, None, 2)]
    + [("tile128_m13", e, bf16, None, 1) for e in ("plain", "dense", "accum_colsum")]
    + [("tile128_kmajor", "plain", bf16, None, 1), ("tile128_kmajor", "atomic", f32, None, 1)]
    + [("tile256x128", e, bf16, None, 1) for e in ("plain", "dense", "fc1", "mulaux_colsum", "accum_colsum")]
    + [("tile256x128", "accum", f32, None, 1)]
    + [("pp256", e, bf16, None, 1) for e in ALL] + [("pp256", e, f32, None, 1) for e in ("accum_colsum", "dgelu_drop")]
    + [("pp256_255tiles", e, bf16, None, 1) for e in ("plain", "dense")]
    + [("pp256p", e, bf16, None, 1) for e in ALL + ["fc1_nodrop"]]
    + [("pp256p_dynamic", e, bf16, None, 1) for e in ("plain", "dense", "fc1_nodrop", "mulaux_colsum", "accum_colsum")]
    + [("w4p", e, bf16, None, 1) for e in ALL + ["fc1_nodrop"]]
    + [("w4p", "dense", bf16, k, 1) for k in (704, 1088)]                  # the 4-wave kernel's explicit-step edges
    + [("w4p_forced_8wave", e, bf16, None, 1) for e in ("dense", "mulaux_colsum")]
    + [("w4p_default", e, bf16, None, 1) for e in ("plain", "bias", "dense", "mulaux_colsum", "res")]
    + [("splitk_pp256", e, f32, None, 4) for e in ("atomic", "atomic_asum")]
    + [("splitk_w4s", e, f32, None, 4) for e in ("atomic", "atomic_asum")]
    + [("asum_fallback", "atomic_asum", f32, None, 4)]
    + [("splitk_pp256_colmajor", e, f32, None, 4) for e in ("atomic", "atomic_asum")]
    + [("splitk_w4s_colmajor", e, f32, None, 4) for e in ("atomic", "atomic_asum")]
    # alpha follows the row's index: the fc1 row sits where it gets 0.75.  At K = 768 and alpha = -1.25 the REFERENCE's own bound
    # for the GELU output is looser than assert_within accepts (median bound / |ref| 8.5e-3 > 2^-7, whatever kernel ran).
    + [("pp_halves", "plain", bf16, None, 1), ("pp_halves_8wave", "fc1_nodrop", bf16, None, 1), ("pp_halves", "dense", bf16, None, 1)]
)
ALPHAS = (1.0, 0.75, -1.25)
assert ALPHAS[MATRIX.index(("pp_halves_8wave", "fc1_nodrop", bf16, None, 1)) % len(ALPHAS)] == 0.75
SUM_ALPHAS = (1.0, -0.5, 2.0)  # column-sum cases: powers of two keep the integer results on a granule whose sums stay exact


def _ids(c):
    route, epi, od, k, split = c
    return f"{route}-{epi}-{'f32' if od == f32 else 'bf16'}" + (f"-K{k}" if k else "") + (f"-split{split}" if split > 1 else "")


@pytest.fixture
def route_env(monkeypatch):
    def set_route(env):
        for k in ROUTE_ENV:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        if env.get("MDT_GEMM_DYNAMIC") == "1":
            L.enable_dynamic_tile_queue()
        L.reload_env()
    return set_route


def run_case(ops, route, epi, out_dtype, K_over=None, split=1, alpha=1.0, nonfinite=False, seed=0):
    """One mdt_gemm call of the matrix: (outputs, fp64 reference, guarded buffers, the reference's inputs)."""
    _, _, dtype, M, N, K, ta, pad = ROUTES[route]
    K = K_over or K
    flags, tb = EPIS[epi]
    dev = "cuda"
    integer = bool(flags & (E.EPI_COLSUM | E.EPI_ASUM))   # column / row sums: exact operands, exact sums (gemm_reference.py)
    if integer:
        a, b = R.int_operands(M, N, K, ta, tb, seed, dtype=dtype, device=dev)
    else:
        a = R.gen((K, M) if ta else (M, K), 100 + seed, dtype=dtype, device=dev)
        b = R.gen((K, N) if tb else (N, K), 200 + seed, scale=R.b_scale(K), dtype=dtype, device=dev)
    if nonfinite:                                     # a NaN in one row of op(A), an Inf in one column of op(B)
        m0, n0, k0 = M // 2, N // 3, K // 2
        a[(k0, m0) if ta else (m0, k0)] = float("nan")
        b[(k0, n0) if tb else (n0, k0)] = float("inf")
    kw, ref_kw, guards = {}, {}, {}
    c0 = R.gen((M, N), 300 + seed, dtype=out_dtype, device=dev) if flags & (E.EPI_ACCUM | E.EPI_ATOMIC) else None
    C = R.Guarded(M, N, out_dtype, dev, ld=N + pad, init=c0)
    guards["C"] = C
    if c0 is not None:
        ref_kw["c_old"] = c0
    if flags & E.EPI_BIAS:
        kw["bias"] = ref_kw["bias"] = R.gen((N,), 400 + seed, 0.5, dtype=dtype, device=dev)
    if flags & E.EPI_RESIDUAL:
        res = R.Guarded(M, N, dtype, dev, ld=N + pad, init=R.gen((M, N), 500 + seed, dtype=dtype, device=dev))
        kw["residual"] = ref_kw["residual"] = res.view
    aux_out = None
    if flags & (E.EPI_MULAUX | E.EPI_DGELU):
        if integer:
            x = R.gen_int((M, N), 600 + seed, R.INT_AUX, dtype=dtype, device=dev)
        else:
            x = R.gen((M, N), 600 + seed, 1.1 if flags & E.EPI_MULAUX else 3.0, dtype=dtype, device=dev)
        ag = R.Guarded(M, N, dtype, dev, ld=N + pad, init=x)
        kw["aux"] = ref_kw["aux"] = ag.view
    if flags & E.EPI_GELU:
        aux_out = R.Guarded(M, N, dtype, dev, ld=N + pad)
        guards["aux"] = aux_out
        kw["aux"] = aux_out.view
    if flags & E.EPI_DROPOUT:
        kw["drop_p"] = P_DROP
        kw["drop_seed"] = ref_kw["drop_seed"] = 7000 + seed
        ref_kw["drop_p"] = P_DROP
    cs = None
    if flags & (E.EPI_COLSUM | E.EPI_ASUM):
        n_cs = M if flags & E.EPI_ASUM else N
        cs0 = R.gen_int((n_cs,), 700 + seed, R.INT_CS, dtype=f32, device=dev)
        cs = R.Guarded(1, n_cs, f32, dev, ld=n_cs + 5, pre=1, post=1, init=cs0[None, :])
        guards["colsum"] = cs
        ref_kw["colsum0"] = cs0
        kw["asum" if flags & E.EPI_ASUM else "colsum"] = cs.view[0]
    ep = flags & ~(E.EPI_BIAS | E.EPI_RESIDUAL | E.EPI_DROPOUT | E.EPI_COLSUM | E.EPI_ASUM)
    ops.gemm(a, b, trans_a=ta, trans_b=tb, out=C.view, epilogue=ep, alpha=alpha, split_k=split, **kw)
    torch.cuda.synchronize()
    assert L.last_route() == ROUTES[route][1], f"{route}-{epi}: ran {L.last_route()}, expected {ROUTES[route][1]}"
    if flags & E.EPI_GELU:
        ref_kw["aux"] = aux_out.view                  # without AUX_GRAD: activated at the stored value, as the kernel does
    ref = R.reference(a, b, trans_a=ta, trans_b=tb, alpha=alpha, epilogue=flags, split_k=split, **ref_kw)
    got = {"out": C.view}
    if aux_out is not None:
        got["aux"] = aux_out.view
    if cs is not None:
        got["asum" if flags & E.EPI_ASUM else "colsum"] = cs.view[0]
    return got, ref, guards, ref_kw


def _check(got, ref, guards, what):
    for name, g in guards.items():
        assert g.untouched(), f"{what}: a write outside the [rows, cols] view of {name} (guard band / row padding changed)"
    R.check(got, ref, {"out": got["out"].dtype, "aux": bf16, "colsum": f32, "asum": f32}, what=what)


@pytest.fixture(scope="module")
def ops():
    from multimodaldiscussiontransformer_amd import ops as o
    assert torch.cuda.is_available(), "GPU tests need a device"
    return o


@pytest.mark.parametrize("case", MATRIX, ids=[_ids(c) for c in MATRIX])
def test_gemm_route_epilogue_within_fp64_bounds(ops, route_env, case):
    route, epi, out_dtype, k_over, split = case
    i = MATRIX.index(case)
    if epi == "atomic_asum":
        alpha = 0.75                                  # ASUM: the row sums must ignore alpha
    else:
        alphas = SUM_ALPHAS if EPIS[epi][0] & E.EPI_COLSUM else ALPHAS
        alpha = alphas[i % len(alphas)]
    route_env(ROUTES[route][0])
    got, ref, guards, _ = run_case(ops, route, epi, out_dtype, k_over, split, alpha=alpha, seed=i)
    _check(got, ref, guards, f"{_ids(case)} alpha={alpha}")
    for name in ("colsum", "asum"):                   # exact operands: the column / row sums are checked bit for bit
        if name in got:
            assert bool((ref[name][1] == 0).all()), f"{name} case whose sums are not provably exact"


NONFINITE = [("generic_bf16", "plain"), ("generic_f32", "bias"), ("tile128", "bias"), ("tile256x128", "res"), ("pp256", "res"),
             ("pp256p", "plain"), ("w4p_default", "bias"), ("w4p", "res")]


@pytest.mark.parametrize("route,epi", NONFINITE, ids=[f"{r}-{e}" for r, e in NONFINITE])
def test_gemm_nonfinite_inputs_propagate_like_ieee(ops, route_env, route, epi):
    """A NaN in one row of op(A) and an Inf in one column of op(B): the output is non-finite exactly on that row and
    column (the reference's pattern), and the finite rest still meets its bound."""
    route_env(ROUTES[route][0])
    od = f32 if ROUTES[route][2] == f32 else bf16
    got, ref, guards, _ = run_case(ops, route, epi, od, alpha=0.75, nonfinite=True, seed=900)
    assert not bool(torch.isfinite(ref["out"][0]).all())
    _check(got, ref, guards, f"nonfinite {route}-{epi}")


@pytest.mark.parametrize("route", ["generic_f32", "generic_bf16", "tile128", "tile256x128", "pp256", "pp256p",
                                   "pp256p_dynamic", "w4p"])
def test_gemm_colsum_with_accum_sums_this_call_only(ops, route_env, route):
    """MDT_EPI_COLSUM with MDT_EPI_ACCUM (include/mdt_hip.h): the column sums are those of this call's fp32 result r, the
    old C not included and r not yet rounded to C's type — on every route.  Both other readings (sum of C_old + r, sum of
    the rounded r) fail the exact check."""
    route_env(ROUTES[route][0])
    od = f32 if route == "generic_f32" else bf16
    got, ref, guards, ref_kw = run_case(ops, route, "accum_colsum", od, alpha=1.0, seed=950)
    _check(got, ref, guards, f"colsum+accum {route}")
    v, d = ref["colsum"]
    other = v + ref_kw["c_old"].double().sum(0)
    with pytest.raises(AssertionError):
        R.assert_within(got["colsum"], other, R.bound(other, d, f32), dtype=f32)
    if od == bf16:
        r = ref["out"][0] - ref_kw["c_old"].double()                  # this call's result, exact
        rounded = ref_kw["colsum0"].double() + r.to(bf16).double().sum(0)
        assert not torch.equal(rounded, v)
        with pytest.raises(AssertionError):
            R.assert_within(got["colsum"], rounded, R.bound(rounded, d, f32), dtype=f32)


def test_dropout_port_equals_the_mask_kernel(ops):
    """The CPU port of the counter hash (tests/gemm_reference.py) against mdt_dropout_mask, bit for bit."""
    for p, seed, n in ((0.4, 77, (1 << 20) + 3), (0.1, 2 ** 63 + 5, 4099), (0.0, 1, 1000), (0.9, 123456789, 65537)):
        got = ops.dropout_mask(n, p, seed).bool()
        want = R.keep_bits(torch.arange(n, device="cuda", dtype=torch.int64), p, seed)
        assert torch.equal(got, want), f"p={p} seed={seed}: {int((got != want).sum())} of {n} keep-bits differ"
