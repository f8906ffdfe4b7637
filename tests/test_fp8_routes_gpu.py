"""Both 8-bit GEMM kernels (routes f8_w4 and f8_pp256p) x the flag sets they are built for x the shapes where they break, and
the fp8 quantiser, against the fp64 reference of tests/fp8_reference.py with per-element bounds.

Every GEMM case asserts the route that ran (mdt_last_route; MDT_GEMM_F8W=0 forces the 8-wave kernel), reads A and B through
views whose row strides exceed K, writes C, the saved aux tensor, the fp8 copy and the column sums into views of larger
sentinel-filled buffers whose row strides exceed N, and requires every sentinel byte to survive.  Two operand families
(tests/fp8_reference.py): "integer" — every bit of the result is determined, delta = 0, column sums exact — and "random", in the
cells where the median condition holds with the measured MFMA constant (fp8_reference.random_allowed, proved by tests/test_fp8_reference_cpu.py; fc1 and
most 32-k cells at K >= 576 are integer-only for that reason)."""
import numpy as np
import pytest
import torch

import tests.fp8_reference as F
import tests.gemm_reference as R
from multimodaldiscussiontransformer_amd import _lib as L

pytestmark = pytest.mark.gpu

bf16, f32 = torch.bfloat16, torch.float32
E = R
P_DROP = 0.4
W4, PP = "f8_w4", "f8_pp256p"
EPIS = {   # name: (flags, A format)
    "bias": (E.EPI_BIAS, F.E4M3),
    "dense": (E.EPI_BIAS | E.EPI_RESIDUAL | E.EPI_DROPOUT, F.E4M3),
    "fc1": (E.EPI_BIAS | E.EPI_GELU | E.EPI_AUX_GRAD, F.E4M3),
    "plain": (0, F.E5M2),
    "res": (E.EPI_RESIDUAL, F.E5M2),
    "mulaux_colsum": (E.EPI_MULAUX | E.EPI_COLSUM, F.E5M2),
    # flag sets neither kernel has an instantiation for: the generic (-1) epilogue of f8_pp256p
    "g_plain": (0, F.E4M3),
    "g_res": (E.EPI_RESIDUAL, F.E4M3),
    "g_mulaux_colsum": (E.EPI_MULAUX | E.EPI_COLSUM, F.E4M3),
    "g_bias": (E.EPI_BIAS, F.E5M2),
    "g_dgelu_drop": (E.EPI_DGELU | E.EPI_DROPOUT, F.E5M2),
    "g_gelu_aux": (E.EPI_BIAS | E.EPI_GELU, F.E4M3),
}
SPECIALISED = ["bias", "dense", "fc1", "plain", "res", "mulaux_colsum"]
GENERIC = ["g_plain", "g_res", "g_mulaux_colsum", "g_bias", "g_dgelu_drop", "g_gelu_aux"]
Q8_OF = {"fc1": F.E4M3, "mulaux_colsum": F.E5M2}          # the flag sets whose 4-wave instantiation also writes the fp8 copy
PERSIST = "P"                                             # M of the persistent cases: derived from the device's CU count


def persistent_m():
    """N = 768 gives 3 column tiles; the row-tile count is chosen so that the tile count exceeds the CU count by 4 to 6: some
    workgroups run a second tile and a pending half crosses a tile boundary (256 CUs: M = 86 * 256 + 37, 261 tiles)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    row_tiles = cus // 3 + 2
    assert 0 < 3 * row_tiles - cus < 8
    return (row_tiles - 1) * 256 + 37


def _kind(epi):
    return epi[2:] if epi.startswith("g_") else epi


def _families(route, epi, K):
    return ["integer", "random"] if F.random_allowed(route, _kind(epi), K) else ["integer"]


def _cases():
    c = []   # (route, force MDT_GEMM_F8W=0, epilogue, M, N, K, family, fused copy)
    def add(route, forced, epi, M, N, K, q8=False, families=None):
        for fam in families or _families(route, epi, K):
            c.append((route, forced, epi, M, N, K, fam, q8))
    for epi in SPECIALISED:                                   # f8_w4, one tile per workgroup: two row tiles, the second ragged
        add(W4, False, epi, 300, 256, 768)
    for epi in ("bias", "res"):                               # fewer rows than one MFMA block
        add(W4, False, epi, 13, 256, 768)
    for K in (640, 896, 1280):                                # five steps (the middle loop runs zero times), seven (odd), ten
        for epi in ("dense", "mulaux_colsum", "fc1"):
            add(W4, False, epi, 300, 256, K)
    for epi in SPECIALISED:                                   # f8_w4 persistent
        add(W4, False, epi, PERSIST, 768, 768)
    for epi in Q8_OF:
        add(W4, False, epi, PERSIST, 768, 768, q8=True, families=["integer"] + (["random"] if epi != "fc1" else []))
        add(W4, False, epi, 300, 256, 896, q8=True, families=["integer"])
    for K, epis in ((256, ("dense", "plain")), (320, ("mulaux_colsum", "bias")), (576, ("bias", "res", "fc1"))):   # f8_pp256p by shape
        for epi in epis:
            add(PP, False, epi, 300, 256, K)
    for K, epi in ((256, "bias"), (320, "res"), (576, "dense")):
        add(PP, False, epi, PERSIST, 768, K)
    for epi in SPECIALISED:                                   # f8_pp256p forced at a shape the 4-wave kernel takes
        add(PP, True, epi, 300, 256, 768)
    add(PP, True, "dense", PERSIST, 768, 768, families=["integer"])
    for epi in GENERIC:                                       # the generic instantiation: integer at K = 768, random at K = 256
        add(PP, False, epi, 300, 256, 768, families=["integer"])
        add(PP, False, epi, 300, 256, 256, families=["random"])
    add(PP, False, "g_mulaux_colsum", PERSIST, 768, 768, families=["integer"])
    # the halved tile order (group_n = tiles_n / 2 on 256 CUs; one byte per element): B panels 18 x 256 x 768 = 3.54 MB > 3.5 MB,
    # one half 1.77 MB <= 2.5 MB, 57 x 18 = 1026 tiles >= 4 x 256.  Last in the table: a case's seed is its index
    add(W4, False, "plain", 57 * 256, 4608, 768)
    return c


CASES = _cases()


def _id(c):
    route, forced, epi, M, N, K, fam, q8 = c
    return f"{route}{'-forced' if forced else ''}-{epi}{'-q8' if q8 else ''}-M{M}-N{N}-K{K}-{fam}"


@pytest.fixture
def f8w(monkeypatch):
    def set_(forced_8wave):
        if forced_8wave:
            monkeypatch.setenv("MDT_GEMM_F8W", "0")
        else:
            monkeypatch.delenv("MDT_GEMM_F8W", raising=False)
        L.reload_env()
    yield set_
    monkeypatch.delenv("MDT_GEMM_F8W", raising=False)
    L.reload_env()


@pytest.fixture(scope="module")
def ops():
    from multimodaldiscussiontransformer_amd import ops as o
    assert torch.cuda.is_available(), "GPU tests need a device"
    return o


def _dev(x):
    return torch.tensor([x], dtype=f32, device="cuda")


WORST = {}      # (route, flag set, family) -> worst err / bound over the cases run, for the closing report


class Call:
    """One mdt_gemm_fp8(_q8) call of the matrix with all its guarded buffers."""

    def __init__(self, epi, M, N, K, family, seed=0, q8=None, a_bytes=None):
        dev = "cuda"
        self.epi, self.M, self.N, self.K, self.family = epi, M, N, K, family
        self.flags, self.fmt = EPIS[epi]
        flags = self.flags
        if family == "integer":
            a8, b8 = F.integer_operands(M, N, K, self.fmt, seed=seed, device=dev)
            # powers of two: column-sum cases keep the integer granule coarse, the others land where GELU bends and bf16 rounds
            self.inv_a, self.inv_b = [(1.0, 1.0), (0.5, 1.0), (4.0, 0.5)][seed % 3] if flags & E.EPI_COLSUM else (2.0 ** -4, 2.0 ** -4)
        else:
            a8, b8, self.inv_a, self.inv_b = F.random_operands(M, N, K, self.fmt, seed=seed, device=dev)
        if a_bytes is not None:
            a_bytes(a8, b8)
        self.A = F.Guarded8(M, K, dev, ld=K + 16, init=a8)
        self.B = F.Guarded8(N, K, dev, ld=K + 48, init=b8)
        self.C = R.Guarded(M, N, bf16, dev, ld=N + 8)
        self.guards = {"C": self.C}
        self.kw, self.ref_kw = {}, {}
        if flags & E.EPI_BIAS:
            self.kw["bias"] = self.ref_kw["bias"] = R.gen((N,), 400 + seed, 0.5, device=dev)
        if flags & E.EPI_RESIDUAL:
            res = R.Guarded(M, N, bf16, dev, ld=N + 8, init=R.gen((M, N), 500 + seed, device=dev))
            self.kw["residual"] = self.ref_kw["residual"] = res.view
        self.aux_out = None
        if flags & (E.EPI_MULAUX | E.EPI_DGELU):
            if flags & E.EPI_DGELU:
                x = R.gen((M, N), 600 + seed, 3.0, device=dev)
            elif family == "integer":
                x = R.gen_int((M, N), 600 + seed, R.INT_AUX, device=dev)
            else:
                x = R.gen((M, N), 600 + seed, 1.1, device=dev)
            self.kw["aux"] = self.ref_kw["aux"] = R.Guarded(M, N, bf16, dev, ld=N + 8, init=x).view
        if flags & E.EPI_GELU:
            self.aux_out = R.Guarded(M, N, bf16, dev, ld=N + 8)
            self.guards["aux"] = self.aux_out
            self.kw["aux"] = self.aux_out.view
        if flags & E.EPI_DROPOUT:
            self.kw["drop_p"] = self.ref_kw["drop_p"] = P_DROP
            self.kw["drop_seed"] = self.ref_kw["drop_seed"] = 9000 + seed
        self.cs = None
        if flags & E.EPI_COLSUM:
            cs0 = R.gen_int((N,), 700 + seed, R.INT_CS, dtype=f32, device=dev)
            self.cs = R.Guarded(1, N, f32, dev, ld=N + 5, pre=1, post=1, init=cs0[None, :])
            self.guards["colsum"] = self.cs
            self.ref_kw["colsum0"] = cs0
            self.kw["colsum"] = self.cs.view[0]
        self.q8 = None
        if q8 is not None:
            fmt, scale, amax0 = q8
            self.q8 = q8
            self.Q = F.Guarded8(M, N, dev, ld=N + 8)
            self.guards["q8"] = self.Q
            self.amax = R.Guarded(1, 1, f32, dev, ld=4, pre=1, post=1, init=torch.full((1, 1), amax0, dtype=f32, device=dev))
            self.guards["q8_amax"] = self.amax
            self.kw.update(q8_out=self.Q.view, q8_format=fmt, q8_scale=_dev(scale), q8_amax=self.amax.view[0])

    def launch(self, ops):
        ep = self.flags & (E.EPI_GELU | E.EPI_AUX_GRAD | E.EPI_MULAUX | E.EPI_DGELU)
        ops.gemm_fp8(self.A.view, self.B.view, _dev(self.inv_a), _dev(self.inv_b), a_format=self.fmt, out=self.C.view, epilogue=ep, **self.kw)
        torch.cuda.synchronize()

    def check(self, route, what):
        assert L.last_route() == route, f"{what}: ran {L.last_route()}, expected {route}"
        assert self.A.untouched() and self.B.untouched(), f"{what}: an operand buffer changed"
        for name, g in self.guards.items():
            assert g.untouched(), f"{what}: a write outside the [rows, cols] view of {name} (guard band / row padding changed)"
        ref_kw = dict(self.ref_kw)
        if self.flags & E.EPI_GELU:
            ref_kw["aux"] = self.aux_out.view              # without AUX_GRAD: activated at the stored value, as the kernel does
        ref = F.reference_gemm_fp8(self.A.view, self.B.view, self.inv_a, self.inv_b, self.fmt, route=route, epilogue=self.flags,
                                   q8=None if self.q8 is None else (*self.q8, self.C.view), **ref_kw)
        got = {"out": self.C.view}
        if self.aux_out is not None:
            got["aux"] = self.aux_out.view
        if self.cs is not None and self.family == "integer":
            got["colsum"] = self.cs.view[0]
            assert bool((ref["colsum"][1] == 0).all()), f"{what}: a column-sum case whose sums are not provably exact"
        if self.family == "integer" and not self.flags & (E.EPI_GELU | E.EPI_DGELU | E.EPI_DROPOUT | E.EPI_BIAS | E.EPI_RESIDUAL):
            assert bool((ref["out"][1] == 0).all()), f"{what}: an integer case whose result is not determined bit for bit"
        v, d = ref["out"]
        fin = torch.isfinite(v)
        ratio = torch.where(fin, (self.C.view.double() - v).abs() / R.bound(v, d, bf16).clamp(min=1e-300), torch.zeros_like(v))
        key = (route, self.epi + ("+q8" if self.q8 else ""), self.family)
        WORST[key] = max(WORST.get(key, 0.0), float(ratio.max()) if ratio.numel() else 0.0)
        R.check(got, ref, {"out": bf16, "aux": bf16, "colsum": f32}, what=what)
        if self.q8 is not None:
            F.assert_bytes(self.Q.view, ref["q8"], self.C.view, self.q8[0], what=f"{what} fp8 copy")
            assert float(self.amax.view[0, 0]) == ref["q8_amax"], f"{what}: running maximum {float(self.amax.view[0, 0])!r}, expected {ref['q8_amax']!r}"
        return ref


def _q8_args(ops, epi, M, N, K, family, seed, amax0=2.0 ** -6):
    """(format, a scale three times the tensor-max scale of the call's own output — part of the copy saturates —, a maximum slot
    that starts above zero) and the bf16 output of the call without the copy."""
    plain = Call(epi, M, N, K, family, seed=seed)
    plain.launch(ops)
    fmt = Q8_OF[epi]
    scale = float(np.float32(3.0 * F.FMAX[fmt] / float(plain.C.view.float().abs().max())))
    return (fmt, scale, amax0), plain.C.view


@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_gemm_fp8_route_epilogue_within_fp64_bounds(ops, f8w, case):
    route, forced, epi, M, N, K, family, q8 = case
    M = persistent_m() if M == PERSIST else M
    seed = CASES.index(case)
    f8w(forced)
    q8_args = None
    if q8:
        q8_args, plain_out = _q8_args(ops, epi, M, N, K, family, seed)
    call = Call(epi, M, N, K, family, seed=seed, q8=q8_args)
    call.launch(ops)
    ref = call.check(route, _id(case))
    if q8:
        assert torch.equal(call.C.view, plain_out), "the bf16 output differs from the call without the fp8 copy"
        sat = int((F.decode(ref["q8"], q8_args[0]).abs() == F.FMAX[q8_args[0]]).sum())
        assert 0 < sat < ref["q8"].numel() // 2, f"{sat} saturated bytes: the scale must saturate part of the tensor"
        assert ref["q8_amax"] > q8_args[2]


@pytest.mark.parametrize("epi", ["fc1", "mulaux_colsum"])
def test_gemm_fp8_copy_keeps_a_running_maximum_above_the_tensors(ops, f8w, epi):
    f8w(False)
    q8_args, _ = _q8_args(ops, epi, 300, 256, 768, "integer", 77, amax0=1.0e9)
    call = Call(epi, 300, 256, 768, "integer", seed=77, q8=q8_args)
    call.launch(ops)
    ref = call.check(W4, f"amax above the tensor's, {epi}")
    assert ref["q8_amax"] == 1.0e9 == float(call.amax.view[0, 0])


UNSERVED = [("bias", 768, False, F.E4M3), ("fc1", 768, False, F.E5M2), ("fc1", 576, False, F.E4M3), ("mulaux_colsum", 768, True, F.E5M2),
            ("g_gelu_aux", 768, False, F.E4M3)]


@pytest.mark.parametrize("epi,K,forced,q8_fmt", UNSERVED, ids=[f"{e}-K{k}{'-forced' if f else ''}-to{q}" for e, k, f, q in UNSERVED])
def test_gemm_fp8_copy_no_kernel_serves_is_refused_and_writes_nothing(ops, f8w, epi, K, forced, q8_fmt):
    """A flag set, copy format, K or switch for which no kernel writes the fp8 copy: MdtUnsupported, every output untouched."""
    f8w(forced)
    call = Call(epi, 300, 256, K, "integer", seed=5, q8=(q8_fmt, 1.0, 0.5))
    cs_before = call.cs.buf.clone() if call.cs is not None else None
    with pytest.raises(L.MdtUnsupported):
        call.launch(ops)
    torch.cuda.synchronize()
    assert F.pristine(call.C) and F.pristine(call.Q) and (call.aux_out is None or F.pristine(call.aux_out))
    assert float(call.amax.view[0, 0]) == 0.5 and call.amax.untouched()
    assert cs_before is None or torch.equal(call.cs.buf.view(torch.int32), cs_before.view(torch.int32))


NONFINITE = [(W4, False, "bias", 0x7F, "NaN"), (PP, True, "res", 0x7F, "NaN"), (W4, False, "res", 0x7C, "e5m2 Inf"),
             (PP, True, "res", 0xFC, "e5m2 -Inf")]


@pytest.mark.parametrize("route,forced,epi,code,name", NONFINITE, ids=[f"{r}-{e}-{n.replace(' ', '_')}" for r, _, e, _, n in NONFINITE])
def test_gemm_fp8_nonfinite_operands_propagate_like_ieee(ops, f8w, route, forced, epi, code, name):
    """A NaN (or e5m2 infinity) byte in one row of A and a NaN byte in one column of B: the output is non-finite exactly on that
    row and that column, and the finite rest still meets its bound."""
    M, N, K = 300, 256, 768
    f8w(forced)

    def poison(a8, b8):
        a8[M // 2, K // 2 + 3] = code
        if name == "NaN":
            b8[N // 3, K // 5] = 0x7F

    call = Call(epi, M, N, K, "random", seed=900, a_bytes=poison)
    call.launch(ops)
    ref = call.check(route, f"nonfinite {route}-{epi}-{name}")
    bad = ~torch.isfinite(ref["out"][0])
    want = torch.zeros(M, N, dtype=torch.bool, device="cuda")
    want[M // 2] = True
    if name == "NaN":
        want[:, N // 3] = True
    assert torch.equal(bad, want) and torch.equal(~torch.isfinite(call.C.view.float()), want)


def test_gemm_fp8_refusals_raise_and_write_nothing(ops, f8w):
    f8w(False)
    dev = "cuda"
    one = _dev(1.0)

    def attempt(M, N, K, exc, lda=None, ldb=None, ldc=None, a_off=0, c_off=0, epilogue=0, what=""):
        A = torch.zeros(M * (lda or K) + 64, dtype=torch.uint8, device=dev)[a_off:].as_strided((M, K), (lda or K, 1))
        B = torch.zeros(N * (ldb or K) + 64, dtype=torch.uint8, device=dev).as_strided((N, K), (ldb or K, 1))
        C = R.Guarded(M + 1, (ldc or N) + 8, bf16, dev)
        out = C.buf.view(-1)[c_off:].as_strided((M, N), (ldc or N, 1))
        with pytest.raises(exc):
            ops.gemm_fp8(A, B, one, one, out=out, epilogue=epilogue)
        torch.cuda.synchronize()
        assert F.pristine(C), f"{what}: a refused call wrote to C"

    U = L.MdtUnsupported
    attempt(300, 384, 768, U, what="N % 256")
    attempt(300, 256, 672, U, what="K % 64")
    attempt(300, 256, 128, U, what="K < 256")
    attempt(300, 256, 768, U, lda=768 + 8, what="lda % 16")
    attempt(300, 256, 768, U, ldb=768 + 8, what="ldb % 16")
    attempt(300, 256, 768, U, ldc=256 + 4, what="ldc % 8")
    attempt(300, 256, 768, U, a_off=8, what="A not on a 16-byte boundary")
    attempt(300, 256, 768, U, c_off=4, what="C not on a 16-byte boundary")
    for flag in (E.EPI_ACCUM, E.EPI_ATOMIC):
        attempt(300, 256, 768, L.MdtError, epilogue=flag, what="ACCUM / ATOMIC")
    # M = 0: a no-op
    C = R.Guarded(4, 256, bf16, dev)
    ops.gemm_fp8(torch.zeros(0, 768, dtype=torch.uint8, device=dev), torch.zeros(256, 768, dtype=torch.uint8, device=dev), one, one,
                 out=C.buf[:0])
    torch.cuda.synchronize()
    assert F.pristine(C)


# ------------------------------------------------------------------------------------------------ the quantiser
def _grid(src_dtype):
    hi = torch.arange(65536, dtype=torch.int64, device="cuda")
    if src_dtype == bf16:
        return torch.where(hi >= 2 ** 15, hi - 2 ** 16, hi).to(torch.int16).view(bf16).view(256, 256)
    bits = (hi << 16) | ((hi * 40503) & 0xFFFF)         # every sign / exponent / leading-mantissa pattern, the low half varying
    return torch.where(bits >= 2 ** 31, bits - 2 ** 32, bits).to(torch.int32).view(f32).view(256, 256)


@pytest.mark.parametrize("fmt", [F.E4M3, F.E5M2])
@pytest.mark.parametrize("src_dtype", [bf16, f32], ids=["bf16", "f32"])
@pytest.mark.parametrize("scale", [1.0, 0.37, 3.0e4])
def test_quantiser_equals_the_reference_on_every_bf16_pattern_and_an_fp32_grid(ops, fmt, src_dtype, scale):
    """All 65 536 bf16 bit patterns / a 2^16-point fp32 grid through every exponent (NaN and Inf patterns, subnormal results and
    subnormal sources included): the bytes equal quantize_reference, any NaN code where the source is NaN."""
    x = _grid(src_dtype)
    q = ops.fp8_quantize(x, fmt, scale=_dev(scale))
    want, _ = F.quantize_reference(x, scale, fmt)
    assert int(((F.decode(want, fmt) != 0) & (F.decode(want, fmt).abs() < 2.0 ** (-6 if fmt == F.E4M3 else -14))).sum()) > 0
    F.assert_bytes(q, want, x, fmt, what=f"quantiser fmt {fmt} scale {scale}")
    fin = torch.isfinite(x.float()).all(1)
    xf = x[fin].contiguous()                            # rows without NaN / Inf: a finite running maximum
    amax = _dev(2.0 ** -100)
    F.assert_bytes(ops.fp8_quantize(xf, fmt, scale=_dev(scale), amax=amax), F.quantize_reference(xf, scale, fmt)[0], xf, fmt)
    assert float(amax) == F.quantize_reference(xf, scale, fmt, 2.0 ** -100)[1]


@pytest.mark.parametrize("fmt", [F.E4M3, F.E5M2])
@pytest.mark.parametrize("src_dtype", [bf16, f32], ids=["bf16", "f32"])
@pytest.mark.parametrize("rows,cols", [(3, 8), (301, 264), (2100, 2056)])      # less than one workgroup; odd sizes; more work than the grid covers in one stride
def test_quantiser_strided_source_and_guarded_destination(ops, fmt, src_dtype, rows, cols):
    g = torch.Generator(device="cuda").manual_seed(rows)
    x0 = (torch.randn(rows, cols, device="cuda", generator=g) * 3).to(src_dtype)
    src = R.Guarded(rows, cols, src_dtype, "cuda", ld=cols + 8, init=x0)
    for amax0 in (2.0 ** -7, 1.0e6):                    # below and above the tensor's own maximum
        dst = F.Guarded8(rows, cols, "cuda", ld=cols + 24)
        amax = R.Guarded(1, 1, f32, "cuda", ld=4, pre=1, post=1, init=torch.full((1, 1), amax0, device="cuda"))
        scale = F.scale_for(x0, fmt) * 4.0              # part of the tensor saturates
        ops.fp8_quantize(src.view, fmt, scale=_dev(scale), amax=amax.view[0], out=dst.view)
        torch.cuda.synchronize()
        want, want_amax = F.quantize_reference(x0, scale, fmt, amax0)
        assert dst.untouched() and amax.untouched() and src.untouched()
        F.assert_bytes(dst.view, want, x0, fmt, what=f"strided quantiser {rows}x{cols}")
        assert float(amax.view[0, 0]) == want_amax == max(amax0, float(x0.float().abs().max()))


@pytest.mark.parametrize("fmt", [F.E4M3, F.E5M2])
def test_quantiser_specials(ops, fmt):
    """NaN goes through as a NaN code, +-Inf saturates, the sign of a zero is kept, the running maximum becomes +inf with any
    NaN / Inf and is left alone by an all-zero tensor."""
    nan, inf = float("nan"), float("inf")
    x = torch.zeros(4, 16, device="cuda", dtype=f32)
    x[0, :8] = torch.tensor([nan, inf, -inf, 0.0, -0.0, 1.0, -2.5, 1e-30], device="cuda")
    x[3, 8:] = torch.tensor([-nan, 3.0e38, -3.0e38, 1.0e-45, -1.0e-45, 0.3, -0.3, 7.0], device="cuda")
    for dt in (f32, bf16):
        xs = x.to(dt)
        amax = _dev(0.25)
        q = ops.fp8_quantize(xs, fmt, scale=_dev(2.0), amax=amax)
        want, want_amax = F.quantize_reference(xs, 2.0, fmt, 0.25)
        F.assert_bytes(q, want, xs, fmt, what=f"specials fmt {fmt}")
        assert float(amax) == want_amax == inf
        d = F.decode(q, fmt)
        assert bool(torch.isnan(d[0, 0])) and float(d[0, 1]) == F.FMAX[fmt] and float(d[0, 2]) == -F.FMAX[fmt]
        assert q[0, 3:5].tolist() == [0x00, 0x80]
        z = torch.zeros(5, 24, device="cuda", dtype=dt)
        z[2, 3] = -0.0
        amax = _dev(0.25)
        qz = ops.fp8_quantize(z, fmt, scale=_dev(2.0), amax=amax)
        assert torch.equal(qz, F.quantize_reference(z, 2.0, fmt)[0]) and float(amax) == 0.25
        amax = _dev(0.0)
        ops.fp8_quantize(z, fmt, amax=amax)
        assert float(amax) == 0.0
        F.assert_bytes(ops.fp8_quantize(xs, fmt), F.quantize_reference(xs, 1.0, fmt)[0], xs, fmt, what="no scale = 1")


@pytest.mark.parametrize("fmt", [F.E4M3, F.E5M2])
@pytest.mark.parametrize("src_dtype", [bf16, f32], ids=["bf16", "f32"])
def test_quantiser_largest_finite_values_are_maxima_not_infinities(ops, fmt, src_dtype):
    """The finite values next to the top of the source type (bf16 0x7F7F = 3.39e38, FLT_MAX) are ordinary maxima: only NaN and
    Inf turn the running maximum into +inf (the all-pattern grids leave these out: they share their rows with the NaN patterns)."""
    top = torch.finfo(src_dtype).max
    x = torch.zeros(3, 16, device="cuda", dtype=src_dtype)
    x[1, 5], x[2, 9], x[0, 0] = top, -top, 3.1e38
    amax = _dev(1.0)
    q = ops.fp8_quantize(x, fmt, scale=_dev(2.0 ** -120), amax=amax)
    want, want_amax = F.quantize_reference(x, 2.0 ** -120, fmt, 1.0)
    F.assert_bytes(q, want, x, fmt, what="largest finite values")
    assert want_amax == float(top) and float(amax) == want_amax, (float(amax), want_amax)
    q = ops.fp8_quantize(x, fmt)                         # unscaled: they saturate
    assert F.decode(q, fmt)[1, 5] == F.FMAX[fmt] and F.decode(q, fmt)[2, 9] == -F.FMAX[fmt]


def test_scale_update_margin_zero_and_infinite_maximum(ops):
    amax = torch.tensor([3.0, 0.0, float("inf"), 0.5, float("nan"), 9.0], device="cuda")
    scale = torch.tensor([1.0, 5.0, 6.0, 1.0, 7.0, 8.0], device="cuda")
    inv = torch.tensor([1.0, 0.2, 0.125, 1.0, 0.5, 0.25], device="cuda")
    fmax = torch.tensor([448.0, 448.0, 57344.0, 57344.0, 448.0, 448.0], device="cuda")
    ops.fp8_scale_update(amax[:5], scale[:5], inv[:5], fmax[:5], margin=4.0)
    s0, s3 = np.float32(448.0) / np.float32(12.0), np.float32(57344.0) / np.float32(2.0)
    assert scale.tolist() == [float(s0), 5.0, 6.0, float(s3), 7.0, 8.0]        # zero, infinite and NaN maxima keep their scale
    assert inv.tolist() == [float(np.float32(1.0) / s0), float(np.float32(0.2)), 0.125, float(np.float32(1.0) / s3), 0.5, 0.25]
    assert amax.tolist() == [0.0, 0.0, 0.0, 0.0, 0.0, 9.0]                     # the maxima are reset; the sixth site was not part of the call


def test_report_worst_error_over_bound():
    """Not a check of its own: prints how much of its bound every route and flag set used (run with -s)."""
    assert WORST, "the matrix did not run"
    for (route, epi, family), w in sorted(WORST.items()):
        print(f"worst err/bound  {route:10s} {epi:20s} {family:8s} {w:.3f}")
        assert w <= 1.0
