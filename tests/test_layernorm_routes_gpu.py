"""Every LayerNorm kernel and form against the fp64 reference of tests/layernorm_reference.py with per-element bounds.

Every case writes into views of larger sentinel-filled buffers whose row strides exceed D (bf16: D + 64 k, fp32: D + 4 k,
inputs strided as well, k differing between the tensors of a call in every other case) and every sentinel byte must
survive; each case asserts the kernel that ran (mdt_last_route).  Operands come from the generator and scales the CPU
mutant tests (tests/test_layernorm_reference_cpu.py) prove the bounds against.

Instantiations reached, by route, dtype, vectors per lane NV (V8: 8-byte vectors) and form (bit 2 dropped copy, bit 1
column sums, bit 0 residual gradient):
  ln_fwd       bf16 NV 1 (D 8, 72, 128, 520 — masked tails 8, 72, 520), 3 V8 (768), 2 (776 masked, 1024), 6 (3072), 8 (4096);
               fp32 NV 1 (4, 132 masked — NV 1 is 256 wide), 3 (768), 4 (1024), 6 (1536), 8 (2048); rows 1, 5, 8197 (two rows
               in flight, the last workgroup with one row) at D 128 and 768
  ln_fwd_q8    bf16 NV 3 V8 e4m3 (768), NV 1 e5m2 (128), 8197 rows
  embedding    bf16 NV 3 V8 (768), 8197 rows
  ln_rows      NV 1-4 (D 256, 512, 768, 1024) x forms 0-7, rows 1, 3, 1031; 33 rows per wave under MDT_LN_BWD_WGS=8
  ln_generic   bf16 NV 1 (128, 256), 2 (512, 776 masked, 1024), 3 V8 (768), 6 (3072), 8 (4096: 64 KiB of dynamic LDS),
               fp32 NV 1 (128), 3 (768), 6 (1536), 8 (2048: 64 KiB) x forms 0-7 (the kernel has three shapes: no tail,
               tail, tail with column sums); 5 rows per wave at 32 791 rows
"""
import pytest
import torch

import tests.layernorm_reference as LR
from multimodaldiscussiontransformer_amd import _lib as L

pytestmark = pytest.mark.gpu

bf16, f32 = torch.bfloat16, torch.float32
DEV = "cuda"
LN_ENV = ("MDT_LN_GENERIC", "MDT_LN_BWD_WGS")
SEED = 4321
BIG_FWD = 8192 + 4 + 1           # some waves take a second row; the last workgroup has one row
BIG_BWD = 32768 + 4 * 5 + 3      # 5 rows per wave on the default grid, a short last wave


@pytest.fixture(scope="module")
def ops():
    from multimodaldiscussiontransformer_amd import ops as o
    assert torch.cuda.is_available(), "GPU tests need a device"
    return o


@pytest.fixture
def ln_env(monkeypatch):
    def set_env(env):
        for k in LN_ENV:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        L.reload_env()
    yield set_env
    monkeypatch.undo()
    L.reload_env()


def _pad(dtype):
    return 64 if dtype == bf16 else 4


def strided(t, k=1):
    """``t`` [rows, D] read through a view of a wider buffer (row stride D + k pads)."""
    rows, D = t.shape
    buf = torch.zeros(rows, D + k * _pad(t.dtype), dtype=t.dtype, device=t.device)
    buf[:, :D] = t
    return buf[:, :D]


def vec(n, init=None):
    """fp32[n] inside a guarded buffer."""
    return LR.Guarded(1, n, f32, DEV, ld=n + 5, pre=1, post=1, init=None if init is None else init[None, :])


def wholly_untouched(g):
    return bool((g.buf.view(g.itype) == g.bits).all())


def call_fwd(x, gamma, beta, eps, y, mean, rstd, q8=None):
    rows, D = x.shape
    if q8 is None:
        L.check(L.lib.mdt_layernorm_fwd(L.stream(), L.dt(x), rows, D, L.ptr(x), x.stride(0), L.ptr(gamma), L.ptr(beta), float(eps),
                                        L.ptr(y), y.stride(0), L.ptr(mean), L.ptr(rstd)), "mdt_layernorm_fwd")
    else:
        q, fmt, scale, amax = q8
        L.check(L.lib.mdt_layernorm_fwd_q8(L.stream(), L.dt(x), rows, D, L.ptr(x), x.stride(0), L.ptr(gamma), L.ptr(beta), float(eps),
                                           L.ptr(y), y.stride(0), L.ptr(mean), L.ptr(rstd), L.ptr(q), q.stride(0), int(fmt),
                                           L.ptr(scale), L.ptr(amax)), "mdt_layernorm_fwd_q8")
    torch.cuda.synchronize()


def call_bwd(dy, x, gamma, mean, rstd, add, dx, dgamma, dbeta, dxd, drop_p, seed, colsum):
    rows, D = x.shape
    L.check(L.lib.mdt_layernorm_bwd(L.stream(), L.dt(x), rows, D, L.ptr(dy), dy.stride(0), L.ptr(x), x.stride(0), L.ptr(gamma),
                                    L.ptr(mean), L.ptr(rstd), L.ptr(add), add.stride(0) if add is not None else 0, L.ptr(dx),
                                    dx.stride(0), L.ptr(dgamma), L.ptr(dbeta), L.ptr(dxd), dxd.stride(0) if dxd is not None else 0,
                                    float(drop_p), int(seed), L.ptr(colsum)), "mdt_layernorm_bwd")
    torch.cuda.synchronize()


def run_fwd(x, gamma, beta, eps, what, route="ln_fwd", q8=None):
    """One forward call into guarded outputs, checked against the reference; returns the stored (y, mean, rstd)."""
    rows, D = x.shape
    y = LR.Guarded(rows, D, x.dtype, DEV, ld=D + 2 * _pad(x.dtype))
    mean, rstd = vec(rows), vec(rows)
    call_fwd(x, gamma, beta, eps, y.view, mean.view[0], rstd.view[0], q8)
    assert L.last_route() == route, f"{what}: ran {L.last_route()}, expected {route}"
    for name, g in (("y", y), ("mean", mean), ("rstd", rstd)):
        assert g.untouched(), f"{what}: a write outside the view of {name}"
    ref = LR.reference_fwd(x, gamma, beta, eps)
    LR.check({"y": y.view, "mean": mean.view[0], "rstd": rstd.view[0]}, ref, {"y": x.dtype, "mean": f32, "rstd": f32}, what=what)
    return y.view, mean.view[0], rstd.view[0]


# ------------------------------------------------------------------------------------------------ forward
FWD = [(t, D, rows, eps) for t in (bf16, f32) for D in LR.FWD_DIMS[t] for rows, eps in ((5, 1e-5), (1, 1e-12))]
FWD += [(t, D, BIG_FWD, eps) for t in (bf16, f32) for D, eps in ((128, 1e-5), (768, 1e-12))]


def _tn(t):
    return "bf16" if t == bf16 else "f32"


@pytest.mark.parametrize("dtype,D,rows,eps", FWD, ids=[f"{_tn(t)}-D{D}-r{r}-eps{e:g}" for t, D, r, e in FWD])
def test_forward_within_fp64_bounds(dtype, D, rows, eps):
    o = LR.operands(rows, D, dtype, SEED + D, DEV)
    run_fwd(strided(o["x"]), o["gamma"], o["beta"], eps, f"fwd {_tn(dtype)} D={D} rows={rows} eps={eps:g}")


@pytest.mark.parametrize("dtype,D", [(bf16, 768), (f32, 768), (bf16, 776), (f32, 132)], ids=["bf16-768", "f32-768", "bf16-776", "f32-132"])
@pytest.mark.parametrize("eps", [1e-5, 1e-12])
def test_forward_special_rows(dtype, D, eps):
    """A constant row (variance 0: y = beta, mean = the constant, rstd = eps^-1/2, all exact but the rsqrt), a row of
    mean 1000 and spread 1, and in bf16 a row at the largest power of two whose squares still sum to a finite fp32
    number in any order."""
    o = LR.operands(5, D, dtype, SEED, DEV)
    x = o["x"]
    x[1] = 3.25
    x[2] = LR.far_mean_row(D, dtype, SEED, DEV)
    if dtype == bf16:
        x[3] = (x[3].float() * LR.largest_scale(D)).to(bf16)
    y, mean, rstd = run_fwd(strided(x), o["gamma"], o["beta"], eps, f"special rows {_tn(dtype)} D={D} eps={eps:g}")
    assert torch.equal(y[1], o["beta"]) and float(mean[1]) == 3.25


@pytest.mark.parametrize("dtype,D", [(bf16, 768), (f32, 128)], ids=["bf16-768", "f32-128"])
def test_forward_small_spread_shows_where_eps_enters(dtype, D):
    """Rows whose variance (2^-14 / 3) is of the order of eps = 1e-5: eps inside the square root, not after it."""
    o = LR.operands(5, D, dtype, SEED, DEV, x_scale=2.0 ** -7)
    run_fwd(strided(o["x"]), o["gamma"], o["beta"], 1e-5, f"small spread {_tn(dtype)} D={D}")


@pytest.mark.parametrize("D,fmt,fmax", [(768, 0, 448.0), (128, 1, 57344.0)], ids=["768-e4m3", "128-e5m2"])
def test_forward_with_fp8_copy_within_fp64_bounds(ops, D, fmt, fmax):
    """mdt_layernorm_fwd_q8 at more than 8192 rows: y / mean / rstd against the reference, the fp8 bytes and the running
    maximum against mdt_fp8_quantize of that y."""
    rows = BIG_FWD
    o = LR.operands(rows, D, bf16, SEED + 7, DEV)
    scale = torch.full((1,), fmax / 1.5, device=DEV)                   # part of the tensor saturates
    amax_a, amax_b = torch.full((1,), 1e-3, device=DEV), torch.full((1,), 1e-3, device=DEV)
    q = torch.full((rows + 2, D + 8), 0x55, device=DEV, dtype=torch.uint8)
    y, _, _ = run_fwd(strided(o["x"]), o["gamma"], o["beta"], 1e-5, f"fwd q8 D={D} fmt={fmt}", route="ln_fwd_q8",
                      q8=(q[1:rows + 1, :D], fmt, scale, amax_a))
    want = ops.fp8_quantize(y, fmt, scale=scale, amax=amax_b)
    assert torch.equal(q[1:rows + 1, :D], want), int((q[1:rows + 1, :D] != want).sum())
    assert bool((q[0] == 0x55).all()) and bool((q[rows + 1] == 0x55).all()) and bool((q[:, D:] == 0x55).all())
    assert float(amax_a) == float(amax_b) == float(y.float().abs().max())


def test_embedding_fused_forward_within_fp64_bounds():
    """mdt_bert_embed_ln_rows at more than 8192 rows: the stored sum against (word + type) + position rounded to bf16,
    then y / mean / rstd against LayerNorm of that stored sum."""
    rows, D, V, NP = BIG_FWD, 768, 997, 130
    word, pos, typ = LR.gen((V, D), 1, 1.0, bf16, DEV), LR.gen((NP, D), 2, 0.5, bf16, DEV), LR.gen((2, D), 3, 0.25, bf16, DEV)
    g = torch.Generator(device=DEV).manual_seed(5)
    ids = torch.randint(0, V, (rows,), generator=g, device=DEV, dtype=torch.int32)
    pos_ids = torch.randint(0, NP, (rows,), generator=g, device=DEV, dtype=torch.int32)
    types = torch.randint(0, 2, (rows,), generator=g, device=DEV, dtype=torch.int32)
    o = LR.operands(1, D, bf16, SEED + 9, DEV)
    xs, y = LR.Guarded(rows, D, bf16, DEV, ld=D + 64), LR.Guarded(rows, D, bf16, DEV, ld=D + 128)
    mean, rstd = vec(rows), vec(rows)
    L.check(L.lib.mdt_bert_embed_ln_rows(L.stream(), L.dt(word), rows, L.ptr(ids), L.ptr(types), L.ptr(pos_ids), L.ptr(word), L.ptr(pos),
                                         L.ptr(typ), D, L.ptr(o["gamma"]), L.ptr(o["beta"]), 1e-12, L.ptr(xs.view), xs.ld, L.ptr(y.view),
                                         y.ld, L.ptr(mean.view[0]), L.ptr(rstd.view[0])), "mdt_bert_embed_ln_rows")
    torch.cuda.synchronize()
    for name, gd in (("xs", xs), ("y", y), ("mean", mean), ("rstd", rstd)):
        assert gd.untouched(), f"embedding: a write outside the view of {name}"
    v, d = LR.reference_embed_sum(word, pos, typ, ids, types, pos_ids)
    LR.assert_within(xs.view, v, LR.bound(v, d, bf16), what="embedding xs", dtype=bf16)
    ref = LR.reference_fwd(xs.view, o["gamma"], o["beta"], 1e-12)
    LR.check({"y": y.view, "mean": mean.view[0], "rstd": rstd.view[0]}, ref, {"y": bf16, "mean": f32, "rstd": f32}, what="embedding")


# ------------------------------------------------------------------------------------------------ backward
def run_bwd(dtype, D, rows, form, route, what, drop_p=LR.P_DROP, int_dy=False, distinct=True, outputs=None):
    """One backward call in the form ``form`` into guarded outputs with non-zero starting sums, checked against the
    reference (``outputs``: the names to check; all by default)."""
    has_add, has_cs, dropped = bool(form & 1), bool(form & 2), bool(form & 4)
    o = LR.operands(rows, D, dtype, SEED + D + form, DEV, int_dy=int_dy)
    k = (1, 2, 3, 2, 3) if distinct else (1, 1, 1, 1, 1)            # row-stride pads of dy, x, add, dx, dxd
    dy, x = strided(o["dy"], k[0]), strided(o["x"], k[1])
    add = strided(o["add"], k[2]) if has_add else None
    _, mean, rstd = L_fwd_stats(x, o["gamma"], o["beta"])
    dx = LR.Guarded(rows, D, dtype, DEV, ld=D + k[3] * _pad(dtype))
    dxd = LR.Guarded(rows, D, dtype, DEV, ld=D + k[4] * _pad(dtype)) if dropped else None
    dg, db = vec(D, o["dgamma0"]), vec(D, o["dbeta0"])
    cs = vec(D, o["colsum0"]) if has_cs else None
    seed = 7000 + D + form
    call_bwd(dy, x, o["gamma"], mean, rstd, add, dx.view, dg.view[0], db.view[0], dxd.view if dropped else None, drop_p, seed,
             cs.view[0] if has_cs else None)
    assert L.last_route() == route, f"{what}: ran {L.last_route()}, expected {route}"
    guards = {"dx": dx, "dxd": dxd, "dgamma": dg, "dbeta": db, "colsum": cs}
    for name, g in guards.items():
        assert g is None or g.untouched(), f"{what}: a write outside the view of {name}"
    ref = LR.reference_bwd(dy, x, o["gamma"], mean, rstd, add=add, drop_p=drop_p, drop_seed=seed, dgamma0=o["dgamma0"],
                           dbeta0=o["dbeta0"], colsum0=o["colsum0"], want_dropped=dropped, want_colsum=has_cs,
                           dx_stored=dx.view, dxd_stored=dxd.view if dropped else None)
    got = {"dx": dx.view, "dgamma": dg.view[0], "dbeta": db.view[0]}
    if dropped:
        got["dxd"] = dxd.view
    if has_cs:
        got["colsum"] = cs.view[0]
    if outputs:
        got = {n: got[n] for n in outputs if n in got}
    LR.check(got, ref, {"dx": dtype, "dxd": dtype}, what=what)
    return ref


def L_fwd_stats(x, gamma, beta, eps=1e-5):
    """The forward's stored statistics of x (checked on their own by the forward tests), for the backward to read."""
    rows, D = x.shape
    y = torch.empty(rows, D, dtype=x.dtype, device=x.device)
    mean, rstd = torch.empty(rows, dtype=f32, device=x.device), torch.empty(rows, dtype=f32, device=x.device)
    call_fwd(x, gamma, beta, eps, y, mean, rstd)
    return y, mean, rstd


ROWS_D = (256, 512, 768, 1024)
# (dtype, D, switches, route)
KERNELS = ([(bf16, D, {}, "ln_rows") for D in ROWS_D] + [(bf16, D, {"MDT_LN_GENERIC": "1"}, "ln_generic") for D in ROWS_D]
           + [(bf16, D, {}, "ln_generic") for D in (128, 776, 3072, 4096)] + [(f32, D, {}, "ln_generic") for D in (128, 768, 1536, 2048)])
KIDS = [f"{r}-{_tn(t)}-D{D}" for t, D, _, r in KERNELS]


@pytest.mark.parametrize("form", LR.FORMS)
@pytest.mark.parametrize("dtype,D,env,route", KERNELS, ids=KIDS)
def test_backward_every_form_within_fp64_bounds(ln_env, dtype, D, env, route, form):
    """1031 rows: the last wave's block is short and some waves of the last workgroup have no row."""
    ln_env(env)
    run_bwd(dtype, D, 1031, form, route, f"bwd {route} {_tn(dtype)} D={D} form {form}", distinct=bool(form & 1) or form == 0 or form == 6)


@pytest.mark.parametrize("rows,form", [(1, 7), (3, 3), (3, 4)], ids=["r1-form7", "r3-form3", "r3-form4"])
@pytest.mark.parametrize("dtype,D,env,route", KERNELS, ids=KIDS)
def test_backward_few_rows(ln_env, dtype, D, env, route, rows, form):
    """One row, and three (waves with no row at all)."""
    ln_env(env)
    run_bwd(dtype, D, rows, form, route, f"bwd {route} {_tn(dtype)} D={D} rows={rows} form {form}")


WALK = [(bf16, 768, {}, "ln_rows", 7), (bf16, 1024, {}, "ln_rows", 2), (bf16, 256, {}, "ln_rows", 5),
        (bf16, 776, {}, "ln_generic", 7), (bf16, 768, {"MDT_LN_GENERIC": "1"}, "ln_generic", 6), (f32, 128, {}, "ln_generic", 5)]


@pytest.mark.parametrize("dtype,D,env,route,form", WALK, ids=[f"{r}-{_tn(t)}-D{D}-form{f}" for t, D, _, r, f in WALK])
def test_backward_wave_walks_33_rows(ln_env, dtype, D, env, route, form):
    """MDT_LN_BWD_WGS=8: 1031 rows in 8 workgroups, 33 consecutive rows per wave (the look-ahead loop, the 32-bit row
    offsets of ln_rows), the last wave short."""
    ln_env(dict(env, MDT_LN_BWD_WGS="8"))
    run_bwd(dtype, D, 1031, form, route, f"bwd 33 rows per wave {route} {_tn(dtype)} D={D} form {form}")


NODROP = [(bf16, 768, {}, "ln_rows"), (bf16, 128, {}, "ln_generic"), (f32, 768, {}, "ln_generic")]


@pytest.mark.parametrize("dtype,D,env,route", NODROP, ids=[f"{r}-{_tn(t)}-D{D}" for t, D, _, r in NODROP])
def test_backward_dropped_copy_with_p_zero_equals_dx(ln_env, dtype, D, env, route):
    ln_env(env)
    run_bwd(dtype, D, 1031, 7, route, f"bwd p=0 {route} {_tn(dtype)} D={D}", drop_p=0.0)


def test_backward_five_rows_per_wave_on_the_default_grid(ln_env):
    """32 791 rows of 128: 5 rows per wave without any switch.  The worst-case bound of a 32 791-term fp32 sum of
    generated values says nothing (check() would refuse it), so dy is integer-valued: dbeta is exact and is checked, dgamma and
    colsum are left to the 1031-row cases, whose bounds are real."""
    ln_env({})
    ref = run_bwd(bf16, 128, BIG_BWD, 7, "ln_generic", "bwd 32791 rows", int_dy=True, outputs=("dx", "dxd", "dbeta"))
    assert float(ref["dbeta"][1].max()) == 0.0, "dbeta of integer dy is not provably exact"


# ------------------------------------------------------------------------------------------------ refusals
def _refused(exc, fn, outs):
    with pytest.raises(L.MdtError) as e:
        fn()
    torch.cuda.synchronize()
    assert type(e.value) is exc and e.value.status == (-2 if exc is L.MdtUnsupported else -1), repr(e.value)
    for g in outs:
        assert wholly_untouched(g), "a refused call wrote to an output"


def _bwd_args(dtype, D, rows=5):
    o = LR.operands(rows, D, dtype, SEED, DEV)
    dx, dxd = LR.Guarded(rows, D, dtype, DEV, ld=D + _pad(dtype)), LR.Guarded(rows, D, dtype, DEV, ld=D + _pad(dtype))
    dg, db, cs = vec(D), vec(D), vec(D)
    mean, rstd = torch.zeros(rows, device=DEV), torch.ones(rows, device=DEV)
    return o, dx, dxd, dg, db, cs, mean, rstd


@pytest.mark.parametrize("dtype,D", [(bf16, 2560), (bf16, 3584), (bf16, 4104), (f32, 1280), (f32, 2052)],
                         ids=["bf16-2560", "bf16-3584", "bf16-4104", "f32-1280", "f32-2052"])
def test_widths_without_a_kernel_are_unsupported(ln_env, dtype, D):
    """5 and 7 vectors per lane are not instantiated and 8 is the ceiling: MdtUnsupported from the forward, the backward
    and the embedding front end, nothing written."""
    ln_env({})
    rows = 5
    o, dx, dxd, dg, db, cs, mean, rstd = _bwd_args(dtype, D)
    y, m, r = LR.Guarded(rows, D, dtype, DEV, ld=D + _pad(dtype)), vec(rows), vec(rows)
    x, dy, add = strided(o["x"]), strided(o["dy"]), strided(o["add"])
    _refused(L.MdtUnsupported, lambda: call_fwd(x, o["gamma"], o["beta"], 1e-5, y.view, m.view[0], r.view[0]), (y, m, r))
    _refused(L.MdtUnsupported, lambda: call_bwd(dy, x, o["gamma"], mean, rstd, add, dx.view, dg.view[0], db.view[0], dxd.view, 0.4, 1,
                                                cs.view[0]), (dx, dxd, dg, db, cs))
    _refused(L.MdtUnsupported, lambda: call_bwd(dy, x, o["gamma"], mean, rstd, None, dx.view, dg.view[0], db.view[0], None, 0.0, 1,
                                                None), (dx, dg, db))
    ids = torch.zeros(rows, dtype=torch.int32, device=DEV)
    table = strided(o["x"]).contiguous()
    _refused(L.MdtUnsupported, lambda: L.check(L.lib.mdt_bert_embed_ln_rows(
        L.stream(), L.dt(table), rows, L.ptr(ids), L.ptr(ids), L.ptr(ids), L.ptr(table), L.ptr(table), L.ptr(table), D, L.ptr(o["gamma"]),
        L.ptr(o["beta"]), 1e-5, None, 0, L.ptr(y.view), y.ld, L.ptr(m.view[0]), L.ptr(r.view[0])), "mdt_bert_embed_ln_rows"), (y, m, r))


def test_contract_violations_are_argument_errors(ln_env):
    """D no multiple of the vector, a row stride no multiple of it, a pointer off the 16-byte grid, p = 1 and fp32 rows
    into the fp8 entry: the argument error (status -1), nothing written."""
    ln_env({})
    rows = 5

    def fwd_case(x, y, dtype=bf16, q8=False):
        D = x.shape[1]
        gamma, beta = torch.ones(D, dtype=dtype, device=DEV), torch.zeros(D, dtype=dtype, device=DEV)
        m, r = vec(rows), vec(rows)
        q = torch.zeros(rows, D, dtype=torch.uint8, device=DEV)
        one = torch.ones(1, device=DEV)
        _refused(L.MdtError, lambda: call_fwd(x, gamma, beta, 1e-5, y.view, m.view[0], r.view[0], (q, 0, one, one) if q8 else None), (y, m, r))
        return gamma

    # D = 132 in bf16
    fwd_case(torch.zeros(rows, 132 + 64, dtype=bf16, device=DEV)[:, :132], LR.Guarded(rows, 132, bf16, DEV, ld=132 + 64))
    # row stride D + 4 in bf16: the input's, then the output's
    fwd_case(torch.zeros(rows, 128 + 4, dtype=bf16, device=DEV)[:, :128], LR.Guarded(rows, 128, bf16, DEV, ld=128 + 64))
    fwd_case(torch.zeros(rows, 128 + 64, dtype=bf16, device=DEV)[:, :128], LR.Guarded(rows, 128, bf16, DEV, ld=128 + 4))
    # x offset by 8 bytes
    flat = torch.zeros(rows * 192 + 8, dtype=bf16, device=DEV)
    x_off = flat[4:4 + rows * 192].view(rows, 192)[:, :128]
    assert x_off.data_ptr() % 16 == 8
    fwd_case(x_off, LR.Guarded(rows, 128, bf16, DEV, ld=128 + 64))
    # fp32 rows into the fp8 entry
    fwd_case(torch.zeros(rows, 128 + 4, dtype=f32, device=DEV)[:, :128], LR.Guarded(rows, 128, f32, DEV, ld=128 + 4), dtype=f32, q8=True)
    # the backward: p = 1, D = 132, a dx stride of D + 4, x off the grid
    o, dx, dxd, dg, db, cs, mean, rstd = _bwd_args(bf16, 128)
    x, dy, add = strided(o["x"]), strided(o["dy"]), strided(o["add"])
    outs = (dx, dxd, dg, db, cs)

    def bwd(x_=x, dy_=dy, dx_=dx, p=0.4, gamma=o["gamma"]):
        return lambda: call_bwd(dy_, x_, gamma, mean, rstd, add, dx_.view, dg.view[0], db.view[0], dxd.view, p, 1, cs.view[0])
    _refused(L.MdtError, bwd(p=1.0), outs)
    x_off.copy_(o["x"])
    _refused(L.MdtError, bwd(x_=x_off), outs)
    dx4 = LR.Guarded(rows, 128, bf16, DEV, ld=128 + 4)
    _refused(L.MdtError, bwd(dx_=dx4), outs + (dx4,))
    o2, dx2, dxd2, dg2, db2, cs2, _, _ = _bwd_args(bf16, 136)
    x2, dy2 = strided(o2["x"])[:, :132], strided(o2["dy"])[:, :132]
    _refused(L.MdtError, lambda: call_bwd(dy2, x2, o2["gamma"], mean, rstd, None, dx2.view[:, :132], dg2.view[0], db2.view[0], None, 0.0, 1,
                                          None), (dx2, dg2, db2))


def test_report_worst_error_over_bound():
    """Not a check of its own: prints the worst err / bound each output reached in this run (pytest -s, or the log)."""
    print("\nlayernorm worst err/bound: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(LR.WORST.items())))
    assert all(v <= 1.0 for v in LR.WORST.values())
