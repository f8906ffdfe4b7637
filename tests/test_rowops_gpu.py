"""Every row mover of csrc/rowops.hip against the fp64 reference of tests/rowops_reference.py: bit equality where the
reference says the bits are determined, its per-element bound elsewhere.

The C entry points are called directly so that strides are free: every output is a view (row stride > D) of a larger
sentinel-filled buffer and every sentinel byte must survive; every input is read through a strided view, the pads
differing between the tensors of a call in every other case.  mdt_row_axpby cases assert the kernel that ran
(mdt_last_route: "row_vec" / "row_scalar") and that the two kernels agree bit for bit on the same operands.  Operands and
forms are those tests/test_rowops_reference_cpu.py proves the bounds against.

Widths: fp32 vectors 4, 256 (one full sweep of the 64 lanes), 260 (a second sweep with one lane), 768, 1024; bf16 vectors 8,
512, 520, 768, 1024; scalar 2, 3, 65, 130.  Rows 1, 3, 4, 5, and 4099 (a partial last workgroup among 1025) at D 128 and 768."""
import pytest
import torch

import tests.rowops_reference as RR
from multimodaldiscussiontransformer_amd import _lib as L
from tests.rowops_reference import bf16, embed_operands, embed_rows, f32, node_operands, scatter_operands

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEED = 9731


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available(), "GPU tests need a device"


def _tn(t):
    return "bf16" if t == bf16 else "f32"


def _pad(dtype):
    return 64 if dtype == bf16 else 4


def strided(t, k=1, odd=False, shift=False):
    """``t`` [rows, D] (host) on the device behind a view of a wider buffer: row stride D + k pads (``odd``: one element
    more, no multiple of the vector), ``shift``: the view starts one element into its allocation (off the 16-byte grid)."""
    if t.dim() == 1:
        t = t[None, :]
    rows, D = t.shape
    ld = D + k * _pad(t.dtype) + (1 if odd else 0)
    flat = torch.zeros(rows * ld + 1, dtype=t.dtype, device=DEV)
    v = flat[1 if shift else 0:][:rows * ld].view(rows, ld)[:, :D]
    v.copy_(t)
    assert (v.data_ptr() % 16 != 0) == shift
    return v


class Out:
    """A guarded output [rows, D] holding ``init``: ``shift`` puts the view one element into its row (off the 16-byte grid)."""

    def __init__(self, init, k=2, odd=False, shift=False, post=3):
        rows, D = init.shape
        ld = D + k * _pad(init.dtype) + (1 if odd else 0)
        # 8 guard rows in front: whatever the stride, the view itself starts on the 16-byte grid
        self.g = RR.Guarded(rows, D + (1 if shift else 0), init.dtype, DEV, ld=ld, pre=8, post=post)
        self.view = self.g.view[:, 1:] if shift else self.g.view
        self.view.copy_(init)
        self.shift = shift
        assert (self.view.data_ptr() % 16 != 0) == shift

    def untouched(self):
        ok = self.g.untouched()
        if self.shift:
            ok = ok and bool((self.g.view[:, 0].contiguous().view(self.g.itype) == self.g.bits).all())
        return ok

    def wholly_untouched(self):
        return bool((self.g.buf.view(self.g.itype) == self.g.bits).all())


def _i32(t):
    return None if t is None else t.to(DEV).contiguous()


def call_axpby(dtype_code, nrows, D, dst, ldd, d, a, lda, am, alpha, b, ldb, bm, beta, accumulate):
    L.check(L.lib.mdt_row_axpby(L.stream(), dtype_code, nrows, D, dst, ldd, L.ptr(d[0]), d[1], d[2], d[3],
                                a, lda, L.ptr(am[0]), am[1], am[2], am[3], float(alpha),
                                b, ldb, L.ptr(bm[0]), bm[1], bm[2], bm[3], float(beta), int(accumulate)), "mdt_row_axpby")
    torch.cuda.synchronize()


def run_axpby(c: RR.Axpby, what, route, pads=(2, 1, 3), scalar_by=None, ref=None):
    """One call on the operands of ``c`` into a guarded destination; asserts the route, the guard bytes and the reference.
    ``scalar_by`` makes the call unvectorisable: "ld_dst" / "ld_a" / "ld_b" (a row stride off the vector), "ptr_dst" /
    "ptr_a" / "ptr_b" (a base pointer off 16 bytes).  Returns the destination buffer (host)."""
    D = c.dst0.shape[1]
    ref = ref if ref is not None else c.reference()              # first: it also asserts that every row is in range
    out = Out(c.dst0, pads[0], odd=scalar_by == "ld_dst", shift=scalar_by == "ptr_dst")
    dst = out.view

    def operand(t, alias, k, name):
        if alias:
            return dst
        if t is None:
            return None
        return strided(t, k, odd=scalar_by == "ld_" + name, shift=scalar_by == "ptr_" + name)

    a, b = operand(c.a, c.a_is_dst, pads[1], "a"), operand(c.b, c.b_is_dst, pads[2], "b")
    d, am, bm = ((_i32(m[0]),) + tuple(m[1:]) for m in (c.d, c.am, c.bm))
    call_axpby(L.dt(dst), c.nrows, D, L.ptr(dst), dst.stride(0), d, L.ptr(a), a.stride(0) if a is not None else 0, am, c.alpha,
               L.ptr(b), b.stride(0) if b is not None else 0, bm, c.beta, c.accumulate)
    assert L.last_route() == route, f"{what}: ran {L.last_route()}, expected {route}"
    assert out.untouched(), f"{what}: a write outside the destination view"
    got = dst.cpu()
    RR.check("row_axpby", got, ref, what=what)
    return got


def expected_route(dtype, D):
    return "row_vec" if RR.vn(dtype, D) > 1 else "row_scalar"


ALL_DIMS = [(t, D) for t in (f32, bf16) for D in RR.VEC_DIMS[t] + RR.SCALAR_DIMS]


@pytest.mark.parametrize("form", list(RR.AXPBY_FORMS))
@pytest.mark.parametrize("dtype,D", ALL_DIMS, ids=[f"{_tn(t)}-D{D}" for t, D in ALL_DIMS])
def test_row_axpby_every_form_and_width(dtype, D, form):
    """1, 3, 4 and 5 rows.  A vectorisable width runs a second time through the scalar kernel (a destination stride off
    the vector) and must give the same bits."""
    for i, n in enumerate(RR.ROWS):
        c = RR.axpby_case(form, n, D, dtype, SEED + D + n)
        ref = c.reference()
        what = f"{form} {_tn(dtype)} D={D} rows={n}"
        pads = (2, 1, 3) if i % 2 == 0 else (1, 1, 1)
        got = run_axpby(c, what, expected_route(dtype, D), pads, ref=ref)
        if RR.vn(dtype, D) > 1:
            again = run_axpby(c, what + " scalar", "row_scalar", pads, scalar_by="ld_dst", ref=ref)
            assert torch.equal(got.view(torch.uint8), again.view(torch.uint8)), f"{what}: the vector and the scalar kernel differ"


BIG = [(t, D) for t in (f32, bf16) for D in RR.BIG_DIMS]


@pytest.mark.parametrize("form", list(RR.AXPBY_FORMS))
@pytest.mark.parametrize("dtype,D", BIG, ids=[f"{_tn(t)}-D{D}" for t, D in BIG])
def test_row_axpby_4099_rows(dtype, D, form):
    """1025 workgroups of four rows, the last with three."""
    c = RR.axpby_case(form, RR.BIG_ROWS, D, dtype, SEED + D)
    run_axpby(c, f"{form} {_tn(dtype)} D={D} rows={RR.BIG_ROWS}", "row_vec")


WAYS = ("ld_dst", "ld_a", "ld_b", "ptr_dst", "ptr_a", "ptr_b")


@pytest.mark.parametrize("way", WAYS)
@pytest.mark.parametrize("dtype,D", [(f32, 260), (bf16, 520), (f32, 4), (bf16, 8)], ids=["f32-260", "bf16-520", "f32-4", "bf16-8"])
def test_row_axpby_takes_the_scalar_kernel_when_one_operand_is_not_vectorisable(dtype, D, way):
    """A row stride that is no multiple of the vector, or a base pointer one element off the 16-byte grid, on dst, on a
    alone and on b alone: the scalar kernel runs and agrees bit for bit with the vector kernel."""
    c = RR.axpby_case("general", 5, D, dtype, SEED + D)
    ref = c.reference()
    vec = run_axpby(c, f"general {_tn(dtype)} D={D}", "row_vec", ref=ref)
    sca = run_axpby(c, f"general {_tn(dtype)} D={D} {way}", "row_scalar", scalar_by=way, ref=ref)
    assert torch.equal(vec.view(torch.uint8), sca.view(torch.uint8))


def test_row_axpby_aliased_operand_off_the_grid():
    """rows_mix in place on a buffer that is not vectorisable: b (and a) alias a shifted destination."""
    for form in ("b_is_dst", "a_is_dst"):
        for dtype, D in ((f32, 260), (bf16, 520)):
            c = RR.axpby_case(form, 5, D, dtype, SEED)
            run_axpby(c, f"{form} shifted", "row_scalar", scalar_by="ptr_dst")


def _refused(fn, outs, status=-1):
    with pytest.raises(L.MdtError) as e:
        fn()
    torch.cuda.synchronize()
    assert e.value.status == status, repr(e.value)
    for o in outs:
        assert o.wholly_untouched(), "a refused call wrote to an output"


def _sentinel_out(rows, D, dtype, k=1, shift=False, odd=False):
    o = Out.__new__(Out)
    ld = D + k * _pad(dtype) + (1 if odd else 0)
    o.g = RR.Guarded(rows, D + (1 if shift else 0), dtype, DEV, ld=ld, pre=8)
    o.view = o.g.view[:, 1:] if shift else o.g.view
    o.shift = shift
    return o


def test_row_axpby_refusals_and_no_ops():
    """nrows = 0 is a no-op whatever the pointers; a null dst and a dtype the library does not know are argument errors;
    none writes anything or records a route."""
    D = 8
    a = strided(RR.values((4, D), 1, 1.0, f32))
    out = _sentinel_out(4, D, f32)
    run_axpby(RR.axpby_case("idx_dst", 1, 4, f32, SEED), "route marker", "row_vec")
    run_axpby(RR.axpby_case("idx_dst", 1, 3, f32, SEED), "route marker", "row_scalar")
    call_axpby(L.MDT_F32, 0, D, L.ptr(out.view), out.view.stride(0), RR.PLAIN, L.ptr(a), a.stride(0), RR.PLAIN, 1.0, None, 0, RR.PLAIN, 1.0, 0)
    call_axpby(L.MDT_F32, 0, D, None, 0, RR.PLAIN, None, 0, RR.PLAIN, 1.0, None, 0, RR.PLAIN, 1.0, 0)
    assert out.wholly_untouched() and L.last_route() == "row_scalar"
    _refused(lambda: call_axpby(L.MDT_F32, 4, D, None, D, RR.PLAIN, L.ptr(a), a.stride(0), RR.PLAIN, 1.0, None, 0, RR.PLAIN, 1.0, 0), (out,))
    _refused(lambda: call_axpby(7, 4, D, L.ptr(out.view), out.view.stride(0), RR.PLAIN, L.ptr(a), a.stride(0), RR.PLAIN, 1.0, None, 0,
                                RR.PLAIN, 1.0, 0), (out,))
    assert L.last_route() == "row_scalar", "a refused call recorded a route"


# ------------------------------------------------------------------------------------------------ scatter-add
@pytest.mark.parametrize("granule", (True, False), ids=["granule", "general"])
@pytest.mark.parametrize("dtype,D", [(f32, 4), (f32, 65), (f32, 260), (bf16, 8), (bf16, 130), (bf16, 520)],
                         ids=lambda v: _tn(v) if isinstance(v, torch.dtype) else f"D{v}")
def test_row_scatter_add(dtype, D, granule):
    """4099 source rows (every second row of the buffer, from row 1) onto 5 table rows of a guarded fp32 table with a
    non-zero start, a seventh of them skipped.  On the 1/16 granule every order of the atomics sums exactly: bit equality;
    general operands: the any-order bound, which must not be vacuous.  Then 5 rows, some table rows untouched."""
    for n in (RR.BIG_ROWS, 5):
        table0, idx, src = scatter_operands(n, D, dtype, SEED + D, granule)
        ref = RR.reference_scatter_add(table0, idx, src, n, 2, 1)
        if granule:
            assert bool(ref[2].all())
        table = Out(table0, k=1)
        s = strided(src, 2)
        ix = _i32(idx)
        L.check(L.lib.mdt_row_scatter_add_f32(L.stream(), L.dt(s), n, D, L.ptr(table.view), table.view.stride(0), L.ptr(ix), L.ptr(s),
                                              s.stride(0), 2, 1), "mdt_row_scatter_add_f32")
        torch.cuda.synchronize()
        assert table.untouched()
        RR.check("row_scatter_add", table.view.cpu(), ref, what=f"scatter {_tn(dtype)} D={D} n={n} granule={granule}", nonvacuous=True)


def test_row_scatter_add_refusals_and_no_ops():
    table = _sentinel_out(5, 8, f32)
    s = strided(RR.values((4, 8), 1, 1.0, f32))
    ix = torch.zeros(4, dtype=torch.int32, device=DEV)
    args = (L.ptr(table.view), table.view.stride(0), L.ptr(ix), L.ptr(s), s.stride(0), 1, 0)
    L.check(L.lib.mdt_row_scatter_add_f32(L.stream(), L.MDT_F32, 0, 8, *args), "nrows = 0")
    torch.cuda.synchronize()
    assert table.wholly_untouched()
    _refused(lambda: L.check(L.lib.mdt_row_scatter_add_f32(L.stream(), L.MDT_F32, 4, 8, None, 8, L.ptr(ix), L.ptr(s), s.stride(0), 1, 0), "null"), (table,))
    _refused(lambda: L.check(L.lib.mdt_row_scatter_add_f32(L.stream(), 7, 4, 8, *args), "dtype"), (table,), status=-2)


# ------------------------------------------------------------------------------------------------ embedding sums
VEC = [(t, D) for t in (f32, bf16) for D in RR.VEC_DIMS[t]]


def call_embed_sum(word, pos, typ, ids, types, out, seq_stride, off):
    M, Lq = ids.shape
    L.check(L.lib.mdt_bert_embed_sum(L.stream(), L.dt(word), M, Lq, L.ptr(ids), L.ptr(types), L.ptr(word), L.ptr(pos), L.ptr(typ),
                                     word.shape[1], L.ptr(out), out.stride(0), seq_stride, off), "mdt_bert_embed_sum")
    torch.cuda.synchronize()


def call_embed_rows(word, pos, typ, ids, types, pos_ids, out):
    L.check(L.lib.mdt_bert_embed_rows(L.stream(), L.dt(word), ids.numel(), L.ptr(ids), L.ptr(types), L.ptr(pos_ids), L.ptr(word),
                                      L.ptr(pos), L.ptr(typ), word.shape[1], L.ptr(out), out.stride(0)), "mdt_bert_embed_rows")
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype,D", VEC, ids=[f"{_tn(t)}-D{D}" for t, D in VEC])
def test_bert_embed_sum_and_rows(dtype, D):
    """out_seq_stride 8 > L = 5 and out_off 2: the two rows in front of every sequence and the one behind keep their
    content; the result equals mdt_bert_embed_rows with pos_ids = l bit for bit."""
    M, Lq, stride, off = 3, 5, 8, 2
    word, pos, typ, ids, types = embed_operands(M, Lq, D, dtype, SEED + D)
    out0 = RR.values((M * stride + 1, D), SEED, 1.0, dtype)
    orow, l = embed_rows(M, Lq, stride, off)
    ref = RR.reference_embed(out0, word, pos, typ, ids, types, l, orow)
    out = Out(out0, k=1)
    dw, dp, dt_, di, dty = word.to(DEV), pos.to(DEV), typ.to(DEV), ids.to(DEV), types.to(DEV)
    call_embed_sum(dw, dp, dt_, di, dty, out.view, stride, off)
    assert out.untouched()
    got = out.view.cpu()
    RR.check("bert_embed_sum", got, ref, what=f"embed sum {_tn(dtype)} D={D}")
    rows0 = RR.values((M * Lq, D), SEED + 1, 1.0, dtype)
    out_r = Out(rows0, k=2)
    call_embed_rows(dw, dp, dt_, di, dty, l.to(torch.int32).to(DEV), out_r.view)
    assert out_r.untouched()
    RR.check("bert_embed_rows", out_r.view.cpu(), RR.reference_embed(rows0, word, pos, typ, ids, types, l, torch.arange(M * Lq)),
             what=f"embed rows {_tn(dtype)} D={D}")
    assert torch.equal(out_r.view.cpu().view(torch.uint8), got[orow].view(torch.uint8)), "embed_sum and embed_rows differ"


def test_embed_sums_refuse_rows_they_cannot_vectorise():
    """vec16_ok: D no multiple of the vector, an output stride no multiple of it, an output pointer off the 16-byte grid;
    M = 0 / rows = 0 are no-ops."""
    M, Lq = 2, 3
    for dtype, D in ((f32, 8), (bf16, 16)):
        word, pos, typ, ids, types = (t.to(DEV) for t in embed_operands(M, Lq, D, dtype, SEED))
        pid = torch.zeros(M * Lq, dtype=torch.int32, device=DEV)
        w = RR.vn(dtype, D)
        bad_d = D - w // 2
        for out, Dc in ((_sentinel_out(M * Lq, D, dtype, odd=True), D), (_sentinel_out(M * Lq, D, dtype, shift=True), D),
                        (_sentinel_out(M * Lq, bad_d, dtype), bad_d)):
            def sum_(o=out, Dc=Dc):
                L.check(L.lib.mdt_bert_embed_sum(L.stream(), L.dt(word), M, Lq, L.ptr(ids), L.ptr(types), L.ptr(word), L.ptr(pos), L.ptr(typ),
                                                 Dc, L.ptr(o.view), o.view.stride(0), Lq, 0), "mdt_bert_embed_sum")

            def rows_(o=out, Dc=Dc):
                L.check(L.lib.mdt_bert_embed_rows(L.stream(), L.dt(word), M * Lq, L.ptr(ids), L.ptr(types), L.ptr(pid), L.ptr(word), L.ptr(pos),
                                                  L.ptr(typ), Dc, L.ptr(o.view), o.view.stride(0)), "mdt_bert_embed_rows")
            _refused(sum_, (out,))
            _refused(rows_, (out,))
        ok = _sentinel_out(M * Lq, D, dtype)
        L.check(L.lib.mdt_bert_embed_sum(L.stream(), L.dt(word), 0, Lq, L.ptr(ids), L.ptr(types), L.ptr(word), L.ptr(pos), L.ptr(typ), D,
                                         L.ptr(ok.view), ok.view.stride(0), Lq, 0), "M = 0")
        L.check(L.lib.mdt_bert_embed_rows(L.stream(), L.dt(word), 0, L.ptr(ids), L.ptr(types), L.ptr(pid), L.ptr(word), L.ptr(pos), L.ptr(typ),
                                          D, L.ptr(ok.view), ok.view.stride(0)), "rows = 0")
        torch.cuda.synchronize()
        assert ok.wholly_untouched()


# ------------------------------------------------------------------------------------------------ ViT
@pytest.mark.parametrize("HW", (32, 48))
@pytest.mark.parametrize("dtype", (f32, bf16), ids=_tn)
def test_vit_patchify(dtype, HW):
    """p = 16, C = 3: gw K = 1536 / 2304 elements per workgroup (the second no multiple of 256), ldc > K.  One rounding
    of an fp32 pixel: bit-equal to .to(dtype)."""
    I, C, p = 3, 3, 16
    K, gw = C * p * p, HW // p
    img = RR.values((I, C, HW, HW), SEED + HW, 2.0, f32)
    cols0 = RR.values((I * gw * gw, K), SEED, 1.0, dtype)
    cols = Out(cols0, k=1)
    dimg = img.to(DEV)
    L.check(L.lib.mdt_vit_patchify(L.stream(), L.dt(cols.view), I, C, HW, p, L.ptr(dimg), L.ptr(cols.view), cols.view.stride(0)), "mdt_vit_patchify")
    torch.cuda.synchronize()
    assert cols.untouched()
    ref = RR.reference_patchify(cols0, img, p)
    assert bool(ref[2].all())
    RR.check("vit_patchify", cols.view.cpu(), ref, what=f"patchify {_tn(dtype)} HW={HW}")


@pytest.mark.parametrize("dtype,D", ALL_DIMS, ids=[f"{_tn(t)}-D{D}" for t, D in ALL_DIMS])
def test_vit_assemble(dtype, D):
    """ldp > D, seq_stride 8 > np + 1 = 5, off 2: the rows between the sequences keep their content."""
    I, npatch, stride, off = 3, 4, 8, 2
    patches, cls, pos = RR.values((I * npatch, D), SEED + 1, 1.0, dtype), RR.values((D,), SEED + 2, 1.0, dtype), \
        RR.values((npatch + 1, D), SEED + 3, 0.5, dtype)
    tok0 = RR.values((I * stride + 1, D), SEED + 4, 1.0, dtype)
    tok = Out(tok0, k=2)
    dp = strided(patches, 1)
    dc, dpos = cls.to(DEV), pos.to(DEV)
    L.check(L.lib.mdt_vit_assemble(L.stream(), L.dt(dp), I, npatch, D, L.ptr(dp), dp.stride(0), L.ptr(dc), L.ptr(dpos), L.ptr(tok.view),
                                   tok.view.stride(0), stride, off), "mdt_vit_assemble")
    torch.cuda.synchronize()
    assert tok.untouched()
    RR.check("vit_assemble", tok.view.cpu(), RR.reference_assemble(tok0, patches, cls, pos, I, npatch, stride, off),
             what=f"assemble {_tn(dtype)} D={D}")


# ------------------------------------------------------------------------------------------------ graph node features
@pytest.mark.parametrize("with_src", (True, False), ids=["src", "no-src"])
@pytest.mark.parametrize("dtype,D", ALL_DIMS, ids=[f"{_tn(t)}-D{D}" for t, D in ALL_DIMS])
def test_graph_node_feature(dtype, D, with_src):
    """lds > D, every third node padding (no source row, degree 0); without src every node_row is negative and src is NULL."""
    B, Tn = 3, 4
    o = node_operands(B, Tn, D, dtype, SEED + D, with_src=with_src)
    x0 = RR.values((B * Tn, D), SEED, 1.0, dtype)
    x = Out(x0, k=1)
    src = strided(o["src"], 3) if with_src else None
    dev = {k: o[k].to(DEV) for k in ("in_emb", "out_emb", "token", "node_row", "ind", "outd")}
    L.check(L.lib.mdt_graph_node_feature(L.stream(), L.dt(x.view), B, Tn, D, L.ptr(src), src.stride(0) if with_src else 0, L.ptr(dev["node_row"]),
                                         L.ptr(dev["ind"]), L.ptr(dev["outd"]), L.ptr(dev["in_emb"]), L.ptr(dev["out_emb"]),
                                         L.ptr(dev["token"]), L.ptr(x.view), x.view.stride(0)), "mdt_graph_node_feature")
    torch.cuda.synchronize()
    assert x.untouched()
    ref = RR.reference_node_feature(x0, o["src"], o["node_row"], o["ind"], o["outd"], o["in_emb"], o["out_emb"], o["token"], B, Tn)
    RR.check("graph_node_feature", x.view.cpu(), ref, what=f"node feature {_tn(dtype)} D={D} src={with_src}")


# ------------------------------------------------------------------------------------------------ tanh
TANH_N = (1, 255, 257, 2048 * 256 + 3)


def _flat(init):
    return Out(init[None, :], k=1, post=1)


@pytest.mark.parametrize("n", TANH_N)
@pytest.mark.parametrize("dtype", (f32, bf16), ids=_tn)
def test_tanh_forward(dtype, n):
    """One element, a short last workgroup, one lane of a second workgroup, and 2048 * 256 + 3: the grid-stride loop takes a
    second trip.  0, ±2^-100, ±9.5 and arguments whose tanh is within 2^-8 of ±1 are among the inputs."""
    x = RR.tanh_inputs(n, dtype, SEED + n)
    y = _flat(RR.values((n,), SEED, 1.0, dtype))
    dx = x.to(DEV)
    L.check(L.lib.mdt_tanh_fwd(L.stream(), L.dt(dx), n, L.ptr(dx), L.ptr(y.view)), "mdt_tanh_fwd")
    torch.cuda.synchronize()
    assert y.untouched()
    got = y.view.cpu()[0]
    RR.check("tanh_fwd", got, RR.reference_tanh_fwd(x), what=f"tanh {_tn(dtype)} n={n}")
    assert float(got[0]) == 0.0 and float(got.abs().max()) <= 1.0


@pytest.mark.parametrize("n", TANH_N)
@pytest.mark.parametrize("dtype", (f32, bf16), ids=_tn)
def test_tanh_backward(dtype, n):
    """dx = dy (1 - t t) with t = 0, ±1 and |t| one unit roundoff (2^-24 / 2^-8) from 1 among the stored values."""
    t, dy = RR.near_one(n, dtype, SEED + n), RR.values((n,), SEED + 1, 2.0, dtype)
    dx = _flat(RR.values((n,), SEED, 1.0, dtype))
    dt_, ddy = t.to(DEV), dy.to(DEV)
    L.check(L.lib.mdt_tanh_bwd(L.stream(), L.dt(dt_), n, L.ptr(dt_), L.ptr(ddy), L.ptr(dx.view)), "mdt_tanh_bwd")
    torch.cuda.synchronize()
    assert dx.untouched()
    RR.check("tanh_bwd", dx.view.cpu()[0], RR.reference_tanh_bwd(t, dy), what=f"tanh_bwd {_tn(dtype)} n={n}")


def test_tanh_no_ops_and_bad_dtype():
    y = _sentinel_out(1, 16, f32)
    x = torch.zeros(16, device=DEV)
    L.check(L.lib.mdt_tanh_fwd(L.stream(), L.MDT_F32, 0, L.ptr(x), L.ptr(y.view)), "n = 0")
    L.check(L.lib.mdt_tanh_bwd(L.stream(), L.MDT_F32, 0, L.ptr(x), L.ptr(x), L.ptr(y.view)), "n = 0")
    torch.cuda.synchronize()
    assert y.wholly_untouched()
    _refused(lambda: L.check(L.lib.mdt_tanh_fwd(L.stream(), 7, 16, L.ptr(x), L.ptr(y.view)), "dtype"), (y,), status=-2)
    _refused(lambda: L.check(L.lib.mdt_tanh_bwd(L.stream(), 7, 16, L.ptr(x), L.ptr(x), L.ptr(y.view)), "dtype"), (y,), status=-2)


def test_report_worst_error_over_bound():
    """Not a check of its own: prints the worst err / bound each entry point reached in this run (pytest -s, or the log)."""
    print("\nrow movers worst err/bound: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(RR.WORST.items())))
    assert all(v <= 1.0 for v in RR.WORST.values())
