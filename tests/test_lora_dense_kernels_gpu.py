"""The epilogue forms of the adapter up-projection (mdt_lora_up_add_drop, mdt_lora_up_add_mul, mdt_lora_up_act) against
tests/lora_dense_reference.py, in bf16 (MFMA kernel) and fp32 (parity loops), on a sparse cross of
R in {1, 15, 16, 17, 255, 257, 1025}, N in {80, 128, 512, 3072} (R <= 17 there), n in {8, 16, 24, 64, 192}: every element within its
bound; operands that are column slices of guarded wider buffers whose other bytes keep their bits; dropped elements keep their
bits and p = 0 is mdt_lora_up_add bit for bit; the five activation kinds with and without dropout, without u and with h = pre,
and T = 0 bit-identical to mdt_act_fwd; one integer-operand case per form that has to come out exactly; routes, no float
atomics, refusals with status and message before any launch.  And the two old kernels at the widths the FFN brings:
mdt_lora_down at K = 3072, mdt_lora_wgrad at N = 3072 over 2 SLAB + 3 rows, exact on integer operands."""
import pytest
import torch

import tests.lora_dense_reference as DR
import tests.lora_reference as LR

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float32]
IDS = ["bf16", "fp32"]
# (R, N, n, j): j = which half of the [R, 2 N] buffer the wide operand is
CASES = [(1, 80, 8, 0), (15, 128, 16, 1), (16, 512, 24, 0), (17, 3072, 64, 1), (255, 80, 192, 1), (257, 128, 64, 0),
         (1025, 512, 8, 1), (16, 3072, 192, 0), (257, 512, 16, 1), (1025, 80, 24, 0), (255, 512, 192, 0), (1025, 128, 16, 1)]
SEED = 0x5EED1234ABCD


@pytest.fixture(scope="module")
def ops():
    from multimodaldiscussiontransformer_amd import ops as _ops
    return _ops


class Wide:
    """A [pre + R + post, 2 N] buffer of data; ``view`` is rows pre .. pre + R, columns j N .. (j + 1) N (row stride 2 N).
    others_untouched(): every element outside the view has the bits it was created with."""

    def __init__(self, R, N, j, dtype, seed, scale=1.0, integer=None, pre=2, post=3):
        shape = (pre + R + post, 2 * N)
        self.buf = LR.gen_int(shape, seed, integer, dtype, DEV) if integer else LR.gen(shape, seed, scale, dtype, DEV)
        self.itype = torch.int16 if dtype == torch.bfloat16 else torch.int32
        self.before = self.buf.clone()
        self.rows, self.cols = slice(pre, pre + R), slice(j * N, (j + 1) * N)
        self.view = self.buf[self.rows, self.cols]
        self.old = self.before[self.rows, self.cols]

    def others_untouched(self):
        same = self.buf.view(self.itype) == self.before.view(self.itype)
        same[self.rows, self.cols] = True
        return bool(same.all())

    def unchanged(self):
        return torch.equal(self.buf.view(self.itype), self.before.view(self.itype))


def _bits(x):
    return x.contiguous().view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32)


def _within(out, ref, dtype, what):
    v, d = ref
    LR.assert_within(out.cpu(), v, LR.bound(v, d, dtype), what=what, dtype=dtype)


def _within_act(out, ref, dtype, what):
    """Every element within its bound, as _within, without assert_within's rounding-bias statistic: that one expects values spread
    evenly over their binades, and activation outputs are not (h piles up at 0, u at 0, at 1 and under the derivative's maximum,
    where whole clusters sit on one side of a bf16 grid point).  The rounding itself is the cast that _drop and _mul share."""
    v, d = ref
    o = out.cpu().double()
    bnd = LR.bound(v, d, dtype)
    assert bool(torch.isfinite(o).all()) and bool(torch.isfinite(v).all()), what
    ratio = (o - v).abs() / bnd.clamp(min=1e-300)
    over = int((ratio > 1).sum())
    assert over == 0, f"{what}: {over} of {v.numel()} elements over their bound, worst err / bound {float(ratio.max()):.3g}"
    if dtype == torch.bfloat16 and what.endswith("h"):
        nz = v != 0
        assert float((bnd / v.abs())[nz].median()) <= 2.0 ** -7, f"{what}: vacuous bound"


def _scale(ops, R, N, p, seed):
    return DR.scale_of(ops.dropout_mask(R * N, p, seed) if p else None, p, R, N)


def _route(ops, name, dtype):
    assert ops.L.last_route() == (name if dtype == torch.bfloat16 else name + "_f32")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("R,N,n,j", CASES)
def test_up_add_drop(ops, R, N, n, j, p, dtype):
    y = Wide(R, N, j, dtype, 3)
    t = Wide(R, n, 1, dtype, 4)
    w = Wide(n, N, 1 - j, dtype, 5, scale=0.25, pre=1, post=1)
    sc = _scale(ops, R, N, p, SEED + R)
    ref = DR.up_add_drop(t.view.cpu(), w.view.cpu(), y.old.cpu(), 1.5, sc)
    before = ops.float_atomic_launches()
    ops.lora_up_add_drop(t.view, w.view, y.view, alpha=1.5, drop_p=p, drop_seed=SEED + R)
    _route(ops, "lora_up_drop", dtype)
    assert ops.float_atomic_launches() == before
    _within(y.view, ref, dtype, f"up_add_drop R={R} N={N} n={n} p={p}")
    dropped = (sc == 0).to(DEV)
    assert 0 < int(dropped.sum()) < R * N or R * N < 200
    assert torch.equal(_bits(y.view)[dropped], _bits(y.old)[dropped])            # a dropped element keeps its bits
    assert y.others_untouched() and t.unchanged() and w.unchanged()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("R,N,n,j", CASES)
def test_drop_p0_is_up_add(ops, R, N, n, j, dtype):
    y = Wide(R, N, j, dtype, 3)
    t = LR.gen((R, n), 4, 1.0, dtype, DEV)
    w = LR.gen((n, N), 5, 0.25, dtype, DEV)
    plain = y.old.clone()
    ops.lora_up_add(t, w, plain, alpha=0.75)
    ops.lora_up_add_drop(t, w, y.view, alpha=0.75, drop_p=0.0, drop_seed=SEED)
    assert torch.equal(_bits(y.view), _bits(plain)) and y.others_untouched()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("R,N,n,j", CASES)
def test_up_add_mul(ops, R, N, n, j, dtype):
    y = Wide(R, N, j, dtype, 6)
    aux = Wide(R, N, 1 - j, dtype, 7)
    t = Wide(R, n, 0, dtype, 8)
    w = LR.gen((n, N), 9, 0.25, dtype, DEV)
    ref = DR.up_add_mul(t.view.cpu(), w.cpu(), y.old.cpu(), aux.view.cpu(), 0.75)
    before = ops.float_atomic_launches()
    ops.lora_up_add_mul(t.view, w, y.view, aux.view, alpha=0.75)
    _route(ops, "lora_up_mul", dtype)
    assert ops.float_atomic_launches() == before
    _within(y.view, ref, dtype, f"up_add_mul R={R} N={N} n={n}")
    assert y.others_untouched() and aux.unchanged() and t.unchanged()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("R,N,n,j", CASES)
def test_up_act(ops, R, N, n, j, dtype):
    """every kind, with and without dropout: one launch writes h and u into guarded buffers of their own, a second one writes h
    over pre and takes no u — the same bits"""
    t = LR.gen((R, n), 11, 1.0, dtype, DEV)
    w = LR.gen((n, N), 12, 0.5, dtype, DEV)
    run = 0
    for kind in DR.KINDS:
        for p in (0.0, 0.1):
            pre = Wide(R, N, j, dtype, 13 + run, scale=2.0)
            sc = _scale(ops, R, N, p, SEED + run)
            ref = DR.up_act(kind, t.cpu(), w.cpu(), pre.old.cpu(), 0.5, sc)
            what = f"up_act {kind} R={R} N={N} n={n} p={p}"
            before = ops.float_atomic_launches()
            h = LR.Guarded(R, N, dtype, DEV, ld=N + 16)
            u = LR.Guarded(R, N, dtype, DEV, ld=N + 8)
            ops.lora_up_act(t, w, pre.view, kind, alpha=0.5, drop_p=p, drop_seed=SEED + run, out=h.view, u=u.view)
            _route(ops, "lora_up_act", dtype)
            _within_act(h.view, ref["h"], dtype, what + " h")
            _within_act(u.view, ref["u"], dtype, what + " u")
            assert h.untouched() and u.untouched() and pre.unchanged()
            out, none = ops.lora_up_act(t, w, pre.view, kind, alpha=0.5, drop_p=p, drop_seed=SEED + run, out=pre.view, want_u=False)
            assert none is None and out.data_ptr() == pre.view.data_ptr()
            assert torch.equal(_bits(pre.view), _bits(h.view)), what + " h in place"
            assert pre.others_untouched()
            assert ops.float_atomic_launches() == before
            run += 1


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", DR.KINDS)
def test_up_act_zero_t_is_act_fwd(ops, kind, dtype):
    R, N, n = 257, 512, 24
    pre = LR.gen((R, N), 21, 3.0, dtype, DEV)
    t = torch.zeros(R, n, dtype=dtype, device=DEV)
    w = LR.gen((n, N), 22, 0.5, dtype, DEV)
    for p in (0.0, 0.25):
        h0, u0 = ops.act_fwd(pre, kind, drop_p=p, drop_seed=SEED)
        h1, u1 = ops.lora_up_act(t, w, pre, kind, alpha=0.5, drop_p=p, drop_seed=SEED)
        assert torch.equal(_bits(h0), _bits(h1)) and torch.equal(_bits(u0), _bits(u1)), f"{kind} p={p}"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_integer_operands_are_exact(ops, dtype):
    """n = 64: two 32-k steps; R = 257: seventeen 16-row steps in two workgroups of rows; N = 128: two waves of columns.  Every
    value stays an integer below 256 in magnitude, so bf16 holds it exactly and a missing step shows as a wrong integer."""
    R, N, n = 257, 128, 64
    t = LR.gen_int((R, n), 31, 1, dtype, DEV)
    w = LR.gen_int((n, N), 32, 1, dtype, DEV)
    y0 = LR.gen_int((R, N), 33, 4, dtype, DEV)
    aux = LR.gen_int((R, N), 34, 1, dtype, DEV)
    acc = t.double() @ w.double()
    assert float(acc.abs().max()) > 16          # not a degenerate product
    sc = _scale(ops, R, N, 0.5, SEED).to(DEV)   # 0 or 2
    # drop
    ref = DR.up_add_drop(t.cpu(), w.cpu(), y0.cpu(), 1.0, sc.cpu())
    assert float(ref[1].max()) == 0.0
    y = y0.clone()
    ops.lora_up_add_drop(t, w, y, alpha=1.0, drop_p=0.5, drop_seed=SEED)
    assert torch.equal(y.double().cpu(), ref[0])
    # mul
    ref = DR.up_add_mul(t.cpu(), w.cpu(), y0.cpu(), aux.cpu(), 2.0)
    assert float(ref[1].max()) == 0.0
    y = y0.clone()
    ops.lora_up_add_mul(t, w, y, aux, alpha=2.0)
    assert torch.equal(y.double().cpu(), ref[0])
    # act: relu and linear are exact on exact sums
    v = y0.double() + acc
    for kind, hv, uv in (("relu", v.clamp(min=0) * sc, (v > 0).double() * sc), ("linear", v * sc, sc)):
        h, u = ops.lora_up_act(t, w, y0, kind, alpha=1.0, drop_p=0.5, drop_seed=SEED)
        assert torch.equal(h.double(), hv) and torch.equal(u.double(), uv.expand_as(hv)), kind


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_old_kernels_at_ffn_widths(ops, dtype):
    S = ops.LORA_WGRAD_SLAB
    R, F, n = 2 * S + 3, 3072, 24
    x = LR.gen_int((R, F), 41, 4, dtype, DEV)
    a = LR.gen_int((n, F), 42, 2, dtype, DEV)
    ref = LR.down(x[:33].cpu(), a.cpu(), 0.5)
    assert float(ref[1].max()) == 0.0
    tt = LR.Guarded(33, n, dtype, DEV, ld=n + 8)
    ops.lora_down(x[:33], a, out=tt.view, alpha=0.5)
    _within(tt.view, ref, dtype, "down K=3072")
    assert tt.untouched()
    t = LR.gen_int((R, n), 43, 2, dtype, DEV)
    dw0 = LR.gen_int((n, F), 44, 50, torch.float32, DEV)
    v, d = LR.wgrad(t.cpu(), x.cpu(), dw0.cpu(), 2.0, S)
    assert float(d.max()) == 0.0
    dw = LR.Guarded(n, F, torch.float32, DEV, ld=F + 4, init=dw0)
    before = ops.float_atomic_launches()
    ops.lora_wgrad(t, x, dw.view, alpha=2.0)
    assert ops.float_atomic_launches() == before and dw.untouched()
    assert torch.equal(dw.view.double().cpu(), v)


def test_zero_rows_is_a_noop(ops):
    for dtype in DTYPES:
        w = LR.gen((8, 16), 1, 1.0, dtype, DEV)
        y = torch.empty(0, 16, dtype=dtype, device=DEV)
        t = torch.empty(0, 8, dtype=dtype, device=DEV)
        ops.lora_up_add_drop(t, w, y, drop_p=0.5, drop_seed=1)
        ops.lora_up_add_mul(t, w, y, y)
        ops.lora_up_act(t, w, y, "gelu", out=y)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_refusals(ops, dtype):
    from multimodaldiscussiontransformer_amd._lib import MdtError
    R, N = 32, 64
    y = LR.gen((R, N), 1, 1.0, dtype, DEV)
    keep = y.clone()
    aux = LR.gen((R, N), 2, 1.0, dtype, DEV)
    ops.lora_down(y, LR.gen((8, N), 2, 1.0, dtype, DEV))
    route = ops.L.last_route()

    def refused(fn, *words):
        with pytest.raises(MdtError) as e:
            fn()
        assert e.value.status == -1
        for wd in words:
            assert wd in str(e.value), str(e.value)

    def three(t, w, yy, *words, aux_=aux):
        refused(lambda: ops.lora_up_add_drop(t, w, yy, drop_p=0.1, drop_seed=3), "mdt_lora_up_add_drop", *words)
        refused(lambda: ops.lora_up_add_mul(t, w, yy, aux_), "mdt_lora_up_add_mul", *words)
        refused(lambda: ops.lora_up_act(t, w, yy, "gelu", out=yy), "mdt_lora_up_act", *words)

    for n in (4, 12, 200):                       # not a multiple of 8, or outside 8 ... 192
        three(LR.gen((R, n), 3, 1.0, dtype, DEV), LR.gen((n, N), 2, 1.0, dtype, DEV), y, f"n={n}")
    t, w = LR.gen((R, 16), 3, 1.0, dtype, DEV), LR.gen((16, N), 2, 1.0, dtype, DEV)
    y40 = y[:, :40]
    three(t, w[:, :40], y40, "N=40", aux_=aux[:, :40])
    for p in (1.0, -0.125):
        refused(lambda: ops.lora_up_add_drop(t, w, y, drop_p=p, drop_seed=3), "drop_p", f"{p:f}"[:5])
        refused(lambda: ops.lora_up_act(t, w, y, "relu", drop_p=p, drop_seed=3, out=y), "drop_p", f"{p:f}"[:5])
    refused(lambda: ops.lora_up_act(t, w, y, 7, out=y), "kind 7")
    # a row stride shorter than the row, straight to the library (torch has no such view)
    es = ops.dt(y)
    st = ops.lib.mdt_lora_up_add_mul(ops.stream(), es, R, 16, N, t.data_ptr(), 16, w.data_ptr(), N, y.data_ptr(), N, aux.data_ptr(), N - 16, 1.0)
    assert st == -1 and b"aux" in ops.lib.mdt_last_error_string() and str(N - 16).encode() in ops.lib.mdt_last_error_string()
    st = ops.lib.mdt_lora_up_act(ops.stream(), es, 0, R, 16, N, t.data_ptr(), 16, w.data_ptr(), N, y.data_ptr(), N, y.data_ptr(), N,
                                 aux.data_ptr(), N - 16, 1.0, 0.0, 0)
    assert st == -1 and b"u " in ops.lib.mdt_last_error_string() + b" "
    # a base that is off its boundary: bf16 one element (2 bytes) off 16, fp32 viewed from a byte buffer 2 bytes off 4
    raw = torch.zeros((R * N + 8) * y.element_size(), dtype=torch.uint8, device=DEV)
    off = raw[2:2 + R * N * y.element_size()]
    if dtype == torch.bfloat16:
        mis = off.view(torch.bfloat16).view(R, N)
        refused(lambda: ops.lora_up_add_drop(t, w, mis, drop_p=0.1), "Y", "16-byte")
        refused(lambda: ops.lora_up_add_mul(t, w, y, mis), "aux", "16-byte")
        refused(lambda: ops.lora_up_act(t, w, y, "gelu", out=mis), "h", "16-byte")
        refused(lambda: ops.lora_up_act(t, w, y, "gelu", out=y, u=mis), "u", "16-byte")
        refused(lambda: ops.lora_up_act(t, w, mis, "gelu", out=y), "pre", "16-byte")
    else:
        st = ops.lib.mdt_lora_up_add_drop(ops.stream(), 0, R, 16, N, t.data_ptr(), 16, w.data_ptr(), N, off.data_ptr(), N, 1.0, 0.1, 3)
        assert st == -1 and b"4-byte" in ops.lib.mdt_last_error_string()
    torch.cuda.synchronize()
    assert torch.equal(y, keep) and ops.L.last_route() == route      # nothing was launched
