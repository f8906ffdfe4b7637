"""The three low-rank adapter kernels (mdt_lora_down, mdt_lora_up_add, mdt_lora_wgrad) against tests/lora_reference.py: every
element within its bound, in bf16 (MFMA kernels) and fp32 (the parity loops), on a sparse cross of
R in {1, 15, 16, 17, 255, SLAB - 1, SLAB, SLAB + 1, 2 SLAB + 3}, D in {80, 128, 768, 1024}, n in {8, 16, 24, 48, 192};
operands and results that are column slices (row stride 3 D, at each c_j = j D) of a guarded [R, 3 D] buffer whose other bytes
keep their bits; T, dW and the workspace between canaries; the weight gradient exact on integer operands, bit-identical when
repeated, accumulating into a non-zero dW and free of float atomics; refusals with status and message before any launch."""
import pytest
import torch

import tests.lora_reference as LR

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from multimodaldiscussiontransformer_amd import ops as _ops
    return _ops


S_ = 1024           # asserted equal to ops.LORA_WGRAD_SLAB below: parametrisation happens before the library is loaded
# (R, D, n, j): j = which third of the [R, 3 D] buffer the wide operand is
CASES = [(1, 80, 8, 0), (15, 128, 16, 1), (16, 768, 24, 2), (17, 1024, 48, 0), (255, 80, 192, 1), (17, 768, 192, 2),
         (S_ - 1, 128, 8, 2), (S_, 768, 16, 0), (S_ + 1, 1024, 24, 1), (2 * S_ + 3, 768, 48, 2), (2 * S_ + 3, 128, 192, 0),
         (2 * S_ + 3, 1024, 16, 1)]
DTYPES = [torch.bfloat16, torch.float32]


def test_slab_constant(ops):
    assert ops.LORA_WGRAD_SLAB == S_


class Wide:
    """A [pre + R + post, 3 D] buffer of data; ``view`` is rows pre .. pre + R, columns j D .. (j + 1) D (row stride 3 D).
    others_untouched(): every element outside the view has the bits it was created with."""

    def __init__(self, R, D, j, dtype, seed, integer=None, pre=2, post=3):
        shape = (pre + R + post, 3 * D)
        self.buf = (LR.gen_int(shape, seed, integer, dtype, DEV) if integer else LR.gen(shape, seed, 1.0, dtype, DEV))
        self.itype = torch.int16 if dtype == torch.bfloat16 else torch.int32
        self.before = self.buf.clone()
        self.rows, self.cols = slice(pre, pre + R), slice(j * D, (j + 1) * D)
        self.view = self.buf[self.rows, self.cols]

    def others_untouched(self):
        same = self.buf.view(self.itype) == self.before.view(self.itype)
        same[self.rows, self.cols] = True
        return bool(same.all())


def _within(out, ref, dtype, what):
    v, d = ref
    LR.assert_within(out, v, LR.bound(v, d, dtype), what=what, dtype=dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("R,D,n,j", CASES)
def test_down(ops, R, D, n, j, dtype):
    x = Wide(R, D, j, dtype, 1)
    w = LR.gen((n, D), 2, 0.25, dtype, DEV)
    t = LR.Guarded(R, n, dtype, DEV, ld=n + 8)
    ops.lora_down(x.view, w, out=t.view, alpha=0.75)
    route = ops.L.last_route()
    assert route == ("lora_down" if dtype == torch.bfloat16 else "lora_down_f32")
    _within(t.view, LR.down(x.view, w, 0.75), dtype, f"down R={R} D={D} n={n}")
    assert t.untouched() and x.others_untouched() and torch.equal(x.buf, x.before)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("R,D,n,j", CASES)
def test_up_add(ops, R, D, n, j, dtype):
    y = Wide(R, D, j, dtype, 3)
    t = LR.gen((R, n), 4, 1.0, dtype, DEV)
    w = LR.gen((n, D), 5, 0.25, dtype, DEV)
    ref = LR.up_add(t, w, y.view.clone(), 1.5)
    ops.lora_up_add(t, w, y.view, alpha=1.5)
    assert ops.L.last_route() == ("lora_up" if dtype == torch.bfloat16 else "lora_up_f32")
    _within(y.view, ref, dtype, f"up_add R={R} D={D} n={n}")
    assert y.others_untouched()                 # the thirds of Y that were not addressed, and the rows around it, keep their bits


def _guarded_ws(nbytes):
    buf = torch.full((nbytes + 128,), 0xA5, dtype=torch.uint8, device=DEV)
    return buf, buf[64:64 + nbytes]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("R,D,n,j", CASES)
def test_wgrad_exact_ordered_guarded(ops, R, D, n, j, dtype):
    x = Wide(R, D, j, dtype, 6, integer=4)
    t = LR.gen_int((R, n), 7, 2, dtype, DEV)
    dw0 = LR.gen_int((n, D), 8, 50, torch.float32, DEV)
    v, d = LR.wgrad(t, x.view, dw0, 2.0, S_)
    assert float(d.max()) == 0.0                 # integer operands: the reference is exact, a missing step cannot hide
    need = ops.lib.mdt_lora_wgrad_workspace_bytes(R, n, D)
    assert need == ((R + S_ - 1) // S_) * n * D * 4
    before = ops.float_atomic_launches()
    outs = []
    for _ in range(2):
        dw = LR.Guarded(n, D, torch.float32, DEV, ld=D + 4, init=dw0)
        wsbuf, ws = _guarded_ws(need)
        ops.lora_wgrad(t, x.view, dw.view, alpha=2.0, ws=ws)
        assert ops.L.last_route() == ("lora_wgrad" if dtype == torch.bfloat16 else "lora_wgrad_f32")
        assert dw.untouched()
        assert bool((wsbuf[:64] == 0xA5).all()) and bool((wsbuf[64 + need:] == 0xA5).all())
        outs.append(dw.view.clone())
    assert ops.float_atomic_launches() == before
    assert torch.equal(outs[0].double(), v), f"wgrad R={R} D={D} n={n}: {int((outs[0].double() != v).sum())} elements differ"
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    assert x.others_untouched() and torch.equal(x.buf, x.before)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("R,D,n,j", [(255, 80, 192, 1), (S_ + 1, 1024, 24, 1), (2 * S_ + 3, 768, 48, 2)])
def test_wgrad_random_operands(ops, R, D, n, j, dtype):
    x = Wide(R, D, j, dtype, 9)
    t = LR.gen((R, n), 10, 1.0, dtype, DEV)
    dw0 = LR.gen((n, D), 11, 3.0, torch.float32, DEV)
    dw = dw0.clone()
    ops.lora_wgrad(t, x.view, dw, alpha=0.75)
    _within(dw, LR.wgrad(t, x.view, dw0, 0.75, S_), torch.float32, f"wgrad R={R} D={D} n={n}")
    again = dw0.clone()
    ops.lora_wgrad(t, x.view, again, alpha=0.75)
    assert torch.equal(dw.view(torch.int32), again.view(torch.int32))


def test_zero_rows_is_a_noop(ops):
    for dtype in DTYPES:
        w = LR.gen((8, 16), 1, 1.0, dtype, DEV)
        x = torch.empty(0, 16, dtype=dtype, device=DEV)
        t = torch.empty(0, 8, dtype=dtype, device=DEV)
        dw = torch.ones(8, 16, device=DEV)
        ops.lora_down(x, w, out=t)
        ops.lora_up_add(t, w, x)
        ops.lora_wgrad(t, x, dw)
        assert bool((dw == 1).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_refusals(ops, dtype):
    from multimodaldiscussiontransformer_amd._lib import MdtError
    R, D = 32, 64
    x = LR.gen((R, D), 1, 1.0, dtype, DEV)
    y = x.clone()
    dw = torch.zeros(16, D, device=DEV)
    ops.lora_down(x, LR.gen((8, D), 2, 1.0, dtype, DEV))
    route = ops.L.last_route()

    def refused(fn, *words):
        with pytest.raises(MdtError) as e:
            fn()
        assert e.value.status == -1
        for w in words:
            assert w in str(e.value), str(e.value)

    for n in (4, 12, 200):                       # not a multiple of 8, or outside 8 ... 192
        w = LR.gen((n, D), 2, 1.0, dtype, DEV)
        t = LR.gen((R, n), 3, 1.0, dtype, DEV)
        refused(lambda: ops.lora_down(x, w), f"n={n}")
        refused(lambda: ops.lora_up_add(t, w, y), f"n={n}")
        refused(lambda: ops.lora_wgrad(t, x, torch.zeros(n, D, device=DEV)), f"n={n}")
    refused(lambda: ops.lora_down(x[:, :40].contiguous(), LR.gen((8, 40), 2, 1.0, dtype, DEV)), "K=40")
    # a base that is off its boundary: bf16 one element (2 bytes) off 16, fp32 viewed from a byte buffer 2 bytes off 4
    w = LR.gen((16, D), 2, 1.0, dtype, DEV)
    t = LR.gen((R, 16), 3, 1.0, dtype, DEV)
    raw = torch.zeros((R * D + 8) * x.element_size(), dtype=torch.uint8, device=DEV)
    off = raw[2:2 + R * D * x.element_size()]
    if dtype == torch.bfloat16:
        mis = off.view(torch.bfloat16).view(R, D)
        refused(lambda: ops.lora_down(mis, w), "X", "16-byte")
        refused(lambda: ops.lora_up_add(t, w, mis), "Y", "16-byte")
        refused(lambda: ops.lora_wgrad(t, mis, dw), "X", "16-byte")
    else:
        # torch refuses a misaligned fp32 view, so the pointer goes to the library directly
        st = ops.lib.mdt_lora_down(ops.stream(), 0, R, 16, D, off.data_ptr(), D, w.data_ptr(), D, t.data_ptr(), 16, 1.0)
        assert st == -1 and b"4-byte" in ops.lib.mdt_last_error_string()
    # a workspace one slice short
    R2 = S_ + 1
    t2 = LR.gen((R2, 16), 3, 1.0, dtype, DEV)
    x2 = LR.gen((R2, D), 1, 1.0, dtype, DEV)
    need = ops.lib.mdt_lora_wgrad_workspace_bytes(R2, 16, D)
    short = torch.empty(need - 16 * D * 4, dtype=torch.uint8, device=DEV)
    refused(lambda: ops.lora_wgrad(t2, x2, dw, ws=short), "workspace", str(need))
    torch.cuda.synchronize()
    assert bool((dw == 0).all()) and torch.equal(y, x) and ops.L.last_route() == route      # nothing was launched
