"""Adapter-input dropout inside the adapter kernels (mdt_lora_down_drop, mdt_lora_wgrad_drop, mdt_lora_up_add_mul_drop) against
tests/lora_dropout_reference.py, in bf16 (MFMA kernels) and fp32 (parity loops), p in {0.1, 0.5}, on the first ten cases of
tests/test_lora_kernels_gpu.py — the K tail (80), half-filled n tiles (8, 24), row tails, one, one + 1 and two + 3 slabs — with
the wide operand a column slice of a guarded [R, 3 D] buffer, so that its row stride differs from its width.

Random operands: every element within bound(v, δ), the bound not vacuous.  Two mutants of the reference — no mask at all, and
counters strided by the row stride 3 D instead of the width — must leave that bound on at least half of the elements, so a kernel
that ignores the mask or counts with ld cannot pass.  Integer operands with p = 0.5 and a power-of-two alpha: exact equality,
the weight gradient bit-identical when repeated and free of float atomics.  The kernels' mask is ops.dropout_mask(R W, p, seed);
drop_p = 0 is the plain entry point bit for bit; NaN and Inf at dropped positions of X leave T and dW finite; write sets (guards,
the untouched thirds, workspace guard bytes), routes, refusals before any launch, the R = 0 no-op."""
import pytest
import torch

import tests.gemm_reference as GR
import tests.lora_dropout_reference as LDR
import tests.lora_reference as LR
from tests.test_lora_dense_kernels_gpu import CASES as DENSE_CASES
from tests.test_lora_dense_kernels_gpu import Wide as Wide2
from tests.test_lora_dense_kernels_gpu import _scale
from tests.test_lora_kernels_gpu import CASES as ALL_CASES
from tests.test_lora_kernels_gpu import S_, Wide, _guarded_ws

pytestmark = pytest.mark.gpu

DEV = "cuda"
CASES = ALL_CASES[:10]
DTYPES = [torch.bfloat16, torch.float32]
IDS = ["bf16", "fp32"]
SEED = 0x10A0D0905EED


@pytest.fixture(scope="module")
def ops():
    from multimodaldiscussiontransformer_amd import ops as _ops
    return _ops


def _bits(x):
    return x.contiguous().view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32)


def _route(ops, name, dtype):
    assert ops.L.last_route() == (name if dtype == torch.bfloat16 else name + "_f32")


def _check(out, ref, mutants, dtype, what):
    """out within the masked reference's bound; every mutant outside it on at least half of the elements"""
    v, d = ref
    bnd = LR.bound(v, d, dtype)
    LR.assert_within(out.cpu(), v, bnd, what=what, dtype=dtype)
    for name, (mv, _) in mutants.items():
        frac = float(((mv - v).abs() > bnd).double().mean())
        assert frac >= 0.5, f"{what}: the mutant '{name}' differs on {frac:.2f} of the elements only: the bound cannot tell it apart"


def _mask_is_dropout_mask(ops, R, W, p, seed):
    keep = ops.dropout_mask(R * W, p, seed).reshape(R, W).cpu() != 0
    assert torch.equal(keep, GR.drop_scale(R, W, p, seed) != 0), "the CPU port of the mask is not ops.dropout_mask"
    assert 0 < int(keep.sum()) < R * W


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("R,D,n,j", CASES)
def test_down_drop(ops, R, D, n, j, p, dtype):
    seed = SEED + R
    x = Wide(R, D, j, dtype, 1)
    w = LR.gen((n, D), 2, 0.25, dtype, DEV)
    t = LR.Guarded(R, n, dtype, DEV, ld=n + 8)
    ops.lora_down_drop(x.view, w, out=t.view, alpha=0.75, drop_p=p, drop_seed=seed)
    _route(ops, "lora_down_drop", dtype)
    _mask_is_dropout_mask(ops, R, D, p, seed)
    xc, wc = x.view.cpu(), w.cpu()
    mutants = {"no mask": LDR.down_drop(xc, wc, 0.75, p, seed, apply_mask=False)}
    if R > 1:
        mutants["counters strided by ld"] = LDR.down_drop(xc, wc, 0.75, p, seed, counter_ld=3 * D)
    _check(t.view, LDR.down_drop(xc, wc, 0.75, p, seed), mutants, dtype, f"down_drop R={R} D={D} n={n} p={p}")
    assert t.untouched() and x.others_untouched() and torch.equal(x.buf, x.before)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("R,D,n,j", CASES)
def test_wgrad_drop(ops, R, D, n, j, p, dtype):
    seed = SEED + 7 * R
    x = Wide(R, D, j, dtype, 9)
    t = LR.gen((R, n), 10, 1.0, dtype, DEV)
    dw0 = LR.gen((n, D), 11, 3.0, torch.float32, DEV)
    dw = LR.Guarded(n, D, torch.float32, DEV, ld=D + 4, init=dw0)
    need = ops.lib.mdt_lora_wgrad_workspace_bytes(R, n, D)
    wsbuf, ws = _guarded_ws(need)
    before = ops.float_atomic_launches()
    ops.lora_wgrad_drop(t, x.view, dw.view, alpha=0.75, drop_p=p, drop_seed=seed, ws=ws)
    _route(ops, "lora_wgrad_drop", dtype)
    assert ops.float_atomic_launches() == before
    tc, xc, d0 = t.cpu(), x.view.cpu(), dw0.cpu()
    # the old dW is common to the reference and its mutants: they are told apart on the product alone
    ref = LDR.wgrad_drop(tc, xc, d0, 0.75, p, seed, S_)
    # an element of dW sums R rows: with R = 1 a mutant differs only where that one row's mask does (a fraction p), so the mutants
    # are asked for where more than half of the sums hold a term whose mask differs — every case but R = 1
    mutants = {}
    if R >= 15:
        mutants = {"no mask": LDR.wgrad_drop(tc, xc, d0, 0.75, p, seed, S_, apply_mask=False),
                   "counters strided by ld": LDR.wgrad_drop(tc, xc, d0, 0.75, p, seed, S_, counter_ld=3 * D)}
    _check(dw.view, ref, mutants, torch.float32, f"wgrad_drop R={R} D={D} n={n} p={p}")
    assert dw.untouched() and x.others_untouched() and torch.equal(x.buf, x.before)
    assert bool((wsbuf[:64] == 0xA5).all()) and bool((wsbuf[64 + need:] == 0xA5).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("R,D,n,j", CASES)
def test_integer_operands_are_exact(ops, R, D, n, j, dtype):
    seed, p = SEED + 3 * R, 0.5
    x = Wide(R, D, j, dtype, 6, integer=4)
    w = LR.gen_int((n, D), 5, 2, dtype, DEV)
    v, d = LDR.down_drop(x.view.cpu(), w.cpu(), 2.0, p, seed)
    assert float(d.max()) == 0.0
    tt = LR.Guarded(R, n, dtype, DEV, ld=n + 8)
    ops.lora_down_drop(x.view, w, out=tt.view, alpha=2.0, drop_p=p, drop_seed=seed)
    v = LR.stored(v, dtype)                      # the fp32 value is exact; T holds its one rounding to the stored type
    assert torch.equal(tt.view.cpu().double(), v), f"down_drop R={R} D={D} n={n}: {int((tt.view.cpu().double() != v).sum())} elements differ"
    assert float((v - LR.stored(LDR.down_drop(x.view.cpu(), w.cpu(), 2.0, p, seed, apply_mask=False)[0], dtype)).abs().max()) > 0
    assert tt.untouched()
    # the weight gradient: exact, repeatable bit for bit, no float atomics
    t = LR.gen_int((R, n), 7, 2, dtype, DEV)
    dw0 = LR.gen_int((n, D), 8, 50, torch.float32, DEV)
    v, d = LDR.wgrad_drop(t.cpu(), x.view.cpu(), dw0.cpu(), 2.0, p, seed, S_)
    assert float(d.max()) == 0.0
    need = ops.lib.mdt_lora_wgrad_workspace_bytes(R, n, D)
    before = ops.float_atomic_launches()
    outs = []
    for _ in range(2):
        dw = LR.Guarded(n, D, torch.float32, DEV, ld=D + 4, init=dw0)
        wsbuf, ws = _guarded_ws(need)
        ops.lora_wgrad_drop(t, x.view, dw.view, alpha=2.0, drop_p=p, drop_seed=seed, ws=ws)
        assert dw.untouched() and bool((wsbuf[:64] == 0xA5).all()) and bool((wsbuf[64 + need:] == 0xA5).all())
        outs.append(dw.view.clone())
    assert ops.float_atomic_launches() == before
    assert torch.equal(outs[0].cpu().double(), v), f"wgrad_drop R={R} D={D} n={n}: {int((outs[0].cpu().double() != v).sum())} elements differ"
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    assert x.others_untouched() and torch.equal(x.buf, x.before)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("R,D,n,j", CASES)
def test_p0_is_the_plain_entry_point(ops, R, D, n, j, dtype):
    x = Wide(R, D, j, dtype, 1)
    w = LR.gen((n, D), 2, 0.25, dtype, DEV)
    assert torch.equal(_bits(ops.lora_down_drop(x.view, w, alpha=0.75, drop_p=0.0, drop_seed=SEED)), _bits(ops.lora_down(x.view, w, alpha=0.75)))
    t = LR.gen((R, n), 10, 1.0, dtype, DEV)
    dw0 = LR.gen((n, D), 11, 3.0, torch.float32, DEV)
    a, b = dw0.clone(), dw0.clone()
    ops.lora_wgrad_drop(t, x.view, a, alpha=0.75, drop_p=0.0, drop_seed=SEED)
    ops.lora_wgrad(t, x.view, b, alpha=0.75)
    assert torch.equal(_bits(a), _bits(b))
    y = Wide(R, D, j, dtype, 3)
    aux = LR.gen((R, D), 4, 1.0, dtype, DEV)
    wu = LR.gen((n, D), 5, 0.25, dtype, DEV)
    plain = y.view.clone()
    ops.lora_up_add_mul(t, wu, plain, aux, alpha=0.75)
    ops.lora_up_add_mul_drop(t, wu, y.view, aux, alpha=0.75, drop_p=0.0, drop_seed=SEED)
    assert torch.equal(_bits(y.view), _bits(plain)) and y.others_untouched()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_non_finite_values_at_dropped_positions_go_no_further(ops, dtype):
    R, D, n, p, seed = 17, 128, 16, 0.5, SEED + 5
    x = Wide(R, D, 1, dtype, 1)
    dropped = torch.nonzero(GR.drop_scale(R, D, p, seed) == 0)
    (r0, c0), (r1, c1) = [int(i) for i in dropped[0]], [int(i) for i in dropped[len(dropped) // 2]]
    x.view[r0, c0] = float("nan")
    x.view[r1, c1] = float("inf")
    w = LR.gen((n, D), 2, 0.25, dtype, DEV)
    t = ops.lora_down_drop(x.view, w, drop_p=p, drop_seed=seed)
    assert bool(torch.isfinite(t).all())
    assert not bool(torch.isfinite(ops.lora_down(x.view, w)).all())          # the plain form does see them
    dw = torch.zeros(n, D, device=DEV)
    ops.lora_wgrad_drop(LR.gen((R, n), 3, 1.0, dtype, DEV), x.view, dw, drop_p=p, drop_seed=seed)
    assert bool(torch.isfinite(dw).all())
    v, d = LDR.down_drop(x.view.cpu(), w.cpu(), 1.0, p, seed)
    LR.assert_within(t.cpu(), v, LR.bound(v, d, dtype), what="down_drop with NaN / Inf under the mask", dtype=dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("R,N,n,j", DENSE_CASES)
def test_up_add_mul_drop(ops, R, N, n, j, p, dtype):
    seed = SEED + 11 * R
    y = Wide2(R, N, j, dtype, 6)
    aux = Wide2(R, N, 1 - j, dtype, 7)
    t = Wide2(R, n, 0, dtype, 8)
    w = LR.gen((n, N), 9, 0.25, dtype, DEV)
    sc = _scale(ops, R, N, p, seed)
    ref = LDR.up_add_mul_drop(t.view.cpu(), w.cpu(), y.old.cpu(), aux.view.cpu(), 0.75, sc)
    before = ops.float_atomic_launches()
    ops.lora_up_add_mul_drop(t.view, w, y.view, aux.view, alpha=0.75, drop_p=p, drop_seed=seed)
    _route(ops, "lora_up_mul_drop", dtype)
    assert ops.float_atomic_launches() == before
    v, d = ref
    LR.assert_within(y.view.cpu(), v, LR.bound(v, d, dtype), what=f"up_add_mul_drop R={R} N={N} n={n} p={p}", dtype=dtype)
    dropped = (sc == 0).to(DEV)
    assert 0 < int(dropped.sum()) < R * N or R * N < 200
    assert torch.equal(_bits(y.view)[dropped], _bits(y.old)[dropped])            # a dropped element keeps its bits
    assert y.others_untouched() and aux.unchanged() and t.unchanged()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_up_add_mul_drop_exact(ops, dtype):
    R, N, n, p, seed = 257, 128, 24, 0.5, SEED + 13
    t, w = LR.gen_int((R, n), 1, 2, dtype, DEV), LR.gen_int((n, N), 2, 2, dtype, DEV)
    y, aux = LR.gen_int((R, N), 3, 8, dtype, DEV), LR.gen_int((R, N), 4, 2, dtype, DEV)
    v, d = LDR.up_add_mul_drop(t.cpu(), w.cpu(), y.cpu(), aux.cpu(), 2.0, _scale(ops, R, N, p, seed))
    assert float(d.max()) == 0.0
    ops.lora_up_add_mul_drop(t, w, y, aux, alpha=2.0, drop_p=p, drop_seed=seed)
    assert torch.equal(y.cpu().double(), LR.stored(v, dtype))


def test_zero_rows_is_a_noop(ops):
    for dtype in DTYPES:
        w = LR.gen((8, 16), 1, 1.0, dtype, DEV)
        x = torch.empty(0, 16, dtype=dtype, device=DEV)
        t = torch.empty(0, 8, dtype=dtype, device=DEV)
        dw = torch.ones(8, 16, device=DEV)
        ops.lora_down_drop(x, w, out=t, drop_p=0.5, drop_seed=1)
        ops.lora_up_add_mul_drop(t, w, x, x, drop_p=0.5, drop_seed=1)
        ops.lora_wgrad_drop(t, x, dw, drop_p=0.5, drop_seed=1)
        assert bool((dw == 1).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_refusals(ops, dtype):
    from multimodaldiscussiontransformer_amd._lib import MdtError
    R, D, n = 32, 64, 16
    x = LR.gen((R, D), 1, 1.0, dtype, DEV)
    w = LR.gen((n, D), 2, 1.0, dtype, DEV)
    t = LR.gen((R, n), 3, 1.0, dtype, DEV)
    y, aux = x.clone(), x.clone()
    dw = torch.zeros(n, D, device=DEV)
    t_out = torch.zeros(R, n, dtype=dtype, device=DEV)
    ops.lora_down(x, w)
    route = ops.L.last_route()

    def refused(fn, *words):
        with pytest.raises(MdtError) as e:
            fn()
        assert e.value.status == -1
        for wd in words:
            assert wd in str(e.value), str(e.value)

    for p in (1.0, -0.1, 1.5, float("nan")):
        refused(lambda: ops.lora_down_drop(x, w, out=t_out, drop_p=p), "mdt_lora_down_drop", "drop_p")
        refused(lambda: ops.lora_wgrad_drop(t, x, dw, drop_p=p), "mdt_lora_wgrad_drop", "drop_p")
        refused(lambda: ops.lora_up_add_mul_drop(t, w, y, aux, drop_p=p), "mdt_lora_up_add_mul_drop", "drop_p")
    # what lora_check refuses for the plain forms
    refused(lambda: ops.lora_down_drop(x, LR.gen((12, D), 2, 1.0, dtype, DEV), drop_p=0.1), "n=12")
    refused(lambda: ops.lora_down_drop(x[:, :40].contiguous(), LR.gen((8, 40), 2, 1.0, dtype, DEV), drop_p=0.1), "K=40")
    # a site of 2^33 counters: 2^23 rows of 1024 — refused from the numbers alone, nothing is read
    big_r, big_w = 1 << 23, 1024
    code = 0 if dtype == torch.float32 else 1          # MDT_F32 / MDT_BF16
    st = ops.lib.mdt_lora_down_drop(ops.stream(), code, big_r, n, big_w, x.data_ptr(), big_w, w.data_ptr(), big_w, t_out.data_ptr(), n, 1.0, 0.1, 1)
    assert st == -1 and b"2^33" in ops.lib.mdt_last_error_string()
    st = ops.lib.mdt_lora_wgrad_drop(ops.stream(), code, big_r, n, big_w, t.data_ptr(), n, x.data_ptr(), big_w, dw.data_ptr(), big_w, 1.0, 0.1, 1,
                                     dw.data_ptr(), 0)
    assert st == -1 and b"2^33" in ops.lib.mdt_last_error_string()
    st = ops.lib.mdt_lora_up_add_mul_drop(ops.stream(), code, big_r, n, big_w, t.data_ptr(), n, w.data_ptr(), big_w, y.data_ptr(), big_w,
                                          aux.data_ptr(), big_w, 1.0, 0.1, 1)
    assert st == -1 and b"2^33" in ops.lib.mdt_last_error_string()
    # a workspace one slice short
    R2 = S_ + 1
    t2 = LR.gen((R2, n), 3, 1.0, dtype, DEV)
    x2 = LR.gen((R2, D), 1, 1.0, dtype, DEV)
    need = ops.lib.mdt_lora_wgrad_workspace_bytes(R2, n, D)
    short = torch.empty(need - n * D * 4, dtype=torch.uint8, device=DEV)
    refused(lambda: ops.lora_wgrad_drop(t2, x2, dw, drop_p=0.1, ws=short), "mdt_lora_wgrad_drop", "workspace", str(need))
    torch.cuda.synchronize()
    assert bool((dw == 0).all()) and bool((t_out == 0).all()) and torch.equal(y, x) and ops.L.last_route() == route      # nothing was launched
