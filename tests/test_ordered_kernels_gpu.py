"""The ordered (deterministic-mode) entry points of include/mdt_hip.h, each alone, on the device.

Where the header defines the bits of a result — the slice reducer, the column sums, the segment sum, the bias histogram —
the check is ``torch.equal`` against the CPU emulators of tests/test_ordered_reference_cpu.py (whose self-tests show that
they tell summation orders apart).  Where a GEMM's MFMA order or the LayerNorm row arithmetic is inside there are two
gates: integer-valued operands, where every fp32 operation is exact and the result is determined (equality), and random
operands against the per-element fp64 bounds of tests/gemm_reference.py / layernorm_reference.py / rowops_reference.py.
Every case is also launched 10 times into poisoned outputs and compared bit for bit with the first launch."""
import pytest
import torch

import tests.gemm_reference as R
import tests.layernorm_reference as LR
import tests.rowops_reference as RR
import tests.test_ordered_reference_cpu as EMU
from multimodaldiscussiontransformer_amd import _lib as L

pytestmark = pytest.mark.gpu

f32, bf16 = torch.float32, torch.bfloat16
DEV = "cuda"
F24 = 2.0 ** 24
REPS = 10


@pytest.fixture(scope="module")
def ops():
    from multimodaldiscussiontransformer_amd import ops as o
    assert torch.cuda.is_available(), "GPU tests need a device"
    return o


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == f32 else torch.int16)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def repeatable(run, what):
    """``run()`` → dict of output tensors, computed from scratch into fresh poisoned buffers: REPS launches, the same bits."""
    first = {k: v.clone() for k, v in run().items()}
    for i in range(1, REPS):
        for k, v in run().items():
            assert same_bits(v, first[k]), f"{what}: {k} of launch {i} differs from launch 0"
    return first


def order_sensitive(shape, seed, big_every=7):
    """fp32 values whose sum depends on the order: ones and small fractions with a +-2^24 here and there."""
    v = R.gen(shape, seed, 4.0, f32, DEV)
    g = torch.Generator(device=DEV).manual_seed(seed + 1)
    m = torch.randint(0, big_every, shape, generator=g, device=DEV)
    v = torch.where(m == 0, torch.full_like(v, F24), v)
    return torch.where(m == 1, torch.full_like(v, -F24), v)


# ------------------------------------------------------------------------------------------------ sum_slices
@pytest.mark.parametrize("accumulate", [False, True], ids=["store", "accumulate"])
@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (129, 257)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("slices", [1, 2, 7, 28])
def test_sum_slices_bits(ops, slices, shape, accumulate):
    rows, cols = shape
    buf = torch.full((slices, rows + 2, cols + 3), float("nan"), dtype=f32, device=DEV)       # padded slice and row strides
    ws = buf[:, :rows, :cols]
    ws.copy_(order_sensitive((slices, rows, cols), 10 * slices + rows))
    c0 = order_sensitive((rows, cols), 77, big_every=5)

    def run():
        out = R.Guarded(rows, cols, f32, DEV, ld=cols + 5, init=c0 if accumulate else None)
        ops.sum_slices(ws, out.view, accumulate=accumulate)
        assert out.untouched(), "sum_slices wrote outside its [rows, cols] view"
        return {"out": out.view}

    got = repeatable(run, "sum_slices")["out"]
    want = EMU.emu_sum_slices(ws.cpu(), c0.cpu() if accumulate else None)
    assert torch.equal(got.cpu(), want)


# ------------------------------------------------------------------------------------------------ ordered split-K GEMM
def _wgrad_case(ops, M, N, K, split, dtype, integer, seed=0):
    """dW[M, N] += dY^T X over K rows: both operands k-major, as engine.wgrad calls it."""
    if integer:
        a, b = R.int_operands(M, N, K, True, True, seed, dtype=dtype, device=DEV)
        c0 = R.gen_int((M, N), 300 + seed, 50, f32, DEV)
    else:
        a = R.gen((K, M), 100 + seed, dtype=dtype, device=DEV)
        b = R.gen((K, N), 200 + seed, scale=R.b_scale(K), dtype=dtype, device=DEV)
        c0 = R.gen((M, N), 300 + seed, dtype=f32, device=DEV)
    route = {}

    def run():
        C = R.Guarded(M, N, f32, DEV, ld=N + 4, init=c0)
        ops.gemm_splitk_ordered(a, b, C.view, trans_a=True, trans_b=True, split_k=split)
        route["r"] = L.last_route()
        assert C.untouched(), "ordered GEMM wrote outside its [M, N] view"
        return {"out": C.view}

    got = repeatable(run, f"ordered gemm {M}x{N}x{K} split {split}")["out"]
    ref = R.reference(a, b, trans_a=True, trans_b=True, epilogue=R.EPI_ATOMIC, c_old=c0, split_k=split)
    return got, ref, route["r"]


@pytest.mark.parametrize("dtype", [bf16, f32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("split", [1, 2, 5])
def test_gemm_splitk_ordered_ragged_last_slab(ops, split, dtype):
    M, N, K = 192, 136, 300
    got, ref, _ = _wgrad_case(ops, M, N, K, split, dtype, integer=True)
    # integers with sum |a| |b| + |c| far below 2^24: every partial sum, in any order and any slab split, is exact
    assert torch.equal(got.double(), ref["out"][0]), "integer-valued operands: every bit of dW is determined"
    got, ref, _ = _wgrad_case(ops, M, N, K, split, dtype, integer=False, seed=3)
    R.check({"out": got}, ref, {"out": f32}, what=f"ordered gemm split {split}")


def test_gemm_splitk_ordered_reaches_the_4wave_kernel(ops):
    M, N, K, split = 256, 256, 1000, 3
    got, ref, route = _wgrad_case(ops, M, N, K, split, bf16, integer=True)
    assert route == "w4s", f"dW[256, 256] over 1000 rows, split 3, ran {route}"
    assert torch.equal(got.double(), ref["out"][0])
    got, ref, route = _wgrad_case(ops, M, N, K, split, bf16, integer=False, seed=5)
    assert route == "w4s"
    R.check({"out": got}, ref, {"out": f32}, what="ordered gemm w4s")


def test_gemm_splitk_ordered_refuses_a_short_workspace(ops):
    M, N, K, split = 192, 136, 300, 2
    a, b = R.int_operands(M, N, K, True, True, 0, dtype=bf16, device=DEV)
    C = torch.zeros(M, N, dtype=f32, device=DEV)
    need = int(L.lib.mdt_gemm_splitk_ordered_workspace_bytes(M, N, split))
    assert need == split * M * N * 4
    short = torch.empty(need - 1, dtype=torch.uint8, device=DEV)
    with pytest.raises(L.MdtError, match="workspace") as e:
        ops.gemm_splitk_ordered(a, b, C, trans_a=True, trans_b=True, split_k=split, ws=short)
    assert e.value.status == -1
    torch.cuda.synchronize()
    assert not bool(C.any()), "a refused call launched something"
    ops.gemm_splitk_ordered(a, b, C, trans_a=True, trans_b=True, split_k=split, ws=torch.empty(need, dtype=torch.uint8, device=DEV))
    assert torch.equal(C.double(), a.double().t() @ b.double())


# ------------------------------------------------------------------------------------------------ column sums
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "row_weight"])
@pytest.mark.parametrize("cols", [8, 768, 1000])
@pytest.mark.parametrize("rows", [1, 255, 256, 257, 4099])
def test_colsum_ordered_bits(ops, rows, cols, weighted):
    dtype = bf16 if (rows + cols) % 2 else f32
    x = R.Guarded(rows, cols, dtype, DEV, ld=cols + 8, init=R.gen((rows, cols), rows + cols, 3.0, dtype, DEV))
    w = None
    if weighted:
        g = torch.Generator(device=DEV).manual_seed(rows)
        w = torch.randint(0, 2, (rows,), generator=g, device=DEV, dtype=torch.int32)
    c0 = R.gen((cols,), 5, 3.0, f32, DEV)

    def run():
        out = R.Guarded(1, cols, f32, DEV, ld=cols + 3, pre=1, post=1, init=c0[None, :])
        ops.colsum_ordered(x.view, out=out.view[0], row_weight=w)
        assert out.untouched()
        return {"out": out.view[0]}

    got = repeatable(run, "colsum_ordered")["out"]
    want = EMU.emu_colsum(x.view.cpu(), c0.cpu(), None if w is None else w.cpu())
    assert torch.equal(got.cpu(), want), "colsum_ordered: not the documented order"
    # ... and, independently of the emulator, inside the fp64 bound of a sum in any order
    t = x.view.double() * (1.0 if w is None else w.double()[:, None])
    LR.assert_within(got, c0.double() + t.sum(0), LR.bound(c0.double() + t.sum(0), LR._sum_err(t, torch.zeros_like(t), 0, c0.double()), f32),
                     what="colsum_ordered")
    # integer terms: exact in any order
    xi = R.gen_int((rows, cols), 9, 4, dtype, DEV)
    exact = ops.colsum_ordered(xi, row_weight=w)
    assert torch.equal(exact.double(), (xi.double() * (1.0 if w is None else w.double()[:, None])).sum(0))


def test_colsum_ordered_refuses_a_short_workspace(ops):
    x = torch.ones(300, 16, dtype=f32, device=DEV)
    need = int(L.lib.mdt_colsum_ordered_workspace_bytes(300, 16))
    assert need == 2 * 16 * 4
    with pytest.raises(L.MdtError, match="workspace"):
        ops.colsum_ordered(x, ws=torch.empty(need - 1, dtype=torch.uint8, device=DEV))


# ------------------------------------------------------------------------------------------------ LayerNorm backward
@pytest.mark.parametrize("dropped", [False, True], ids=["plain", "dropped"])
@pytest.mark.parametrize("D", [128, 768])
@pytest.mark.parametrize("rows", [1, 5, 1025])
@pytest.mark.parametrize("dtype", [bf16, f32], ids=["bf16", "fp32"])
def test_layernorm_bwd_ordered(ops, dtype, rows, D, dropped):
    p, seed = (LR.P_DROP, 4242) if dropped else (0.0, 0)
    for int_dy in (True, False):
        o = LR.operands(rows, D, dtype, 31 * rows + D, DEV, int_dy=int_dy)
        _, mean, rstd = ops.layernorm_fwd(o["x"], o["gamma"], o["beta"], 1e-5)
        sums0 = {n: o[n + "0"] for n in LR.SUMS}

        def call(fn):
            s = {n: R.Guarded(1, D, f32, DEV, ld=D + 4, pre=1, post=1, init=v[None, :]) for n, v in sums0.items()}
            dx = torch.full((rows, D), float("nan"), dtype=dtype, device=DEV)
            r = fn(o["dy"], o["x"], o["gamma"], mean, rstd, add=o["add"], dgamma=s["dgamma"].view[0], dbeta=s["dbeta"].view[0],
                   dx=dx, drop_p=p, drop_seed=seed, colsum=s["colsum"].view[0], want_dropped=True)
            assert all(g.untouched() for g in s.values())
            return {"dx": r[0], "dxd": r[1], **{n: g.view[0] for n, g in s.items()}}

        got = repeatable(lambda: call(ops.layernorm_bwd_ordered), "layernorm_bwd_ordered")
        base = call(ops.layernorm_bwd)
        assert same_bits(got["dx"], base["dx"]) and same_bits(got["dxd"], base["dxd"]), "dx / dxd must keep mdt_layernorm_bwd's bits"
        ref = LR.reference_bwd(o["dy"], o["x"], o["gamma"], mean, rstd, add=o["add"], drop_p=p, drop_seed=seed,
                               dgamma0=sums0["dgamma"], dbeta0=sums0["dbeta"], colsum0=sums0["colsum"], want_dropped=dropped,
                               want_colsum=True, dx_stored=got["dx"], dxd_stored=got["dxd"])
        sums = {n: got[n] for n in LR.SUMS}
        if int_dy:      # dbeta sums integers: exact in any order
            assert torch.equal(sums["dbeta"].double(), ref["dbeta"][0]), "dbeta of integer dy is determined"
        LR.check(sums, ref, {n: f32 for n in LR.SUMS}, what=f"layernorm_bwd_ordered {rows}x{D}")


def test_layernorm_bwd_ordered_workspace_is_a_function_of_the_shape(ops, monkeypatch):
    need = int(L.lib.mdt_layernorm_bwd_ordered_workspace_bytes(1025, 768))
    assert need == 3 * 65 * 768 * 4                 # 4 waves x 4 rows per workgroup: 65 workgroups
    monkeypatch.setenv("MDT_LN_BWD_WGS", "3")       # the tuning switch of the atomic form is not read
    L.reload_env()
    try:
        assert int(L.lib.mdt_layernorm_bwd_ordered_workspace_bytes(1025, 768)) == need
        o = LR.operands(1025, 768, bf16, 1, DEV)
        _, mean, rstd = ops.layernorm_fwd(o["x"], o["gamma"], o["beta"], 1e-5)
        g = torch.zeros(768, dtype=f32, device=DEV)
        with pytest.raises(L.MdtError, match="workspace"):
            ops.layernorm_bwd_ordered(o["dy"], o["x"], o["gamma"], mean, rstd, dgamma=g, ws=torch.empty(need - 16, dtype=torch.uint8, device=DEV))
        a = ops.layernorm_bwd_ordered(o["dy"], o["x"], o["gamma"], mean, rstd, dgamma=g)
        monkeypatch.delenv("MDT_LN_BWD_WGS")
        L.reload_env()
        g2 = torch.zeros(768, dtype=f32, device=DEV)
        b = ops.layernorm_bwd_ordered(o["dy"], o["x"], o["gamma"], mean, rstd, dgamma=g2)
        assert same_bits(a, b) and same_bits(g, g2)
    finally:
        monkeypatch.delenv("MDT_LN_BWD_WGS", raising=False)
        L.reload_env()


# ------------------------------------------------------------------------------------------------ segment sum
SEG_CASES = {
    "one_segment": lambda n, T: torch.full((n,), 2, dtype=torch.int32),                 # longer than the chunk length
    "all_distinct": lambda n, T: torch.randperm(T, generator=torch.Generator().manual_seed(1))[:n].to(torch.int32),
    "mixed_with_empty_and_skipped": lambda n, T: (torch.randint(-1, T // 3, (n,), generator=torch.Generator().manual_seed(2)) * 3
                                                   ).clamp(min=-1).to(torch.int32),
}


@pytest.mark.parametrize("stride", [(1, 0), (2, 1)], ids=["dense", "strided"])
@pytest.mark.parametrize("dtype", [bf16, f32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("D", [8, 128, 776])
@pytest.mark.parametrize("case", list(SEG_CASES))
def test_row_segment_sum_bits(ops, case, D, dtype, stride):
    n, T = 3 * EMU.CHUNK + 9, 3 * EMU.CHUNK + 40
    s_stride, s_off = stride
    idx = SEG_CASES[case](n, T).to(DEV)
    src = R.gen((n * s_stride + s_off, D), n + D, 3.0, dtype, DEV)
    src[::5] = src[::5] * 4096.0                      # a wide range of magnitudes: the order shows in the last bits
    t0 = R.gen((T, D), 9, 3.0, f32, DEV)
    seg_row, seg_off, order = ops.segments_of(idx, T)
    cr, co, cord = EMU.segments_of(idx.cpu(), T)
    assert torch.equal(seg_row.cpu(), cr) and torch.equal(seg_off.cpu(), co) and torch.equal(order.cpu(), cord)

    def run():
        tab = R.Guarded(T, D, f32, DEV, ld=D + 4, init=t0)
        ops.row_segment_sum(tab.view, seg_row, seg_off, order, src, s_stride=s_stride, s_off=s_off)
        assert tab.untouched()
        return {"table": tab.view}

    got = repeatable(run, "row_segment_sum")["table"]
    want = EMU.emu_segment_sum(t0.cpu(), cr, co, cord, src.cpu(), s_stride, s_off)
    assert torch.equal(got.cpu(), want), "row_segment_sum: not the documented two-level order"
    V, DL, _ = RR.reference_scatter_add(t0, idx, src, n, s_stride, s_off)
    RR.assert_within(got, V, RR.bound(V, DL, f32), what="row_segment_sum")
    untouched = torch.ones(T, dtype=torch.bool)
    untouched[idx.cpu()[idx.cpu() >= 0].long()] = False
    assert same_bits(got[untouched.to(DEV)], t0[untouched.to(DEV)]), "rows of empty segments changed"


# ------------------------------------------------------------------------------------------------ bias histogram
@pytest.mark.parametrize("ns", [23, 512], ids=["23rows_256threads", "512rows_32threads"])
@pytest.mark.parametrize("S", [8, 65, 81])
def test_attn_bias_grad_ordered(ops, S, ns):
    """``ns`` table rows: 23 is what a spatial_pos_max of 5 uses (256 histogram threads), 512 is the model's num_spatial (32)."""
    nseq, H = 3, 3
    g = torch.Generator(device=DEV).manual_seed(S)
    sp = torch.randint(0, 23, (nseq, S - 1, S - 1), generator=g, device=DEV, dtype=torch.int32)
    if ns > 23:
        sp[:, 0, :] = ns - 1                          # the last table row is reached too
    t0 = R.gen((ns, H), 1, 2.0, f32, DEV)
    t0[0] = 0.0
    v0 = R.gen((H,), 2, 2.0, f32, DEV)

    def run_with(dS):
        def run():
            tab = R.Guarded(ns, H, f32, DEV, ld=H, init=t0)
            virt = R.Guarded(1, H, f32, DEV, ld=H, pre=1, post=1, init=v0[None, :])
            ops.attn_bias_grad_ordered(dS, sp, tab.view, virt.view[0])
            assert tab.untouched() and virt.untouched()
            return {"table": tab.view, "virt": virt.view[0]}
        return repeatable(run, f"attn_bias_grad_ordered S={S}")

    def index_add(dS):      # fp64, the bins of attn_bias_grad_add
        d = dS.double()
        tab = torch.zeros(ns, H, dtype=torch.float64, device=DEV)
        inner = d[:, :, 1:, 1:].permute(0, 2, 3, 1).reshape(-1, H)
        tab.index_add_(0, sp.reshape(-1).long(), inner)
        tab[0] = 0.0
        virt = d[:, :, 0, :].sum((0, 2)) + d[:, :, 1:, 0].sum((0, 2))
        mag = torch.zeros(ns, H, dtype=torch.float64, device=DEV)
        mag.index_add_(0, sp.reshape(-1).long(), inner.abs())
        vmag = d[:, :, 0, :].abs().sum((0, 2)) + d[:, :, 1:, 0].abs().sum((0, 2))
        return tab, virt, mag, vmag

    # integer dS: every sum exact
    dS = R.gen_int((nseq, H, S, S), 3, 8, f32, DEV)
    got = run_with(dS)
    tab, virt, _, _ = index_add(dS)
    # the integer sums are exact, the old value joins them with ONE rounding: every bit is determined
    assert torch.equal(got["table"], (t0.double() + tab).float()) and torch.equal(got["virt"], (v0.double() + virt).float())
    # random dS: the documented order, bit for bit, and the sum-rule bound γ_n Σ|terms| (n = all elements of a launch, at most)
    dS = order_sensitive((nseq, H, S, S), 4, big_every=50) * (torch.rand(nseq, H, S, S, generator=g, device=DEV) + 0.5)
    got = run_with(dS)
    et, ev = EMU.emu_bias_hist(dS.cpu(), sp.cpu(), t0.cpu(), v0.cpu())
    assert torch.equal(got["table"].cpu(), et) and torch.equal(got["virt"].cpu(), ev), "not the documented histogram order"
    tab, virt, mag, vmag = index_add(dS)
    n_terms = nseq * S * S + 1
    gam = R._gamma(n_terms)
    R.assert_within(got["table"], t0.double() + tab, R.bound(t0.double() + tab, gam * (mag + t0.double().abs()), f32), what="d_sp_table")
    R.assert_within(got["virt"], v0.double() + virt, R.bound(v0.double() + virt, gam * (vmag + v0.double().abs()), f32), what="d_virt")
    assert same_bits(got["table"][0], t0[0]) and not bool(got["table"][0].any()), "table row 0 (the padding index) must stay exactly zero"


def test_attn_bias_grad_ordered_refuses_a_short_workspace(ops):
    need = int(L.lib.mdt_attn_bias_grad_ordered_workspace_bytes(3, 3, 23))
    assert need == 3 * 24 * 3 * 4
    dS = torch.zeros(3, 3, 8, 8, dtype=f32, device=DEV)
    sp = torch.zeros(3, 7, 7, dtype=torch.int32, device=DEV)
    with pytest.raises(L.MdtError, match="workspace"):
        ops.attn_bias_grad_ordered(dS, sp, torch.zeros(23, 3, device=DEV), torch.zeros(3, device=DEV),
                                   ws=torch.empty(need - 1, dtype=torch.uint8, device=DEV))


def test_float_atomic_launch_counter(ops):
    x = torch.ones(64, 16, dtype=f32, device=DEV)
    ops.float_atomic_launches(reset=True)
    ops.colsum_ordered(x)
    ops.sum_slices(x.view(4, 16, 16), torch.zeros(16, 16, device=DEV))
    assert ops.float_atomic_launches() == 0, "an ordered entry point counted as a float-atomic launch"
    ops.colsum(x)
    ops.row_scatter_add(torch.zeros(4, 16, device=DEV), torch.zeros(64, dtype=torch.int32, device=DEV), x, 64)
    assert ops.float_atomic_launches(reset=True) == 2 and ops.float_atomic_launches() == 0
