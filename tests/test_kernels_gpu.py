"""Kernel-level parity: every C-ABI entry point against a plain PyTorch fp32 computation
of the same op on the CPU.  fp32 kernels: atol 2e-4 (1e-3 is the gate in north_star);
bf16 kernels: compared on bf16-rounded inputs with a bf16-sized tolerance stated per test.

The strict gate for attention is tests/test_attention_routes_gpu.py: every kernel and route against the fp64 reference of
tests/attention_reference.py with a derived bound per element; the assert_close gates here are wide enough for a skipped key.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from multimodaldiscussiontransformer_amd import _lib as L
from tests import attention_reference as A
from tests import gemm_reference as GR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from multimodaldiscussiontransformer_amd import ops as o
    assert torch.cuda.is_available(), "GPU tests need a device"
    return o


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def dev(t, dtype=None):
    t = t.cuda()
    return t.to(dtype) if dtype is not None else t


def rel_err(a, b):
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


# ----------------------------------------------------------------------------- GEMM
@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("M,N,K", [(70, 35, 19), (128, 64, 64), (1, 2, 768), (200, 130, 100)])
def test_gemm_generic_f32(ops, ta, tb, M, N, K):
    a = rnd(K, M, seed=1) if ta else rnd(M, K, seed=1)
    b = rnd(K, N, seed=2) if tb else rnd(N, K, seed=2)
    ref = (a.t() if ta else a) @ (b if tb else b.t())
    out = ops.gemm(dev(a), dev(b), trans_a=bool(ta), trans_b=bool(tb))
    torch.testing.assert_close(out.cpu(), ref, atol=2e-4, rtol=1e-5)


def test_gemm_f32_epilogues(ops):
    M, N, K = 50, 40, 36
    a, b, bias, res = rnd(M, K, seed=1), rnd(N, K, seed=2), rnd(N, seed=3), rnd(M, N, seed=4)
    u = a @ b.t() + bias
    aux = torch.empty(M, N).cuda()
    out = ops.gemm(dev(a), dev(b), bias=dev(bias), aux=aux, epilogue=ops.EPI_GELU)
    torch.testing.assert_close(aux.cpu(), u, atol=2e-4, rtol=1e-5)
    torch.testing.assert_close(out.cpu(), F.gelu(u), atol=2e-4, rtol=1e-5)
    out = ops.gemm(dev(a), dev(b), bias=dev(bias), residual=dev(res))
    torch.testing.assert_close(out.cpu(), u + res, atol=2e-4, rtol=1e-5)
    # dgelu: out = (a @ b^T) * gelu'(aux)
    x = u.clone().requires_grad_(True)
    F.gelu(x).backward(a @ b.t())
    out = ops.gemm(dev(a), dev(b), aux=dev(u), epilogue=ops.EPI_DGELU)
    torch.testing.assert_close(out.cpu(), x.grad, atol=2e-4, rtol=1e-5)
    # accumulate + atomic split-K
    c = dev(res.clone())
    ops.gemm(dev(a), dev(b), out=c, epilogue=ops.EPI_ACCUM)
    torch.testing.assert_close(c.cpu(), res + a @ b.t(), atol=2e-4, rtol=1e-5)
    c = dev(res.clone())
    ops.gemm(dev(a), dev(b), out=c, epilogue=ops.EPI_ATOMIC, split_k=3)
    torch.testing.assert_close(c.cpu(), res + a @ b.t(), atol=2e-4, rtol=1e-5)


@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("M,N,K", [(256, 128, 64), (300, 256, 192), (128, 384, 1024)])
def test_gemm_bf16_tile128(ops, ta, tb, M, N, K):
    if ta and M % 128:
        M = 384
    a = (rnd(K, M, seed=1) if ta else rnd(M, K, seed=1)).bfloat16()
    b = (rnd(K, N, seed=2) if tb else rnd(N, K, seed=2)).bfloat16()
    af, bf = a.float(), b.float()
    ref = (af.t() if ta else af) @ (bf if tb else bf.t())
    out32 = ops.gemm(dev(a), dev(b), trans_a=bool(ta), trans_b=bool(tb), out_dtype=torch.float32)
    # fp32 accumulation of exact bf16 products: only summation-order error
    torch.testing.assert_close(out32.cpu(), ref, atol=1e-3, rtol=1e-4)
    out16 = ops.gemm(dev(a), dev(b), trans_a=bool(ta), trans_b=bool(tb))
    torch.testing.assert_close(out16.float().cpu(), ref, atol=0.06, rtol=1e-2)   # bf16 rounding of |x| <~ 8
    v, d = GR.reference(a, b, trans_a=bool(ta), trans_b=bool(tb))["out"]       # per element: ½ ulp of bf16 + the fp32 sum's bound
    GR.assert_within(out16.cpu(), v, GR.bound(v, d, torch.bfloat16), what="tile128 bf16 out")
    GR.assert_within(out32.cpu(), v, GR.bound(v, d, torch.float32), what="tile128 fp32 out")


def test_gemm_bf16_wgrad_splitk_and_epilogues(ops):
    # weight gradient shape: dW[N,K] = dY[M,N]^T X[M,K], reduction over M tokens with a ragged tail
    M, N, K = 1000, 256, 128
    dy, x = rnd(M, N, seed=5).bfloat16(), rnd(M, K, seed=6).bfloat16()
    ref = dy.float().t() @ x.float()
    c = torch.zeros(N, K, dtype=torch.float32).cuda()
    ops.gemm(dev(dy), dev(x), trans_a=True, trans_b=True, out=c, epilogue=ops.EPI_ATOMIC, split_k=4)
    torch.testing.assert_close(c.cpu(), ref, atol=5e-3, rtol=1e-4)
    # bias + gelu + aux, bias + residual on the tile kernel
    M, N, K = 260, 128, 128
    a, b = rnd(M, K, seed=1).bfloat16(), rnd(N, K, seed=2, scale=0.2).bfloat16()
    bias, res = rnd(N, seed=3).bfloat16(), rnd(M, N, seed=4).bfloat16()
    u = a.float() @ b.float().t() + bias.float()
    aux = torch.empty(M, N, dtype=torch.bfloat16).cuda()
    out = ops.gemm(dev(a), dev(b), bias=dev(bias), aux=aux, epilogue=ops.EPI_GELU)
    torch.testing.assert_close(aux.float().cpu(), u, atol=0.03, rtol=1e-2)
    torch.testing.assert_close(out.float().cpu(), F.gelu(u), atol=0.03, rtol=1e-2)
    out = ops.gemm(dev(a), dev(b), bias=dev(bias), residual=dev(res))
    torch.testing.assert_close(out.float().cpu(), u + res.float(), atol=0.03, rtol=1e-2)


@pytest.mark.parametrize("rows,N,K,split", [(9000, 2304, 768, 5), (4100, 768, 3072, 3), (1000, 256, 128, 4), (300, 2304, 768, 1)])
def test_gemm_wgrad_with_bias_gradient_riding(ops, rows, N, K, split):
    """MDT_EPI_ASUM: db = colsum(dY) accumulated by the weight-gradient GEMM dW = dY^T X itself (256 x 256 ping-pong
    kernel: one MFMA against ones per A fragment in tile column 0) or, on every other path, by the column-sum kernel
    the entry point runs first.  Both outputs ACCUMULATE into what the buffers held."""
    dy, x = rnd(rows, N, seed=21).bfloat16(), rnd(rows, K, seed=22).bfloat16()
    w0, b0 = rnd(N, K, seed=23), rnd(N, seed=24)
    gw, gb = dev(w0.clone()), dev(b0.clone())
    ops.gemm(dev(dy), dev(x), trans_a=True, trans_b=True, out=gw, epilogue=ops.EPI_ATOMIC, split_k=split, asum=gb)
    ref_w = w0 + dy.float().t() @ x.float()
    ref_b = b0 + dy.float().sum(0)
    torch.testing.assert_close(gw.cpu(), ref_w, atol=2e-2, rtol=1e-4)
    torch.testing.assert_close(gb.cpu(), ref_b, atol=2e-3 * (rows ** 0.5), rtol=1e-4)


@pytest.mark.parametrize("rows,N,K,split,asum", [(30000, 768, 3072, 7, True), (30011, 3072, 768, 7, True), (20037, 2304, 768, 12, True),
                                                 (30000, 768, 3072, 7, False), (1100, 1024, 1024, 4, False)])
def test_gemm_wgrad_four_wave_split_k(ops, rows, N, K, split, asum, monkeypatch):
    """gemm_bf16_w4s (gemm_wgrad.hip): the split-K weight gradient dW[N, K] = dY[rows, N]^T X[rows, K] in the 4-wave form —
    both operands k-major, fp32 atomics into what the buffer held, the bias gradient riding in tile column 0
    (MDT_EPI_ASUM), a reduction length that is not a multiple of 64 (zero-filled through the descriptor) and slabs as short
    as four K-tiles — against fp32 torch and against the 8-wave kernel (MDT_GEMM_ROUTE=pp256) on the same inputs.  (The last
    case's 140-row slab is too short for the 4-wave kernel: the default route runs there.)"""
    from multimodaldiscussiontransformer_amd import _lib as L
    dy, x = rnd(rows, N, seed=41, scale=0.25).bfloat16(), rnd(rows, K, seed=42, scale=0.25).bfloat16()
    w0, b0 = rnd(N, K, seed=43), rnd(N, seed=44)
    dyd, xd = dev(dy), dev(x)
    ref_w = (dev(w0).double() + dyd.double().t() @ xd.double()).float().cpu()
    ref_b = b0 + dy.float().sum(0)
    outs = {}
    for route in ("w4s", "pp256"):
        monkeypatch.setenv("MDT_GEMM_ROUTE", route)
        L.reload_env()
        gw, gb = dev(w0.clone()), dev(b0.clone())
        ops.gemm(dyd, xd, trans_a=True, trans_b=True, out=gw, epilogue=ops.EPI_ATOMIC, split_k=split, asum=gb if asum else None)
        torch.cuda.synchronize()
        assert L.last_route() == (route if rows != 1100 or route == "pp256" else "tile128"), L.last_route()
        outs[route] = (gw.cpu(), gb.cpu())
        torch.testing.assert_close(outs[route][0], ref_w, atol=2e-2, rtol=1e-4, msg=f"dW, MDT_GEMM_ROUTE={route}")
        if asum:
            torch.testing.assert_close(outs[route][1], ref_b, atol=2e-3 * (rows ** 0.5), rtol=1e-4, msg=f"db, MDT_GEMM_ROUTE={route}")
        else:
            assert torch.equal(outs[route][1], b0)
    monkeypatch.delenv("MDT_GEMM_ROUTE")
    L.reload_env()
    # the two kernels add the same per-slab partial sums (same k order inside a slab); only the atomics' order differs
    torch.testing.assert_close(outs["w4s"][0], outs["pp256"][0], atol=2e-3, rtol=1e-5)


@pytest.mark.parametrize("tb,kind", [(False, "bias"), (False, "dense"), (True, "plain"), (True, "res"), (False, "res"), (False, "plain"),
                                     (True, "mulaux"), (False, "mulaux"), (False, "gelu")])
def test_gemm_four_wave_form_is_bit_identical(ops, tb, kind, monkeypatch):
    """MDT_GEMM_ROUTE=w4p: the 4-wave persistent kernel (gemm_bf16_w4p: one wave per SIMD, 128 x 128 per wave, hand-ordered
    MFMA / fragment-read / LDS-DMA stream, half of a finished tile leaving during the next tile's first steps) accumulates
    every element in the same k order through the same epilogue code as the 8-wave kernel (MDT_GEMM_ROUTE=pp256p): identical
    bits, ragged last row tile included — forced on any persistent launch (k-major operands, heavy epilogues too)."""
    from multimodaldiscussiontransformer_amd import _lib as L
    M, N, K = 66000 + 37, 768, 768
    bf = torch.bfloat16
    a = dev(rnd(M, K, seed=31).to(bf))
    b = dev((rnd(K, N, seed=32) if tb else rnd(N, K, seed=32)).to(bf))
    kw = dict(trans_b=tb)
    if kind in ("bias", "dense"):
        kw["bias"] = dev(rnd(N, seed=33).to(bf))
    if kind in ("dense", "res"):
        kw["residual"] = dev(rnd(M, N, seed=34).to(bf))
    if kind == "dense":
        kw.update(drop_p=0.4, drop_seed=7)
    if kind == "mulaux":                             # fc2's input gradient: saved derivative x product, bias-gradient column sums
        kw.update(aux=dev(rnd(M, N, seed=35).to(bf)), epilogue=ops.EPI_MULAUX)
    if kind == "gelu":                               # fc1 forward: two outputs
        kw.update(bias=dev(rnd(N, seed=33).to(bf)), epilogue=ops.EPI_GELU | ops.EPI_AUX_GRAD)
    outs, extra = [], []
    try:
        for v in ("pp256p", "w4p"):
            monkeypatch.setenv("MDT_GEMM_ROUTE", v)
            L.reload_env()
            kw2 = dict(kw)
            if kind == "mulaux":
                kw2["colsum"] = torch.zeros(N, device="cuda", dtype=torch.float32)
            if kind == "gelu":
                kw2["aux"] = torch.empty(M, N, device="cuda", dtype=bf)
            outs.append(ops.gemm(a, b, **kw2).clone())
            assert L.last_route() == v
            extra.append(kw2.get("colsum", kw2.get("aux") if kind == "gelu" else None))
    finally:
        monkeypatch.delenv("MDT_GEMM_ROUTE")
        L.reload_env()
    assert torch.equal(outs[0], outs[1])
    if kind == "gelu":
        assert torch.equal(extra[0], extra[1])
    if kind == "mulaux":                             # fp32 atomics: the order of the partial sums differs
        torch.testing.assert_close(extra[0], extra[1], atol=2e-2, rtol=1e-3)
    ref = a.float() @ (b.float() if tb else b.float().t())
    if kind == "plain":
        torch.testing.assert_close(outs[1].float(), ref, atol=0.5, rtol=2e-2)


@pytest.mark.parametrize("K", [576, 640, 704, 1088])
def test_gemm_four_wave_form_short_and_odd_k(ops, K, monkeypatch):
    """The 4-wave kernel walks 18 explicit steps, a loop and two closing steps per tile: K = 640 is the shortest launch it takes
    (20 steps, empty loop), 704 the next (22), 1088 has an odd number of 64-deep K-tiles behind the explicit steps; K = 576 must
    stay on the 8-wave kernel even when the 4-wave one is forced.  Same bits as the 8-wave kernel everywhere."""
    from multimodaldiscussiontransformer_amd import _lib as L
    M, N = 33000 + 5, 512
    bf = torch.bfloat16
    a = dev(rnd(M, K, seed=41).to(bf))
    for tb in (False, True):
        b = dev((rnd(K, N, seed=42) if tb else rnd(N, K, seed=42)).to(bf))
        kw = dict(trans_b=tb, bias=dev(rnd(N, seed=43).to(bf)), residual=dev(rnd(M, N, seed=44).to(bf)), drop_p=0.4, drop_seed=9)
        outs = []
        try:
            for v in ("pp256p", "w4p"):
                monkeypatch.setenv("MDT_GEMM_ROUTE", v)
                L.reload_env()
                outs.append(ops.gemm(a, b, **kw).clone())
                assert L.last_route() == ("pp256p" if K == 576 else v)
        finally:
            monkeypatch.delenv("MDT_GEMM_ROUTE")
            L.reload_env()
        assert torch.equal(outs[0], outs[1])
        ref = a.float() @ (b.float() if tb else b.float().t())
        plain = ops.gemm(a, b, trans_b=tb)
        torch.testing.assert_close(plain.float(), ref, atol=0.6, rtol=2e-2)


@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_gemm_bf16_tile256_pipeline(ops, ta, tb):
    """Shapes large enough for the 256x128 three-stage kernel (>= 256 tiles), ragged M tail,
    K from 1 to many pipeline steps, every operand layout."""
    for (M, N, K) in [(33000, 256, 64), (33000, 256, 192), (16640, 512, 1024), (66000, 512, 192), (131072 + 77, 256, 64)]:
        if ta:
            M = (M // 256) * 256
        a = (rnd(K, M, seed=1) if ta else rnd(M, K, seed=1)).bfloat16()
        b = (rnd(K, N, seed=2) if tb else rnd(N, K, seed=2)).bfloat16()
        ad, bd = dev(a), dev(b)
        ref = ((ad.float().t() if ta else ad.float()) @ (bd.float() if tb else bd.float().t())).cpu()
        out32 = ops.gemm(ad, bd, trans_a=bool(ta), trans_b=bool(tb), out_dtype=torch.float32)
        torch.testing.assert_close(out32.cpu(), ref, atol=2e-3, rtol=1e-3)
    # epilogues through the pipeline kernel
    if not ta and not tb:
        M, N, K = 33000, 256, 128
        a, b = rnd(M, K, seed=1).bfloat16(), rnd(N, K, seed=2, scale=0.2).bfloat16()
        bias, res = rnd(N, seed=3).bfloat16(), rnd(M, N, seed=4).bfloat16()
        u = a.float() @ b.float().t() + bias.float()
        aux = torch.empty(M, N, dtype=torch.bfloat16).cuda()
        out = ops.gemm(dev(a), dev(b), bias=dev(bias), aux=aux, epilogue=ops.EPI_GELU)
        torch.testing.assert_close(aux.float().cpu(), u, atol=0.03, rtol=1e-2)
        torch.testing.assert_close(out.float().cpu(), F.gelu(u), atol=0.03, rtol=1e-2)
        out = ops.gemm(dev(a), dev(b), bias=dev(bias), residual=dev(res))
        torch.testing.assert_close(out.float().cpu(), u + res.float(), atol=0.03, rtol=1e-2)
        x = u.clone().requires_grad_(True)
        F.gelu(x).backward(a.float() @ b.float().t())
        out = ops.gemm(dev(a), dev(b), aux=dev(u.bfloat16()), epilogue=ops.EPI_DGELU, out_dtype=torch.float32)
        xb = u.bfloat16().float().requires_grad_(True)
        F.gelu(xb).backward(a.float() @ b.float().t())
        torch.testing.assert_close(out.cpu(), xb.grad, atol=2e-3, rtol=1e-3)
    if ta and tb:   # split-K weight gradient with a ragged reduction tail
        Mred, N, K = 50000, 1024, 1024
        dy, x = rnd(Mred, N, seed=5, scale=0.1).bfloat16(), rnd(Mred, K, seed=6, scale=0.1).bfloat16()
        dyd, xd = dev(dy), dev(x)
        ref = (dyd.float().t() @ xd.float()).cpu()
        c = torch.zeros(N, K, dtype=torch.float32).cuda()
        ops.gemm(dyd, xd, trans_a=True, trans_b=True, out=c, epilogue=ops.EPI_ATOMIC, split_k=8)
        torch.testing.assert_close(c.cpu(), ref, atol=5e-3, rtol=2e-3)
        c.zero_()                                   # 16 slices -> the 256x256 tile variant
        ops.gemm(dyd, xd, trans_a=True, trans_b=True, out=c, epilogue=ops.EPI_ATOMIC, split_k=16)
        torch.testing.assert_close(c.cpu(), ref, atol=5e-3, rtol=2e-3)


@pytest.mark.parametrize("tb", [0, 1])
@pytest.mark.parametrize("M,N,K", [(16640, 1024, 256), (16677, 1024, 768), (70000, 768, 128), (66000, 3072, 192)])
def test_gemm_bf16_out_big_tiles(ops, M, N, K, tb, monkeypatch):
    """bf16 OUTPUT through the 256x256 ping-pong kernels: register-resident epilogue (transposed accumulators +
    lane swaps), persistent tile loop (more tiles than CUs) and its one-tile-per-workgroup form, ragged last row
    tile, bias / residual / column sums.  (The fp32-output tests above take the LDS-parked epilogue instead.)"""
    a = rnd(M, K, seed=1).bfloat16()
    b = (rnd(K, N, seed=2, scale=0.3) if tb else rnd(N, K, seed=2, scale=0.3)).bfloat16()
    bias, res = rnd(N, seed=3).bfloat16(), rnd(M, N, seed=4).bfloat16()
    ad, bd = dev(a), dev(b)
    ref = ad.float() @ (bd.float() if tb else bd.float().t())
    tol = dict(atol=0.06, rtol=1.5e-2)
    walk = K >= 512 and -(-M // 256) * (N // 256) > 256             # 16 32-deep steps per tile, more tiles than CUs
    default = ("w4p" if K >= 640 else "pp256p") if walk else "pp256"
    # static walk, dynamic tile queue, one tile per workgroup
    for route, dynamic, want in (("", "0", default), ("", "1", "pp256p" if walk else "pp256"), ("pp256", "0", "pp256")):
        monkeypatch.setenv("MDT_GEMM_ROUTE", route)
        monkeypatch.setenv("MDT_GEMM_DYNAMIC", dynamic)
        L.enable_dynamic_tile_queue()                                 # caller-owned queue memory (the library allocates nothing)
        L.reload_env()                                                # the switches are cached: say that they changed
        for _ in range(2):                                            # twice: the queue must come back zeroed
            out = ops.gemm(ad, bd, trans_b=bool(tb))
            assert L.last_route() == want, (route, dynamic, L.last_route())
            torch.testing.assert_close(out.float(), ref, **tol)
    monkeypatch.setenv("MDT_GEMM_DYNAMIC", "0")
    monkeypatch.delenv("MDT_GEMM_ROUTE")
    L.reload_env()
    cs = torch.zeros(N, dtype=torch.float32).cuda()
    out = ops.gemm(ad, bd, trans_b=bool(tb), bias=dev(bias), residual=dev(res), colsum=cs)
    full = ref + dev(bias).float() + dev(res).float()
    torch.testing.assert_close(out.float(), full, **tol)
    torch.testing.assert_close(cs, full.sum(0), atol=1.0, rtol=2e-2)


def test_gemm_training_epilogues_persistent(ops):
    """The epilogue flag sets of a training step each have their own instantiation of the persistent 256x256 kernel
    (flags folded at compile time, operand vectors requested a column pair ahead): bias; bias + dropout + residual;
    bias + GELU + saved derivative; plain and residual input gradients; saved-derivative multiply + column sums.
    More tiles than CUs (persistent walk) and a ragged last row tile."""
    M, N, K = 16640 + 13, 1280, 768
    bf = torch.bfloat16
    a, w, bias = dev(rnd(M, K, seed=1).to(bf)), dev(rnd(N, K, seed=2, scale=0.05).to(bf)), dev(rnd(N, seed=3).to(bf))
    tol = dict(atol=0.06, rtol=2e-2)
    u = a.float() @ w.float().t() + bias.float()
    torch.testing.assert_close(ops.gemm(a, w, bias=bias).float(), u, **tol)                                   # 1
    aux = torch.empty(M, N, device="cuda", dtype=bf)
    h = ops.gemm(a, w, bias=bias, aux=aux, epilogue=ops.EPI_GELU | ops.EPI_AUX_GRAD)                          # 259
    torch.testing.assert_close(h.float(), F.gelu(u), **tol)
    ur = u.clone().requires_grad_(True)
    F.gelu(ur).sum().backward()
    torch.testing.assert_close(aux.float(), ur.grad, **tol)
    res = dev(rnd(M, N, seed=4, scale=0.5).to(bf))
    mask = ops.dropout_mask(M * N, 0.4, 77).view(M, N).float() / 0.6
    y = ops.gemm(a, w, bias=bias, residual=res, drop_p=0.4, drop_seed=77)                                     # 69
    torch.testing.assert_close(y.float(), u * mask + res.float(), **tol)
    dy = dev(rnd(M, N, seed=5, scale=0.1).to(bf))
    dref = dy.float() @ w.float()
    dg = ops.gemm(dy, w, trans_b=True)                                                                       # 0
    torch.testing.assert_close(dg.float(), dref, **tol)
    v, d = GR.reference(dy, w, trans_b=True)["out"]
    GR.assert_within(dg, v, GR.bound(v, d, bf), what="dgrad dy @ w")
    resk = dev(rnd(M, K, seed=6, scale=0.5).to(bf))
    torch.testing.assert_close(ops.gemm(dy, w, trans_b=True, residual=resk).float(), dref + resk.float(), **tol)   # 4
    w2 = dev(rnd(K, N, seed=7, scale=0.05).to(bf))
    dz = dev(rnd(M, K, seed=8, scale=0.1).to(bf))
    cs = torch.zeros(N, device="cuda", dtype=torch.float32)
    du = ops.gemm(dz, w2, trans_b=True, aux=aux, epilogue=ops.EPI_MULAUX, colsum=cs)                          # 640
    du_ref = (dz.float() @ w2.float()) * aux.float()
    torch.testing.assert_close(du.float(), du_ref, **tol)
    torch.testing.assert_close(cs, du_ref.sum(0), atol=1.0, rtol=3e-2)
    r = GR.reference(dz, w2, trans_b=True, epilogue=GR.EPI_MULAUX, aux=aux)   # (exact column sums: tests/test_gemm_routes_gpu.py)
    GR.check({"out": du}, r, {"out": bf}, what="d fc1 saved-derivative product")


def test_colsum_cast_transpose(ops):
    x = rnd(1037, 200, seed=9)
    torch.testing.assert_close(ops.colsum(dev(x)).cpu(), x.sum(0), atol=1e-3, rtol=1e-5)
    xb = x.bfloat16()
    torch.testing.assert_close(ops.colsum(dev(xb)).cpu(), xb.float().sum(0), atol=1e-3, rtol=1e-5)
    assert torch.equal(ops.cast(dev(x), torch.bfloat16).cpu(), xb)
    assert torch.equal(ops.transpose2d(dev(x), torch.bfloat16).cpu(), xb.t().contiguous())


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "row_weight"])
@pytest.mark.parametrize("dtype,N", [(torch.bfloat16, 72), (torch.float32, 36)], ids=["bf16-N72", "f32-N36"])
def test_colsum_vector_and_scalar_forms_agree_bit_for_bit(ops, dtype, N, weighted):
    """colsum_kernel<T, VN> (csrc/elementwise.hip) in its 16-byte form (contiguous rows) and, forced by a row stride of
    N + 1 elements, in its scalar form.  M = 30 rows are one row block in either form, so every column receives exactly
    one atomic add into a zeroed output and its bits are determined: row lane j adds rows j, j + 4, ..., the four lanes
    are added in order.  N is nine vectors: a partial last group of lanes, and in the scalar form a second column group.
    Both forms must agree bit for bit, and each must meet the fp64 bound of tests/gemm_reference.py for an fp32 sum of
    30 terms in any order (a term w * x carries one fp32 rounding where the product is no fp32 number)."""
    M = 30
    vn = 16 // torch.empty(0, dtype=dtype).element_size()
    x = rnd(M, N, seed=11).to(dtype)
    w = torch.randint(0, 4, (M,), generator=torch.Generator().manual_seed(12), dtype=torch.int32) if weighted else None
    xv = dev(x)
    xs = torch.zeros(M, N + 1, dtype=dtype, device="cuda")[:, :N]
    xs.copy_(xv)
    assert xv.stride(0) % vn == 0 and xv.data_ptr() % 16 == 0 and N % vn == 0 and xs.stride(0) % vn != 0
    wd = None if w is None else dev(w)
    vec = ops.colsum(xv, row_weight=wd).cpu()
    sca = ops.colsum(xs, row_weight=wd).cpu()
    terms = x.double() if w is None else x.double() * w.double()[:, None]
    d = torch.where(GR._rep32(terms), torch.zeros_like(terms), terms.abs() * GR.U32)
    ref = terms.sum(0)
    bnd = GR.bound(ref, GR._sum_bound(terms, d, torch.zeros(N, dtype=torch.float64), M, 0), torch.float32)
    for name, got in (("vector", vec), ("scalar", sca)):
        GR.assert_within(got, ref, bnd, what=f"colsum {name} form", dtype=torch.float32, median_limit=2.0 ** -7)
    assert torch.equal(vec.view(torch.int32), sca.view(torch.int32)), "the vector and the scalar colsum kernel differ"


def test_empty_inputs_are_no_ops(ops):
    """A batch may carry no image, a rank no labelled comment, a length bin no sequence: every entry point the step calls takes
    zero rows / sequences / images as a no-op (MDT_OK, nothing launched, outputs of the right — empty — shape)."""
    bf = torch.bfloat16
    D = 128
    z = lambda *shape, dtype=bf: torch.empty(*shape, dtype=dtype, device="cuda")
    w, b = dev(rnd(D, D, seed=1).to(bf)), dev(rnd(D, seed=2).to(bf))
    assert ops.gemm(z(0, D), w, bias=b).shape == (0, D)
    y, mean, rstd = ops.layernorm_fwd(z(0, D), b, b, 1e-5)
    assert y.shape == (0, D) and mean.numel() == 0
    dg = torch.zeros(D, dtype=torch.float32, device="cuda")
    assert ops.layernorm_bwd(z(0, D), z(0, D), b, mean, rstd, dgamma=dg, dbeta=dg.clone()).shape == (0, D)
    assert float(dg.abs().max()) == 0.0
    out, lse = ops.attention_fwd(z(0, 3 * D), 0, 16, 2)
    assert out.shape == (0, D)
    dq, _ = ops.attention_bwd(z(0, D), z(0, 3 * D), out, lse, 0, 16, 2)
    assert dq.shape == (0, 3 * D)
    off = dev(torch.zeros(1, dtype=torch.int32))
    out, lse = ops.attention_fwd(z(0, 3 * D), 0, 16, 2, seq_offsets=off)
    assert out.shape == (0, D)
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device="cuda")
    word = dev(rnd(10, D, seed=3).to(bf))
    ops.bert_embed_rows(i32(0), i32(0), i32(0), word, word, word[:2], z(0, D))
    y, _, _, xs = ops.bert_embed_ln_rows(i32(0), i32(0), i32(0), word, word, word[:2], b, b, 1e-5)
    assert y.shape == (0, D) and xs.shape == (0, D)
    tok = z(0, 768)
    ops.vit_patch_embed(torch.empty(0, 3, 32, 32, device="cuda"), 16, dev(rnd(768, 768, seed=4).to(bf)), dev(rnd(768, seed=5).to(bf)),
                        dev(rnd(768, seed=6).to(bf)), dev(rnd(5, 768, seed=7).to(bf)), tok, seq_stride=5, off=0)
    assert ops.vit_patchify(torch.empty(0, 3, 32, 32, device="cuda"), 16, bf).shape == (0, 768)
    ops.row_axpby(z(4, D), 0, a=z(0, D))
    table = torch.zeros(10, D, dtype=torch.float32, device="cuda")
    ops.row_scatter_add(table, i32(0), z(0, D), 0)
    assert float(table.abs().max()) == 0.0
    assert ops.dropout(z(0, D), 0.3, 7).shape == (0, D)
    assert ops.colsum(z(0, D)).shape == (D,) and float(ops.colsum(z(0, D)).abs().max()) == 0.0
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("D", [128, 768, 1024])
def test_layernorm(ops, dtype, D):
    rows = 77
    x = rnd(rows, D, seed=1, scale=2.0).to(dtype)
    g = (1 + 0.1 * rnd(D, seed=2)).to(dtype)
    b = (0.1 * rnd(D, seed=3)).to(dtype)
    dy = rnd(rows, D, seed=4).to(dtype)
    add = rnd(rows, D, seed=5).to(dtype)
    xr = x.float().requires_grad_(True)
    gr, br = g.float().requires_grad_(True), b.float().requires_grad_(True)
    yr = F.layer_norm(xr, (D,), gr, br, 1e-12)
    yr.backward(dy.float())
    tol = dict(atol=2e-4, rtol=1e-4) if dtype == torch.float32 else dict(atol=0.05, rtol=2e-2)
    y, mean, rstd = ops.layernorm_fwd(dev(x), dev(g), dev(b), 1e-12)
    torch.testing.assert_close(y.float().cpu(), yr.detach(), **tol)
    dg = torch.zeros(D, dtype=torch.float32).cuda()
    db = torch.zeros(D, dtype=torch.float32).cuda()
    dx = ops.layernorm_bwd(dev(dy), dev(x), dev(g), mean, rstd, add=dev(add), dgamma=dg, dbeta=db)
    torch.testing.assert_close(dx.float().cpu(), xr.grad + add.float(), **tol)
    torch.testing.assert_close(dg.cpu(), gr.grad, atol=5e-3 if dtype == torch.bfloat16 else 2e-4, rtol=1e-3)
    torch.testing.assert_close(db.cpu(), br.grad, atol=5e-3 if dtype == torch.bfloat16 else 2e-4, rtol=1e-3)


@pytest.mark.parametrize("D", [256, 512, 768, 1024])
@pytest.mark.parametrize("form", range(8))
def test_layernorm_backward_with_scalar_row_addresses_changes_no_bit(ops, D, form):
    """bf16 rows of 256 * NV elements take layernorm_bwd_rows_kernel (row offsets in SGPRs through buffer descriptors: 88-114
    VGPRs against 134-202, csrc/layernorm.hip); MDT_LN_GENERIC=1 sends the same call to the generic kernel.  Same arithmetic, and for
    768 columns in the same order: dx and the dropped copy are bit-identical there (within a bf16 ulp for the other widths) in all eight forms (residual gradient / dropped copy / column sums
    present or not), strided rows included; the three column sums are fp32 atomics across workgroups — equal up to their order.
    1031 rows: the last wave's block is short, some waves of the last workgroup have no row at all."""
    import os
    bf = torch.bfloat16
    rows, ld = 1031, D + 64
    has_add, has_cs, has_drop = bool(form & 1), bool(form & 2), bool(form & 4)
    x = dev(rnd(rows, ld, seed=1, scale=2.0).to(bf))[:, :D]
    dy = dev(rnd(rows, ld, seed=2).to(bf))[:, :D]
    add = dev(rnd(rows, ld, seed=3).to(bf))[:, :D] if has_add else None
    g = dev((1 + 0.1 * rnd(D, seed=4)).to(bf))
    b = dev((0.1 * rnd(D, seed=5)).to(bf))
    _, mean, rstd = ops.layernorm_fwd(x.contiguous(), g, b, 1e-12)

    def run():
        dg, db = torch.zeros(D, dtype=torch.float32).cuda(), torch.zeros(D, dtype=torch.float32).cuda()
        cs = torch.zeros(D, dtype=torch.float32).cuda() if has_cs else None
        dx = torch.full((rows, ld), 3.0, dtype=bf).cuda()[:, :D]
        out = ops.layernorm_bwd(dy, x, g, mean, rstd, add=add, dgamma=dg, dbeta=db, dx=dx, drop_p=0.4 if has_drop else 0.0, drop_seed=77,
                                colsum=cs, want_dropped=has_drop)
        dxd = out[1] if has_drop else None
        torch.cuda.synchronize()
        return dx.clone(), None if dxd is None else dxd.clone(), dg, db, cs

    try:
        os.environ["MDT_LN_GENERIC"] = "1"
        L.reload_env()
        ref = run()
    finally:
        os.environ.pop("MDT_LN_GENERIC", None)
        L.reload_env()
    got = run()
    def same(a, r):
        if D == 768:                    # the generic kernel on the same 8-byte vectors: the same sums in the same order
            assert torch.equal(a, r)
        else:                           # the generic kernel sums a row over 16-byte vectors on fewer lanes: another order, <= 1 bf16 ulp
            torch.testing.assert_close(a.float(), r.float(), atol=2e-3, rtol=2.0 ** -7)
    same(got[0], ref[0])
    if has_drop:
        same(got[1], ref[1])
        assert not torch.equal(got[1], got[0])
    for a, r in zip(got[2:], ref[2:]):
        if r is not None:
            torch.testing.assert_close(a, r, atol=2e-4 * max(1.0, float(r.abs().max())), rtol=1e-5)


# ----------------------------------------------------------------------------- attention
def ref_attention(qkv, nseq, S, H, scale, bias):
    """qkv [nseq,S,3D] fp32 (requires_grad), bias [nseq,H,S,S] additive (may hold -inf)."""
    D = qkv.shape[-1] // 3
    hd = D // H
    q, k, v = qkv.split(D, dim=-1)
    q = q.view(nseq, S, H, hd).transpose(1, 2)
    k = k.view(nseq, S, H, hd).transpose(1, 2)
    v = v.view(nseq, S, H, hd).transpose(1, 2)
    s = q @ k.transpose(-1, -2) * scale + bias
    p = torch.softmax(s, dim=-1)
    return (p @ v).transpose(1, 2).reshape(nseq, S, D), torch.logsumexp(s, dim=-1)


def make_struct(nseq, S, H, seed):
    g = torch.Generator().manual_seed(seed)
    N = S - 1
    sp = torch.randint(1, 22, (nseq, N, N), generator=g, dtype=torch.int32)
    ab = torch.zeros(nseq, S, S)
    far = torch.rand(nseq, N, N, generator=g) < 0.3
    idx = torch.arange(N)
    far[:, idx, idx] = False
    ab[:, 1:, 1:][far] = -math.inf
    kpad = torch.zeros(nseq, S, dtype=torch.uint8)
    for b in range(nseq):
        npad = (b * 3) % max(1, S // 2)
        if npad:
            kpad[b, S - npad:] = 1
            ab[b, :, S - npad:] = -math.inf
            ab[b, S - npad:, : S - npad] = 0
            sp[b, N - npad:, :] = 0
            sp[b, :, N - npad:] = 0
    table = rnd(64, H, seed=seed + 1, scale=0.5)
    virt = rnd(H, seed=seed + 2, scale=0.5)
    return sp, ab, kpad, table, virt


def dense_from_struct(sp, ab, kpad, table, virt, H):
    nseq, S, _ = ab.shape
    bias = (2 * ab).unsqueeze(1).repeat(1, H, 1, 1)
    bias[:, :, 1:, 1:] += table[sp.long()].permute(0, 3, 1, 2)
    bias[:, :, 1:, 0] += virt.view(1, H, 1)
    bias[:, :, 0, :] += virt.view(1, H, 1)
    bias = bias.masked_fill(kpad.bool()[:, None, None, :], -math.inf)
    return bias


CASES = [  # (nseq, S, H, hd, mode)
    (3, 8, 2, 64, "mask"), (2, 14, 12, 64, "none"), (3, 65, 4, 64, "struct"), (2, 104, 3, 64, "mask"),
    (2, 201, 2, 64, "none"), (2, 33, 4, 64, "dense"), (3, 8, 8, 16, "struct"), (2, 129, 2, 64, "struct"),
]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("nseq,S,H,hd,mode", CASES)
@pytest.mark.parametrize("time_major", [False, True])
def test_attention(ops, dtype, nseq, S, H, hd, mode, time_major):
    if dtype == torch.bfloat16 and hd != 64:
        pytest.skip("bf16 kernel: head_dim 64 only")
    if time_major and mode not in ("struct", "dense"):
        pytest.skip("time-major layout is the graph path")
    D = H * hd
    scale = hd ** -0.5
    qkv = rnd(nseq, S, 3 * D, seed=7).to(dtype)
    dout = rnd(nseq, S, D, seed=8).to(dtype)
    kw = {}
    bias = torch.zeros(nseq, H, S, S)
    if mode == "mask":
        km = torch.ones(nseq, S, dtype=torch.uint8)
        for b in range(nseq):
            km[b, max(1, S - 1 - 2 * b):] = 0
        km[0] = 1
        kw["key_mask"] = dev(km)
        bias = bias.masked_fill(~km.bool()[:, None, None, :], -math.inf)
    elif mode == "dense":
        bias = rnd(nseq, H, S, S, seed=9)
        bias[:, :, :, S - 2] = -math.inf
        kw["dense_bias"] = dev(bias)
    elif mode == "struct":
        sp, ab, kpad, table, virt = make_struct(nseq, S, H, seed=11)
        table, virt = table.to(dtype), virt.to(dtype)
        bias = dense_from_struct(sp, ab, kpad, table.float(), virt.float(), H)
        kw.update(attn_bias=dev(ab), spatial_pos=dev(sp), sp_table=dev(table), virt=dev(virt), key_pad=dev(kpad))
    qr = qkv.float().requires_grad_(True)
    br = bias.clone().requires_grad_(True)
    oref, lref = ref_attention(qr, nseq, S, H, scale, br)
    oref.backward(dout.float())

    if time_major:   # rows ordered [S, nseq]
        q2 = dev(qkv.transpose(0, 1).contiguous().view(S * nseq, 3 * D))
        d2 = dev(dout.transpose(0, 1).contiguous().view(S * nseq, D))
        lay = dict(seq_stride=1, pos_stride=nseq)
    else:
        q2 = dev(qkv.view(nseq * S, 3 * D))
        d2 = dev(dout.view(nseq * S, D))
        lay = dict(seq_stride=S, pos_stride=1)
    out, lse = ops.attention_fwd(q2, nseq, S, H, scale=scale, **lay, **kw)
    if dtype == torch.bfloat16:       # a dense bias without structural terms: the only way to the bf16 v1 kernels
        assert L.last_route() == ("v1" if mode == "dense" else "v2"), L.last_route()

    def unlay(t, width):
        t = t.float().cpu()
        return t.view(S, nseq, width).transpose(0, 1) if time_major else t.view(nseq, S, width)

    tol = dict(atol=2e-4, rtol=1e-4) if dtype == torch.float32 else dict(atol=0.03, rtol=2e-2)
    torch.testing.assert_close(unlay(out, D), oref.detach(), **tol)
    torch.testing.assert_close(lse.cpu(), lref.detach(), atol=2e-4 if dtype == torch.float32 else 0.03, rtol=1e-3)

    extra = {}
    if mode == "struct":
        extra = dict(d_sp_table=torch.zeros(64, H, dtype=torch.float32).cuda(),
                     d_virt=torch.zeros(H, dtype=torch.float32).cuda())
    dqkv, dbias = ops.attention_bwd(d2, q2, out, lse, nseq, S, H, scale=scale, **lay, **kw,
                                    want_dense_dbias=(mode == "dense"), **extra)
    gtol = dict(atol=5e-4, rtol=1e-3) if dtype == torch.float32 else dict(atol=0.06, rtol=5e-2)
    torch.testing.assert_close(unlay(dqkv, 3 * D), qr.grad, **gtol)
    if mode == "dense":
        ref_db = torch.nan_to_num(br.grad, nan=0.0)
        torch.testing.assert_close(dbias.cpu(), ref_db, **gtol)
    if mode == "struct":
        db = torch.nan_to_num(br.grad, nan=0.0)      # [nseq,H,S,S]
        ref_tab = torch.zeros(64, H)
        for b in range(nseq):
            for h in range(H):
                ref_tab[:, h].index_add_(0, sp[b].long().flatten(), db[b, h, 1:, 1:].flatten())
        ref_tab[0] = 0                                 # padding_idx row
        ref_virt = db[:, :, 0, :].sum(dim=(0, 2)) + db[:, :, 1:, 0].sum(dim=(0, 2))
        torch.testing.assert_close(extra["d_sp_table"].cpu(), ref_tab, atol=gtol["atol"] * 4, rtol=gtol["rtol"])
        torch.testing.assert_close(extra["d_virt"].cpu(), ref_virt, atol=gtol["atol"] * 8, rtol=gtol["rtol"])
        dense = ops.graph_attn_bias(dev(ab), dev(sp), dev(table), dev(virt)).cpu()
        want = dense_from_struct(sp, ab, torch.zeros_like(kpad), table.float(), virt.float(), H)
        assert torch.equal(torch.isinf(dense), torch.isinf(want))
        torch.testing.assert_close(torch.nan_to_num(dense, neginf=0.0), torch.nan_to_num(want, neginf=0.0),
                                   atol=1e-6, rtol=1e-6)


# ----------------------------------------------------------------------------- row movers
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_row_ops(ops, dtype):
    D = 128
    a, b = rnd(10, D, seed=1).to(dtype), rnd(6, D, seed=2).to(dtype)
    dst = rnd(12, D, seed=3).to(dtype)
    di = torch.tensor([3, 0, 7, 11], dtype=torch.int32)
    ai = torch.tensor([9, 9, 1, 4], dtype=torch.int32)
    bi = torch.tensor([0, 5, 2, 2], dtype=torch.int32)
    ref = dst.float().clone()
    ref[di.long()] = 0.5 * a.float()[ai.long()] + 0.5 * b.float()[bi.long()]
    got = ops.row_axpby(dev(dst.clone()), 4, di=dev(di), a=dev(a), ai=dev(ai), alpha=0.5, b=dev(b), bi=dev(bi), beta=0.5)
    torch.testing.assert_close(got.float().cpu(), ref.to(dtype).float(), atol=1e-6, rtol=1e-6)
    # strided source (token 0 of every 3-token sequence), accumulate into dst rows 2..5
    ref = dst.float().clone()
    ref[2:6] += a.float()[0:10:3][:4]
    got = ops.row_axpby(dev(dst.clone()), 4, d_stride=1, d_off=2, a=dev(a), a_stride=3, a_off=0, accumulate=True)
    torch.testing.assert_close(got.float().cpu(), ref.to(dtype).float(), atol=1e-2 if dtype == torch.bfloat16 else 1e-6,
                               rtol=1e-2)
    # scatter-add with duplicate and skipped rows
    table = torch.zeros(5, D).cuda()
    idx = torch.tensor([1, 4, 1, -1, 0, 1], dtype=torch.int32)
    ops.row_scatter_add(table, dev(idx), dev(b), 6)
    ref = torch.zeros(5, D)
    for r, t in enumerate(idx.tolist()):
        if t >= 0:
            ref[t] += b.float()[r]
    torch.testing.assert_close(table.cpu(), ref, atol=1e-5, rtol=1e-5)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("rows,D", [(1, 128), (37, 768), (4099, 768), (260, 1024)])
def test_bert_embeddings_and_their_layernorm_in_one_pass(ops, dtype, rows, D):
    """mdt_bert_embed_ln_rows = mdt_bert_embed_rows + mdt_layernorm_fwd, bit for bit (output, statistics and the
    summed rows backward reads), and against the fp32 formula on the CPU; without the summed rows (inference) the same output."""
    V, P = 211, 40
    g = torch.Generator().manual_seed(rows + D)
    ids = torch.randint(0, V, (rows,), generator=g, dtype=torch.int32)
    types = torch.randint(0, 2, (rows,), generator=g, dtype=torch.int32)
    pos_ids = torch.randint(0, P, (rows,), generator=g, dtype=torch.int32)
    word, pos, typ = rnd(V, D, seed=1).to(dtype), rnd(P, D, seed=2, scale=0.5).to(dtype), rnd(2, D, seed=3, scale=0.2).to(dtype)
    gamma, beta = (1 + rnd(D, seed=4, scale=0.2)).to(dtype), rnd(D, seed=5, scale=0.1).to(dtype)
    args = (dev(ids), dev(types), dev(pos_ids), dev(word), dev(pos), dev(typ))
    y, mean, rstd, xs = ops.bert_embed_ln_rows(*args, dev(gamma), dev(beta), 1e-12)
    two = torch.empty(rows, D, dtype=dtype).cuda()
    ops.bert_embed_rows(*args, two)
    y2, mean2, rstd2 = ops.layernorm_fwd(two, dev(gamma), dev(beta), 1e-12)
    assert torch.equal(xs, two) and torch.equal(y, y2) and torch.equal(mean, mean2) and torch.equal(rstd, rstd2)
    y3, _, _, none = ops.bert_embed_ln_rows(*args, dev(gamma), dev(beta), 1e-12, keep_sum=False)
    assert none is None and torch.equal(y3, y)
    x = (word.float()[ids.long()] + typ.float()[types.long()] + pos.float()[pos_ids.long()]).to(dtype).float()
    ref = F.layer_norm(x, (D,), gamma.float(), beta.float(), 1e-12)
    tol = 2e-5 if dtype == torch.float32 else 2e-2
    torch.testing.assert_close(y.float().cpu(), ref, atol=tol, rtol=tol)


@pytest.mark.parametrize("I,HW,D,nb", [(3, 224, 768, 0), (5, 64, 256, 4), (1, 32, 128, 2)])
def test_vit_patch_embed_in_one_launch(ops, I, HW, D, nb):
    """Conv2d(3, D, k = s = 16) + bias + [CLS] + position add with the GEMM's A loader gathering from pixel_values
    (csrc/patch_embed.hip) against (a) F.conv2d in fp64 on the bf16-rounded pixels and weights — the one rounding of the result
    to bf16 allows half a bf16 ulp (2^-9 relative) plus the fp32 accumulation order; (b) the three-launch route
    (vit_patchify + gemm + vit_assemble), which rounds twice (the patch value, then the sum): within an ulp of the larger of the two.  M = I * (HW / 16)^2 is not a multiple
    of the 128-row tile in any case; rows in front of the image tokens (bottleneck slots, off = nb) stay untouched."""
    bf = torch.bfloat16
    p, C = 16, 3
    gw = HW // p
    npatch = gw * gw
    img = rnd(I, C, HW, HW, seed=21, scale=2.0)
    w = rnd(D, C, p, p, seed=22, scale=0.05).to(bf)
    b, cls, pos = rnd(D, seed=23, scale=0.3).to(bf), rnd(D, seed=24).to(bf), rnd(npatch + 1, D, seed=25, scale=0.5).to(bf)
    S = nb + npatch + 1
    tok = torch.full((I * S, D), 7.0, dtype=bf).cuda()
    ops.vit_patch_embed(dev(img), p, dev(w).view(D, -1), dev(b), dev(cls), dev(pos), tok, seq_stride=S, off=nb)
    got = tok.float().cpu().view(I, S, D)
    conv = F.conv2d(img.to(bf).double(), w.double(), b.double(), stride=p).flatten(2).transpose(1, 2)      # [I, np, D]
    ref = torch.cat([cls.double().expand(I, 1, D), conv], 1) + pos.double()[None]
    err = (got[:, nb:].double() - ref).abs()
    tol = ref.abs() * 2.0 ** -8 + 2e-4                 # half an ulp of the result + accumulation order + margin
    assert bool((err <= tol).all()), (float(err.max()), float((err / tol).max()))
    if nb:
        assert float((got[:, :nb] - 7.0).abs().max()) == 0.0
    # the three-launch route on the same inputs
    cols = ops.vit_patchify(dev(img), p, bf)
    patches = ops.gemm(cols, dev(w).view(D, -1), bias=dev(b))
    tok3 = torch.full((I * S, D), 7.0, dtype=bf).cuda()
    ops.vit_assemble(patches, dev(cls), dev(pos), tok3, I, npatch, seq_stride=S, off=nb)
    d3 = (tok.float() - tok3.float()).abs().cpu().view(I, S, D)[:, nb:].double()
    mag = torch.cat([cls.double().abs().expand(I, 1, D), conv.abs()], 1) + pos.double().abs()[None]     # the first rounding is of the patch value, not of the sum
    assert bool((d3 <= mag * 2.0 ** -7 + 1e-3).all()), float(d3.max())
    # and it is closer to the exact result than the route that rounds twice (mean error)
    e3 = (tok3.float().cpu().view(I, S, D)[:, nb:].double() - ref).abs().mean()
    assert float(err.mean()) <= float(e3) * 1.02, (float(err.mean()), float(e3))


def test_vit_patch_embed_refuses_what_it_has_no_kernel_for(ops):
    """14 x 14 patches (ViT-L/14) take the three-launch route: the entry point says so with MDT_ERR_UNSUPPORTED, not with garbage."""
    bf = torch.bfloat16
    img = rnd(1, 3, 28, 28, seed=1)
    w = rnd(128, 3 * 14 * 14 + 4, seed=2).to(bf)[:, :588]
    tok = torch.zeros(5, 128, dtype=bf).cuda()
    with pytest.raises(L.MdtUnsupported):
        ops.vit_patch_embed(dev(img), 14, dev(w), dev(rnd(128).to(bf)), dev(rnd(128).to(bf)), dev(rnd(5, 128).to(bf)), tok, seq_stride=5, off=0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_embeddings_and_features(ops, dtype):
    D, L, M, V = 128, 6, 5, 50
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(0, V, (M, L), generator=g, dtype=torch.int32)
    types = torch.randint(0, 2, (M, L), generator=g, dtype=torch.int32)
    word, pos, typ = rnd(V, D, seed=1).to(dtype), rnd(16, D, seed=2).to(dtype), rnd(2, D, seed=3).to(dtype)
    nb = 4
    out = torch.zeros(M * (nb + L), D, dtype=dtype).cuda()
    ops.bert_embed_sum(dev(ids), dev(types), dev(word), dev(pos), dev(typ), out, out_seq_stride=nb + L, out_off=nb)
    ref = word.float()[ids.long()] + pos.float()[:L][None] + typ.float()[types.long()]
    got = out.float().cpu().view(M, nb + L, D)
    torch.testing.assert_close(got[:, nb:], ref.to(dtype).float(), atol=1e-6, rtol=1e-6)
    assert float(got[:, :nb].abs().max()) == 0.0
    # ViT patches
    I, p, HW = 3, 16, 32
    img = rnd(I, 3, HW, HW, seed=5)
    cols = ops.vit_patchify(dev(img), p, dtype)
    ref = F.unfold(img, kernel_size=p, stride=p).transpose(1, 2).reshape(I * 4, 3 * p * p)
    torch.testing.assert_close(cols.float().cpu(), ref.to(dtype).float(), atol=1e-6, rtol=1e-6)
    patches = rnd(I * 4, D, seed=6).to(dtype)
    cls, ppos = rnd(D, seed=7).to(dtype), rnd(5, D, seed=8).to(dtype)
    tok = torch.zeros(I * (nb + 5), D, dtype=dtype).cuda()
    ops.vit_assemble(dev(patches), dev(cls), dev(ppos), tok, I, 4, seq_stride=nb + 5, off=nb)
    ref = torch.cat([cls.float().expand(I, 1, D), patches.float().view(I, 4, D)], 1) + ppos.float()[None]
    torch.testing.assert_close(tok.float().cpu().view(I, nb + 5, D)[:, nb:], ref.to(dtype).float(), atol=1e-6, rtol=1e-6)
    # graph node features
    B, T = 2, 4
    src = rnd(7, D, seed=9).to(dtype)
    node_row = torch.tensor([0, 3, 6, 2, -1, -1], dtype=torch.int32)
    deg = torch.tensor([2, 3, 1, 1, 0, 0], dtype=torch.int32)
    ine, oute, tokn = rnd(8, D, seed=10).to(dtype), rnd(8, D, seed=11).to(dtype), rnd(1, D, seed=12).to(dtype)
    x = ops.graph_node_feature(dev(src), dev(node_row), dev(deg), dev(deg), dev(ine), dev(oute), dev(tokn), B, T)
    ref = torch.zeros(B, T, D)
    ref[:, 0] = tokn.float()
    nr = node_row.view(B, T - 1)
    for b in range(B):
        for n in range(T - 1):
            v = ine.float()[deg.view(B, T - 1)[b, n]] + oute.float()[deg.view(B, T - 1)[b, n]]
            if nr[b, n] >= 0:
                v = v + src.float()[nr[b, n]]
            ref[b, 1 + n] = v
    torch.testing.assert_close(x.float().cpu().view(B, T, D), ref.to(dtype).float(), atol=1e-6, rtol=1e-6)
    y = rnd(33, seed=1).to(dtype)
    torch.testing.assert_close(ops.tanh_fwd(dev(y)).float().cpu(), torch.tanh(y.float()).to(dtype).float(),
                               atol=1e-6 if dtype == torch.float32 else 1e-2, rtol=1e-2)


def test_node_ce_matches_oracle(ops):
    from oracle import mdt_ref_cpu as R
    g = torch.Generator().manual_seed(5)
    M = 40
    logits = (torch.rand(M, 2, generator=g) * 4 - 2)
    y_mask = torch.rand(M, generator=g) < 0.4
    y = (torch.rand(int(y_mask.sum()), generator=g) < 0.4).float()
    hp = R.hparams(pos_weight=1.5, neg_weight=1.0)
    lr = logits.clone().requires_grad_(True)
    loss, counters = R.node_cross_entropy(lr, y, y_mask, hp)
    loss.backward()
    rows = torch.nonzero(y_mask).flatten().int()
    l, c, dl = ops.node_ce(dev(logits), dev(rows), dev(y.int()), 1.0, 1.5)
    assert abs(float(l.cpu()) - float(loss)) <= 2e-2
    assert c.cpu().tolist() == [counters["ncorrect"], counters["num_positive_correct"], counters["total_positive"],
                                counters["num_pred_positive"]]
    torch.testing.assert_close(dl.cpu(), lr.grad, atol=1e-3, rtol=1e-3)


@pytest.mark.parametrize("n,near_tie", [(7, False), (32, False), (33, True), (300, False), (1000, True), (2500, False)])
def test_node_ce_matches_torch_cpu_half(ops, n, near_tie):
    """The reference's loss runs in HALF precision whatever the model dtype (criterions/hatespeech_loss.py:58-64,95).
    The kernel follows PyTorch's CPU Half kernels step by step (where they round: csrc/rowops.hip node_ce_kernel):
    the loss VALUE (Half cascade sum), the counters (ties of the rounded softmax go to class 0) and d logits are
    bit-equal to torch.nn.functional.cross_entropy on CPU half tensors, except where a 1-ulp difference between the
    device's expf / logf and the host's lands on a rounding boundary (allowed: a few elements, one half-ulp each)."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(100 + n)
    M = n + 9
    logits = torch.randn(M, 2, generator=g) * 1.5
    if near_tie:                                             # margins far inside one half ulp
        logits[:, 1] = logits[:, 0] + torch.randn(M, generator=g) * 2e-3
    rows = torch.randperm(M, generator=g)[:n].sort().values
    y = (torch.rand(n, generator=g) < 0.4).long()
    lr = logits.clone().requires_grad_(True)
    lh = lr[rows].type(torch.HalfTensor)
    w = torch.tensor([1.0, 1.5]).type(torch.HalfTensor)
    pred = torch.argmax(F.softmax(lh, dim=-1), dim=-1)
    loss = F.cross_entropy(lh, y, reduction="sum", weight=w)
    loss.backward()
    l, c, dl = ops.node_ce(dev(logits), dev(rows.int()), dev(y.int()), 1.0, 1.5)
    want = [int((pred == y).sum()), int(((pred == y) & (pred == 1)).sum()), int((y == 1).sum()), int((pred == 1).sum())]
    got = c.cpu().tolist()
    assert got[2] == want[2]
    assert max(abs(a - b) for a, b in zip(got, want)) <= (2 if near_tie else 0), (got, want)
    ulp = 2.0 ** (max(-14, int(np.floor(np.log2(max(abs(float(loss)), 1e-6))))) - 10)
    assert abs(float(l.cpu()) - float(loss)) <= ulp, (float(l.cpu()), float(loss))      # within one Half ulp (usually equal)
    d = (dl.cpu() - lr.grad).abs()
    assert float(d.max()) <= 2.0 ** -10                                                   # one half-ulp step of a value < 2
    assert int((d > 0).sum()) <= max(2, n // 50), int((d > 0).sum())


# ----------------------------------------------------------------------------- ragged attention
@pytest.mark.parametrize("dtype,bwd", [(torch.float32, None), (torch.bfloat16, None), (torch.bfloat16, "v1"), (torch.bfloat16, "v2")])
@pytest.mark.parametrize("Smax,H", [(40, 2), (104, 3), (201, 2)])
def test_attention_ragged_sequences_equal_masked_padding(ops, dtype, bwd, Smax, H, monkeypatch):
    """seq_offsets (valid tokens packed back to back) against the same sequences padded to Smax behind a key mask:
    outputs and gradients at the valid rows agree, for every kernel family, with attention dropout on (the counters
    keep the padded geometry, so the two runs draw the same masks)."""
    if bwd == "v2" and Smax > 112:
        pytest.skip("whole-row backward covers S <= 112")
    if bwd:
        monkeypatch.setenv("MDT_ATTN_BWD", bwd)
        L.reload_env()
    hd, p, seed = 64, 0.25, 31
    D = H * hd
    lens = [Smax, 1, 17, Smax - 3, 5, 33 if Smax > 33 else 2]
    nseq = len(lens)
    off = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32)
    rows = int(off[-1])
    qkv_r = rnd(rows, 3 * D, seed=3).to(dtype)
    dout_r = rnd(rows, D, seed=4).to(dtype)
    qkv_p = torch.zeros(nseq, Smax, 3 * D, dtype=dtype)
    dout_p = torch.zeros(nseq, Smax, D, dtype=dtype)
    km = torch.zeros(nseq, Smax, dtype=torch.uint8)
    for s_, n in enumerate(lens):
        qkv_p[s_, :n] = qkv_r[off[s_]:off[s_] + n]
        dout_p[s_, :n] = dout_r[off[s_]:off[s_] + n]
        km[s_, :n] = 1
    out_p, lse_p = ops.attention_fwd(dev(qkv_p.view(-1, 3 * D)), nseq, Smax, H, key_mask=dev(km), drop_p=p, drop_seed=seed)
    dq_p, _ = ops.attention_bwd(dev(dout_p.view(-1, D)), dev(qkv_p.view(-1, 3 * D)), out_p, lse_p, nseq, Smax, H,
                                key_mask=dev(km), drop_p=p, drop_seed=seed)
    out_r, lse_r = ops.attention_fwd(dev(qkv_r), nseq, Smax, H, seq_offsets=dev(off), drop_p=p, drop_seed=seed)
    dq_r, _ = ops.attention_bwd(dev(dout_r), dev(qkv_r), out_r, lse_r, nseq, Smax, H, seq_offsets=dev(off), drop_p=p, drop_seed=seed)
    assert L.last_route() == A.bwd_route(dtype, hd, Smax, "none", p, forced=bwd), L.last_route()
    tol = dict(atol=1e-5, rtol=1e-5) if dtype == torch.float32 else dict(atol=2e-2, rtol=2e-2)
    out_p, dq_p = out_p.view(nseq, Smax, D).float().cpu(), dq_p.view(nseq, Smax, 3 * D).float().cpu()
    for s_, n in enumerate(lens):
        torch.testing.assert_close(out_r[off[s_]:off[s_] + n].float().cpu(), out_p[s_, :n], **tol)
        torch.testing.assert_close(dq_r[off[s_]:off[s_] + n].float().cpu(), dq_p[s_, :n], **tol)
        torch.testing.assert_close(lse_r[s_, :, :n].cpu(), lse_p[s_, :, :n].cpu(), atol=1e-4, rtol=1e-5)


@pytest.mark.parametrize("route", [None, "v1", "v2", "v3"])
@pytest.mark.parametrize("Smax,qlim", [(40, 0), (104, 0), (201, 0), (88, 0), (104, 9), (201, 33)])
def test_attention_backward_never_reads_what_forward_did_not_write(ops, route, Smax, qlim, monkeypatch):
    """Forward leaves the log-sum-exp of positions past a sequence's length (ragged batches: [nseq, H, Smax] is a dense buffer) and
    of query rows past q_limit (rounded up to its 16-row tile) unwritten, and with q_limit the output rows past that too: stale bytes of whatever the allocator handed
    out.  Backward must not let them reach a result — not even multiplied by a zero dO (inf * 0).  The same backward call with
    those positions set to NaN, to +inf, to -1e30 and to 0: bit-identical, finite gradients, on every kernel family (tools/op_trace.py
    found the unwritten positions differing between repetitions of one training step)."""
    bf = torch.bfloat16
    if route == "v2" and Smax > 112:
        pytest.skip("whole-row backward covers S <= 112")
    if route:
        monkeypatch.setenv("MDT_ATTN_BWD", route)
        L.reload_env()
    H, hd, p, seed = 3, 64, 0.2, 5
    D = H * hd
    lens = [Smax, 1, 17, Smax - 3, 5, min(33, Smax - 1), Smax - 16, 16]
    nseq = len(lens)
    off = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32)
    rows = int(off[-1])
    qkv = dev(rnd(rows, 3 * D, seed=3).to(bf))
    dout = rnd(rows, D, seed=4).to(bf)
    valid_q = torch.zeros(nseq, Smax, dtype=torch.bool)
    row_live = torch.ones(rows, dtype=torch.bool)
    for s_, n in enumerate(lens):
        nq = min(n, qlim) if qlim else n
        nw = min(n, (qlim + 15) & ~15) if qlim else n      # forward computes (and writes) whole 16-row query tiles
        valid_q[s_, :nw] = True
        row_live[int(off[s_]) + nw:int(off[s_]) + n] = False
        dout[int(off[s_]) + nq:int(off[s_]) + n] = 0       # what the engine hands over for rows nobody asked for
    dout = dev(dout)
    kw = dict(drop_p=p, drop_seed=seed, seq_offsets=dev(off), q_limit=qlim)
    out, lse = ops.attention_fwd(qkv, nseq, Smax, H, **kw)
    vq = dev(valid_q)[:, None, :].expand(nseq, H, Smax)
    live = dev(row_live)[:, None]
    res = []
    real_empty_like = torch.empty_like
    for poison in (float("nan"), float("inf"), -1e30, 0.0):
        lse_p = torch.where(vq, lse, torch.full_like(lse, poison))
        out_p = torch.where(live, out, torch.full_like(out, poison))
        # the gradient buffer the wrapper allocates starts out as the same poison: whatever backward does not write shows
        monkeypatch.setattr(torch, "empty_like", lambda t, *a, **k: real_empty_like(t, *a, **k).fill_(poison) if t.is_floating_point() else real_empty_like(t, *a, **k))
        dq, _ = ops.attention_bwd(dout, qkv, out_p, lse_p, nseq, Smax, H, **kw)
        monkeypatch.setattr(torch, "empty_like", real_empty_like)
        # v1 / v2 never take q_limit: the family's default kernel runs instead
        assert L.last_route() == A.bwd_route(bf, hd, Smax, "none", p, qlim, forced=route), L.last_route()
        assert bool(torch.isfinite(dq.float()).all()), poison
        res.append(dq)
    for r in res[1:]:
        assert torch.equal(r, res[0])
    # ... and forward leaves nothing unwritten that anybody reads: the same forward into poisoned buffers gives the same gradients
    real_empty = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, **k: real_empty(*a, **k).fill_(float("nan")) if k.get("dtype", torch.float32).is_floating_point else real_empty(*a, **k))
    out_n, lse_n = ops.attention_fwd(qkv, nseq, Smax, H, **kw)
    monkeypatch.setattr(torch, "empty", real_empty)
    dq_n, _ = ops.attention_bwd(dout, qkv, out_n, lse_n, nseq, Smax, H, **kw)
    assert torch.equal(dq_n, res[0])
    assert torch.equal(out_n[dev(row_live)], out[dev(row_live)])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("S,H,qlim", [(104, 3, 5), (201, 2, 1), (40, 2, 17)])
def test_attention_query_limit(ops, dtype, S, H, qlim):
    """q_limit: only the first rows of each sequence are needed as queries (keys / values stay the whole sequence);
    outputs of those rows, and the gradients when dout is zero elsewhere, equal the unrestricted call."""
    nseq, hd, p, seed = 3, 64, 0.2, 77
    D = H * hd
    qkv = dev(rnd(nseq * S, 3 * D, seed=5).to(dtype))
    dout = rnd(nseq, S, D, seed=6).to(dtype)
    dout[:, qlim:] = 0
    dout = dev(dout.view(nseq * S, D))
    kw = dict(drop_p=p, drop_seed=seed)
    o_full, l_full = ops.attention_fwd(qkv, nseq, S, H, **kw)
    g_full, _ = ops.attention_bwd(dout, qkv, o_full, l_full, nseq, S, H, **kw)
    o_lim, l_lim = ops.attention_fwd(qkv, nseq, S, H, q_limit=qlim, **kw)
    g_lim, _ = ops.attention_bwd(dout, qkv, o_lim, l_lim, nseq, S, H, q_limit=qlim, **kw)
    tol = dict(atol=1e-5, rtol=1e-5) if dtype == torch.float32 else dict(atol=1e-2, rtol=1e-2)
    torch.testing.assert_close(o_lim.view(nseq, S, D)[:, :qlim].float(), o_full.view(nseq, S, D)[:, :qlim].float(), **tol)
    torch.testing.assert_close(l_lim[:, :, :qlim], l_full[:, :, :qlim], atol=1e-4, rtol=1e-5)
    torch.testing.assert_close(g_lim.float(), g_full.float(), **tol)


# ----------------------------------------------------------------------------- one-pass backward against the two-pass kernels
ONE_PASS = {201: "v5", 104: "v4", 65: "v4x", 224: "v3", 17: "v4x"}     # the kernel the v3 family picks for rows of S tokens


@pytest.mark.parametrize("S,ragged,qlim,p", [(201, False, 0, 0.1), (104, False, 0, 0.3), (104, True, 0, 0.1), (201, True, 0, 0.0),
                                               (65, False, 33, 0.1), (224, False, 0, 0.1), (17, False, 0, 0.2)])
def test_attention_backward_one_pass_equals_two_pass(ops, S, ragged, qlim, p, monkeypatch):
    """csrc/attention_v2.hip attn_bwd_v4 (dS^T parked in LDS, dQ from a transposed read) against attn_bwd_v3 (S and dP
    computed twice) on the same inputs and dropout masks: the same operands reach the same MFMAs, so the gradients may
    differ only by the summation order of delta = rowsum(dO * O).  ONE_PASS[S]: the kernel the v3 family picks for S (S = 224: the
    one-pass dS image does not fit LDS, v3 both times)."""
    one_pass = ONE_PASS[S]
    from multimodaldiscussiontransformer_amd import _lib as L
    nseq, H, hd = 5, 3, 64
    g = torch.Generator().manual_seed(S + 7)
    kw = dict(drop_p=p, drop_seed=11)
    if ragged:
        lens = torch.randint(1, S + 1, (nseq,), generator=g, dtype=torch.int32)
        lens[0] = S
        off = torch.zeros(nseq + 1, dtype=torch.int32)
        off[1:] = torch.cumsum(lens, 0)
        rows = int(off[-1])
        kw["seq_offsets"] = dev(off)
    else:
        rows = nseq * S
    if qlim:
        kw["q_limit"] = qlim
    qkv = dev((torch.randn(rows, 3 * H * hd, generator=g) * 0.7).to(torch.bfloat16))
    dout = dev(torch.randn(rows, H * hd, generator=g).to(torch.bfloat16))
    out, lse = ops.attention_fwd(qkv, nseq, S, H, **kw)
    grads = []
    try:
        for v in ("v3", one_pass):
            monkeypatch.setenv("MDT_ATTN_BWD", v)
            L.reload_env()
            d, _ = ops.attention_bwd(dout, qkv, out, lse, nseq, S, H, **kw)
            assert L.last_route() == v
            grads.append(d.float().cpu())
    finally:
        monkeypatch.delenv("MDT_ATTN_BWD")
        L.reload_env()
    assert A.bwd_route(torch.bfloat16, hd, S, "none", cap=S) == one_pass      # a length bin of cap S takes the family as it is
    assert torch.isfinite(grads[1]).all()
    scale = grads[0].abs().max().item()
    assert (grads[0] - grads[1]).abs().max().item() <= 8e-3 * max(scale, 1.0)
    # rows of at most 96 tokens: the one-pass kernel sums delta = sum P o dP itself (attn_bwd_v4x) where the two-pass kernels take
    # rowsum(dO o O) from the bf16 output — the two differ by that rounding (dedicated test below)
    assert ((grads[0] - grads[1]).norm() / grads[0].norm()).item() <= (3e-3 if S <= 96 else 1e-3)


# ----------------------------------------------------------------------------- persistent one-pass backward (long rows)
@pytest.mark.parametrize("S,ragged,qlim,p", [(201, False, 0, 0.1), (197, True, 0, 0.3), (130, False, 0, 0.0), (208, True, 16, 0.2),
                                               (150, "mask", 0, 0.2)])
def test_attention_backward_persistent_is_bit_identical(ops, S, ragged, qlim, p, monkeypatch):
    """csrc/attention_v2.hip attn_bwd_v5 (8 waves walking (sequence, head) items, two key tiles per wave through one
    query-pair loop, the next item requested under phase 2) against attn_bwd_v4 (one workgroup per item): same operands,
    same summation orders, same dropout counters — bit-identical gradients.  360 items on at most 256 workgroups, so some
    walk two items; the ragged cases mix rows of 1 ... S tokens (items of one to thirteen key tiles) in one launch."""
    from multimodaldiscussiontransformer_amd import _lib as L
    nseq, H, hd = 30, 12, 64
    g = torch.Generator().manual_seed(S + 3)
    kw = dict(drop_p=p, drop_seed=23)
    if ragged == "mask":          # padded layout: a key mask per sequence (one sequence fully visible, one with a single key)
        ragged = False
        km = (torch.rand(nseq, S, generator=g) < 0.8).to(torch.uint8)
        km[:, 0] = 1
        km[0] = 1
        km[1, 1:] = 0
        kw["key_mask"] = dev(km)
    if ragged:
        lens = torch.randint(1, S + 1, (nseq,), generator=g, dtype=torch.int32)
        lens[0], lens[1], lens[2] = S, 1, 17
        off = torch.zeros(nseq + 1, dtype=torch.int32)
        off[1:] = torch.cumsum(lens, 0)
        rows = int(off[-1])
        kw["seq_offsets"] = dev(off)
    else:
        rows = nseq * S
    if qlim:
        kw["q_limit"] = qlim
    qkv = dev((torch.randn(rows, 3 * H * hd, generator=g) * 0.7).to(torch.bfloat16))
    dout = dev(torch.randn(rows, H * hd, generator=g).to(torch.bfloat16))
    out, lse = ops.attention_fwd(qkv, nseq, S, H, **kw)
    grads = []
    try:
        for v in ("v4", "v5"):
            monkeypatch.setenv("MDT_ATTN_BWD", v)
            L.reload_env()
            d, _ = ops.attention_bwd(dout, qkv, out, lse, nseq, S, H, **kw)
            assert L.last_route() == v
            grads.append(d.float().cpu())
    finally:
        monkeypatch.delenv("MDT_ATTN_BWD")
        L.reload_env()
    assert torch.isfinite(grads[1]).all()
    assert torch.equal(grads[0], grads[1])


# ----------------------------------------------------------------------------- ragged attention in length bins
@pytest.mark.parametrize("p,qlim,S", [(0.0, 0, 104), (0.2, 0, 104), (0.1, 20, 104), (0.2, 0, 200)])
def test_attention_length_bins_equal_single_launch(ops, p, qlim, S):
    """mdt_attn_fwd_args.seq_ids / s_cap: a ragged set processed as one launch per length bin (short comments with the
    small kernels) gives bit-identical out / lse / dQKV — lse rows and dropout counters are those of the sequence's own
    index, whichever launch computes it.  S = 200: the longest bin (13 tiles) goes through the persistent backward, which
    walks the bin's sequence ids itself."""
    from multimodaldiscussiontransformer_amd.data.packer import RaggedText
    nseq, H, hd = 37, 3, 64
    g = torch.Generator().manual_seed(5)
    lens = torch.randint(1, S + 1, (nseq,), generator=g, dtype=torch.int32)
    lens[3], lens[4], lens[5] = S, 64, 65
    off = torch.zeros(nseq + 1, dtype=torch.int32)
    off[1:] = torch.cumsum(lens, 0)
    rows = int(off[-1])
    sl, order = torch.sort(lens.long(), stable=True)
    rt = RaggedText(rows=rows, max_len=int(lens.max()), offsets=dev(off), ids=None, types=None, pos=None, comment=None,
                    order=dev(order.to(torch.int32)), sorted_lens=sl.numpy())
    bins = rt.length_bins(0, caps=(32, 64))
    assert bins is not None and len(bins) == 3 and sum(int(i.numel()) for i, _ in bins) == nseq
    for ids, cap in bins:
        assert int(lens[ids.cpu().long()].max()) <= cap
    qkv = dev((torch.randn(rows, 3 * H * hd, generator=g) * 0.7).to(torch.bfloat16))
    dout = dev(torch.randn(rows, H * hd, generator=g).to(torch.bfloat16))
    kw = dict(drop_p=p, drop_seed=9, seq_offsets=dev(off), q_limit=qlim)
    o1, l1 = ops.attention_fwd(qkv, nseq, S, H, **kw)
    d1, _ = ops.attention_bwd(dout, qkv, o1, l1, nseq, S, H, **kw)
    o2, l2 = ops.attention_fwd(qkv, nseq, S, H, bins=bins, **kw)
    d2, _ = ops.attention_bwd(dout, qkv, o2, l2, nseq, S, H, bins=bins, **kw)
    valid = torch.zeros(nseq, H, S, dtype=torch.bool)
    for s_ in range(nseq):
        n = int(lens[s_]) if not qlim else min(int(lens[s_]), qlim)
        valid[s_, :, :n] = True
    if not qlim:
        assert torch.equal(o1, o2)
    assert torch.equal(l1.cpu()[valid], l2.cpu()[valid])
    # without dropout the single launch takes the whole-row backward (exp instead of exp2 arithmetic): bf16-rounding apart
    torch.testing.assert_close(d2.float(), d1.float(), atol=8e-3 * float(d1.float().abs().max()), rtol=0)
    assert ((d1.float() - d2.float()).norm() / d1.float().norm()).item() <= 3e-3


# ----------------------------------------------------------------------------- error behaviour of the C ABI
def test_abi_rejects_bad_arguments_loudly(ops):
    """Every entry point returns a negative status (raised as MdtError with the library's message) instead of
    launching something undefined: bad epilogue combinations, unsupported shapes, inconsistent ragged arguments."""
    from multimodaldiscussiontransformer_amd._lib import MdtError
    bf = torch.bfloat16
    a, b = dev(rnd(64, 64, seed=1).to(bf)), dev(rnd(64, 64, seed=2).to(bf))
    with pytest.raises(MdtError, match="split_k"):
        ops.gemm(a, b, split_k=4)                                   # split-K without the atomic epilogue
    with pytest.raises(MdtError, match="MULAUX|DGELU"):
        ops.gemm(a, b, epilogue=ops.EPI_MULAUX)                     # multiply-by-aux without aux
    with pytest.raises(MdtError, match="AUX_GRAD"):
        ops.gemm(a, b, aux=torch.empty_like(a), epilogue=ops.EPI_AUX_GRAD)   # derivative of nothing
    with pytest.raises(MdtError, match="dropout"):
        ops.gemm(a, b, epilogue=ops.EPI_DROPOUT, drop_p=1.0)
    H, hd = 2, 64
    with pytest.raises(MdtError, match="272|exceeds|limit"):
        S = 300     # longer than the single-pass kernels hold: plain sequences take the key-chunked path, RAGGED ones are refused
        ops.attention_fwd(dev(rnd(S, 3 * H * hd, seed=3).to(bf)), 1, S, H, seq_offsets=dev(torch.tensor([0, S], dtype=torch.int32)))
    S = 40
    qkv = dev(rnd(2 * S, 3 * H * hd, seed=4).to(bf))
    off = dev(torch.tensor([0, S, 2 * S], dtype=torch.int32))
    km = dev(torch.ones(2, S, dtype=torch.uint8))
    with pytest.raises(MdtError, match="ragged"):
        ops.attention_fwd(qkv, 2, S, H, seq_offsets=off, key_mask=km)        # ragged sequences take no masks
    with pytest.raises(MdtError, match="head_dim"):
        ops.attention_fwd(dev(rnd(S, 3 * 2 * 32, seed=5).to(bf)), 1, S, 2)  # bf16 path: head_dim 64 only
    # the library stays usable after errors
    out = ops.gemm(a, b)
    torch.testing.assert_close(out.float(), a.float() @ b.float().t(), atol=0.1, rtol=2e-2)


# ----------------------------------------------------------------------------- long sequences (trees of > 271 comments)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("S,struct,p", [(300, True, 0.0), (273, True, 0.25), (700, False, 0.2)])
def test_attention_beyond_272_tokens_key_chunked_path(ops, dtype, S, struct, p):
    """csrc/attention_long.hip: graph attention over more comments than the single-pass kernels hold.  Against torch fp32
    on the same inputs and the same dropout masks: output, log-sum-exp, dQ / dK / dV and the structural-bias gradients."""
    import math
    nseq, H, hd, seed = 2, 3, 64, 77
    D = H * hd
    g = torch.Generator().manual_seed(S)
    qkv = (torch.randn(nseq * S, 3 * D, generator=g) * 0.5).to(dtype)
    dout = torch.randn(nseq * S, D, generator=g).to(dtype)
    kpad = torch.zeros(nseq, S, dtype=torch.uint8)
    kpad[1, S - 40:] = 1
    kw = {}
    bias_ref = torch.zeros(nseq, H, S, S)
    table = virt = None
    if struct:
        ab = torch.zeros(nseq, S, S)
        far = torch.rand(nseq, S, S, generator=g) < 0.3
        far[:, 0, :] = False
        far[:, :, 0] = False
        far = far | far.transpose(1, 2)
        idx = torch.arange(S)
        far[:, idx, idx] = False
        ab[far] = float("-inf")
        sp = torch.randint(1, 22, (nseq, S - 1, S - 1), generator=g, dtype=torch.int32)
        table = (torch.randn(32, H, generator=g) * 0.3).to(dtype)
        virt = (torch.randn(H, generator=g) * 0.3).to(dtype)
        kw = dict(attn_bias=dev(ab), spatial_pos=dev(sp), sp_table=dev(table), virt=dev(virt))
        tb = table.float().requires_grad_(True)
        vt = virt.float().requires_grad_(True)
        b = 2 * ab[:, None].expand(nseq, H, S, S).clone()
        b[:, :, 1:, 1:] = b[:, :, 1:, 1:] + tb[sp.long()].permute(0, 3, 1, 2)
        b[:, :, 1:, 0] = b[:, :, 1:, 0] + vt.view(1, H, 1)
        b[:, :, 0, :] = b[:, :, 0, :] + vt.view(1, H, 1)
        bias_ref = b
    S2 = S + (S & 1)
    mk = torch.ones(nseq, H, S, S)
    if p > 0:
        mk = ops.dropout_mask(nseq * H * S * S2, p, seed).view(nseq, H, S, S2)[..., :S].float().cpu() / (1 - p)
    qr = qkv.float().view(nseq, S, 3 * D).requires_grad_(True)
    q, k, v = qr.split(D, dim=-1)
    hv = lambda t: t.reshape(nseq, S, H, hd).transpose(1, 2)
    sc = hv(q) @ hv(k).transpose(-1, -2) * hd ** -0.5 + bias_ref
    sc = sc.masked_fill(kpad.bool()[:, None, None, :], -math.inf)
    oref = ((torch.softmax(sc, -1) * mk) @ hv(v)).transpose(1, 2).reshape(nseq * S, D)
    lse_ref = torch.logsumexp(sc, -1)
    oref.backward(dout.float())
    out, lse = ops.attention_fwd(dev(qkv), nseq, S, H, key_pad=dev(kpad), drop_p=p, drop_seed=seed, **kw)
    tol = dict(atol=2e-4, rtol=2e-4) if dtype == torch.float32 else dict(atol=4e-2, rtol=4e-2)
    torch.testing.assert_close(out.float().cpu(), oref.detach(), **tol)
    torch.testing.assert_close(lse.cpu(), lse_ref.detach(), atol=2e-3 if dtype == torch.float32 else 3e-2, rtol=1e-3)
    extra = {}
    if struct:
        extra = dict(d_sp_table=torch.zeros(32, H, device="cuda"), d_virt=torch.zeros(H, device="cuda"))
    dqkv, _ = ops.attention_bwd(dev(dout), dev(qkv), out, lse, nseq, S, H, key_pad=dev(kpad), drop_p=p, drop_seed=seed, **kw, **extra)
    gt = dict(atol=1e-3, rtol=1e-3) if dtype == torch.float32 else dict(atol=0.12, rtol=6e-2)
    torch.testing.assert_close(dqkv.float().cpu().view(nseq, S, 3 * D), qr.grad, **gt)
    if struct:
        st = dict(atol=2e-3, rtol=2e-3) if dtype == torch.float32 else dict(atol=0.3, rtol=0.1)
        want = tb.grad.clone()
        want[0] = 0                                   # padding_idx row never receives a gradient
        torch.testing.assert_close(extra["d_sp_table"].cpu(), want, **st)
        torch.testing.assert_close(extra["d_virt"].cpu(), vt.grad, **st)


# ----------------------------------------------------------------------------- delta = sum P o dP formed in the one-pass backward (short rows)
@pytest.mark.parametrize("S,ragged,p", [(52, False, 0.0), (80, True, 0.0), (96, False, 0.3), (33, True, 0.1)])
def test_attention_backward_v4x_sums_delta_itself_on_short_rows(ops, S, ragged, p, monkeypatch):
    """VERDICT r3 item 6.  Where the value rows of a sequence are nearly equal (the deep pre-fusion blocks of the C4F fixture) the
    query / key gradients are what is left after dP - delta almost cancels, and
    delta = rowsum(dO o O) taken from the forward's bf16-rounded O is off by dO . (O_bf16 - O): the same offset for every key of a
    row, a large fraction of that remnant.  attn_bwd_v4x (rows <= 96 tokens) sums delta = sum_j P_ij dP_ij itself in fp32: dQ / dK
    must sit within 2 % (relative L2) of an fp64 computation on the same bf16 inputs and masks, and the old form
    (attn_bwd_v4: delta from the bf16 output) must be visibly worse on the same launch — otherwise this test would not be testing anything."""
    from multimodaldiscussiontransformer_amd import _lib as L
    nseq, H, hd = 6, 2, 64
    D = H * hd
    g = torch.Generator().manual_seed(100 + S)
    if ragged:
        lens = torch.randint(max(2, S // 2), S + 1, (nseq,), generator=g, dtype=torch.int32)
        lens[0] = S
    else:
        lens = torch.full((nseq,), S, dtype=torch.int32)
    off = torch.zeros(nseq + 1, dtype=torch.int32)
    off[1:] = torch.cumsum(lens, 0)
    rows = int(off[-1])
    qkv = torch.randn(rows, 3 * D, generator=g)
    qkv[:, :2 * D] *= 0.5
    # value rows that differ by 3 % around a common vector (representation collapse of the deep blocks): dP_ij = dO_i . V_j is then
    # nearly the same for every key j and dP - delta is what is left of it
    qkv[:, 2 * D:] = torch.randn(1, D, generator=g) + 0.03 * qkv[:, 2 * D:]
    qkv = qkv.to(torch.bfloat16)
    dout = torch.randn(rows, D, generator=g).to(torch.bfloat16)
    kw = dict(drop_p=p, drop_seed=77)
    if ragged:
        kw["seq_offsets"] = dev(off)
    out, lse = ops.attention_fwd(dev(qkv), nseq, S, H, **kw)
    # fp64 reference on the same bf16 inputs and the kernels' own dropout mask
    ref = torch.zeros(rows, 3 * D, dtype=torch.float64)
    S2 = S + (S & 1)
    keep = None
    if p > 0:
        keep = ops.dropout_mask(nseq * H * S * S2, p, 77).view(nseq, H, S, S2)[..., :S].cpu().double() / (1.0 - p)
    for s_ in range(nseq):
        r0, n = int(off[s_]), int(lens[s_])
        x = qkv[r0:r0 + n].double().requires_grad_(True)
        q, k, v = x.split(D, dim=-1)
        hv = lambda t: t.view(n, H, hd).transpose(0, 1)
        pr = torch.softmax(hv(q) @ hv(k).transpose(-1, -2) * hd ** -0.5, -1)
        if keep is not None:
            pr = pr * keep[s_, :, :n, :n]
        o = (pr @ hv(v)).transpose(0, 1).reshape(n, D)
        o.backward(dout[r0:r0 + n].double())
        ref[r0:r0 + n] = x.grad
    res = {}
    try:
        for exact, kernel in (("1", "v4x"), ("0", "v4")):   # the one-pass kernels of the length-binned production launches
            monkeypatch.setenv("MDT_ATTN_BWD", kernel)
            L.reload_env()
            d, _ = ops.attention_bwd(dev(dout), dev(qkv), out, lse, nseq, S, H, **kw)
            assert L.last_route() == kernel
            d = d.double().cpu()
            res[exact] = [float((d[:, i * D:(i + 1) * D] - ref[:, i * D:(i + 1) * D]).norm() / ref[:, i * D:(i + 1) * D].norm()) for i in range(3)]
    finally:
        monkeypatch.delenv("MDT_ATTN_BWD")
        L.reload_env()
    print(f"[S {S} ragged {ragged} p {p}] rel-L2 of dQ / dK / dV: delta summed in the kernel {res['1']}, from the bf16 output {res['0']}")
    assert res["1"][0] < 2e-2 and res["1"][1] < 2e-2 and res["1"][2] < 1e-2, res
    if p == 0:     # (dropout decorrelates dP along a row: the remnant is no longer small there, either form is at the bf16 floor)
        assert res["0"][0] > 10 * res["1"][0] and res["0"][1] > 10 * res["1"][1], res
    else:
        assert res["0"][0] >= res["1"][0] and res["0"][1] >= res["1"][1], res
