"""bf16 attention over 16-wide heads (the graph heads of Tiny mDT: D 128, 8 heads): every kernel a head_dim 16 launch can
reach — the v2 forward, the v1 forward (dense bias), the v1 / v2 / v3 backward, the key-chunked long path — against torch
fp32 on the same bf16-rounded inputs, with the gates the head_dim 64 tests of test_kernels_gpu.py / test_dropout_gpu.py
use; and against the head_dim 64 kernels themselves on zero-padded heads.

A 16-wide head is half of the K = 32 contraction step of v_mfma_f32_16x16x32_bf16: the upper half is fed zeros, and the 16
columns behind a head belong to the NEXT head (or the k block, or the next row).  Every case therefore has H >= 3 heads
with independent random data per head: a fragment that strayed into its neighbour would show in out, lse and gradients.

The strict gate for attention is tests/test_attention_routes_gpu.py: every kernel and route against the fp64 reference of
tests/attention_reference.py with a derived bound per element; the assert_close gates here are wide enough for a skipped key.
"""
import math

import numpy as np
import pytest
import torch

import tests.attention_reference as A
from multimodaldiscussiontransformer_amd import _lib as L
from tests.test_dropout_gpu import attn_mask
from tests.test_kernels_gpu import dense_from_struct, dev, make_struct, ref_attention, rnd

pytestmark = pytest.mark.gpu

HD = 16
BF = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    from multimodaldiscussiontransformer_amd import ops as o
    assert torch.cuda.is_available(), "GPU tests need a device"
    return o


@pytest.fixture
def force_bwd(monkeypatch):
    def set_(route):
        if route:
            monkeypatch.setenv("MDT_ATTN_BWD", route)
        else:
            monkeypatch.delenv("MDT_ATTN_BWD", raising=False)
        L.reload_env()
    yield set_
    monkeypatch.delenv("MDT_ATTN_BWD", raising=False)
    L.reload_env()


# ----------------------------------------------------------------------------- forward + backward against torch fp32
CASES = [  # (nseq, S, H, mode, time_major)
    (3, 8, 8, "struct", False), (3, 8, 8, "struct", True),                  # v1 backward (struct, S <= 80)
    (2, 17, 8, "mask", False), (2, 17, 3, "dense", False), (2, 17, 3, "dense", True),
    (2, 33, 4, "none", False), (2, 33, 3, "dense", False),
    (3, 65, 4, "struct", False), (3, 65, 4, "struct", True), (2, 65, 3, "mask", False),
    (2, 104, 3, "mask", False), (2, 104, 3, "struct", False), (2, 104, 3, "struct", True), (2, 104, 3, "none", False),   # v2 backward
    (2, 129, 3, "struct", False), (2, 129, 3, "struct", True), (2, 129, 3, "none", False),                               # v3 backward
    (2, 201, 3, "none", False), (2, 201, 3, "dense", True), (2, 201, 4, "struct", False),
    (2, 261, 3, "mask", False), (2, 261, 3, "struct", False), (1, 261, 3, "dense", False),
]


@pytest.mark.parametrize("nseq,S,H,mode,time_major", CASES)
def test_attention_head_dim_16_bf16(ops, nseq, S, H, mode, time_major):
    """tests/test_kernels_gpu.py::test_attention at head_dim 16 in bf16, with its gates: out 0.03 / 2e-2, lse 0.03,
    dqkv / dense dbias 0.06 / 5e-2, d_sp_table 4 x and d_virt 8 x that atol."""
    D = H * HD
    scale = HD ** -0.5
    qkv = rnd(nseq, S, 3 * D, seed=7).to(BF)
    dout = rnd(nseq, S, D, seed=8).to(BF)
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
        table, virt = table.to(BF), virt.to(BF)
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
    assert L.last_route() == A.fwd_route(BF, HD, S, mode), L.last_route()

    def unlay(t, width):
        t = t.float().cpu()
        return t.view(S, nseq, width).transpose(0, 1) if time_major else t.view(nseq, S, width)

    o_err = float((unlay(out, D) - oref.detach()).abs().max())
    l_err = float(torch.nan_to_num(lse.cpu() - lref.detach(), nan=0.0, posinf=0.0, neginf=0.0).abs().max())
    print(f"[hd16 {mode} S={S} tm={time_major}] out |err| {o_err:.3e}, lse |err| {l_err:.3e}")
    torch.testing.assert_close(unlay(out, D), oref.detach(), atol=0.03, rtol=2e-2)
    torch.testing.assert_close(lse.cpu(), lref.detach(), atol=0.03, rtol=1e-3)

    extra = {}
    if mode == "struct":
        extra = dict(d_sp_table=torch.zeros(64, H, dtype=torch.float32).cuda(),
                     d_virt=torch.zeros(H, dtype=torch.float32).cuda())
    dqkv, dbias = ops.attention_bwd(d2, q2, out, lse, nseq, S, H, scale=scale, **lay, **kw,
                                    want_dense_dbias=(mode == "dense"), **extra)
    assert L.last_route() == A.bwd_route(BF, HD, S, mode), L.last_route()
    gtol = dict(atol=0.06, rtol=5e-2)
    print(f"[hd16 {mode} S={S}] dqkv |err| {float((unlay(dqkv, 3 * D) - qr.grad).abs().max()):.3e} on {L.last_route()}")
    torch.testing.assert_close(unlay(dqkv, 3 * D), qr.grad, **gtol)
    if mode == "dense":
        torch.testing.assert_close(dbias.cpu(), torch.nan_to_num(br.grad, nan=0.0), **gtol)
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


def test_cases_reach_every_backward_kernel():
    routes = {A.bwd_route(BF, HD, S, mode) for _, S, _, mode, _ in CASES}
    assert routes == {"v1", "v2", "v3"}
    assert {S for _, S, _, _, _ in CASES} == {8, 17, 33, 65, 104, 129, 201, 261}


# ----------------------------------------------------------------------------- dropout
@pytest.mark.parametrize("bwd", [None, "v1", "v3", "v4x", "v5"])
@pytest.mark.parametrize("nseq,S,H", [(3, 20, 3), (2, 104, 3), (2, 201, 4)])
def test_attention_dropout_head_dim_16(ops, bwd, nseq, S, H, force_bwd):
    """tests/test_dropout_gpu.py::test_attention_dropout at head_dim 16 (p = 0.3, the kernels' own masks through
    ops.dropout_mask, gates out 0.04 / 3e-2 and gradients 0.08 / 6e-2).  With dropout the default backward is v3; v1 and v3
    can be forced; the one-pass kernels are for 64-wide heads, so MDT_ATTN_BWD=v4x|v5 runs the default kernel, same bits."""
    p, seed = 0.3, 4242
    D = H * HD
    qkv = rnd(nseq, S, 3 * D, seed=7).to(BF)
    dout = rnd(nseq, S, D, seed=8).to(BF)
    km = torch.ones(nseq, S, dtype=torch.uint8)
    km[1, S - 3:] = 0
    m = attn_mask(ops, nseq, H, S, p, seed)
    qr = qkv.float().requires_grad_(True)
    q, k, v = qr.split(D, dim=-1)
    hv = lambda t: t.view(nseq, S, H, HD).transpose(1, 2)
    s = hv(q) @ hv(k).transpose(-1, -2) * HD ** -0.5
    s = s.masked_fill(~km.bool()[:, None, None, :], -math.inf)
    pr = torch.softmax(s, -1) * m
    oref = (pr @ hv(v)).transpose(1, 2).reshape(nseq, S, D)
    oref.backward(dout.float())
    q2, d2 = qkv.view(nseq * S, 3 * D).cuda(), dout.view(nseq * S, D).cuda()
    kw = dict(key_mask=km.cuda(), drop_p=p, drop_seed=seed)
    out, lse = ops.attention_fwd(q2, nseq, S, H, **kw)
    assert L.last_route() == "v2"
    torch.testing.assert_close(out.float().cpu().view(nseq, S, D), oref.detach(), atol=0.04, rtol=3e-2)
    force_bwd(None)
    d_default, _ = ops.attention_bwd(d2, q2, out, lse, nseq, S, H, **kw)
    assert L.last_route() == "v3", L.last_route()
    force_bwd(bwd)
    dqkv, _ = ops.attention_bwd(d2, q2, out, lse, nseq, S, H, **kw)
    assert L.last_route() == (bwd if bwd in ("v1", "v3") else "v3"), L.last_route()
    print(f"[hd16 dropout S={S} {bwd}] dqkv |err| {float((dqkv.float().cpu().view(nseq, S, 3 * D) - qr.grad).abs().max()):.3e}")
    torch.testing.assert_close(dqkv.float().cpu().view(nseq, S, 3 * D), qr.grad, atol=0.08, rtol=6e-2)
    if bwd in (None, "v3", "v4x", "v5"):
        assert torch.equal(dqkv, d_default)


# ----------------------------------------------------------------------------- ragged sequences, length bins, q_limit
@pytest.mark.parametrize("Smax,H,bwd", [(40, 3, None), (40, 3, "v1"), (40, 3, "v2"), (104, 3, None), (104, 3, "v1"), (104, 3, "v2"),
                                        (201, 4, None), (201, 4, "v1")])        # the whole-row v2 backward covers S <= 112
def test_ragged_sequences_equal_masked_padding_head_dim_16(ops, bwd, Smax, H, force_bwd):
    """tests/test_kernels_gpu.py::test_attention_ragged_sequences_equal_masked_padding at head_dim 16 (gates 2e-2 / 2e-2,
    lse 1e-4), lengths from 1 to Smax; with ``bins`` the call runs as ONE launch over seq_offsets (length bins are for
    64-wide heads) and gives the same bits."""
    force_bwd(bwd)
    p, seed = 0.25, 31
    D = H * HD
    lens = [Smax, 1, 17, Smax - 3, 5, 33 if Smax > 33 else 2]
    nseq = len(lens)
    off = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32)
    rows = int(off[-1])
    qkv_r = rnd(rows, 3 * D, seed=3).to(BF)
    dout_r = rnd(rows, D, seed=4).to(BF)
    qkv_p = torch.zeros(nseq, Smax, 3 * D, dtype=BF)
    dout_p = torch.zeros(nseq, Smax, D, dtype=BF)
    km = torch.zeros(nseq, Smax, dtype=torch.uint8)
    for s_, n in enumerate(lens):
        qkv_p[s_, :n] = qkv_r[off[s_]:off[s_] + n]
        dout_p[s_, :n] = dout_r[off[s_]:off[s_] + n]
        km[s_, :n] = 1
    kwp = dict(key_mask=dev(km), drop_p=p, drop_seed=seed)
    out_p, lse_p = ops.attention_fwd(dev(qkv_p.view(-1, 3 * D)), nseq, Smax, H, **kwp)
    dq_p, _ = ops.attention_bwd(dev(dout_p.view(-1, D)), dev(qkv_p.view(-1, 3 * D)), out_p, lse_p, nseq, Smax, H, **kwp)
    kwr = dict(seq_offsets=dev(off), drop_p=p, drop_seed=seed)
    out_r, lse_r = ops.attention_fwd(dev(qkv_r), nseq, Smax, H, **kwr)
    assert L.last_route() == "v2"
    dq_r, _ = ops.attention_bwd(dev(dout_r), dev(qkv_r), out_r, lse_r, nseq, Smax, H, **kwr)
    assert L.last_route() == (bwd or "v3"), L.last_route()      # dropout: never the default v2
    tol = dict(atol=2e-2, rtol=2e-2)
    out_p, dq_p = out_p.view(nseq, Smax, D).float().cpu(), dq_p.view(nseq, Smax, 3 * D).float().cpu()
    for s_, n in enumerate(lens):
        torch.testing.assert_close(out_r[off[s_]:off[s_] + n].float().cpu(), out_p[s_, :n], **tol)
        torch.testing.assert_close(dq_r[off[s_]:off[s_] + n].float().cpu(), dq_p[s_, :n], **tol)
        torch.testing.assert_close(lse_r[s_, :, :n].cpu(), lse_p[s_, :, :n].cpu(), atol=1e-4, rtol=1e-5)
    # the same call with length bins
    short = [i for i, n in enumerate(lens) if n <= 48]
    long_ = [i for i, n in enumerate(lens) if n > 48]
    bins = [(dev(torch.tensor(short, dtype=torch.int32)), 48)] + ([(dev(torch.tensor(long_, dtype=torch.int32)), Smax)] if long_ else [])
    out_b, lse_b = ops.attention_fwd(dev(qkv_r), nseq, Smax, H, bins=bins, **kwr)
    dq_b, _ = ops.attention_bwd(dev(dout_r), dev(qkv_r), out_b, lse_b, nseq, Smax, H, bins=bins, **kwr)
    assert torch.equal(out_b, out_r) and torch.equal(dq_b, dq_r)
    for s_, n in enumerate(lens):
        assert torch.equal(lse_b[s_, :, :n], lse_r[s_, :, :n])


@pytest.mark.parametrize("S,H,qlim", [(104, 3, 9), (201, 4, 33)])
def test_query_limit_head_dim_16(ops, S, H, qlim):
    """q_limit (tests/test_kernels_gpu.py::test_attention_query_limit, bf16 gates 1e-2 / 1e-2): outputs of the requested rows and
    the gradients (dout zero elsewhere) equal the unrestricted call; dQ of every other row is zero."""
    nseq, p, seed = 3, 0.2, 77
    D = H * HD
    qkv = dev(rnd(nseq * S, 3 * D, seed=5).to(BF))
    dout = rnd(nseq, S, D, seed=6).to(BF)
    dout[:, qlim:] = 0
    dout = dev(dout.view(nseq * S, D))
    kw = dict(drop_p=p, drop_seed=seed)
    o_full, l_full = ops.attention_fwd(qkv, nseq, S, H, **kw)
    g_full, _ = ops.attention_bwd(dout, qkv, o_full, l_full, nseq, S, H, **kw)
    o_lim, l_lim = ops.attention_fwd(qkv, nseq, S, H, q_limit=qlim, **kw)
    assert L.last_route() == "v2"
    g_lim, _ = ops.attention_bwd(dout, qkv, o_lim, l_lim, nseq, S, H, q_limit=qlim, **kw)
    assert L.last_route() == "v3", L.last_route()
    tol = dict(atol=1e-2, rtol=1e-2)
    torch.testing.assert_close(o_lim.view(nseq, S, D)[:, :qlim].float(), o_full.view(nseq, S, D)[:, :qlim].float(), **tol)
    torch.testing.assert_close(l_lim[:, :, :qlim], l_full[:, :, :qlim], atol=1e-4, rtol=1e-5)
    torch.testing.assert_close(g_lim.float(), g_full.float(), **tol)
    assert float(g_lim.view(nseq, S, 3 * D)[:, qlim:, :D].float().abs().max()) == 0.0


@pytest.mark.parametrize("Smax,qlim", [(40, 0), (104, 9), (201, 33)])
def test_backward_v3_never_reads_what_forward_did_not_write_head_dim_16(ops, Smax, qlim, force_bwd, monkeypatch):
    """The poisoned-buffer construction of test_attention_backward_never_reads_what_forward_did_not_write at head_dim 16 on v3:
    lse positions past a sequence's length and lse / out rows past q_limit's tile set to NaN, +inf, -1e30 and 0, and the
    gradient buffer pre-filled with the same poison — bit-identical, finite gradients."""
    force_bwd("v3")
    H, p, seed = 3, 0.2, 5
    D = H * HD
    lens = [Smax, 1, 17, Smax - 3, 5, min(33, Smax - 1), Smax - 16, 16]
    nseq = len(lens)
    off = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32)
    rows = int(off[-1])
    qkv = dev(rnd(rows, 3 * D, seed=3).to(BF))
    dout = rnd(rows, D, seed=4).to(BF)
    valid_q = torch.zeros(nseq, Smax, dtype=torch.bool)
    row_live = torch.ones(rows, dtype=torch.bool)
    for s_, n in enumerate(lens):
        nq = min(n, qlim) if qlim else n
        nw = min(n, (qlim + 15) & ~15) if qlim else n      # forward computes (and writes) whole 16-row query tiles
        valid_q[s_, :nw] = True
        row_live[int(off[s_]) + nw:int(off[s_]) + n] = False
        dout[int(off[s_]) + nq:int(off[s_]) + n] = 0
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
        monkeypatch.setattr(torch, "empty_like", lambda t, *a, **k: real_empty_like(t, *a, **k).fill_(poison) if t.is_floating_point() else real_empty_like(t, *a, **k))
        dq, _ = ops.attention_bwd(dout, qkv, out_p, lse_p, nseq, Smax, H, **kw)
        monkeypatch.setattr(torch, "empty_like", real_empty_like)
        assert L.last_route() == "v3", L.last_route()
        assert bool(torch.isfinite(dq.float()).all()), poison
        res.append(dq)
    for r in res[1:]:
        assert torch.equal(r, res[0])


# ----------------------------------------------------------------------------- 16-wide heads against the 64-wide kernels
@pytest.mark.parametrize("S,mode,p,bwd", [(40, "mask", 0.0, "v1"), (65, "struct", 0.0, None), (104, "none", 0.0, "v2"),
                                          (129, "struct", 0.0, None), (201, "none", 0.1, "v3"), (104, "mask", 0.3, "v3")])
def test_head_dim_16_equals_zero_padded_head_dim_64(ops, S, mode, p, bwd, force_bwd):
    """A head of 16 is a head of 64 whose other 48 q / k / v columns are zero (scale = 16^-0.5 passed explicitly).  Out columns
    0..15 of every head, lse and the gradients of the live columns of the head_dim 16 launch against the head_dim 64 launch
    on the same route: no torch in between.  Both evaluate the same fp32 expressions (the padded columns add exact
    zeros), so they differ by the rounding of the outputs to bf16, 2^-8 relative, plus the reordering of fp32 sums of
    terms of magnitude <= a few units (atol 1e-5)."""
    nseq, H = 2, 3
    D16, D64 = H * 16, H * 64
    force_bwd(bwd)
    qkv16 = rnd(nseq * S, 3 * D16, seed=21).to(BF)
    dout16 = rnd(nseq * S, D16, seed=22).to(BF)
    qkv64 = torch.zeros(nseq * S, 3, H, 64, dtype=BF)
    qkv64[..., :16] = qkv16.view(nseq * S, 3, H, 16)
    dout64 = torch.zeros(nseq * S, H, 64, dtype=BF)
    dout64[..., :16] = dout16.view(nseq * S, H, 16)
    kw = dict(scale=16 ** -0.5, drop_p=p, drop_seed=99)
    extra16, extra64 = {}, {}
    if mode == "mask":
        km = torch.ones(nseq, S, dtype=torch.uint8)
        km[1, S - 5:] = 0
        kw["key_mask"] = dev(km)
    elif mode == "struct":
        sp, ab, kpad, table, virt = make_struct(nseq, S, H, seed=11)
        kw.update(attn_bias=dev(ab), spatial_pos=dev(sp), sp_table=dev(table.to(BF)), virt=dev(virt.to(BF)), key_pad=dev(kpad))
        extra16 = dict(d_sp_table=torch.zeros(64, H, device="cuda"), d_virt=torch.zeros(H, device="cuda"))
        extra64 = dict(d_sp_table=torch.zeros(64, H, device="cuda"), d_virt=torch.zeros(H, device="cuda"))
    q16, d16 = dev(qkv16), dev(dout16)
    q64, d64 = dev(qkv64.view(nseq * S, 3 * D64)), dev(dout64.view(nseq * S, D64))
    o16, l16 = ops.attention_fwd(q16, nseq, S, H, **kw)
    r16 = L.last_route()
    o64, l64 = ops.attention_fwd(q64, nseq, S, H, **kw)
    assert r16 == L.last_route() == "v2"
    g16, _ = ops.attention_bwd(d16, q16, o16, l16, nseq, S, H, **kw, **extra16)
    r16 = L.last_route()
    g64, _ = ops.attention_bwd(d64, q64, o64, l64, nseq, S, H, **kw, **extra64)
    assert r16 == L.last_route() == (bwd or A.bwd_route(BF, HD, S, mode, p)), (r16, L.last_route())
    tol = dict(rtol=2.0 ** -8, atol=1e-5)
    torch.testing.assert_close(o16.float().view(-1, H, 16), o64.float().view(-1, H, 64)[..., :16], **tol)
    fin = torch.isfinite(l64)
    assert torch.equal(fin, torch.isfinite(l16))
    torch.testing.assert_close(l16[fin], l64[fin], **tol)
    torch.testing.assert_close(g16.float().view(-1, 3, H, 16), g64.float().view(-1, 3, H, 64)[..., :16], **tol)
    assert float(o64.float().view(-1, H, 64)[..., 16:].abs().max()) == 0.0
    if mode == "struct":      # fp32 atomics: the order of the partial sums is not fixed
        torch.testing.assert_close(extra16["d_sp_table"], extra64["d_sp_table"], rtol=2.0 ** -8, atol=1e-3)
        torch.testing.assert_close(extra16["d_virt"], extra64["d_virt"], rtol=2.0 ** -8, atol=1e-3)


# ----------------------------------------------------------------------------- long path
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_beyond_272_tokens_key_chunked_path_head_dim_16(ops, dtype):
    """tests/test_kernels_gpu.py::test_attention_beyond_272_tokens_key_chunked_path (S = 300, structural bias) at head_dim 16,
    with its gates."""
    S, p, nseq, H, seed = 300, 0.0, 2, 3, 77
    D = H * HD
    g = torch.Generator().manual_seed(S)
    qkv = (torch.randn(nseq * S, 3 * D, generator=g) * 0.5).to(dtype)
    dout = torch.randn(nseq * S, D, generator=g).to(dtype)
    kpad = torch.zeros(nseq, S, dtype=torch.uint8)
    kpad[1, S - 40:] = 1
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
    qr = qkv.float().view(nseq, S, 3 * D).requires_grad_(True)
    q, k, v = qr.split(D, dim=-1)
    hv = lambda t: t.reshape(nseq, S, H, HD).transpose(1, 2)
    sc = hv(q) @ hv(k).transpose(-1, -2) * HD ** -0.5 + b
    sc = sc.masked_fill(kpad.bool()[:, None, None, :], -math.inf)
    oref = (torch.softmax(sc, -1) @ hv(v)).transpose(1, 2).reshape(nseq * S, D)
    lse_ref = torch.logsumexp(sc, -1)
    oref.backward(dout.float())
    out, lse = ops.attention_fwd(dev(qkv), nseq, S, H, key_pad=dev(kpad), drop_p=p, drop_seed=seed, **kw)
    assert L.last_route() == "long"
    tol = dict(atol=2e-4, rtol=2e-4) if dtype == torch.float32 else dict(atol=4e-2, rtol=4e-2)
    torch.testing.assert_close(out.float().cpu(), oref.detach(), **tol)
    torch.testing.assert_close(lse.cpu(), lse_ref.detach(), atol=2e-3 if dtype == torch.float32 else 3e-2, rtol=1e-3)
    extra = dict(d_sp_table=torch.zeros(32, H, device="cuda"), d_virt=torch.zeros(H, device="cuda"))
    dqkv, _ = ops.attention_bwd(dev(dout), dev(qkv), out, lse, nseq, S, H, key_pad=dev(kpad), drop_p=p, drop_seed=seed, **kw, **extra)
    assert L.last_route() == "long"
    gt = dict(atol=1e-3, rtol=1e-3) if dtype == torch.float32 else dict(atol=0.12, rtol=6e-2)
    torch.testing.assert_close(dqkv.float().cpu().view(nseq, S, 3 * D), qr.grad, **gt)
    st = dict(atol=2e-3, rtol=2e-3) if dtype == torch.float32 else dict(atol=0.3, rtol=0.1)
    want = tb.grad.clone()
    want[0] = 0                                   # padding_idx row never receives a gradient
    torch.testing.assert_close(extra["d_sp_table"].cpu(), want, **st)
    torch.testing.assert_close(extra["d_virt"].cpu(), vt.grad, **st)


# ----------------------------------------------------------------------------- module level
def test_multihead_attention_128_by_8_in_bf16():
    """MultiheadAttention(128, 8) — the graph attention of Tiny mDT — in bf16 with an attention bias and a padding mask,
    against the same module in fp32 on the bf16-rounded weights and inputs: output 0.03 / 2e-2, parameter gradients and the
    input gradient 0.06 / 5e-2 (the kernel gates above)."""
    from multimodaldiscussiontransformer_amd.modules.multihead_attention import MultiheadAttention
    T, B, D, H = 17, 4, 128, 8
    torch.manual_seed(5)
    ref = MultiheadAttention(D, H, dropout=0.0, self_attention=True)
    with torch.no_grad():
        for i, prm in enumerate(ref.parameters()):
            prm.copy_(rnd(*prm.shape, seed=200 + i, scale=0.3 if prm.dim() > 1 else 0.1).bfloat16().float())
    prod = MultiheadAttention(D, H, dropout=0.0, self_attention=True)
    prod.load_state_dict(ref.state_dict())
    ref, prod = ref.cuda(), prod.cuda().to(BF)
    x = rnd(T, B, D, seed=1).bfloat16()
    bias = rnd(B, H, T, T, seed=2, scale=2.0)
    bias[1, :, :, 13:] = float("-inf")
    kpm = torch.zeros(B, T, dtype=torch.bool)
    kpm[2, 9:] = True
    cot = rnd(T, B, D, seed=3).bfloat16()
    xr = x.float().cuda().requires_grad_(True)
    yr, _ = ref(xr, xr, xr, bias.cuda(), key_padding_mask=kpm.cuda(), need_weights=False)
    yr.backward(cot.float().cuda())
    xp = x.cuda().requires_grad_(True)
    yp, _ = prod(xp, xp, xp, bias.cuda(), key_padding_mask=kpm.cuda(), need_weights=False)
    assert yp.dtype == BF
    yp.backward(cot.cuda())
    assert L.last_route() != "", "the bf16 module ran a HIP attention kernel"
    print(f"[MHA 128 x 8 bf16] out |err| {float((yp.float() - yr).detach().abs().max()):.3e}")
    torch.testing.assert_close(yp.float(), yr.detach(), atol=0.03, rtol=2e-2)
    torch.testing.assert_close(xp.grad.float(), xr.grad, atol=0.06, rtol=5e-2)
    gp = dict(prod.named_parameters())
    for n, prm in ref.named_parameters():
        print(f"[MHA 128 x 8 bf16] d{n} |err| {float((gp[n].grad.float() - prm.grad).abs().max()):.3e} of {float(prm.grad.abs().max()):.3e}")
        torch.testing.assert_close(gp[n].grad.float(), prm.grad, atol=0.06, rtol=5e-2, msg=n)


# ----------------------------------------------------------------------------- refusals that remain
def test_widths_and_launches_still_refused(ops):
    from multimodaldiscussiontransformer_amd._lib import MdtError
    import ctypes as C
    S, H = 40, 2
    with pytest.raises(MdtError, match="head_dim"):
        ops.attention_fwd(dev(rnd(S, 3 * H * 32, seed=5).to(BF)), 1, S, H)       # bf16, 32-wide heads
    # length bins handed to the C ABI directly at head_dim 16: refused, with the message the 64-only bins always had
    qkv = dev(rnd(2 * S, 3 * H * HD, seed=4).to(BF))
    out = torch.empty(2 * S, H * HD, dtype=BF, device="cuda")
    lse = torch.empty(2, H, S, dtype=torch.float32, device="cuda")
    off = dev(torch.tensor([0, S, 2 * S], dtype=torch.int32))
    ids = dev(torch.tensor([0, 1], dtype=torch.int32))
    a = ops._attn_args(qkv, out, lse, 2, S, H, HD, S, 1, HD ** -0.5, None, None, None, None, None, None, None,
                       seq_offsets=off, seq_ids=ids, s_cap=S)
    with pytest.raises(MdtError, match="seq_ids / s_cap are for ragged bf16 launches with head_dim 64"):
        ops.check(ops.lib.mdt_attention_fwd(ops.stream(), C.byref(a)), "mdt_attention_fwd")
    # ... and the same launch without them runs
    o2, _ = ops.attention_fwd(qkv, 2, S, H, seq_offsets=off)
    assert bool(torch.isfinite(o2.float()).all())
