"""Attention over 96- and 128-wide heads (graph heads of D 768 / 1024 with 8 heads — the registered multi_graphormer
architecture's default is 1024 / 8 = 128), fp32 and bf16: every kernel such a launch can reach against torch fp32 on the same
inputs with the head_dim 64 gates, and against the head_dim 64 kernels themselves on zero-padded heads.

A 96-wide head is three K = 32 contraction steps and six 16-column output tiles, a 128-wide head four and eight.  Every case
has H >= 3 heads with independent random data per head: a fragment that strayed into its neighbour would show.

Routing of the backward (bf16), as attn_plan (csrc/attention.hip) states it for every width but 64 — the one-pass kernels are 64-only:
    dense bias                                   v1, except head_dim 128 with S > 208: the two [288][136] images of the v1
                                                 kernels are past 160 KiB there, forward and backward take the long path
    structural bias, S <= 80, no q_limit         v1
    no dropout, no q_limit, S <= 112             v2
    otherwise                                    v3 (head_dim 128, S > 256: its 288-row form with 32-key chunks)

The strict gate for attention is tests/test_attention_routes_gpu.py: every kernel and route against the fp64 reference of
tests/attention_reference.py with a derived bound per element; the assert_close gates here are wide enough for a skipped key.
"""
import math

import numpy as np
import pytest
import torch

import tests.attention_reference as A
from multimodaldiscussiontransformer_amd import _lib as L
from tests.test_attention_head_dim_gpu import force_bwd, ops  # noqa: F401  (fixtures)
from tests.test_dropout_gpu import attn_mask
from tests.test_kernels_gpu import dense_from_struct, dev, make_struct, ref_attention, rnd

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
WIDTHS = [96, 128]


# ----------------------------------------------------------------------------- forward + backward against torch fp32
CASES = [  # (nseq, S, H, mode, time_major); boundaries: 80 | 81 (struct v1 -> v2), 112 | 113 (v2 -> v3), 208 | 209 (dense, 128-wide:
    # v1 -> long), 256 | 257 (128-wide: the v3 kernel with 64-key chunks -> the one with 32-key chunks and 272-byte rows)
    (3, 8, 3, "struct", True),
    (2, 17, 3, "mask", False), (2, 17, 3, "dense", True),
    (2, 33, 4, "none", False),
    (2, 65, 3, "struct", False), (2, 65, 3, "struct", True),
    (2, 80, 3, "struct", False), (2, 81, 3, "struct", False),
    (2, 104, 3, "mask", False), (2, 104, 3, "none", False),
    (2, 112, 3, "none", False), (2, 113, 3, "none", False),
    (2, 129, 3, "struct", True),
    (2, 201, 3, "none", False), (1, 208, 3, "dense", True), (1, 209, 3, "dense", False),
    (2, 256, 3, "none", False), (2, 257, 3, "struct", False),
    (2, 261, 3, "mask", False), (2, 261, 3, "none", False), (2, 261, 3, "struct", False), (1, 261, 3, "dense", False),
]


def run_case(ops, dtype, hd, nseq, S, H, mode, time_major, tag):
    bf = dtype == BF
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
    assert L.last_route() == A.fwd_route(dtype, hd, S, mode), L.last_route()

    def unlay(t, width):
        t = t.float().cpu()
        return t.view(S, nseq, width).transpose(0, 1) if time_major else t.view(nseq, S, width)

    o_err = float((unlay(out, D) - oref.detach()).abs().max())
    l_err = float(torch.nan_to_num(lse.cpu() - lref.detach(), nan=0.0, posinf=0.0, neginf=0.0).abs().max())
    print(f"[{tag} hd{hd} {mode} S={S} tm={time_major}] out |err| {o_err:.3e}, lse |err| {l_err:.3e} on {L.last_route()}")
    tol = dict(atol=0.03, rtol=2e-2) if bf else dict(atol=2e-4, rtol=1e-4)
    torch.testing.assert_close(unlay(out, D), oref.detach(), **tol)
    torch.testing.assert_close(lse.cpu(), lref.detach(), atol=0.03 if bf else 2e-4, rtol=1e-3)

    extra = {}
    if mode == "struct":
        extra = dict(d_sp_table=torch.zeros(64, H, dtype=torch.float32).cuda(),
                     d_virt=torch.zeros(H, dtype=torch.float32).cuda())
    dqkv, dbias = ops.attention_bwd(d2, q2, out, lse, nseq, S, H, scale=scale, **lay, **kw,
                                    want_dense_dbias=(mode == "dense"), **extra)
    assert L.last_route() == A.bwd_route(dtype, hd, S, mode), L.last_route()
    gtol = dict(atol=0.06, rtol=5e-2) if bf else dict(atol=5e-4, rtol=1e-3)
    print(f"[{tag} hd{hd} {mode} S={S}] dqkv |err| {float((unlay(dqkv, 3 * D) - qr.grad).abs().max()):.3e} on {L.last_route()}")
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
        print(f"[{tag} hd{hd} struct S={S}] d_sp_table |err| {float((extra['d_sp_table'].cpu() - ref_tab).abs().max()):.3e}, "
              f"d_virt |err| {float((extra['d_virt'].cpu() - ref_virt).abs().max()):.3e}")
        torch.testing.assert_close(extra["d_sp_table"].cpu(), ref_tab, atol=gtol["atol"] * 4, rtol=gtol["rtol"])
        torch.testing.assert_close(extra["d_virt"].cpu(), ref_virt, atol=gtol["atol"] * 8, rtol=gtol["rtol"])


@pytest.mark.parametrize("hd", WIDTHS)
@pytest.mark.parametrize("nseq,S,H,mode,time_major", CASES)
def test_attention_wide_heads_bf16(ops, hd, nseq, S, H, mode, time_major):
    """tests/test_kernels_gpu.py::test_attention at head_dim 96 / 128 in bf16, with its gates: out 0.03 / 2e-2, lse 0.03 / 1e-3,
    dqkv / dense dbias 0.06 / 5e-2, d_sp_table 4 x and d_virt 8 x that atol; forward and backward route asserted."""
    run_case(ops, BF, hd, nseq, S, H, mode, time_major, "bf16")


def test_cases_reach_every_route_and_boundary():
    for hd in WIDTHS:
        got = {(mode, A.bwd_route(BF, hd, S, mode)) for _, S, _, mode, _ in CASES}
        want = {("none", "v2"), ("none", "v3"), ("mask", "v2"), ("mask", "v3"), ("struct", "v1"), ("struct", "v2"), ("struct", "v3"),
                ("dense", "v1")} | ({("dense", "long")} if hd == 128 else set())
        assert got == want, (hd, got ^ want)
        # every route the rule can return, over the whole domain
        every = {A.bwd_route(BF, hd, S, mode, p, q) for S in range(1, 273) for mode in ("none", "mask", "dense", "struct")
                 for p in (0.0, 0.1) for q in (0, 9)}
        assert every == {r for _, r in want}
    sizes = {S for _, S, _, _, _ in CASES}
    assert {8, 17, 33, 65, 104, 129, 201, 261} <= sizes
    assert {80, 81, 112, 113, 208, 209, 256, 257} <= sizes
    for mode in ("none", "mask", "dense", "struct"):
        assert max(S for _, S, _, m, _ in CASES if m == mode) == 261


@pytest.mark.parametrize("hd", WIDTHS)
@pytest.mark.parametrize("mode", ["none", "mask", "dense", "struct"])
@pytest.mark.parametrize("S", [17, 65, 129, 261])
def test_attention_wide_heads_fp32(ops, hd, S, mode):
    """The same in fp32 (gates of test_attention: out 2e-4 / 1e-4, lse 2e-4, gradients 5e-4 / 1e-3); the graph layout for the
    per-pair biases."""
    run_case(ops, torch.float32, hd, 2, S, 3, mode, mode in ("struct", "dense") and S != 261, "fp32")


# ----------------------------------------------------------------------------- dropout
@pytest.mark.parametrize("hd", WIDTHS)
@pytest.mark.parametrize("bwd", [None, "v1", "v3", "v4x", "v5"])
@pytest.mark.parametrize("nseq,S,H", [(3, 20, 3), (2, 104, 3), (2, 201, 3)])
def test_attention_dropout_wide_heads(ops, hd, bwd, nseq, S, H, force_bwd):
    """tests/test_dropout_gpu.py::test_attention_dropout at head_dim 96 / 128 (p = 0.3, the kernels' own masks through
    ops.dropout_mask, gates out 0.04 / 3e-2 and gradients 0.08 / 6e-2).  With dropout the default backward is v3; v1 and v3
    can be forced; MDT_ATTN_BWD=v4x|v5 (64-only kernels) runs the default kernel, same bits."""
    p, seed = 0.3, 4242
    D = H * hd
    qkv = rnd(nseq, S, 3 * D, seed=7).to(BF)
    dout = rnd(nseq, S, D, seed=8).to(BF)
    km = torch.ones(nseq, S, dtype=torch.uint8)
    km[1, S - 3:] = 0
    m = attn_mask(ops, nseq, H, S, p, seed)
    qr = qkv.float().requires_grad_(True)
    q, k, v = qr.split(D, dim=-1)
    hv = lambda t: t.view(nseq, S, H, hd).transpose(1, 2)
    s = hv(q) @ hv(k).transpose(-1, -2) * hd ** -0.5
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
    print(f"[hd{hd} dropout S={S} {bwd}] dqkv |err| {float((dqkv.float().cpu().view(nseq, S, 3 * D) - qr.grad).abs().max()):.3e}")
    torch.testing.assert_close(dqkv.float().cpu().view(nseq, S, 3 * D), qr.grad, atol=0.08, rtol=6e-2)
    if bwd in (None, "v3", "v4x", "v5"):
        assert torch.equal(dqkv, d_default)


# ----------------------------------------------------------------------------- ragged sequences, q_limit, poisoned buffers
@pytest.mark.parametrize("hd", WIDTHS)
@pytest.mark.parametrize("Smax,bwd", [(40, None), (40, "v1"), (40, "v2"), (104, None), (104, "v2"), (201, None), (201, "v1"), (261, None)])
def test_ragged_sequences_equal_masked_padding_wide_heads(ops, hd, bwd, Smax, force_bwd):
    """tests/test_kernels_gpu.py::test_attention_ragged_sequences_equal_masked_padding at head_dim 96 / 128 (gates 2e-2 / 2e-2,
    lse 1e-4), lengths from 1 to Smax; Smax 261 is the 288-row form of 128-wide heads.  With ``bins`` the call runs as ONE
    launch over seq_offsets (length bins are for 64-wide heads) and gives the same bits."""
    force_bwd(bwd)
    H, p, seed = 3, 0.25, 31
    D = H * hd
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
    short = [i for i, n in enumerate(lens) if n <= 48]
    long_ = [i for i, n in enumerate(lens) if n > 48]
    bins = [(dev(torch.tensor(short, dtype=torch.int32)), 48)] + ([(dev(torch.tensor(long_, dtype=torch.int32)), Smax)] if long_ else [])
    out_b, lse_b = ops.attention_fwd(dev(qkv_r), nseq, Smax, H, bins=bins, **kwr)
    dq_b, _ = ops.attention_bwd(dev(dout_r), dev(qkv_r), out_b, lse_b, nseq, Smax, H, bins=bins, **kwr)
    assert torch.equal(out_b, out_r) and torch.equal(dq_b, dq_r)
    for s_, n in enumerate(lens):
        assert torch.equal(lse_b[s_, :, :n], lse_r[s_, :, :n])


@pytest.mark.parametrize("hd", WIDTHS)
@pytest.mark.parametrize("S,qlim", [(104, 9), (201, 33), (261, 40)])
def test_query_limit_wide_heads(ops, hd, S, qlim):
    """q_limit (tests/test_kernels_gpu.py::test_attention_query_limit, bf16 gates 1e-2 / 1e-2): outputs of the requested rows and
    the gradients (dout zero elsewhere) equal the unrestricted call; dQ of every other row is zero."""
    nseq, H, p, seed = 3, 3, 0.2, 77
    D = H * hd
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


@pytest.mark.parametrize("hd", WIDTHS)
@pytest.mark.parametrize("Smax,qlim", [(40, 0), (104, 9), (201, 33), (261, 40)])
def test_backward_v3_never_reads_what_forward_did_not_write_wide_heads(ops, hd, Smax, qlim, force_bwd, monkeypatch):
    """The poisoned-buffer construction of test_attention_backward_never_reads_what_forward_did_not_write on v3: lse positions
    past a sequence's length and lse / out rows past q_limit's tile set to NaN, +inf, -1e30 and 0, and the gradient buffer
    pre-filled with the same poison — bit-identical, finite gradients."""
    force_bwd("v3")
    H, p, seed = 3, 0.2, 5
    D = H * hd
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


# ----------------------------------------------------------------------------- wide heads against the 64-wide kernels
@pytest.mark.parametrize("hd", WIDTHS)
@pytest.mark.parametrize("S,mode,p,bwd", [(40, "mask", 0.0, "v1"), (65, "struct", 0.0, None), (104, "none", 0.0, "v2"),
                                          (129, "struct", 0.0, None), (201, "none", 0.1, "v3"), (104, "mask", 0.3, "v3")])
def test_wide_heads_equal_zero_padded_head_dim_64(ops, hd, S, mode, p, bwd, force_bwd):
    """A head of 64 is a head of 96 / 128 whose other q / k / v columns are zero (scale = 64^-0.5 passed explicitly).  The live
    out columns, lse and the live gradient columns of the wide launch on zero-padded data against the head_dim 64 launch on
    the unpadded data, on the same route (forced where the 64-wide default would be a one-pass kernel): no torch in between.
    Both evaluate the same fp32 expressions (the padded columns add exact zeros), so they differ by the rounding of the
    outputs to bf16, 2^-8 relative, plus the reordering of fp32 sums (atol 1e-5); padded out columns are exactly 0."""
    nseq, H = 2, 3
    D64, DW = H * 64, H * hd
    force_bwd(bwd)
    qkv64 = rnd(nseq * S, 3 * D64, seed=21).to(BF)
    dout64 = rnd(nseq * S, D64, seed=22).to(BF)
    qkvw = torch.zeros(nseq * S, 3, H, hd, dtype=BF)
    qkvw[..., :64] = qkv64.view(nseq * S, 3, H, 64)
    doutw = torch.zeros(nseq * S, H, hd, dtype=BF)
    doutw[..., :64] = dout64.view(nseq * S, H, 64)
    kw = dict(scale=64 ** -0.5, drop_p=p, drop_seed=99)
    extraw, extra64 = {}, {}
    if mode == "mask":
        km = torch.ones(nseq, S, dtype=torch.uint8)
        km[1, S - 5:] = 0
        kw["key_mask"] = dev(km)
    elif mode == "struct":
        sp, ab, kpad, table, virt = make_struct(nseq, S, H, seed=11)
        kw.update(attn_bias=dev(ab), spatial_pos=dev(sp), sp_table=dev(table.to(BF)), virt=dev(virt.to(BF)), key_pad=dev(kpad))
        extraw = dict(d_sp_table=torch.zeros(64, H, device="cuda"), d_virt=torch.zeros(H, device="cuda"))
        extra64 = dict(d_sp_table=torch.zeros(64, H, device="cuda"), d_virt=torch.zeros(H, device="cuda"))
    q64, d64 = dev(qkv64), dev(dout64)
    qw, dw = dev(qkvw.view(nseq * S, 3 * DW)), dev(doutw.view(nseq * S, DW))
    ow, lw = ops.attention_fwd(qw, nseq, S, H, **kw)
    rw = L.last_route()
    o64, l64 = ops.attention_fwd(q64, nseq, S, H, **kw)
    assert rw == L.last_route() == "v2"
    gw, _ = ops.attention_bwd(dw, qw, ow, lw, nseq, S, H, **kw, **extraw)
    rw = L.last_route()
    g64, _ = ops.attention_bwd(d64, q64, o64, l64, nseq, S, H, **kw, **extra64)
    assert rw == L.last_route() == (bwd or A.bwd_route(BF, hd, S, mode, p)), (rw, L.last_route())
    tol = dict(rtol=2.0 ** -8, atol=1e-5)
    torch.testing.assert_close(ow.float().view(-1, H, hd)[..., :64], o64.float().view(-1, H, 64), **tol)
    fin = torch.isfinite(l64)
    assert torch.equal(fin, torch.isfinite(lw))
    torch.testing.assert_close(lw[fin], l64[fin], **tol)
    torch.testing.assert_close(gw.float().view(-1, 3, H, hd)[..., :64], g64.float().view(-1, 3, H, 64), **tol)
    assert float(ow.float().view(-1, H, hd)[..., 64:].abs().max()) == 0.0
    if mode == "struct":      # fp32 atomics: the order of the partial sums is not fixed
        torch.testing.assert_close(extraw["d_sp_table"], extra64["d_sp_table"], rtol=2.0 ** -8, atol=1e-3)
        torch.testing.assert_close(extraw["d_virt"], extra64["d_virt"], rtol=2.0 ** -8, atol=1e-3)


@pytest.mark.parametrize("hd", WIDTHS)
def test_fp32_structural_bias_with_dropout_past_208_tokens_takes_key_chunked_backward(ops, hd):
    """fp32, wide heads, structural bias AND dropout, S > 208: the 17-tile backward of attention.hip would not fit the register
    file (it is not instantiated), so the backward is the key-chunked path — same dropout counters, same lse.  Held against
    the 64-wide fp32 launch (v1 both ways) on the unpadded data with the fp32 gates of test_attention: out 2e-4 / 1e-4,
    gradients 5e-4 / 1e-3, table 4 x and virt 8 x that atol.  S = 208 stays on v1."""
    nseq, H, p = 2, 3, 0.1
    for S, want in ((208, "v1"), (261, "long")):
        qkv64 = rnd(nseq * S, 3 * H * 64, seed=21)
        dout64 = rnd(nseq * S, H * 64, seed=22)
        qkvw = torch.zeros(nseq * S, 3, H, hd)
        qkvw[..., :64] = qkv64.view(nseq * S, 3, H, 64)
        doutw = torch.zeros(nseq * S, H, hd)
        doutw[..., :64] = dout64.view(nseq * S, H, 64)
        sp, ab, kpad, table, virt = make_struct(nseq, S, H, seed=11)
        kw = dict(scale=64 ** -0.5, drop_p=p, drop_seed=99, attn_bias=dev(ab), spatial_pos=dev(sp), sp_table=dev(table), virt=dev(virt),
                  key_pad=dev(kpad))
        ew = dict(d_sp_table=torch.zeros(64, H, device="cuda"), d_virt=torch.zeros(H, device="cuda"))
        e64 = dict(d_sp_table=torch.zeros(64, H, device="cuda"), d_virt=torch.zeros(H, device="cuda"))
        qw, dw = dev(qkvw.view(nseq * S, -1)), dev(doutw.view(nseq * S, -1))
        ow, lw = ops.attention_fwd(qw, nseq, S, H, **kw)
        assert L.last_route() == "v1"
        gw, _ = ops.attention_bwd(dw, qw, ow, lw, nseq, S, H, **kw, **ew)
        assert L.last_route() == want, L.last_route()
        o64, l64 = ops.attention_fwd(dev(qkv64), nseq, S, H, **kw)
        g64, _ = ops.attention_bwd(dev(dout64), dev(qkv64), o64, l64, nseq, S, H, **kw, **e64)
        assert L.last_route() == "v1"
        print(f"[fp32 hd{hd} struct dropout S={S} {want}] dqkv |diff| {float((gw.view(-1, 3, H, hd)[..., :64] - g64.view(-1, 3, H, 64)).abs().max()):.3e}")
        torch.testing.assert_close(ow.view(-1, H, hd)[..., :64], o64.view(-1, H, 64), atol=2e-4, rtol=1e-4)
        torch.testing.assert_close(gw.view(-1, 3, H, hd)[..., :64], g64.view(-1, 3, H, 64), atol=5e-4, rtol=1e-3)
        assert float(gw.view(-1, 3, H, hd)[..., 64:].abs().max()) == 0.0
        torch.testing.assert_close(ew["d_sp_table"], e64["d_sp_table"], atol=2e-3, rtol=1e-3)
        torch.testing.assert_close(ew["d_virt"], e64["d_virt"], atol=4e-3, rtol=1e-3)


# ----------------------------------------------------------------------------- long path
@pytest.mark.parametrize("hd", WIDTHS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_beyond_272_tokens_key_chunked_path_wide_heads(ops, hd, dtype):
    """tests/test_kernels_gpu.py::test_attention_beyond_272_tokens_key_chunked_path (S = 300, structural bias) at head_dim
    96 / 128, with its gates."""
    S, p, nseq, H, seed = 300, 0.0, 2, 3, 77
    D = H * hd
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
    hv = lambda t: t.reshape(nseq, S, H, hd).transpose(1, 2)
    sc = hv(q) @ hv(k).transpose(-1, -2) * hd ** -0.5 + b
    sc = sc.masked_fill(kpad.bool()[:, None, None, :], -math.inf)
    oref = (torch.softmax(sc, -1) @ hv(v)).transpose(1, 2).reshape(nseq * S, D)
    lse_ref = torch.logsumexp(sc, -1)
    oref.backward(dout.float())
    out, lse = ops.attention_fwd(dev(qkv), nseq, S, H, key_pad=dev(kpad), drop_p=p, drop_seed=seed, **kw)
    assert L.last_route() == "long"
    print(f"[long hd{hd} {dtype}] out |err| {float((out.float().cpu() - oref.detach()).abs().max()):.3e}")
    tol = dict(atol=2e-4, rtol=2e-4) if dtype == torch.float32 else dict(atol=4e-2, rtol=4e-2)
    torch.testing.assert_close(out.float().cpu(), oref.detach(), **tol)
    torch.testing.assert_close(lse.cpu(), lse_ref.detach(), atol=2e-3 if dtype == torch.float32 else 3e-2, rtol=1e-3)
    extra = dict(d_sp_table=torch.zeros(32, H, device="cuda"), d_virt=torch.zeros(H, device="cuda"))
    dqkv, _ = ops.attention_bwd(dev(dout), dev(qkv), out, lse, nseq, S, H, key_pad=dev(kpad), drop_p=p, drop_seed=seed, **kw, **extra)
    assert L.last_route() == "long"
    print(f"[long hd{hd} {dtype}] dqkv |err| {float((dqkv.float().cpu().view(nseq, S, 3 * D) - qr.grad).abs().max()):.3e}")
    gt = dict(atol=1e-3, rtol=1e-3) if dtype == torch.float32 else dict(atol=0.12, rtol=6e-2)
    torch.testing.assert_close(dqkv.float().cpu().view(nseq, S, 3 * D), qr.grad, **gt)
    st = dict(atol=2e-3, rtol=2e-3) if dtype == torch.float32 else dict(atol=0.3, rtol=0.1)
    want = tb.grad.clone()
    want[0] = 0                                   # padding_idx row never receives a gradient
    torch.testing.assert_close(extra["d_sp_table"].cpu(), want, **st)
    torch.testing.assert_close(extra["d_virt"].cpu(), vt.grad, **st)


# ----------------------------------------------------------------------------- module level
@pytest.mark.parametrize("D,H", [(1024, 8), (768, 8)])
def test_multihead_attention_wide_heads_in_bf16(D, H):
    """MultiheadAttention(1024, 8) — the registered architecture's default — and (768, 8) in bf16 with a dense bias holding a
    -inf block and a padding mask, against the same module in fp32 on the bf16-rounded weights and inputs: output
    0.03 / 2e-2, input and parameter gradients 0.06 / 5e-2.  need_weights / need_head_weights: rows sum to 1 over the
    unmasked keys and equal softmax of the before_softmax scores, within 1e-3."""
    from multimodaldiscussiontransformer_amd.modules.multihead_attention import MultiheadAttention
    T, B = 17, 4
    torch.manual_seed(5)
    ref = MultiheadAttention(D, H, dropout=0.0, self_attention=True)
    with torch.no_grad():
        for i, prm in enumerate(ref.parameters()):
            prm.copy_(rnd(*prm.shape, seed=200 + i, scale=(0.3 * (128 / D) ** 0.5) if prm.dim() > 1 else 0.1).bfloat16().float())
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
    print(f"[MHA {D} x {H} bf16] out |err| {float((yp.float() - yr).detach().abs().max()):.3e}")
    torch.testing.assert_close(yp.float(), yr.detach(), atol=0.03, rtol=2e-2)
    torch.testing.assert_close(xp.grad.float(), xr.grad, atol=0.06, rtol=5e-2)
    gp = dict(prod.named_parameters())
    for n, prm in ref.named_parameters():
        print(f"[MHA {D} x {H} bf16] d{n} |err| {float((gp[n].grad.float() - prm.grad).abs().max()):.3e} of {float(prm.grad.abs().max()):.3e}")
        torch.testing.assert_close(gp[n].grad.float(), prm.grad, atol=0.06, rtol=5e-2, msg=n)
    # attention weights.  fp32 module: against softmax of its own before_softmax scores.  bf16 module: its before_softmax scores
    # are the kernel's fp32 scores rounded to bf16 (2^-9 of |score| ~ 5 is 1e-2, past the 1e-3 asked of the probabilities), so
    # the probabilities are held against softmax of those fp32 scores, and the module's scores against their rounding.
    from multimodaldiscussiontransformer_amd import ops as O
    live = (~kpm)[:, None, :].expand(B, T, T).clone()
    live[1, :, 13:] = False
    for mod, xin in ((ref, xr.detach()), (prod, xp.detach())):
        with torch.no_grad():
            _, w_mean = mod(xin, xin, xin, bias.cuda(), key_padding_mask=kpm.cuda(), need_weights=True)
            _, w_head = mod(xin, xin, xin, bias.cuda(), key_padding_mask=kpm.cuda(), need_head_weights=True)
            sc, _ = mod(xin, xin, xin, bias.cuda(), key_padding_mask=kpm.cuda(), before_softmax=True)
            if xin.dtype == BF:
                qkv = O.gemm(xin.view(T * B, D), mod.qkv_weight.data, bias=mod.qkv_bias.data)
                raw = O.attention_head_weights(qkv, None, B, T, H, raw_scores=True, seq_stride=1, pos_stride=B, scale=mod.scaling,
                                               dense_bias=bias.cuda().contiguous(), key_pad=kpm.cuda().to(torch.uint8))
                assert torch.equal(sc.view(B, H, T, T), raw.to(BF))
                sc = raw
        w_mean, w_head = w_mean.float().cpu(), w_head.float().cpu()            # [B, T, T], [H, B, T, T]
        assert w_mean.shape == (B, T, T) and w_head.shape == (H, B, T, T)
        assert float(w_mean[~live].abs().max()) == 0.0 and float(w_head[:, ~live].abs().max()) == 0.0
        torch.testing.assert_close(w_mean.sum(-1), torch.ones(B, T), atol=1e-3, rtol=0)
        torch.testing.assert_close(w_head.sum(-1), torch.ones(H, B, T), atol=1e-3, rtol=0)
        want = torch.softmax(sc.float().cpu().view(B, H, T, T), -1).transpose(0, 1)
        print(f"[MHA {D} x {H} {xin.dtype}] head weights vs softmax(scores) |err| {float((w_head - want).abs().max()):.3e}")
        torch.testing.assert_close(w_head, want, atol=1e-3, rtol=0)
        torch.testing.assert_close(w_mean, want.mean(0), atol=1e-3, rtol=0)


# ----------------------------------------------------------------------------- architecture default
def test_registered_architecture_default_head_shape_runs(ops):
    """multi_graphormer's defaults give graph heads of 1024 / 8 = 128: one forward at that H and hd on a 2 x 65-row batch with
    the structural bias (the first graph layer's launch)."""
    from argparse import Namespace
    import multimodaldiscussiontransformer_amd.models  # noqa: F401
    from multimodaldiscussiontransformer_amd.registry import ARCH_CONFIG_REGISTRY
    args = Namespace()
    ARCH_CONFIG_REGISTRY["multi_graphormer"](args)
    H, hd = args.encoder_attention_heads, args.encoder_embed_dim // args.encoder_attention_heads
    assert (H, hd) == (8, 128)
    nseq, S = 2, 65
    sp, ab, kpad, table, virt = make_struct(nseq, S, H, seed=11)
    for dtype in (torch.float32, BF):
        qkv = dev(rnd(S * nseq, 3 * H * hd, seed=7).to(dtype))
        out, lse = ops.attention_fwd(qkv, nseq, S, H, seq_stride=1, pos_stride=nseq, attn_bias=dev(ab), spatial_pos=dev(sp),
                                     sp_table=dev(table.to(dtype)), virt=dev(virt.to(dtype)), key_pad=dev(kpad))
        assert out.shape == (S * nseq, H * hd) and bool(torch.isfinite(out.float()).all())


# ----------------------------------------------------------------------------- refusals that remain
def test_other_widths_and_bins_still_refused(ops):
    from multimodaldiscussiontransformer_amd._lib import MdtError
    import ctypes as C
    S, H = 40, 2
    for dtype in (torch.float32, BF):
        for w in (32, 80):
            with pytest.raises(MdtError, match="head_dim"):
                ops.attention_fwd(dev(rnd(S, 3 * H * w, seed=5).to(dtype)), 1, S, H)
            with pytest.raises(MdtError, match="head_dim"):      # the long path
                ops.attention_fwd(dev(rnd(300, 3 * H * w, seed=5).to(dtype)), 1, 300, H)
    # length bins handed to the C ABI directly at head_dim 128: refused, with the message the 64-only bins always had
    hd = 128
    qkv = dev(rnd(2 * S, 3 * H * hd, seed=4).to(BF))
    out = torch.empty(2 * S, H * hd, dtype=BF, device="cuda")
    lse = torch.empty(2, H, S, dtype=torch.float32, device="cuda")
    off = dev(torch.tensor([0, S, 2 * S], dtype=torch.int32))
    ids = dev(torch.tensor([0, 1], dtype=torch.int32))
    a = ops._attn_args(qkv, out, lse, 2, S, H, hd, S, 1, hd ** -0.5, None, None, None, None, None, None, None,
                       seq_offsets=off, seq_ids=ids, s_cap=S)
    with pytest.raises(MdtError, match="seq_ids / s_cap are for ragged bf16 launches with head_dim 64"):
        ops.check(ops.lib.mdt_attention_fwd(ops.stream(), C.byref(a)), "mdt_attention_fwd")
    # ... and the same launch without them runs
    o2, _ = ops.attention_fwd(qkv, 2, S, H, seq_offsets=off)
    assert bool(torch.isfinite(o2.float()).all())
