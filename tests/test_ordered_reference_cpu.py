"""The orders the ordered (deterministic-mode) kernels document in include/mdt_hip.h, restated in torch on the CPU: what
tests/test_ordered_kernels_gpu.py compares the kernels with, bit for bit.  fp32 CPU adds are IEEE round-to-nearest, one
rounding each, exactly what the kernels do (the library is built with -ffp-contract=off, and these sums have no multiply).

The self-tests feed each emulator inputs on which another summation order gives other bits (a 2^24 among ones: 2^24 + 1
rounds back to 2^24, so the ones vanish one at a time but survive when they are added to each other first), compare with
the value worked out by hand, and show that ``torch.sum`` — some other order — does not reproduce it: a GPU test that
passes against these emulators has told the orders apart."""
import torch

CHUNK = 64                  # mdt_row_segment_sum_f32: sources of a segment per chunk
HIST_THREADS = 256          # mdt_attn_bias_grad_ordered: threads (private histograms) per workgroup for up to 95 table rows
COLSUM_BLOCK = 256          # mdt_colsum_ordered: rows per block
F24 = 2.0 ** 24


# ------------------------------------------------------------------------------------------------ emulators
def emu_sum_slices(ws: torch.Tensor, out0=None) -> torch.Tensor:
    """(out0 or 0) + (((ws[0] + ws[1]) + ws[2]) + ...): fp32, left to right, the old value last."""
    assert ws.dtype == torch.float32 and ws.shape[0] >= 1
    s = ws[0].clone()
    for z in range(1, ws.shape[0]):
        s = s + ws[z]
    base = torch.zeros_like(s) if out0 is None else out0.float()
    return base + s


def emu_colsum(x: torch.Tensor, out0: torch.Tensor, row_weight=None) -> torch.Tensor:
    """mdt_colsum_ordered: blocks of 256 rows; in a block row lane j of 4 adds rows j, j + 4, ... (each w * x rounded first),
    the block partial is ((l0 + l1) + l2) + l3; the blocks, then the old value, through emu_sum_slices."""
    M, N = x.shape
    xf = x.float()
    if row_weight is not None:
        xf = row_weight.float()[:, None] * xf
    parts = []
    for r0 in range(0, M, COLSUM_BLOCK):
        blk = xf[r0:r0 + COLSUM_BLOCK]
        lanes = []
        for j in range(4):
            s = torch.zeros(N, dtype=torch.float32)
            for r in range(j, blk.shape[0], 4):
                s = s + blk[r]
            lanes.append(s)
        parts.append(((lanes[0] + lanes[1]) + lanes[2]) + lanes[3])
    return emu_sum_slices(torch.stack(parts), out0)


def emu_segment_sum(table0: torch.Tensor, seg_row, seg_off, order, src: torch.Tensor, s_stride=1, s_off=0) -> torch.Tensor:
    """mdt_row_segment_sum_f32: per segment the sources in the order listed, in chunks of 64; a chunk left to right, the
    chunk sums left to right, the table's old value last; empty segments and seg_row < 0 leave the table alone."""
    table = table0.clone()
    rows = src.float()
    for s, t in enumerate(seg_row.tolist()):
        o0, o1 = int(seg_off[s]), int(seg_off[s + 1])
        if t < 0 or o0 >= o1:
            continue
        total = None
        for b in range(o0, o1, CHUNK):
            cs = rows[int(order[b]) * s_stride + s_off].clone()
            for o in range(b + 1, min(b + CHUNK, o1)):
                cs = cs + rows[int(order[o]) * s_stride + s_off]
            total = cs if total is None else total + cs
        table[t] = table[t] + total
    return table


def segments_of(idx: torch.Tensor, n_table_rows: int):
    """The CSR ops.segments_of builds (one segment per table row, a stable sort inside), on the CPU."""
    sorted_idx, order = torch.sort(idx.long(), stable=True)
    bounds = torch.arange(n_table_rows + 1)
    seg_off = torch.searchsorted(sorted_idx, bounds)
    return bounds[:-1].to(torch.int32), seg_off.to(torch.int32), order.to(torch.int32)


def hist_threads(num_spatial: int) -> int:
    """Threads per workgroup of mdt_attn_bias_grad_ordered: the largest of 256, 128, 64, 32 whose (num_spatial + 1) x T fp32
    histograms fit 96 KiB."""
    for t in (256, 128, 64, 32):
        if (num_spatial + 1) * t * 4 <= 96 * 1024:
            return t
    raise ValueError(f"{num_spatial} table rows: no histogram layout")


def emu_bias_hist(dS: torch.Tensor, spatial_pos: torch.Tensor, table0: torch.Tensor, virt0: torch.Tensor):
    """mdt_attn_bias_grad_ordered → (d_sp_table, d_virt): per (sequence, head) thread t of T = hist_threads(num_spatial) adds elements t, t + T, ... of
    the row-major S x S matrix into its histogram (bin = spatial_pos for q, key >= 1 — bin 0 dropped —, the last bin for
    q == 0 or key == 0); the histograms fold by halving (t += t + T / 2, ..., t += t + 1); sequences, then the old value,
    through emu_sum_slices."""
    nseq, H, S, _ = dS.shape
    ns = table0.shape[0]
    bins = ns + 1
    T = hist_threads(ns)
    e = torch.arange(S * S)
    q, key = e // S, e % S
    ws = torch.zeros(nseq, bins, H, dtype=torch.float32)
    for s in range(nseq):
        b = torch.full((S * S,), ns, dtype=torch.long)
        inner = (q >= 1) & (key >= 1)
        b[inner] = spatial_pos[s].long()[q[inner] - 1, key[inner] - 1]
        live = (b > 0) & (b < bins)
        for h in range(H):
            d = dS[s, h].reshape(-1).float()
            hist = torch.zeros(T, bins, dtype=torch.float32)
            for r0 in range(0, S * S, T):          # one element per thread and round: no two share a cell
                sl = slice(r0, min(r0 + T, S * S))
                t = torch.arange(sl.stop - sl.start)[live[sl]]
                hist[t, b[sl][live[sl]]] = hist[t, b[sl][live[sl]]] + d[sl][live[sl]]
            stride = T // 2
            while stride >= 1:
                hist[:stride] = hist[:stride] + hist[stride:2 * stride]
                stride //= 2
            ws[s, :, h] = hist[0]
    return emu_sum_slices(ws[:, :ns, :], table0), emu_sum_slices(ws[:, ns, :], virt0)


# ------------------------------------------------------------------------------------------------ self-tests
def test_sum_slices_is_left_to_right_with_the_old_value_last():
    ws = torch.ones(28, 3, 5)
    ws[0] = F24                                    # 2^24 + 1 rounds back to 2^24, 27 times
    got = emu_sum_slices(ws)
    assert torch.equal(got, torch.full((3, 5), F24))
    assert not torch.equal(torch.sum(ws, 0), got), "torch.sum reproduces the sequential order: the pattern tells nothing apart"
    assert torch.equal(emu_sum_slices(ws.flip(0)), torch.full((3, 5), F24 + 28.0))      # the ones first: 27, and 2^24 + 27 rounds (to even) to 2^24 + 28
    # the old value joins LAST: (2^24 - 2^24) + 1 = 1, whereas an old value added first would vanish in 2^24
    ws2 = torch.stack([torch.full((2, 2), F24), torch.full((2, 2), -F24)])
    assert torch.equal(emu_sum_slices(ws2, torch.ones(2, 2)), torch.ones(2, 2))
    # 1, 2^24, -2^24: left to right the one is lost
    ws3 = torch.tensor([1.0, F24, -F24]).view(3, 1, 1)
    assert float(emu_sum_slices(ws3)) == 0.0 and float(emu_sum_slices(ws3.flip(0))) == 1.0


def test_segment_sum_is_chunked_then_sequential():
    # one segment of 3 chunks: chunk 0 = 2^24 then 63 ones (the ones vanish), chunks 1 and 2 = 64 ones each (64 + 64 survive)
    n, D = 3 * CHUNK, 4
    src = torch.ones(n, D)
    src[0] = F24
    idx = torch.zeros(n, dtype=torch.int32)
    seg = segments_of(idx, 2)
    got = emu_segment_sum(torch.zeros(2, D), *seg, src)
    assert torch.equal(got[0], torch.full((D,), F24 + 128.0)) and torch.equal(got[1], torch.zeros(D))
    assert not torch.equal(torch.sum(src, 0), got[0])                          # another order: other bits
    flat = emu_sum_slices(src.view(n, 1, D))[0]                                # no chunks: every one vanishes
    assert torch.equal(flat, torch.full((D,), F24))
    # the table's old value joins last, empty and negative segments leave it alone
    t0 = torch.full((3, D), -F24)
    got = emu_segment_sum(t0, torch.tensor([0, -1, 2], dtype=torch.int32), torch.tensor([0, n, n, n], dtype=torch.int32),
                          torch.arange(n, dtype=torch.int32), src)
    assert torch.equal(got[0], torch.full((D,), 128.0)) and torch.equal(got[1:], t0[1:])
    # sources of a segment in ascending source-row order, strided sources
    src2 = torch.arange(12.0).view(12, 1)
    seg_row, seg_off, order = segments_of(torch.tensor([1, 0, 1, -1, 0], dtype=torch.int32), 2)
    assert order.tolist() == [3, 1, 4, 0, 2] and seg_off.tolist() == [1, 3, 5]
    got = emu_segment_sum(torch.zeros(2, 1), seg_row, seg_off, order, src2, s_stride=2, s_off=1)
    assert got.view(-1).tolist() == [3.0 + 9.0, 1.0 + 5.0]


def test_colsum_blocks_and_lanes():
    # rows 0, 4, 8, ... (lane 0 of block 0) start with 2^24: the ones of lane 0 vanish, lanes 1-3 keep theirs (3 * 64 = 192)
    x = torch.ones(COLSUM_BLOCK + 3, 2)
    x[0] = F24
    got = emu_colsum(x, torch.zeros(2))
    assert torch.equal(got, torch.full((2,), F24 + 192.0 + 3.0))
    assert not torch.equal(torch.sum(x, 0), got)
    w = torch.zeros(COLSUM_BLOCK + 3, dtype=torch.int32)
    w[-1] = 3
    assert torch.equal(emu_colsum(x, torch.ones(2), w), torch.full((2,), 4.0))


def test_bias_histogram_order():
    nseq, H, S, ns = 2, 1, 20, 3
    sp = torch.ones(nseq, S - 1, S - 1, dtype=torch.int32)          # every inner element feeds table row 1
    sp[:, 0, 0] = 0                                                 # ... but one, the padding index
    dS = torch.zeros(nseq, H, S, S)
    # thread 22 owns elements 22 (q 1, key 2) and 278 (q 13, key 18): 1 + 2^24 = 2^24; the first fold adds thread 150
    # (element 150: q 7, key 10) = -2^24: 0.  Any order that meets 2^24 - 2^24 first keeps the 1.
    dS[0, 0, 1, 2], dS[0, 0, 13, 18], dS[0, 0, 7, 10] = 1.0, F24, -F24
    dS[1, 0, 1, 3] = 5.0
    dS[:, 0, 1, 1] = 7.0                    # the padding index: lands nowhere
    dS[0, 0, 0, 5], dS[1, 0, 3, 0] = 2.0, 3.0
    t, v = emu_bias_hist(dS, sp, torch.zeros(ns, H), torch.zeros(H))
    assert float(t[0, 0]) == 0.0 and float(t[2, 0]) == 0.0
    assert float(t[1, 0]) == 5.0 and float(dS[:, :, 1:, 1:].double().sum()) - 14.0 == 6.0
    assert float(v[0]) == 5.0
    # the fold by halving: 2^24 on thread 18, ones on threads 146 (= 18 + 128), 82 (= 18 + 64) and 210 (= 82 + 128).
    # stride 128: t18 = 2^24 + 1 = 2^24, t82 = 1 + 1 = 2; stride 64: t18 = 2^24 + 2.  Element order loses all three ones.
    S2 = 17
    sp2 = torch.ones(1, S2 - 1, S2 - 1, dtype=torch.int32)
    dS2 = torch.zeros(1, 1, S2, S2)
    flat = dS2.view(-1)
    flat[18], flat[146], flat[82], flat[210] = F24, 1.0, 1.0, 1.0
    assert all(e // S2 >= 1 and e % S2 >= 1 for e in (18, 146, 82, 210))
    t2, _ = emu_bias_hist(dS2, sp2, torch.zeros(2, 1), torch.zeros(1))
    assert float(t2[1, 0]) == F24 + 2.0
    assert float(emu_sum_slices(flat.view(-1, 1, 1))) == F24                   # element order: another result
    # 512 table rows (the model's num_spatial): 32 threads — thread 18 owns elements 18 and 50 now, and 146 = 18 + 4 * 32 too
    assert hist_threads(23) == hist_threads(95) == 256 and hist_threads(96) == 128 and hist_threads(512) == 32
    t3, _ = emu_bias_hist(dS2, sp2, torch.zeros(512, 1), torch.zeros(1))
    # thread 18: 2^24 (e 18), + 1 (e 82 = 18 + 2 * 32) lost, + 1 (e 146) lost, + 1 (e 210 = 18 + 6 * 32) lost
    assert float(t3[1, 0]) == F24
