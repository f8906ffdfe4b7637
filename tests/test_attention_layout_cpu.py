"""The attention layout harness (tests/attention_layout.py) proven on the CPU, the way the reference suites prove their bounds
with mutants: an emulated launch — the reference's own result, rounded to the storage type and moved through the guarded
buffers by flat address arithmetic with the four row strides, in 16-row tiles — is accepted at every case of
tests/test_attention_layout_gpu.py, and the same emulation with one addressing defect is rejected by check_layout at the
smallest case that can show the defect.

The emulation reads what a backward reads of `out` through the stride it was told (delta = rowsum(dO . O) enters dQ and dK
linearly, so what it read wrongly is carried into them exactly); it stores rows by base + row * ld + column into the
buffer's flat storage, so a wrong stride, a wrong sequence stride or a missing guard lands where a kernel's would.

Exclusion cap: in no case does the value check leave out more than 5 % of an output's in-bounds elements (the rows that exist);
the q_limit cases are the ABI's own exception (rows at or past q_limit of out / lse are unspecified: 24 of 33 rows at S = 33)
— there the excluded set is asserted to be exactly those rows, dqkv to be compared everywhere, and the same launch without
the limit, which the GPU test runs beside it, to exclude nothing.
"""
import pytest
import torch

import tests.attention_layout as Y
import tests.attention_reference as A
from tests.attention_layout import H, NSEQ, TILE, Layout, check_layout
from tests.attention_reference import BF, F32

MUTANTS = ("out_ld_dout", "dqkv_ld_qkv", "seq_stride_S", "spill", "lse_outside", "virt_to_table", "dbias_pad", "pad_hit")


def _store(g, prow, vals, ld, col0=0):
    flat = g.buf.view(-1)
    idx = g.pre * g.ld + prow[:, None] * ld + col0 + torch.arange(vals.shape[1])[None, :]
    flat[idx] = vals.to(flat.dtype)


def _load(g, prow, width, ld):
    flat = g.buf.view(-1)
    return flat[g.pre * g.ld + prow[:, None] * ld + torch.arange(width)[None, :]].float()


class Emulated:
    """One launch of a Layout, emulated; ``mutant``: one of MUTANTS or None."""

    def __init__(self, lay: Layout, mutant=None):
        assert mutant is None or mutant in MUTANTS
        self.lay, self.mutant = lay, mutant

    def prow(self, seq, pos, seq_stride=None):
        lay = self.lay
        if lay.c.lens:
            return int(lay.off[seq]) + pos
        return seq * (lay.seq_stride if seq_stride is None else seq_stride) + pos * lay.pos_stride

    def computed(self, seq):
        """The query rows a launch computes: all, or q_limit rounded up to the tile where the kernels honour it (bf16)."""
        n = self.lay.lens[seq]
        c = self.lay.c
        if c.qlim and c.dtype == BF:
            return min(n, -(-c.qlim // TILE) * TILE)
        return n

    def _tiles(self, g, seq, vals, ld, nrows, col0=0, seq_stride=None):
        """vals [S, w] of one sequence into g, a 16-row tile at a time, rows below ``nrows`` — the whole last tile under
        "spill" (zeros where there is no row: what a kernel's padded lanes hold)."""
        for q0 in range(0, nrows, TILE):
            hi = q0 + TILE if self.mutant == "spill" else min(q0 + TILE, nrows)
            pos = torch.arange(q0, hi)
            v = torch.zeros(len(pos), vals.shape[1], dtype=vals.dtype)
            v[pos < nrows] = vals[pos[pos < nrows]]
            _store(g, self.prow(seq, pos, seq_stride), v, ld, col0)

    def forward(self, seqs=None, order=None):
        lay, c = self.lay, self.lay.c
        seqs = list(range(NSEQ)) if seqs is None else list(seqs)
        out = lay.ref["out"][0].to(c.dtype)
        lse = lay.ref["lse"][0].float()
        g, t = lay.g["out"], lay.flat["lse"].t
        for s in (order or seqs):
            self._tiles(g, s, out[s], lay.ld["out"], self.computed(s), seq_stride=lay.S if self.mutant == "seq_stride_S" else None)
        if self.mutant == "pad_hit":            # one 16-byte store that begins in the row's last 8 columns
            n = 16 // g.buf.element_size()
            v = torch.zeros(1, n, dtype=c.dtype)
            v[0, :n // 2] = out[seqs[0], 0, lay.D - n // 2:]
            _store(g, self.prow(seqs[0], torch.arange(1)), v, lay.ld["out"], lay.D - n // 2)
        for s in (range(NSEQ) if self.mutant == "lse_outside" else seqs):
            n = self.computed(s)
            t[s, :, :n] = lse[s, :, :n]

    def backward(self, seqs=None, order=None):
        lay, c = self.lay, self.lay.c
        seqs = list(range(NSEQ)) if seqs is None else list(seqs)
        D, S = lay.D, lay.S
        val = lay.ref["dqkv"][0].clone()
        # what the launch reads of out: through ld_out — or through the stride the mutant takes for it
        ld_read = lay.ld["dout"] if self.mutant == "out_ld_dout" else lay.ld["out"]
        o_read, o_true = torch.zeros(NSEQ, S, D), torch.zeros(NSEQ, S, D)
        for s in seqs:
            n = self.computed(s)
            rows = self.prow(s, torch.arange(n))
            o_read[s, :n] = _load(lay.g["out"], rows, D, ld_read)
            o_true[s, :n] = _load(lay.g["out"], rows, D, lay.ld["out"])
        if not torch.equal(o_read.view(torch.int32), o_true.view(torch.int32)):
            sc = c.hd ** -0.5
            P = lay.ref["probs"][0]
            Q, K = (A._heads(lay.qkv[..., i * D:(i + 1) * D], H) for i in range(2))
            d_delta = (A._heads(o_read - o_true, H) * A._heads(lay.dout, H)).sum(-1)            # [nseq, H, S]
            ds = -P * d_delta[..., None]
            val[..., :D] += A._unheads(sc * (ds @ K))
            val[..., D:2 * D] += A._unheads(sc * (ds.transpose(-1, -2) @ Q))
        val = val.to(c.dtype)
        g = lay.g["dqkv"]
        ld = lay.ld["qkv"] if self.mutant == "dqkv_ld_qkv" else lay.ld["dqkv"]
        if c.qlim:
            g.view[:, :D] = 0                                                      # the wrapper's fill
        for s in (order or seqs):
            n = lay.lens[s]
            self._tiles(g, s, val[s, :, :D], ld, self.computed(s))
            self._tiles(g, s, val[s, :, D:], ld, n, col0=D)
        if "dbias" in lay.flat:
            f = lay.flat["dbias"]
            f.t.zero_()                                                            # the wrapper's fill
            flat, base = f.g.buf.view(-1), f.g.pre * f.g.ld
            row0 = base + torch.arange(NSEQ * H * S)[:, None] * S
            if self.mutant == "dbias_pad":                                         # keys S .. s_pad of every row: the next row's first columns
                s_pad = (S + 31) & ~31
                flat[row0 + torch.arange(S, s_pad)[None, :]] = 0.0
            flat[row0 + torch.arange(S)[None, :]] = lay.ref["dbias"][0].float().reshape(NSEQ * H * S, S)
        if "d_sp_table" in lay.flat:
            ft, fv = lay.flat["d_sp_table"], lay.flat["d_virt"]
            ft.t += lay.ref["d_sp_table"][0].float()
            virt = lay.ref["d_virt"][0].float()
            if self.mutant == "virt_to_table":                                     # bin num_spatial flushed as a row of the table
                flat, base = ft.g.buf.view(-1), ft.g.pre * ft.g.ld
                flat[base + ft.t.numel() + torch.arange(H)] = virt
            else:
                fv.t += virt


def run(sp, mutant=None, launch="both", **kw):
    """The emulated launches of a "train" / "qlim" case and their checks; raises what check_layout raises, returns the layout."""
    lay = Layout(sp.case, sp.tm)
    e = Emulated(lay, mutant)
    e.forward(**kw)
    if launch in ("both", "fwd"):
        check_layout(lay, Y.FWD_OUT, what=f"{sp.id} fwd")
    e.backward(**kw)
    if launch in ("both", "bwd"):
        check_layout(lay, Y.BWD_OUT, interior=sp.kind != "qlim", what=f"{sp.id} bwd")
    return lay


def spec(id_):
    return next(s for s in Y.SPECS if s.id == id_)


# ------------------------------------------------------------------------------------------------ the faithful emulation
@pytest.mark.parametrize("sp", [s for s in Y.SPECS if s.kind in ("train", "qlim")], ids=lambda s: s.id)
def test_faithful_emulation_is_accepted(sp):
    lay = run(sp)
    assert sp.fwd == A.fwd_route(sp.case.dtype, sp.case.hd, sp.case.S, sp.case.mode)
    assert sp.bwd == A.bwd_route(sp.case.dtype, sp.case.hd, sp.case.S, sp.case.mode, sp.case.p, sp.case.qlim)
    assert set(Y.forced_routes(sp)) == set(sp.forced) - {sp.bwd} or sp.forced == A.ROUTES      # the listed routes can be honoured
    for name in ("qkv", "dout"):
        assert lay.g[name].untouched()
    assert_cap(sp, lay)


def test_faithful_emulation_of_the_bins_case():
    sp = spec("bf16-bins")
    lay = Layout(sp.case)
    bins = Y.bins_of(sp)
    assert all(len(ids) == 1 for ids, _ in bins)
    for ids, _ in bins:
        lay.fresh("out", "lse", "dqkv")
        e = Emulated(lay)
        e.forward(ids)
        check_layout(lay, Y.FWD_OUT, seqs=ids, values=False, what=f"bin {ids} fwd")
        e.backward(ids)
        check_layout(lay, Y.BWD_OUT, seqs=ids, values=False, what=f"bin {ids} bwd")
    lay.fresh("out", "lse", "dqkv")
    for ids, _ in bins:
        Emulated(lay).forward(ids)
    check_layout(lay, Y.FWD_OUT, what="both bins fwd")
    for ids, _ in bins:
        Emulated(lay).backward(ids)
    check_layout(lay, Y.BWD_OUT, what="both bins bwd")
    assert_cap(sp, lay)


@pytest.mark.parametrize("sp", [s for s in Y.SPECS if s.kind == "weights"], ids=lambda s: s.id)
def test_faithful_emulation_of_the_non_training_outputs(sp):
    lay = Layout(sp.case, sp.tm, want_bwd=False)
    S = sp.case.S
    for name, shape in (("probs", (NSEQ, H, S, S)), ("scores", (NSEQ, H, S, S)), ("mean_probs", (NSEQ, S, S))):
        lay.add_flat(name, shape).copy_(lay.ref[name][0].float())
    check_layout(lay, ("probs", "scores", "mean_probs"), what=sp.id)
    assert_cap(sp, lay, want_bwd=False)
    if sp.case.mode == "struct":
        v, _ = A.reference_graph_bias(*(lay.kw[k] for k in ("attn_bias", "spatial_pos", "sp_table", "virt")))
        lay.add_flat("graph_bias", (NSEQ, H, S, S)).copy_(v.float())
        Y.check_graph_bias(lay, sp.id)
        lay.flat["graph_bias"].g.buf[2, 0] = 0.0                      # one element past the end
        with pytest.raises(AssertionError, match="before / after"):
            Y.check_graph_bias(lay, sp.id)


# ------------------------------------------------------------------------------------------------ the exclusion cap
def assert_cap(sp, lay, want_bwd=True):
    ex = Y.excluded(lay, want_bwd)
    if sp.kind != "qlim":
        assert max(ex.values()) <= Y.EXCLUSION_CAP, ex
        return
    q = sp.case.qlim
    assert ex["dqkv"] == 0.0
    assert torch.equal(lay.exists & ~lay.ref["valid"], lay.exists & (torch.arange(sp.case.S)[None, :] >= q)), "more than the ABI's unspecified rows is left out"
    whole = Layout(sp.case._replace(qlim=0), sp.tm)
    assert max(Y.excluded(whole).values()) == 0.0


# ------------------------------------------------------------------------------------------------ the mutants
def rejected(match=None):
    return pytest.raises(AssertionError, match=match)


def test_mutant_out_read_with_ld_dout():
    """bf16 S = 33: the backward's rows of `out` taken with dout's stride meet other rows and the padding's NaNs."""
    with rejected("dqkv"):
        run(spec("bf16-S33-none-drop"), "out_ld_dout", "bwd")


def test_mutant_dqkv_written_with_ld_qkv():
    with rejected("dqkv: a padding column|dqkv: physical rows"):
        run(spec("bf16-S33-none-drop"), "dqkv_ld_qkv", "bwd")


def test_mutant_seq_stride_taken_as_S():
    """Batch-major with gaps: sequence 1 lands three rows early, on the gap rows after sequence 0."""
    with rejected("out: physical rows"):
        run(spec("fp32-S33-none-drop-gaps"), "seq_stride_S", "fwd")


def test_mutant_whole_last_tile_spills_into_the_next_sequence():
    """Ragged (33, 16): rows 33 .. 47 of sequence 0's last tile are sequence 1's rows.  Stored after sequence 1 they destroy its
    values; stored before, sequence 1 overwrites them and nothing shows (the race) — a launch of sequence 0 alone, as one
    length bin into fresh buffers, shows it whatever the order."""
    sp = spec("bf16-ragged-33")
    with rejected():
        run(sp, "spill", "fwd", order=[1, 0])
    with rejected():
        run(sp, "spill", "bwd", order=[1, 0])
    run(sp, "spill", order=[0, 1])                                   # hidden: why the bins case launches each bin alone
    sp = spec("bf16-bins")
    lay = Layout(sp.case)
    (short, _), (long_, _) = Y.bins_of(sp)
    Emulated(lay, "spill").forward(long_)
    with rejected("out: physical rows"):
        check_layout(lay, Y.FWD_OUT, seqs=long_, values=False)
    Emulated(lay, "spill").backward(long_)
    with rejected("dqkv: physical rows"):
        check_layout(lay, Y.BWD_OUT, seqs=long_, values=False)


def test_mutant_whole_last_tile_spills_past_the_last_row():
    """The last sequence of the bins case has 47 rows: row 47 of its last tile is past the end of the tensor; and the dense
    batch-major case, where the tile runs over the gap rows into the band."""
    sp = spec("bf16-bins")
    lay = Layout(sp.case)
    (short, _), _ = Y.bins_of(sp)
    Emulated(lay, "spill").forward(short)
    with rejected("out: a padding column or a byte before / after"):
        check_layout(lay, Y.FWD_OUT, seqs=short, values=False)
    Emulated(lay, "spill").backward(short)
    with rejected("dqkv: a padding column or a byte before / after"):
        check_layout(lay, Y.BWD_OUT, seqs=short, values=False)
    with rejected("out: a padding column or a byte before / after"):
        run(spec("fp32-S33-none-drop-gaps"), "spill", "fwd")


def test_mutant_lse_of_a_sequence_outside_seq_ids():
    sp = spec("bf16-bins")
    lay = Layout(sp.case)
    (short, _), _ = Y.bins_of(sp)
    Emulated(lay, "lse_outside").forward(short)
    with rejected("lse: .* outside the launch's write set"):
        check_layout(lay, Y.FWD_OUT, seqs=short, values=False)


def test_mutant_graph_token_bin_flushed_into_the_table():
    with rejected("d_sp_table: a byte before / after"):
        run(spec("fp32-S33-struct-tm"), "virt_to_table", "bwd")


def test_mutant_dense_dbias_stored_for_padded_keys():
    with rejected("dbias: a byte before / after"):
        run(spec("bf16-S33-dense"), "dbias_pad", "bwd")


@pytest.mark.parametrize("id_", ("bf16-S33-none-drop", "fp32-S33-none-drop-gaps"))
def test_mutant_vector_store_over_the_padding_columns(id_):
    with rejected("out: a padding column"):
        run(spec(id_), "pad_hit", "fwd")


def test_cases_sit_on_the_geometries_they_are_there_for():
    """What the case table promises beyond the route name, by the routing mirror of attention_reference.py (which
    tests/test_attention_plan_cpu.py holds against the library): the v2 forward on 8 waves and on its last rung, v3 on 512 threads,
    the bins on both sides of the one-pass families."""
    assert A.fwd_rung("v2", 33, "none") == (4, 4) and A.fwd_rung("v2", 145, "none") == (13, 8) and A.fwd_rung("v2", 209, "none") == (17, 8)
    assert A.bwd_rung("v3", 64, 209) == (256, 512) and A.bwd_rung("v3", 64, 33, mode="struct") == (64, 256)
    S, lens, cap = A.BINS[0]
    assert [A.bwd_route(BF, 64, S, "none", A.P_DROP, 0, c) for c in (cap, S)] == ["v4x", "v5"]
    assert {s.case.hd for s in Y.SPECS} == {16, 64, 96, 128} and {s.case.dtype for s in Y.SPECS} == {F32, BF}


def test_strides_are_distinct_and_vector_aligned():
    lay = Layout(spec("bf16-S33-none-drop").case)
    assert len(set(Y.PAD.values())) == 4 and all(p * 2 % 16 == 0 for p in Y.PAD.values())
    assert len({lay.ld[k] - lay.width[k] for k in lay.ld}) == 4
    for k, g in lay.g.items():
        assert g.view.stride(0) == lay.ld[k] and g.view.data_ptr() % 16 == 0
        assert (g.buf.shape[0] - g.pre) * g.ld >= lay.rows * (3 * lay.D + 32)
    dense = Layout(spec("fp32-S33-none-drop-gaps").case)
    assert dense.seq_stride == 33 + Y.GAP and dense.rows == NSEQ * 36
    ws = dense.write_set()
    assert int(ws["out"][:, 0].sum()) == NSEQ * 33 and not bool(ws["out"][33:36].any()) and not bool(ws["out"][69:].any())
