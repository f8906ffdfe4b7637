"""Where an attention launch reads and writes: guarded, strided buffers for the four row tensors of the attention ABI (qkv,
out, dout, dqkv; include/mdt_hip.h) and for its flat fp32 outputs, the write set of a launch, and the check that holds a launch
to it.  Pure torch: no device and no native library are needed (tests/test_attention_layout_cpu.py drives an emulated launch
through it, tests/test_attention_layout_gpu.py the kernels).

Strides.  Every row tensor has its own row stride, natural width + PAD[name] elements: four different numbers, each a multiple
of 16 bytes in fp32 and in bf16, so a kernel body that takes one tensor's stride for another's addresses other rows.
Everything that is not an operand holds a NaN bit pattern (gemm_reference.Guarded): the padding columns of qkv and dout, the
rows between two sequences, the bands before and after every buffer.  A read with the wrong stride meets NaNs; a write with
the wrong stride, or past a sequence's length, changes a sentinel.  Every row buffer, counted from its first row to the end of
its trailing band, holds at least rows x (3 D + 32) elements — the reach of the widest of the four strides — so a kernel that
takes any of the other three still writes inside the buffer: a failed assertion, not a fault.

Layouts.  Batch-major dense cases put GAP = 3 rows between the sequences (seq_stride = S + 3; the rows after the last sequence
too); time-major cases interleave the sequences (seq_stride 1, pos_stride nseq); ragged cases pack them (seq_offsets).

Write set (write_set): rows below the length of the sequences the launch names, columns below the tensor's width; lse[seq, :, :S]
of those sequences; d_dense_bias[seq] of those sequences; all of d_sp_table and d_virt.  Rows at or past q_limit and lse
positions past a ragged length are inside it (the ABI leaves them unspecified, not forbidden).  Everything else — padding
columns, gap rows, bands, whole sequences a length-bin launch does not name — must still hold the sentinel bit for bit.

Values.  check_layout hands the logical tensors to attention_reference.check: the same fp64 bounds as every other attention
test, no tolerance of its own.
"""
from __future__ import annotations

from collections import namedtuple

import torch

import tests.attention_reference as A
from tests.attention_reference import BF, F32, Case
from tests.gemm_reference import Guarded

NSEQ, H = A.NSEQ, A.HEADS
PAD = {"qkv": 8, "out": 16, "dout": 24, "dqkv": 32}
GAP = 3
TILE = 16
EXCLUSION_CAP = 0.05
TENSORS = ("key_mask", "key_pad", "dense_bias", "attn_bias", "spatial_pos", "sp_table", "virt")
FWD_OUT, BWD_OUT = ("out", "lse"), ("dqkv", "dbias", "d_sp_table", "d_virt")


def name_of(dtype):
    return "bf16" if dtype == BF else "fp32"


class Flat:
    """A contiguous fp32 tensor of ``shape`` with a band of its own size before and after it (Guarded with one row).  ``zero``:
    the tensor starts as zeros (what a launch accumulates into), the bands keep the sentinel."""

    def __init__(self, shape, device, zero=False):
        n = 1
        for s in shape:
            n *= s
        self.g = Guarded(1, n, F32, device, pre=1, post=1)
        self.t = self.g.view.view(*shape)
        if zero:
            self.t.zero_()

    def untouched(self):
        return self.g.untouched()

    def sentinel(self):
        return self.t.view(self.g.itype) == self.g.bits


class Layout:
    """One case (attention_reference.Case) laid out for a launch: the guarded row buffers, the flat outputs, the launch's
    layout arguments, and the way from physical rows back to logical [nseq, S, width] tensors."""

    def __init__(self, c: Case, tm=False, device="cpu", want_bwd=True):
        assert not (tm and c.lens)
        self.c, self.tm, self.device = c, tm, device
        self.qkv, self.dout, self.kw, self.ref = A.case_reference(c, want_bwd)
        S, D = c.S, H * c.hd
        self.S, self.D = S, D
        self.lens = tuple(c.lens) if c.lens else (S,) * NSEQ
        pos = torch.arange(S)
        if c.lens:
            self.off = torch.tensor([0] + [sum(self.lens[:i + 1]) for i in range(NSEQ)], dtype=torch.int32)
            self.seq_stride, self.pos_stride, self.rows = 0, 1, int(self.off[-1])
            row = self.off[:NSEQ, None].long() + pos[None, :]
            self.lay = dict(seq_offsets=self.off.to(device))
        elif tm:
            self.seq_stride, self.pos_stride, self.rows = 1, NSEQ, S * NSEQ
            row = torch.arange(NSEQ)[:, None] + pos[None, :] * NSEQ
            self.lay = dict(seq_stride=1, pos_stride=NSEQ)
        else:
            self.seq_stride, self.pos_stride, self.rows = S + GAP, 1, NSEQ * (S + GAP)
            row = torch.arange(NSEQ)[:, None] * (S + GAP) + pos[None, :]
            self.lay = dict(seq_stride=S + GAP, pos_stride=1)
        self.exists = pos[None, :] < torch.tensor(self.lens)[:, None]              # [nseq, S]: the rows there are
        self.row = torch.where(self.exists, row, torch.full_like(row, -1))         # [nseq, S] -> physical row
        self.width = {"qkv": 3 * D, "out": D, "dout": D, "dqkv": 3 * D}
        self.ld = {k: w + PAD[k] for k, w in self.width.items()}
        reach = self.rows * (3 * D + PAD["dqkv"])
        self.g = {}
        for k, w in self.width.items():
            # first row .. end of the band >= reach, and a whole query tile of every sequence past the last row (time-major: NSEQ rows
            # per position) still lands in the band
            post = -(-reach // self.ld[k]) - self.rows + TILE * NSEQ + 1
            self.g[k] = Guarded(self.rows, w, c.dtype, device, ld=self.ld[k], pre=2, post=post)
            assert (self.rows + post) * self.ld[k] >= reach + TILE * NSEQ * self.ld[k]
        for k, t in (("qkv", self.qkv), ("dout", self.dout)):
            self.g[k].view[self.row[self.exists].to(device)] = t[self.exists].to(c.dtype).to(device)
        self.flat = {"lse": Flat((NSEQ, H, S), device)}
        if want_bwd and c.mode == "dense":
            self.flat["dbias"] = Flat((NSEQ, H, S, S), device)
        if want_bwd and c.mode == "struct":
            ns = self.kw["sp_table"].shape[0]
            self.flat["d_sp_table"] = Flat((ns, H), device, zero=True)
            self.flat["d_virt"] = Flat((H,), device, zero=True)
        self.args = {k: (v if v.numel() else torch.zeros(1, dtype=v.dtype)).to(device) for k, v in self.kw.items() if k in TENSORS}
        self.args.update({k: v for k, v in self.kw.items() if k in ("drop_p", "drop_seed", "q_limit")})
        self.args["scale"] = c.hd ** -0.5

    # ------------------------------------------------------------------ the launch's tensors
    def view(self, name):
        return self.g[name].view

    def fresh(self, *names):
        """New sentinel-filled buffers for these outputs (what a launch into "fresh buffers" gets)."""
        for k in names:
            if k in self.g:
                g = self.g[k]
                self.g[k] = Guarded(g.rows, g.cols, self.c.dtype, self.device, ld=g.ld, pre=g.pre, post=g.buf.shape[0] - g.pre - g.rows)
            elif k in self.flat:
                self.flat[k] = Flat(tuple(self.flat[k].t.shape), self.device, zero=k in ("d_sp_table", "d_virt"))

    def add_flat(self, name, shape):
        """A further guarded fp32 output (the non-training ones: probs, scores, mean_probs, graph_bias)."""
        self.flat[name] = Flat(tuple(shape), self.device)
        return self.flat[name].t

    def logical(self, name):
        """[nseq, S, width] fp32 on the host from the physical rows (zeros where a ragged sequence has no row)."""
        v = self.g[name].view.float().cpu()
        out = torch.zeros(NSEQ, self.S, v.shape[1])
        out[self.exists] = v[self.row[self.exists]]
        return out

    def got(self, names):
        return {k: (self.logical(k) if k in self.g else self.flat[k].t.cpu()) for k in names if k in self.g or k in self.flat}

    # ------------------------------------------------------------------ the write set
    def write_set(self, seqs=None):
        """{output: bool mask of the elements a launch over the sequences ``seqs`` (None: all) may write}: [rows, width] over the
        view of out / dqkv, the tensor's own shape for the flat outputs."""
        seqs = list(range(NSEQ)) if seqs is None else [int(s) for s in seqs]
        rows = torch.zeros(self.rows, dtype=torch.bool)
        for s in seqs:
            rows[self.row[s][self.exists[s]]] = True
        m = {k: rows[:, None].expand(self.rows, self.width[k]).clone() for k in ("out", "dqkv")}
        for k, f in self.flat.items():
            fm = torch.zeros(f.t.shape, dtype=torch.bool)
            if k in ("d_sp_table", "d_virt"):
                fm[...] = True
            else:
                fm[seqs] = True
            m[k] = fm
        return m

    def assert_write_set(self, names, seqs=None, interior=True, what=""):
        """Every byte outside the write set of these outputs still holds the sentinel.  ``interior`` False: only what lies
        outside the tensor (bands and padding columns) — for launches whose wrapper fills part of the tensor itself."""
        ws = self.write_set(seqs)
        for k in names:
            if k in self.g:
                g = self.g[k]
                assert g.untouched(), f"{what} {k}: a padding column or a byte before / after the buffer was written"
                if interior:
                    clean = (g.view.view(g.itype) == g.bits).cpu()
                    bad = ~clean & ~ws[k]
                    assert not bool(bad.any()), f"{what} {k}: physical rows {sorted(set(bad.nonzero()[:, 0].tolist()))[:8]} are outside the launch's write set and were written"
            elif k in self.flat:
                f = self.flat[k]
                assert f.untouched(), f"{what} {k}: a byte before / after the tensor was written"
                if interior:
                    bad = ~f.sentinel().cpu() & ~ws[k]
                    assert not bool(bad.any()), f"{what} {k}: {int(bad.sum())} elements outside the launch's write set were written"


def check_layout(lay: Layout, names, seqs=None, values=True, interior=True, what=""):
    """The write set of the launch that just filled ``names`` (assert_write_set), then its values against the fp64 reference
    with the bounds of attention_reference.check.  ``values`` False: a launch over part of the set (one length bin) — the
    reference check wants every sequence.  Returns check()'s worst err / bound per output."""
    lay.assert_write_set(names, seqs, interior, what)
    if not values:
        return {}
    return A.check(lay.got(names), lay.ref, lay.c.dtype, what=what)


def check_graph_bias(lay: Layout, what=""):
    """The materialised structural bias in lay.flat["graph_bias"]: its bands, then reference_graph_bias as the routes test holds it."""
    lay.assert_write_set(("graph_bias",), what=what)
    b = lay.flat["graph_bias"].t.cpu()
    v, d = A.reference_graph_bias(*(lay.kw[k] for k in ("attn_bias", "spatial_pos", "sp_table", "virt")))
    assert bool(((b.double() == v) | torch.isfinite(v)).all()), f"{what}: a -inf entry of the structural bias is not -inf"
    A.assert_within(b, v, A.bound(torch.nan_to_num(v, neginf=0.0), d, F32), what=f"{what} graph_attn_bias", dtype=F32)


def excluded(lay: Layout, want_bwd=True):
    """{output: fraction of its in-bounds elements — the rows that exist, lse positions below the length — that the value check
    leaves out}; the reference's masks decide: out / lse are compared on ref["valid"], dqkv on ref["rows"]."""
    inb = lay.exists
    n = float(inb.sum())
    valid, rows = lay.ref["valid"], lay.ref["rows"]
    ex = {"out": float((inb & ~valid).sum()) / n, "lse": float((inb & ~valid).sum()) / n}
    if want_bwd:
        ex["dqkv"] = float((inb & ~rows).sum()) / n
        for k in lay.flat:
            if k != "lse":
                ex[k] = 0.0
    return ex


# ------------------------------------------------------------------------------------------------ the cases
# kind "train": forward, the default backward and the forced ones; "qlim": the same with q_limit and only bands + values in the
# backward (the wrapper zeroes the dQ third, gap rows included); "bins": A.BINS[0]; "weights": the non-training outputs.
Spec = namedtuple("Spec", "id case tm fwd bwd forced kind")


def _c(dtype, hd, S, mode, p=0.0, qlim=0, lens=None, family=None):
    return Case(dtype, hd, S, mode, family or ("uniform" if p else "soft"), p, qlim, lens)


def specs():
    P = A.P_DROP
    out = [
        Spec("fp32-S33-none-drop-gaps", _c(F32, 64, 33, "none", P), False, "v1", "v1", (), "train"),
        Spec("fp32-S33-struct-tm", _c(F32, 64, 33, "struct"), True, "v1", "v1", (), "train"),
        Spec("bf16-S33-none-drop", _c(BF, 64, 33, "none", P), False, "v2", "v4x", ("v1", "v2", "v3", "v4"), "train"),
        Spec("bf16-S145-none-drop", _c(BF, 64, 145, "none", P), False, "v2", "v5", ("v1", "v3", "v4"), "train"),
        Spec("bf16-S209-none", _c(BF, 64, 209, "none"), False, "v2", "v3", (), "train"),
        Spec("bf16-S33-dense", _c(BF, 64, 33, "dense"), False, "v1", "v1", (), "train"),
        Spec("bf16-S33-struct-tm", _c(BF, 64, 33, "struct"), True, "v2", "v1", ("v2", "v3"), "train"),
    ]
    for dtype in (F32, BF):
        for mode in ("none", "dense"):
            out.append(Spec(f"{name_of(dtype)}-S273-{mode}", _c(dtype, 64, 273, mode), False, "long", "long", (), "train"))
    for hd in (16, 96, 128):
        out.append(Spec(f"bf16-hd{hd}-S33-none", _c(BF, hd, 33, "none"), False, "v2", A.bwd_route(BF, hd, 33, "none"), (), "train"))
    for dtype, (S, lens) in ((F32, A.RAGGED[0]), (BF, A.RAGGED[0]), (BF, A.RAGGED[2])):
        c = _c(dtype, 64, S, "none", P, 0, lens, "soft")
        out.append(Spec(f"{name_of(dtype)}-ragged-{S}", c, False, A.fwd_route(dtype, 64, S, "none"), A.bwd_route(dtype, 64, S, "none", P),
                        A.ROUTES if dtype == BF else (), "train"))
    S, lens, _ = A.BINS[0]
    out.append(Spec("bf16-bins", _c(BF, 64, S, "none", P, 0, lens, "soft"), False, "v2", None, ("v3", "v4", "v5"), "bins"))
    for S in (33, 129):
        out.append(Spec(f"bf16-S{S}-qlim", _c(BF, 64, S, "none", P, A.QLIM, None, "soft"), False, "v2", A.bwd_route(BF, 64, S, "none", P, A.QLIM), (), "qlim"))
    for dtype in (F32, BF):
        out.append(Spec(f"{name_of(dtype)}-S33-struct-tm-weights", _c(dtype, 64, 33, "struct"), True, A.fwd_route(dtype, 64, 33, "struct"), None, (), "weights"))
        out.append(Spec(f"{name_of(dtype)}-S33-mask-weights", _c(dtype, 64, 33, "mask"), False, A.fwd_route(dtype, 64, 33, "mask"), None, (), "weights"))
    return out


SPECS = specs()


def forced_routes(sp: Spec, cap=0):
    """The forced backwards of a case: those of its list that attn_plan may honour (A.bwd_ok) and that are not its default."""
    c = sp.case
    return [r for r in sp.forced if r != sp.bwd and A.bwd_ok(r, c.hd, c.S, c.mode, c.qlim, cap)]


def bins_of(sp: Spec):
    """[(sequence indices, cap), ...] of the bins case: the short bin with its cap, the long one with S."""
    S, lens, cap = A.BINS[0]
    assert sp.case.S == S
    return [([i for i, n in enumerate(lens) if n <= cap], cap), ([i for i, n in enumerate(lens) if n > cap], S)]
