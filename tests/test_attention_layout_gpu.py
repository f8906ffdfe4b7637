"""Where the attention kernels read and write: every route launched on guarded buffers with four different row strides
(tests/attention_layout.py — qkv + 8, out + 16, dout + 24, dqkv + 32 elements, NaN sentinels in every padding column, gap row and
band), its write set asserted bit for bit and its values held to the fp64 bounds of tests/attention_reference.py.  The other
attention suites launch contiguous tensors the wrappers allocate, where ld_qkv == ld_dqkv and ld_out == ld_dout and a store past
a sequence's length lands in memory nobody looks at; tests/test_attention_layout_cpu.py proves on the CPU that this harness
rejects exactly those defects.

Cases (attention_layout.SPECS), nseq = 2, H = 3: the smallest lengths that reach each family and rung edge — v1 in fp32 (batch-major
with gap rows, and time-major with the guarded structural-bias gradient), the v2 forward on 4 and 8 waves and on its last rung,
every backward route at S = 33 and 145, v3 on 512 threads, the dense-bias kernels with a guarded dbias, the key-chunked path in
both types, the three store shapes of the v2 forward (head widths 16, 96, 128), ragged sequences one row past and on a tile
edge, length bins launched one bin at a time, q_limit, and the non-training outputs.  Every launch asserts the route it took.

Not exercised, on purpose: the s_cap promise that a sequence longer than the cap is skipped — that is a launch whose LDS image
is too small for its input, nothing to try on a device.
"""
import pytest
import torch

import tests.attention_layout as Y
import tests.attention_reference as A
from multimodaldiscussiontransformer_amd import _lib as L
from tests.attention_layout import H, NSEQ, Layout, check_layout
from tests.attention_reference import BF
from tests.test_attention_head_dim_gpu import force_bwd, ops  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

REACHED = {"fwd": {}, "bwd": {}}        # route -> the cases that ran it (the report at the end of the file)


def show(tag, worst):
    print(f"[{tag}] err/bound " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def ids_of(bins):
    return None if bins is None else [(torch.tensor(ids, dtype=torch.int32, device="cuda"), cap) for ids, cap in bins]


def forward(ops, lay: Layout, want, tag, bins=None, seqs=None, values=True):
    out, lse = ops.attention_fwd(lay.view("qkv"), NSEQ, lay.S, H, bins=ids_of(bins), out=lay.view("out"), lse=lay.flat["lse"].t, **lay.lay, **lay.args)
    torch.cuda.synchronize()
    route = L.last_route()
    assert route == want, f"{tag}: forward took {route}, expected {want}"
    assert out.data_ptr() == lay.view("out").data_ptr() and lse.data_ptr() == lay.flat["lse"].t.data_ptr()
    REACHED["fwd"].setdefault(route, []).append(tag)
    show(f"{tag} fwd {route}", check_layout(lay, Y.FWD_OUT, seqs, values, what=f"{tag} fwd {route}"))


def backward(ops, lay: Layout, want, tag, bins=None, seqs=None, values=True, interior=True):
    lay.fresh(*Y.BWD_OUT)
    extra = {k: lay.flat[k].t for k in ("d_sp_table", "d_virt") if k in lay.flat}
    dbias = lay.flat["dbias"].t if "dbias" in lay.flat else None
    dqkv, db = ops.attention_bwd(lay.view("dout"), lay.view("qkv"), lay.view("out"), lay.flat["lse"].t, NSEQ, lay.S, H, bins=ids_of(bins),
                                 dqkv=lay.view("dqkv"), dbias=dbias, **lay.lay, **lay.args, **extra)
    torch.cuda.synchronize()
    route = L.last_route()
    assert route == want, f"{tag}: backward took {route}, expected {want}"
    assert dqkv.data_ptr() == lay.view("dqkv").data_ptr() and (dbias is None or db.data_ptr() == dbias.data_ptr())
    REACHED["bwd"].setdefault(route, []).append(tag)
    show(f"{tag} bwd {route}", check_layout(lay, Y.BWD_OUT, seqs, values, interior, what=f"{tag} bwd {route}"))


def inputs_intact(lay):
    for k in ("qkv", "dout"):
        assert lay.g[k].untouched(), f"{k}: the launch wrote into an input's padding or bands"


def train(ops, force_bwd, sp, case=None, interior=True):
    """Forward, the default backward and the forced ones of a case, every launch into fresh guarded outputs."""
    force_bwd(None)
    lay = Layout(case or sp.case, sp.tm, "cuda")
    forward(ops, lay, sp.fwd, sp.id)
    backward(ops, lay, sp.bwd, sp.id, interior=interior)
    for r in (Y.forced_routes(sp) if case is None else ()):
        force_bwd(r)
        backward(ops, lay, r, f"{sp.id} MDT_ATTN_BWD={r}", interior=interior)
    force_bwd(None)
    inputs_intact(lay)
    return lay


@pytest.mark.parametrize("sp", [s for s in Y.SPECS if s.kind == "train"], ids=lambda s: s.id)
def test_write_set_and_strides(ops, force_bwd, sp):
    train(ops, force_bwd, sp)


@pytest.mark.parametrize("sp", [s for s in Y.SPECS if s.kind == "qlim"], ids=lambda s: s.id)
def test_query_limit(ops, force_bwd, sp):
    """q_limit = 9: the forward may write whole 16-row tiles of its sequences and nothing else; the backward's wrapper zeroes the
    dQ third of every physical row, so there only the bands, the padding columns and the values are held.  The same launch
    without the limit runs beside it: together they compare every element."""
    train(ops, force_bwd, sp, interior=False)
    c = sp.case._replace(qlim=0)
    whole = sp._replace(id=sp.id + "-whole", case=c, bwd=A.bwd_route(c.dtype, c.hd, c.S, c.mode, c.p))
    train(ops, force_bwd, whole, case=c)


def test_length_bins_one_bin_at_a_time(ops, force_bwd):
    """A.BINS[0], lengths (129, 47).  Each bin alone, forward and every backward, into fresh buffers: the other bin's rows of out /
    dqkv and its lse[seq] stay sentinel (a tile that runs past 129 rows lands on the short sequence, one that runs past 47 rows
    behind the tensor).  Both bins into one buffer: every value inside its bound.  Against the launch of the whole set without
    bins: the long sequence runs the same kernels at the same geometry either way, so its rows are the same bits; the short
    one runs smaller kernels in its bin (another summation order), so both are held to the same fp64 bounds."""
    sp = next(s for s in Y.SPECS if s.kind == "bins")
    c, S = sp.case, sp.case.S
    bins = Y.bins_of(sp)
    routes = [None] + Y.forced_routes(sp, cap=S)
    assert routes == [None, "v3", "v4", "v5"]
    want = lambda cap, r: A.bwd_route(BF, c.hd, S, c.mode, c.p, 0, cap, r)
    force_bwd(None)
    lay = Layout(c, False, "cuda")
    for ids, cap in bins:
        tag = f"{sp.id} bin {ids} cap {cap}"
        lay.fresh(*Y.FWD_OUT)
        forward(ops, lay, "v2", tag, bins=[(ids, cap)], seqs=ids, values=False)
        for r in routes:
            force_bwd(r)
            backward(ops, lay, want(cap, r), f"{tag} MDT_ATTN_BWD={r}", bins=[(ids, cap)], seqs=ids, values=False)
        force_bwd(None)
    lay.fresh(*Y.FWD_OUT)
    forward(ops, lay, "v2", f"{sp.id} both bins", bins=bins)
    binned = {"out": lay.view("out").clone(), "lse": lay.flat["lse"].t.clone()}
    for r in routes:
        force_bwd(r)
        backward(ops, lay, want(S, r), f"{sp.id} both bins MDT_ATTN_BWD={r}", bins=bins)
        binned[r] = lay.view("dqkv").clone()
    force_bwd(None)
    inputs_intact(lay)
    # the whole set in one launch
    (long_seq,), _ = bins[1]
    rows = lay.row[long_seq][lay.exists[long_seq]].cuda()
    lay.fresh(*Y.FWD_OUT)
    forward(ops, lay, "v2", f"{sp.id} one launch")
    assert torch.equal(lay.view("out")[rows].view(torch.int16), binned["out"][rows].view(torch.int16))
    n = c.lens[long_seq]
    assert torch.equal(lay.flat["lse"].t[long_seq, :, :n].view(torch.int32), binned["lse"][long_seq, :, :n].view(torch.int32))
    for r in routes:
        force_bwd(r)
        one = A.bwd_route(BF, c.hd, S, c.mode, c.p, 0, 0, r)
        backward(ops, lay, one, f"{sp.id} one launch MDT_ATTN_BWD={r}")
        if one == want(S, r):
            assert torch.equal(lay.view("dqkv")[rows].view(torch.int16), binned[r][rows].view(torch.int16)), f"MDT_ATTN_BWD={r}: the long sequence differs"
    force_bwd(None)


@pytest.mark.parametrize("sp", [s for s in Y.SPECS if s.kind == "weights"], ids=lambda s: s.id)
def test_non_training_outputs(ops, force_bwd, sp):
    """mdt_attention_head_weights (probabilities and raw scores), mdt_attention_mean_probs and mdt_graph_attn_bias into guarded
    outputs, reading the strided qkv."""
    force_bwd(None)
    c, S = sp.case, sp.case.S
    lay = Layout(c, sp.tm, "cuda", want_bwd=False)
    forward(ops, lay, sp.fwd, sp.id)
    kw = {k: v for k, v in lay.args.items() if k in Y.TENSORS + ("scale",)}
    q, lse = lay.view("qkv"), lay.flat["lse"].t
    ops.attention_head_weights(q, lse, NSEQ, S, H, out=lay.add_flat("probs", (NSEQ, H, S, S)), **lay.lay, **kw)
    ops.attention_head_weights(q, None, NSEQ, S, H, raw_scores=True, out=lay.add_flat("scores", (NSEQ, H, S, S)), **lay.lay, **kw)
    ops.attention_mean_probs(q, lse, NSEQ, S, H, out=lay.add_flat("mean_probs", (NSEQ, S, S)), **lay.lay, **kw)
    torch.cuda.synchronize()
    show(f"{sp.id}", check_layout(lay, ("probs", "scores", "mean_probs"), what=sp.id))
    assert lay.g["out"].untouched() and lay.flat["lse"].untouched()
    if c.mode == "struct":
        ops.graph_attn_bias(*(lay.args[k] for k in ("attn_bias", "spatial_pos", "sp_table", "virt")), out=lay.add_flat("graph_bias", (NSEQ, H, S, S)))
        torch.cuda.synchronize()
        Y.check_graph_bias(lay, sp.id)
    inputs_intact(lay)


def test_routes_reached_report():
    """Runs last in this file: which cases reached which route; every route of the family must have been reached."""
    if not REACHED["fwd"]:
        return                                      # selected alone: nothing ran before it
    for side in ("fwd", "bwd"):
        for route, tags in sorted(REACHED[side].items()):
            print(f"[reached] {side} {route}: " + "; ".join(tags))
    assert set(REACHED["fwd"]) == {"v1", "v2", "long"}, REACHED["fwd"].keys()
    assert set(REACHED["bwd"]) == {"v1", "v2", "v3", "v4", "v4x", "v5", "long"}, REACHED["bwd"].keys()
