"""The attention routing table, checked over its whole domain without a device: mdt_attention_route (attn_plan of
csrc/attention.hip behind the argument checks, nothing launched, no pointer followed) against the independent restatement
in tests/attention_reference.py — fwd_route, bwd_route, fwd_rung, bwd_rung, refusal.

The grid: dtype {fp32, bf16} x head width {16, 64, 96, 128} x every S in 1 .. 288 and 320, 700 x bias mode {none, mask, dense,
struct} x dropout {0, 0.25} x q_limit {0, 9} x layout {padded, ragged, ragged as one length bin with s_cap on every tile
edge <= S at which a ladder or the family changes} x MDT_ATTN_BWD {unset, v1 .. v5} for the backward.  A ragged launch takes
no masks or biases (an argument error, not a routing decision: asserted once), so the ragged layouts run in mode "none".
The pointers of the argument blocks are non-null, 16-byte aligned integers.

Refusals.  "bins" and "long" (refusal() of the reference) occur inside the grid and must be refused by both sides; a head
width outside the four and a v3 launch whose histogram does not fit LDS lie outside it and are asserted with the others'
messages in test_refusal_messages.  Two more refusals of attn_plan — a whole-row route past 272 tokens, the v2 backward past
112 keys — cannot be reached through the ABI (S > 272 goes to the key-chunked path first, and the v2 backward is only ever
chosen or forced for S <= 112): they guard the ladder lookups and have no case.
"""
import ctypes as C
import os

import pytest
import torch

import tests.attention_reference as A

BF, F32 = torch.bfloat16, torch.float32
NSEQ, H, NUM_SPATIAL = 2, 3, 24
PTR = 0x7000_0000_1000                                 # non-null, 16-byte aligned, never followed
SIZES = tuple(range(1, 289)) + (320, 700)
CAPS = (32, 64, 80, 96, 112, 128, 144, 208, 256, 272)   # tile edges where a ladder rung (v2), the family (v4x | v4 | v5 | v3) or v3's form changes
FORCED = (None,) + A.ROUTES
UNSUPPORTED = -2                                       # MDT_ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def ops():
    from multimodaldiscussiontransformer_amd import ops as o
    return o


@pytest.fixture
def force(ops):
    """MDT_ATTN_BWD in the environment, applied with mdt_reload_env; restored on the way out."""
    before = os.environ.get("MDT_ATTN_BWD")

    def set_(route):
        if route:
            os.environ["MDT_ATTN_BWD"] = route
        else:
            os.environ.pop("MDT_ATTN_BWD", None)
        ops.L.reload_env()
    yield set_
    set_(before)


def block(ops, dtype, hd, S, mode, p=0.0, qlim=0, ragged=False, cap=0, num_spatial=NUM_SPATIAL):
    """The argument block of a backward launch (its .f is the forward's) over dummy pointers."""
    b = ops.L.AttnBwdArgs()
    a = b.f
    D = H * hd
    a.dtype = ops.L.MDT_BF16 if dtype == BF else ops.L.MDT_F32
    a.nseq, a.S, a.H, a.hd = NSEQ, S, H, hd
    a.seq_stride, a.pos_stride, a.scale = S, 1, hd ** -0.5
    a.qkv, a.ld_qkv, a.out, a.ld_out, a.lse = PTR, 3 * D, PTR, D, PTR
    b.dout, b.ld_dout, b.dqkv, b.ld_dqkv = PTR, D, PTR, 3 * D
    a.drop_p, a.drop_seed, a.q_limit = p, 7, qlim
    if mode == "mask":
        a.key_mask = PTR
    elif mode == "dense":
        a.dense_bias = b.d_dense_bias = PTR
    elif mode == "struct":
        a.attn_bias = a.spatial_pos = a.sp_table = a.virt = a.key_pad = PTR
        a.num_spatial = num_spatial
        b.d_sp_table = b.d_virt = PTR
    if ragged:
        a.seq_offsets = PTR
    if cap:
        a.seq_ids, a.s_cap, a.nseq_total = PTR, cap, NSEQ
    return b


def expected(bwd, dtype, hd, S, mode, p, qlim, cap, forced):
    """(route, geometry) by the reference."""
    if not bwd:
        r = A.fwd_route(dtype, hd, S, mode)
        g = A.fwd_rung(r, S, mode, cap)
        return r, (g if isinstance(g, tuple) else (g, 0))
    r = A.bwd_route(dtype, hd, S, mode, p, qlim, cap, forced if dtype == BF else None)
    g = A.bwd_rung(r, hd, S, cap, mode)
    return r, (g if isinstance(g, tuple) else (g, 0))


def layouts(S, mode):
    yield False, 0
    if mode == "none":
        yield True, 0
        for cap in CAPS:
            if cap <= S:
                yield True, cap


def test_route_table_over_the_whole_domain(ops, force):
    compared, refused = 0, {}
    seen = {False: set(), True: set()}
    # the raw entry with one result buffer, not ops.attention_route (the tests below go through that): 760 000 calls
    name, geo, query = C.create_string_buffer(16), (C.c_int32 * 2)(), ops.lib.mdt_attention_route
    for forced in FORCED:
        force(forced)
        for dtype in (F32, BF):
            for hd in A.WIDTHS:
                for S in SIZES:
                    for mode in ("none", "mask", "dense", "struct"):
                        for ragged, cap in layouts(S, mode):
                            for qlim in (0, 9):
                                why = A.refusal(dtype, hd, S, qlim, ragged, cap)
                                b = block(ops, dtype, hd, S, mode, 0.0, qlim, ragged, cap)
                                for p in (0.0, 0.25):
                                    b.f.drop_p = p
                                    for bwd in ((True,) if forced else (False, True)):      # the forward knows no forcing
                                        compared += 1
                                        status = query(C.byref(b), bwd, name, 16, geo)
                                        got = (name.value.decode(), (geo[0], geo[1]))
                                        if why:
                                            assert (status, got) == (UNSUPPORTED, ("", (0, 0))), (why, status, got, dtype, hd, S, mode, p, qlim, ragged, cap)
                                            refused[why] = refused.get(why, 0) + 1
                                            continue
                                        want = expected(bwd, dtype, hd, S, mode, p, qlim, cap, forced)
                                        if status != 0 or got != want:
                                            pytest.fail(f"{'bwd' if bwd else 'fwd'} {dtype} hd{hd} S={S} {mode} p={p} q{qlim} ragged={ragged} cap={cap} "
                                                        f"MDT_ATTN_BWD={forced}: library {got} (status {status}), reference {want}")
                                        seen[bwd].add(want[0])
    print(f"{compared} grid points compared, {sum(refused.values())} of them refusals {refused}")
    assert compared > 500_000                           # comparing nothing is not a pass
    assert seen[False] == {"v1", "v2", "long"}, seen[False]
    assert seen[True] == {"v1", "v2", "v3", "v4", "v4x", "v5", "long"}, seen[True]
    assert set(refused) == {"bins", "long"} and min(refused.values()) > 100, refused


def test_forced_routes_are_taken_where_they_may_be(ops, force):
    """Every route name can be forced somewhere and is refused (the default runs) somewhere else: the forcing column of the
    grid above is no column of defaults."""
    for forced in A.ROUTES:
        force(forced)
        took = {S: ops.attention_route(block(ops, BF, 64, S, "none", 0.25), True)[0] for S in (40, 104, 201, 261)}
        assert forced in took.values(), (forced, took)
        assert any(A.bwd_route(BF, 64, S, "none", 0.25) != forced for S in took)
        assert ops.attention_route(block(ops, F32, 64, 104, "none", 0.25), True)[0] == "v1"      # fp32 is never forced


def test_refusal_messages(ops, force):
    """One message per refusal kind, with the texts the GPU tests match; a refused block leaves no route behind."""
    force(None)
    cases = {
        "bins": (block(ops, BF, 128, 40, "none", ragged=True, cap=40), "seq_ids / s_cap are for ragged bf16 launches with head_dim 64"),
        "bins fp32": (block(ops, F32, 64, 40, "none", ragged=True, cap=40), "seq_ids / s_cap are for ragged bf16 launches with head_dim 64"),
        "head_dim bf16": (block(ops, BF, 32, 40, "none"), r"attention\(bf16\): head_dim 32 unsupported \(16, 64, 96 or 128\)"),
        "head_dim fp32": (block(ops, F32, 80, 40, "none"), r"attention: head_dim 80 unsupported \(16, 64, 96 or 128\)"),
        "head_dim long": (block(ops, BF, 32, 300, "none"), r"attention \(long sequences\): head_dim 32 unsupported"),
        "long ragged": (block(ops, BF, 64, 300, "none", ragged=True), "exceeds the 272-token limit of the single-pass kernels and the key-chunked path takes neither"),
        "long q_limit": (block(ops, F32, 64, 273, "struct", qlim=9), "takes neither ragged sequences nor q_limit"),
        # v3 with 128-wide heads at 272 tokens: two 288-row images and three rows of floats leave 3712 bytes for the histogram
        "v3 LDS": (block(ops, BF, 128, 272, "struct", num_spatial=1000), r"attention_bwd_v3: S=272 needs 164144 bytes of LDS"),
    }
    for kind, (b, text) in cases.items():
        for bwd in ((True,) if kind == "v3 LDS" else (False, True)):
            with pytest.raises(ops.L.MdtUnsupported, match=text):
                ops.attention_route(b, bwd)
    assert ops.attention_route(cases["v3 LDS"][0], False)[0] == "v2"           # the forward of that launch runs
    assert ops.attention_route(block(ops, BF, 128, 272, "struct", num_spatial=900), True) == ("v3", (288, 256))
    # what the argument checks refuse is an argument error here too, before any plan: a ragged launch with a mask, a null pointer
    for b in (block(ops, BF, 64, 40, "mask", ragged=True), block(ops, BF, 64, 40, "none")):
        if not b.f.seq_offsets:
            b.dout = None
        with pytest.raises(ops.L.MdtError) as e:
            ops.attention_route(b, True)
        assert e.value.status == -1, e.value


def test_row_alignment_of_every_row_tensor(ops, force):
    """qkv, out, dout and dqkv each get the rule the widest access to them needs (include/mdt_hip.h): in bf16 a base on a
    16-byte boundary and a row stride of a multiple of 8 elements — out and dqkv are stored in 16-byte vectors as qkv and dout
    are loaded in them; in fp32, where every kernel moves one element at a time, only the base on an element boundary.
    Refused blocks name the tensor; they are only ever routed, never launched."""
    force(None)
    hd, S = 64, 40
    D = H * hd

    def shifted(dtype, **fields):
        b = block(ops, dtype, hd, S, "none", 0.25)
        for k, v in fields.items():
            setattr(b.f if k in ("qkv", "ld_qkv", "out", "ld_out") else b, k, v)
        return b

    whole = {bwd: ops.attention_route(block(ops, BF, hd, S, "none", 0.25), bwd) for bwd in (False, True)}
    refused = {"ld_out": (dict(ld_out=D + 4), r"attention\(bf16\): out must be 16-byte aligned rows", (False, True)),
               "out": (dict(out=PTR + 8), r"attention\(bf16\): out must be 16-byte aligned rows", (False, True)),
               "ld_dqkv": (dict(ld_dqkv=3 * D + 4), r"attention_bwd\(bf16\): dqkv must be 16-byte aligned rows", (True,)),
               "dqkv": (dict(dqkv=PTR + 8), r"attention_bwd\(bf16\): dqkv must be 16-byte aligned rows", (True,)),
               "ld_qkv": (dict(ld_qkv=3 * D + 4), r"attention\(bf16\): qkv must be 16-byte aligned rows", (False, True)),
               "ld_dout": (dict(ld_dout=D + 4), r"attention_bwd\(bf16\): dout must be 16-byte aligned rows", (True,))}
    for kind, (fields, text, launches) in refused.items():
        for bwd in launches:
            with pytest.raises(ops.L.MdtError, match=text) as e:
                ops.attention_route(shifted(BF, **fields), bwd)
            assert e.value.status == -1, (kind, e.value)
    # the backward block's own tensors do not concern the forward
    assert ops.attention_route(shifted(BF, ld_dqkv=3 * D + 4, dqkv=PTR + 8), False) == whole[False]
    # + 8 elements and + 16 bytes: accepted, and routed as the contiguous block is
    for fields in (dict(ld_out=D + 8), dict(ld_dqkv=3 * D + 8), dict(out=PTR + 16, dqkv=PTR + 16),
                   dict(ld_qkv=3 * D + 8, ld_out=D + 16, ld_dout=D + 24, ld_dqkv=3 * D + 32)):
        for bwd in (False, True):
            assert ops.attention_route(shifted(BF, **fields), bwd) == whole[bwd], fields
    # fp32: any row stride and any element-aligned base; half an element off is refused
    whole32 = {bwd: ops.attention_route(block(ops, F32, hd, S, "none", 0.25), bwd) for bwd in (False, True)}
    for fields in (dict(ld_out=D + 4), dict(ld_dqkv=3 * D + 4), dict(out=PTR + 8, dqkv=PTR + 8), dict(ld_out=D + 1, ld_dqkv=3 * D + 3, ld_qkv=3 * D + 1, ld_dout=D + 5),
                   dict(qkv=PTR + 4, dout=PTR + 12)):
        for bwd in (False, True):
            assert ops.attention_route(shifted(F32, **fields), bwd) == whole32[bwd], fields
    for name, launches in (("qkv", (False, True)), ("out", (False, True)), ("dout", (True,)), ("dqkv", (True,))):
        for bwd in launches:
            with pytest.raises(ops.L.MdtError, match=rf"\(fp32\): {name} must be 4-byte aligned"):
                ops.attention_route(shifted(F32, **{name: PTR + 2}), bwd)
    # a row stride below the width is refused for dout as for the others
    with pytest.raises(ops.L.MdtError, match="ld_dout too small"):
        ops.attention_route(shifted(BF, ld_dout=D - 8), True)


def test_fp32_wide_heads_fall_back_to_the_key_chunked_backward(ops, force):
    """The one line of the table the launchers used to hide: fp32, head width 96 | 128, the 17-tile rung (S 209 .. 272),
    structural bias and dropout — the backward takes "long", the forward and every neighbour of that point v1."""
    force(None)
    for hd in (96, 128):
        for S in (209, 257, 272):
            assert ops.attention_route(block(ops, F32, hd, S, "struct", 0.25), True) == ("long", (0, 0))
            assert ops.attention_route(block(ops, F32, hd, S, "struct", 0.25), False) == ("v1", (17, 0))
            assert ops.attention_route(block(ops, F32, hd, S, "struct", 0.0), True) == ("v1", (17, 0))
            assert ops.attention_route(block(ops, F32, hd, S, "mask", 0.25), True) == ("v1", (17, 0))
            assert ops.attention_route(block(ops, F32, 64, S, "struct", 0.25), True) == ("v1", (17, 0))
        assert ops.attention_route(block(ops, F32, hd, 208, "struct", 0.25), True) == ("v1", (13, 0))
        assert ops.attention_route(block(ops, F32, hd, 273, "struct", 0.25), True) == ("long", (0, 0))
