"""The bounds of tests/rowops_reference.py can fail: a CPU emulation of the row movers' arithmetic (fp32, one rounding per
product and per add, the kernels' order of operations, round-to-nearest-even to the storage type; a second variant
contracts every add that follows a product into one FMA) is accepted at every (dtype, D, rows, form) of the GPU matrix
(tests/test_rowops_gpu.py), and each listed mutant of it, a subtly wrong kernel, is rejected at the same shapes.  The
emulation decodes rows with // and % on its own; the reference is the only judge.

The last two tests are about the engine, not the kernels: mdt_row_axpby(accumulate) is a plain read-modify-write, correct
only while no destination row appears twice, and the index vectors the encoder builds are checked for exactly that; then
the vectors themselves (data/geometry.py, fed from the host and from the batch's tensors) against the plain loops of
rowops_reference.reference_text_rows / reference_prune_rows."""
import numpy as np
import pytest
import torch

import tests.rowops_reference as RR
from tests.rowops_reference import bf16, embed_operands, embed_rows, f32, node_operands, scatter_operands

SEED = 9731
DIMS = [(t, D) for t in (f32, bf16) for D in RR.VEC_DIMS[t] + RR.SCALAR_DIMS + (RR.BIG_DIMS[0],)]
CONTRACT = (False, True)


def _id(v):
    return "bf16" if v is bf16 else "f32" if v is f32 else str(v)


def _store(v, dtype, mutant=None):
    if mutant == "truncate" and dtype == bf16:
        return (v.contiguous().view(torch.int32) & ~0xFFFF).view(f32).to(bf16)
    return v.to(dtype)


def _fma(c, x, v):
    """fl(c x + v) for fp32 tensors: the product is exact in fp64; the fp64 sum rounds at 2^-53 before the fp32 rounding,
    far inside every bound."""
    return (c.double() * x.double() + v.double()).to(f32)


def _second_sweep_shift(x, D, w):
    """mutant: from the second sweep of the 64-lane loop on, column c + 1 is read instead of c (the last column wraps)."""
    c = torch.arange(D)
    return x[:, torch.where(c >= 64 * w, (c + 1) % D, c)]


# ------------------------------------------------------------------------------------------------ row_axpby
def emulate_axpby(c: RR.Axpby, contract=False, mutant=None):
    """The destination buffer after the call, computed as the kernels compute it."""
    T = c.dst0.dtype
    D = c.dst0.shape[1]
    w = RR.vn(T, D)
    r = torch.arange(c.nrows)

    def rows(m, limit):
        idx, inner, stride, off = m
        if idx is not None:
            x = idx.long()[r]
            return torch.where(x >= 0, (x + off) % limit, x) if mutant == "off_with_idx" else x
        if mutant == "off_dropped":
            off = 0
        if mutant == "stride0_as_1" and stride == 0:
            stride = 1
        if inner <= 1:
            return r * stride + off
        if mutant == "inner_mod_only":
            return r % inner + off
        return (r // inner) * stride + r % inner + off

    dr = rows(c.d, c.dst0.shape[0])
    if mutant == "neg_dst_row0":
        dr = dr.clamp(min=0)
    live = dr >= 0
    alpha, beta = (c.beta, c.alpha) if mutant == "alpha_beta_swapped" else (c.alpha, c.beta)
    v = torch.zeros(c.nrows, D, dtype=f32)
    started = torch.zeros(c.nrows, dtype=torch.bool)
    for src, m, coef, alias in ((c.a, c.am, alpha, c.a_is_dst), (c.b, c.bm, beta, c.b_is_dst)):
        src = c.dst0 if alias else src
        if src is None:
            continue
        sr = rows(m, src.shape[0])
        if mutant == "neg_src_row0":
            sr = sr.clamp(min=0)
        have = sr >= 0
        x = src.float()[sr.clamp(min=0)]
        if mutant == "second_sweep_col_plus_1":
            x = _second_sweep_shift(x, D, w)
        k = torch.tensor(coef, dtype=f32)
        p = k * x                                                  # one fp32 product
        summed = _fma(k, x, v) if contract else v + p              # one fp32 add, or one FMA
        vn_ = torch.where(started[:, None], summed, p)             # 0 + p = p
        v = torch.where(have[:, None], vn_, v)
        started |= have
    if c.accumulate and mutant != "accumulate_ignored":
        v = v + c.dst0.float()[dr.clamp(min=0)]
    out = c.dst0.clone()
    new = _store(v, T, mutant)
    if mutant == "last_vector_dropped" and D % (64 * w) != 0:
        new[:, D - w:] = c.dst0[dr.clamp(min=0), D - w:]
    out[dr[live]] = new[live]
    return out


def run_axpby(form, n, D, dtype, contract=False, mutant=None):
    c = RR.axpby_case(form, n, D, dtype, SEED + D + n)
    RR.check("row_axpby", emulate_axpby(c, contract, mutant), c.reference(), what=f"{form} {_id(dtype)} D={D} rows={n} {mutant}")


@pytest.mark.parametrize("contract", CONTRACT, ids=["rounded", "fma"])
@pytest.mark.parametrize("dtype,D", DIMS, ids=_id)
def test_faithful_row_axpby_is_accepted_in_every_form(dtype, D, contract):
    for form in RR.AXPBY_FORMS:
        for n in RR.ROWS:
            run_axpby(form, n, D, dtype, contract)


@pytest.mark.parametrize("contract", CONTRACT, ids=["rounded", "fma"])
@pytest.mark.parametrize("dtype", (f32, bf16), ids=_id)
def test_faithful_row_axpby_is_accepted_at_4099_rows(dtype, contract):
    """Every form at D = 128; at D = 768 the forms with arithmetic (the row maps do not depend on D)."""
    for form in RR.AXPBY_FORMS:
        run_axpby(form, RR.BIG_ROWS, 128, dtype, contract)
    for form in ("general", "b_is_dst"):
        run_axpby(form, RR.BIG_ROWS, 768, dtype, contract)


def test_reference_marks_the_bit_equal_cases():
    """Copies, the zero fill, untouched rows and the fp32 one-add forms have δ = 0 everywhere; the general form has none
    on the rows it writes; a bf16 one-add form is bit-determined only where its sum is an fp32 number (two halves of bf16
    values nearly always are)."""
    for dtype in (f32, bf16):
        D = 260 if dtype == f32 else 520
        for form in ("idx_dst", "idx_src", "idx_both", "idx_wins", "inner_dst", "inner_src", "broadcast", "offset", "zero_fill",
                     "a_is_dst", "negative"):
            v, d, ex = RR.axpby_case(form, 5, D, dtype, SEED).reference()
            assert bool(ex.all()) and float(d.max()) == 0.0, (form, dtype)
        for form in ("b_off", "b_is_dst", "accumulate"):
            v, d, ex = RR.axpby_case(form, 5, D, dtype, SEED).reference()
            if dtype == f32:                                       # sums that are no fp32 numbers, yet determined
                assert bool(ex.all()) and not bool(RR._rep32(v).all()), (form, dtype)
            else:                                                  # determined exactly where the fp32 add does not round
                assert bool((ex == RR._rep32(v)).all()), (form, dtype)
        c = RR.axpby_case("general", 5, D, dtype, SEED)
        v, d, ex = c.reference()
        written = c.d[0].long()
        assert not bool(ex[written].any()) and bool(ex.sum() == (c.dst0.shape[0] - 5) * D)
    # 0.5 a + 0.5 b in fp32 is the correctly rounded sum: one ulp off is refused although it is inside half an ulp + u |v|
    c = RR.axpby_case("b_off", 5, 256, f32, SEED)
    good = emulate_axpby(c)
    RR.check("row_axpby", good, c.reference())
    bad = good.clone()
    row = 0
    bad[row, 7] = torch.nextafter(bad[row, 7], torch.tensor(9.0))
    with pytest.raises(AssertionError, match="bit-determined|over their bound"):
        RR.check("row_axpby", bad, c.reference())


def test_row_index_is_the_twin_of_pick_row():
    idx = torch.tensor([5, -1, 0, 7], dtype=torch.int32)
    r = torch.arange(4)
    assert RR.row_index(r, idx, 3, 9, 2).tolist() == [5, -1, 0, 7]                # idx wins, the map is ignored
    assert RR.row_index(r, None, 1, 3, 2).tolist() == [2, 5, 8, 11]
    assert RR.row_index(r, None, 0, 3, 2).tolist() == [2, 5, 8, 11]               # inner <= 1
    assert RR.row_index(torch.arange(7), None, 3, 5, 2).tolist() == [2, 3, 4, 7, 8, 9, 12]
    assert RR.row_index(torch.arange(5), None, 2, 0, 0).tolist() == [0, 1, 0, 1, 0]   # stride 0: broadcast
    assert RR.row_index(4, None, 3, 5, 2) == 8
    dst0 = RR.values((4, 8), 1, 1.0, f32)
    with pytest.raises(AssertionError, match="twice"):
        RR.reference_row_axpby(dst0, 2, d=(torch.tensor([1, 1], dtype=torch.int32), 1, 1, 0), a=dst0)


# (mutant, the forms that must reject it, a filter on (dtype, D))
AXPBY_MUTANTS = [
    ("off_dropped", ("inner_dst", "inner_src", "offset", "b_off"), None),
    ("off_with_idx", ("idx_wins",), None),
    ("inner_mod_only", ("inner_dst", "inner_src"), None),
    ("stride0_as_1", ("broadcast",), None),
    ("neg_src_row0", ("negative",), None),
    ("neg_dst_row0", ("negative",), None),
    ("alpha_beta_swapped", ("general",), None),
    ("accumulate_ignored", ("accumulate", "general"), None),
    ("truncate", ("general", "b_is_dst"), lambda t, D: t == bf16),
    ("last_vector_dropped", ("idx_both", "general", "zero_fill"), lambda t, D: D % (64 * RR.vn(t, D)) != 0),
    ("second_sweep_col_plus_1", ("idx_src", "general"), lambda t, D: D > 64 * RR.vn(t, D)),
]


@pytest.mark.parametrize("contract", CONTRACT, ids=["rounded", "fma"])
@pytest.mark.parametrize("mutant,forms,applies", AXPBY_MUTANTS, ids=[m[0] for m in AXPBY_MUTANTS])
def test_row_axpby_mutant_is_rejected(mutant, forms, applies, contract):
    """5 rows (more than one sequence of the two-level maps, a negative entry in di and in ai) at every width."""
    hit = 0
    for dtype, D in DIMS:
        if applies is not None and not applies(dtype, D):
            continue
        for form in forms:
            run_axpby(form, 5, D, dtype, contract)                 # the faithful kernel passes the very same check
            with pytest.raises(AssertionError):
                run_axpby(form, 5, D, dtype, contract, mutant=mutant)
            hit += 1
    assert hit >= 4, "a mutant that no shape of the matrix exercises proves nothing"


# ------------------------------------------------------------------------------------------------ embedding sums
def emulate_embed_sum(out0, word, pos, typ, ids, types, seq_stride, off, mutant=None):
    M, L = ids.shape
    orow, l = embed_rows(M, L, seq_stride, off)
    p = torch.arange(M * L) if mutant == "pos_from_r" else l
    v = (word.float()[ids.view(-1).long()] + typ.float()[types.view(-1).long()]) + pos.float()[p]
    out = out0.clone()
    out[orow] = v.to(out0.dtype)
    return out


@pytest.mark.parametrize("dtype,D", [(t, D) for t in (f32, bf16) for D in RR.VEC_DIMS[t]], ids=_id)
def test_embedding_sum_emulation_and_position_mutant(dtype, D):
    M, L, stride, off = 3, 5, 8, 2
    word, pos, typ, ids, types = embed_operands(M, L, D, dtype, SEED + D)
    out0 = RR.values((M * stride + 1, D), SEED, 1.0, dtype)
    orow, l = embed_rows(M, L, stride, off)
    ref = RR.reference_embed(out0, word, pos, typ, ids, types, l, orow)
    RR.check("bert_embed_sum", emulate_embed_sum(out0, word, pos, typ, ids, types, stride, off), ref)
    with pytest.raises(AssertionError):
        RR.check("bert_embed_sum", emulate_embed_sum(out0, word, pos, typ, ids, types, stride, off, "pos_from_r"), ref)


# ------------------------------------------------------------------------------------------------ ViT
def emulate_patchify(cols0, img, p):
    I, C, HW, _ = img.shape
    gw = HW // p
    out = cols0.clone()
    for i in range(I):
        for py in range(gw):
            for px in range(gw):
                out[i * gw * gw + py * gw + px, :C * p * p] = img[i, :, py * p:(py + 1) * p, px * p:(px + 1) * p].reshape(-1).to(cols0.dtype)
    return out


def emulate_assemble(tokens0, patches, cls, pos, I, npatch, seq_stride, off, mutant=None):
    out = tokens0.clone()
    P = pos.float()
    for i in range(I):
        lo = i * seq_stride + off
        first = cls.float().view(-1)
        if mutant == "cls_adds_patch":
            first = first + patches.float()[i * npatch]
        out[lo] = (first + P[0]).to(tokens0.dtype)
        out[lo + 1:lo + 1 + npatch] = (patches.float()[i * npatch:(i + 1) * npatch] + P[1:npatch + 1]).to(tokens0.dtype)
    return out


@pytest.mark.parametrize("dtype", (f32, bf16), ids=_id)
def test_vit_emulations_and_cls_mutant(dtype):
    for HW in (32, 48):
        img = RR.values((2, 3, HW, HW), SEED + HW, 2.0, f32)
        K = 3 * 256
        cols0 = RR.values((2 * (HW // 16) ** 2, K + 8), SEED, 1.0, dtype)
        ref = RR.reference_patchify(cols0, img, 16)
        assert bool(ref[2].all())
        RR.check("vit_patchify", emulate_patchify(cols0, img, 16), ref)
        with pytest.raises(AssertionError):
            RR.check("vit_patchify", emulate_patchify(cols0, img.transpose(2, 3).contiguous(), 16), ref)
    for D in RR.VEC_DIMS[dtype] + RR.SCALAR_DIMS:
        I, npatch, stride, off = 3, 4, 8, 2
        patches, cls, pos = RR.values((I * npatch, D), SEED + 1, 1.0, dtype), RR.values((D,), SEED + 2, 1.0, dtype), \
            RR.values((npatch + 1, D), SEED + 3, 0.5, dtype)
        tok0 = RR.values((I * stride + 1, D), SEED + 4, 1.0, dtype)
        ref = RR.reference_assemble(tok0, patches, cls, pos, I, npatch, stride, off)
        RR.check("vit_assemble", emulate_assemble(tok0, patches, cls, pos, I, npatch, stride, off), ref)
        with pytest.raises(AssertionError):
            RR.check("vit_assemble", emulate_assemble(tok0, patches, cls, pos, I, npatch, stride, off, "cls_adds_patch"), ref)


# ------------------------------------------------------------------------------------------------ graph node features
def emulate_node_feature(x0, o, B, Tn, contract_unused=False):
    out = x0.clone()
    T = x0.dtype
    for b in range(B):
        out[b * Tn] = o["token"]
        for t in range(1, Tn):
            n = b * (Tn - 1) + t - 1
            v = o["in_emb"].float()[int(o["ind"][n])] + o["out_emb"].float()[int(o["outd"][n])]
            if int(o["node_row"][n]) >= 0:
                v = v + o["src"].float()[int(o["node_row"][n])]
            out[b * Tn + t] = v.to(T)
    return out


@pytest.mark.parametrize("dtype", (f32, bf16), ids=_id)
def test_graph_node_feature_emulation_is_accepted(dtype):
    B, Tn = 2, 4
    for D in RR.VEC_DIMS[dtype] + RR.SCALAR_DIMS:
        for with_src in (True, False):
            o = node_operands(B, Tn, D, dtype, SEED + D, with_src=with_src)
            x0 = RR.values((B * Tn, D), SEED, 1.0, dtype)
            ref = RR.reference_node_feature(x0, o["src"], o["node_row"], o["ind"], o["outd"], o["in_emb"], o["out_emb"], o["token"], B, Tn)
            got = emulate_node_feature(x0, o, B, Tn)
            RR.check("graph_node_feature", got, ref)
            bad = got.clone()
            bad[0], bad[1] = got[1], got[0]                        # the token row and the first node exchanged
            with pytest.raises(AssertionError):
                RR.check("graph_node_feature", bad, ref)


# ------------------------------------------------------------------------------------------------ tanh
def test_tanh_forward_reference_allows_twice_the_measured_error():
    assert RR.TANH_REL == 2 * RR.TANH_MEASURED >= RR.U32
    for dtype in (f32, bf16):
        x = RR.tanh_inputs(2048, dtype, SEED)
        ref = RR.reference_tanh_fwd(x)
        y = torch.tanh(x.double())
        RR.check("tanh_fwd", (y * (1 + RR.TANH_MEASURED)).to(dtype), ref)
        assert float(ref[0][0]) == 0.0 and bool(ref[2][0])         # tanh(0) = 0 exactly
        with pytest.raises(AssertionError):
            RR.check("tanh_fwd", (y * (1 + (2.0 ** -7 if dtype == bf16 else 4 * RR.TANH_REL))).to(dtype), ref)


def emulate_tanh_bwd(y, dy, contract=False, mutant=None):
    t, g = y.float(), dy.float()
    if mutant == "one_minus_t":
        return (g * (1.0 - t)).to(y.dtype)
    s = (1.0 - t.double() * t.double()).to(f32) if contract else 1.0 - t * t
    return (g * s).to(y.dtype)


@pytest.mark.parametrize("contract", CONTRACT, ids=["rounded", "fma"])
@pytest.mark.parametrize("dtype", (f32, bf16), ids=_id)
def test_tanh_backward_emulation_and_mutant(dtype, contract):
    n = 2048
    y, dy = RR.near_one(n, dtype, SEED), RR.values((n,), SEED + 1, 2.0, dtype)
    ref = RR.reference_tanh_bwd(y, dy)
    RR.check("tanh_bwd", emulate_tanh_bwd(y, dy, contract), ref)
    with pytest.raises(AssertionError):
        RR.check("tanh_bwd", emulate_tanh_bwd(y, dy, contract, "one_minus_t"), ref)
    if dtype == f32:
        # |t| = 1 - 2^-24: t t rounds by 2^-48 against s = 2^-23, far more than u s: only the absolute t² term covers it,
        # and it stays an absolute error of a few u per unit of dy, however small s is
        i = 3
        assert float(y[i]) == 1.0 - 2.0 ** -24 and float(ref[0][i]) != 0.0
        assert abs(float(dy[i])) * 2.0 ** -48 <= float(ref[1][i]) <= abs(float(dy[i])) * 3 * RR.U32


# ------------------------------------------------------------------------------------------------ scatter-add
def emulate_scatter_add(table0, idx, src, n, s_stride, s_off, order="ltr", mutant=None):
    out = table0.clone()
    seen = set()
    rs = range(n) if order == "ltr" else range(n - 1, -1, -1)
    for r in rs:
        t = int(idx[r])
        if t < 0:
            continue
        if mutant == "duplicate_once" and t in seen:
            continue
        seen.add(t)
        s = src[r * s_stride + (0 if mutant == "s_off_ignored" else s_off)].float()
        out[t] = out[t] + s
    return out


@pytest.mark.parametrize("order", ("ltr", "rtl"))
@pytest.mark.parametrize("dtype", (f32, bf16), ids=_id)
def test_scatter_add_emulation_and_mutants(dtype, order):
    for D in (4, 65, 260):
        for n in (5, 211):
            for granule in (True, False):
                table0, idx, src = scatter_operands(n, D, dtype, SEED + D, granule)
                ref = RR.reference_scatter_add(table0, idx, src, n, 2, 1)
                if granule:
                    assert bool(ref[2].all()), "operands on the 1/16 granule must make every order exact"
                RR.check("row_scatter_add", emulate_scatter_add(table0, idx, src, n, 2, 1, order), ref, nonvacuous=True)
                for mutant in ("duplicate_once", "s_off_ignored"):
                    if mutant == "duplicate_once" and n == 5 and int((idx >= 0).sum()) == int(idx[idx >= 0].unique().numel()):
                        continue
                    with pytest.raises(AssertionError):
                        RR.check("row_scatter_add", emulate_scatter_add(table0, idx, src, n, 2, 1, order, mutant), ref, nonvacuous=True)


def test_scatter_add_with_a_vacuous_bound_is_refused():
    """Three million general terms onto one row: γ_n Σ|terms| is a large fraction of the sum, which check() will not call a test."""
    n = 3_000_000
    src = RR.gen((n, 1), SEED, 1.0, f32)
    table0 = torch.zeros(1, 1)
    idx = torch.zeros(n, dtype=torch.int32)
    ref = RR.reference_scatter_add(table0, idx, src, n)
    with pytest.raises(AssertionError, match="vacuous"):
        RR.check("row_scatter_add", ref[0].float(), ref, nonvacuous=True)


# ------------------------------------------------------------------------------------------------ index invariants
def _no_repeat(name, v, rows, call):
    v = np.asarray(v.cpu().numpy() if torch.is_tensor(v) else v, dtype=np.int64)
    live = v[v >= 0]
    assert live.size == np.unique(live).size, f"{name} repeats a destination row of {call}"
    assert live.size == 0 or int(live.max()) < rows, f"{name} addresses row {int(live.max())} of {rows} in {call}"


@pytest.mark.parametrize("host", (True, False), ids=["host-built", "device-arithmetic"])
@pytest.mark.parametrize("ragged", (False, True), ids=["padded", "ragged"])
@pytest.mark.parametrize("kind", ("A", "B", "M"))
def test_destination_index_vectors_never_repeat_a_row(kind, ragged, host):
    """Every index vector the engine passes as a DESTINATION of mdt_row_axpby, for the batches of oracle/cases.py in both
    text layouts and from both builders (numpy on the host, torch arithmetic): no non-negative entry twice, all in range."""
    from multimodaldiscussiontransformer_amd.data.packer import get_ragged, pack_batch
    from multimodaldiscussiontransformer_amd.models import GraphormerModel
    from oracle import cases
    from tests.util_model import model_args
    hp = cases.real_hparams(kind) if kind == "M" else cases.tiny_hparams(kind)
    trees = cases.real_trees(kind, hp) if kind == "M" else cases.tiny_trees(kind, hp)
    ge = GraphormerModel.build_model(model_args(hp), task=None).encoder.graph_encoder
    ge.ragged_tokens = ragged
    pb = pack_batch(trees, 5, device="cpu")
    if not host:
        pb.host = None
    ix = ge._indices(pb)
    assert ix["ragged"] == ragged
    nb, M, I = ge.num_bottle_neck, pb.M, pb.I
    rows_fus, rows_vit, rows_graph = ix["rows_fus"], I * ix["Sv"], pb.B * pb.T
    # expand_rows forward (di = body_idx / front_idx) and, ragged, the scatter_rows adjoint (di = s_idx = pre2fus)
    _no_repeat("pre2fus", ix["pre2fus"], rows_fus, "expand_rows: row_axpby(out, rows_in, di=body_idx)")
    # expand_rows forward for the learned rows and the take_rows(s_idx=bn_rows_all) adjoint (accumulate)
    _no_repeat("bn_rows_all", ix["bn_rows_all"], rows_fus, "expand_rows: row_axpby(out, nfront, di=front_idx); take_rows adjoint")
    both = np.concatenate([ix["pre2fus"].cpu().numpy(), ix["bn_rows_all"].cpu().numpy()]).astype(np.int64)
    assert np.array_equal(np.sort(both), np.arange(rows_fus)), "pre2fus and bn_rows_all must tile rows_fus exactly (expand_rows asserts only the count)"
    assert ix["pre2fus"].numel() == ix["rows_pre"] and ix["bn_rows_all"].numel() == M * nb
    # rows_mix(1, 0, d_idx=bn0_rows) graph -> text; the adjoints of graph_node_features and classifier_head (accumulate)
    _no_repeat("bn0_rows", ix["bn0_rows"], rows_fus, "rows_mix(d_idx=bn0_rows); graph_node_features / classifier_head adjoints")
    _no_repeat("cls_rows", ix["cls_rows"], rows_fus, "classifier_head adjoint: row_axpby(gt, M, di=cls_rows, accumulate)")
    # rows_mix(0.5, 0.5, d_idx=img_text_bn_rows) and the adjoint of rows_mix(1, 0, s_idx=img_text_bn_rows)
    _no_repeat("img_text_bn_rows", ix["img_text_bn_rows"], rows_fus, "rows_mix(0.5, 0.5, d_idx=img_text_bn_rows) and the (1, 0) adjoint")
    # rows_mix(1, 0, d_idx=vit_bn_rows) and the adjoint of rows_mix(0.5, 0.5, s_idx=vit_bn_rows)
    _no_repeat("vit_bn_rows", ix["vit_bn_rows"], max(rows_vit, 1), "rows_mix(1, 0, d_idx=vit_bn_rows) and the (0.5, 0.5) adjoint")
    assert ix["img_text_bn_rows"].numel() == ix["vit_bn_rows"].numel() == I * nb
    # rows_mix(1, 0, d_idx=graph_row) text -> graph and the adjoint of rows_mix(d_idx=bn0_rows, s_idx=graph_row)
    _no_repeat("graph_row", pb.graph_row, rows_graph, "rows_mix(1, 0, d_idx=graph_row) and the graph -> text adjoint")
    assert pb.graph_row.numel() == M and bool((pb.graph_row % pb.T != 0).all()), "a comment on a graph-token row"
    # graph_node_features adjoint: the source rows of the comments are a subset of bn0_rows; padding nodes are -1
    trn = ix["text_row_of_node"].cpu().numpy()
    assert set(trn[trn >= 0].tolist()) == set(ix["bn0_rows"].cpu().numpy().tolist())
    # the pruned last fusion layer: transformer_block adjoint row_axpby(full, R, di=keep_rows); rows_mix(d_idx=img_bn0_compact)
    prune, compact = ge._prune_indices(pb, ix)
    _no_repeat("text_keep", prune["text_keep"], rows_fus, "transformer_block(keep_rows): row_axpby(full, R, di=keep_rows)")
    _no_repeat("vit_keep", prune["vit_keep"], max(rows_vit, 1), "transformer_block(keep_rows) of the image block")
    _no_repeat("img_bn0_compact", prune["img_bn0_compact"], 2 * M, "rows_mix(0.5, 0.5, d_idx=img_bn0_compact) on the [2M, D] output")
    _no_repeat("compact bn0_rows", compact["bn0_rows"], 2 * M, "classifier_head adjoint on the compact rows")
    _no_repeat("compact cls_rows", compact["cls_rows"], 2 * M, "classifier_head adjoint on the compact rows")
    assert np.array_equal(prune["text_keep"].cpu().numpy()[0::2], ix["bn0_rows"].cpu().numpy())
    assert np.array_equal(prune["text_keep"].cpu().numpy()[1::2], ix["cls_rows"].cpu().numpy())
    # the ragged -> padded scatter of forward(): scatter_rows(d_idx=dense_rows, s_idx=pre2fus), both directions
    rt = get_ragged(pb)
    dense_rows = rt.comment.long() * pb.L + rt.pos.long()
    _no_repeat("dense_rows", dense_rows, M * pb.L, "scatter_rows forward: row_axpby(out, n, di=d_idx)")
    if ragged:
        assert dense_rows.numel() == ix["pre2fus"].numel() == rt.rows


# ------------------------------------------------------------------------------------------------ row geometry against loops
GEOMETRY_KINDS = ("A", "B", "M", "no_image", "all_images", "single", "one_token")


def _geometry_case(kind):
    """(hyper-parameters, host trees): the batches of oracle/cases.py and one batch each without any image, with an image on
    every comment, of a single one-comment tree, and of one-token texts (two of them with an image)."""
    from multimodaldiscussiontransformer_amd import synthetic
    from oracle import cases
    if kind in ("A", "B"):
        hp = cases.tiny_hparams(kind)
        return hp, cases.tiny_trees(kind, hp)
    if kind == "M":
        hp = cases.real_hparams(kind)
        return hp, cases.real_trees(kind, hp)
    hp = cases.tiny_hparams("A")
    spec = dict(no_image=((5, 0.0, "bushy"), (3, 0.0, "deep"), (6, 0.0, "bushy")), all_images=((4, 1.0, "bushy"), (3, 1.0, "deep")),
                single=((1, 0.0, "bushy"),), one_token=((4, 0.5, "bushy"), (2, 0.0, "deep")))[kind]
    rng = np.random.Generator(np.random.PCG64(4242))
    trees = [synthetic.make_tree(n, rng, seq_len=16, vocab_size=hp.vocab_size, image_frac=f, image_size=hp.image_size, shape=s,
                                 min_len=3) for n, f, s in spec]
    if kind == "one_token":
        for t in trees:
            t["attention_mask"][:, 1:] = 0
            t["input_ids"] *= t["attention_mask"]
    return hp, trees


def _same(got, want, path):
    """Equal key by key: tensors by value, dtype, shape and both contiguous; scalars by value and type."""
    if torch.is_tensor(got) or torch.is_tensor(want):
        assert torch.is_tensor(got) and torch.is_tensor(want), path
        assert got.dtype == want.dtype and got.shape == want.shape and torch.equal(got, want), f"{path}: {got} != {want}"
        assert got.is_contiguous() and want.is_contiguous(), f"{path} is not contiguous"
    elif isinstance(want, dict):
        assert isinstance(got, dict) and list(sorted(got)) == list(sorted(want)), f"{path}: keys {sorted(got)} != {sorted(want)}"
        for k in want:
            _same(got[k], want[k], f"{path}.{k}")
    elif isinstance(want, (list, tuple)):
        assert isinstance(got, (list, tuple)) and len(got) == len(want), path
        for i, (g, w) in enumerate(zip(got, want)):
            _same(g, w, f"{path}[{i}]")
    else:
        assert type(got) is type(want) and got == want, f"{path}: {got!r} != {want!r}"


def _geometry_mutant(name, ix, prune, nb):
    """A subtly wrong builder: the faithful result with one vector derived by a wrong rule."""
    ix, prune = dict(ix), dict(prune)
    I = prune["vit_keep"].numel()
    if name == "cls_off_by_one":
        ix["cls_rows"] = ix["cls_rows"] + 1
    elif name == "pre2fus_without_nb":
        ix["pre2fus"] = ix["pre2fus"] - nb
    elif name == "img_rows_in_node_order":                        # the first I comments instead of the image comments
        ix["img_text_bn_rows"] = ix["bn_rows_all"][:I * nb].clone()
    elif name == "vit_keep_stride_P":
        prune["vit_keep"] = torch.arange(I, dtype=torch.int32) * ix["P"]
    else:
        raise KeyError(name)
    return ix, prune


GEOMETRY_MUTANTS = ("cls_off_by_one", "pre2fus_without_nb", "img_rows_in_node_order", "vit_keep_stride_P")


@pytest.fixture(scope="module")
def geometry_encoder():
    from multimodaldiscussiontransformer_amd.models import GraphormerModel
    from tests.util_model import model_args
    made = {}

    def get(hp):
        key = repr(sorted(vars(hp).items()))
        if key not in made:
            made[key] = GraphormerModel.build_model(model_args(hp), task=None).encoder.graph_encoder
        return made[key]
    return get


@pytest.mark.parametrize("ragged", (False, True), ids=["padded", "ragged"])
@pytest.mark.parametrize("kind", GEOMETRY_KINDS)
def test_index_vectors_equal_the_loop_reference_from_both_feeds(kind, ragged, geometry_encoder):
    """_indices and _prune_indices fed with the packer's host arrays, fed with the batch's tensors (``pb.host = None``) and
    the plain loops of rowops_reference over the host trees give the same vectors: equal values, dtypes and scalars, all
    contiguous.  On batch A and M (three and four images on scattered comments) four wrong rules are rejected by the same
    comparison."""
    from multimodaldiscussiontransformer_amd.data.packer import pack_batch
    hp, trees = _geometry_case(kind)
    ge = geometry_encoder(hp)
    ge.ragged_tokens = ragged
    nb = ge.num_bottle_neck
    mask, node_comment, img_comment = RR.batch_layout(trees)
    Sv = nb + (hp.image_size // hp.patch) ** 2 + 1
    want = RR.reference_text_rows(nb, Sv, mask, node_comment, img_comment, ragged, length_bins=ge.length_bins)
    want_prune = RR.reference_prune_rows(nb, Sv, mask, img_comment, ragged)
    got = {}
    for feed in ("host", "device"):
        pb = pack_batch(trees, 5, device="cpu")
        assert pb.host is not None
        if feed == "device":
            pb.host = None
        ix = ge._indices(pb)
        assert ix["ragged"] == ragged and ge._indices(pb) is ix
        pr = ge._prune_indices(pb, ix)
        assert isinstance(pr, tuple) and len(pr) == 2 and ge._prune_indices(pb, ix) is pr
        _same(ix, want, f"{feed}-fed _indices")
        _same(pr, want_prune, f"{feed}-fed _prune_indices")
        got[feed] = (ix, pr)
    _same(got["host"], got["device"], "host-fed against device-fed")
    assert (pb.M, pb.I) == (len(mask), len(img_comment))
    if kind in ("A", "M"):
        assert img_comment != list(range(len(img_comment))) and len(img_comment) > 1
        for name in GEOMETRY_MUTANTS:
            bad_ix, bad_prune = _geometry_mutant(name, got["host"][0], got["host"][1][0], nb)
            with pytest.raises(AssertionError):
                _same(bad_ix, want, name)
                _same((bad_prune, got["host"][1][1]), want_prune, name)
