"""The checks of tests/test_engine_embeddings_gpu.py can fail.  The engine's embedding adjoints are written once here as a small
torch model (index_add_ with fp32 accumulation, the token-type split as tot - one, a matmul for the ViT weight gradient, the
dropout mask of the CPU port); the checks of the GPU file accept it at the very shapes, operands and both kinds of upstream
gradient the GPU file uses, and reject each listed mutant of it, a subtly wrong adjoint.  The references are the only judge.

Also shown here: the granule inputs determine every bit of every table gradient (the "exact" condition the GPU file asserts),
and for the random inputs the reference alone meets the non-vacuity cap of the sums (median bound / |ref| <= 2^-7)."""
import pytest
import torch

import tests.gemm_reference as GR
import tests.layernorm_reference as LR
import tests.rowops_reference as RR
import tests.test_engine_embeddings_gpu as T
from tests.rowops_reference import bf16, f32
from tests.test_engine_rows_gpu import CASES, IDS

FORMS = ("padded", "ragged")
TEXT_MUTANTS = {   # mutant -> the forms whose check must reject it
    "duplicate_of_id0_dropped": FORMS,
    "last_write_wins": FORMS,
    "pos_shifted_one_row": ("padded",),
    "pos_ids_from_arange": ("ragged",),
    "type_rows_swapped": FORMS,
    "type_row0_gets_total": FORMS,
    "overwrite": FORMS,
}


@pytest.fixture(autouse=True)
def _worst_ratios_are_left_alone():
    """The mutants' err / bound must not reach the reports of the GPU files that run in the same session."""
    saved = [(d, dict(d)) for d in (RR.WORST, LR.WORST, T.WORST)]
    yield
    for d, was in saved:
        d.clear()
        d.update(was)


# ------------------------------------------------------------------------------------------------ the model
def model_text_adjoint(start, geo, G, times=1, mutant=None):
    """The three table gradient buffers after ``times`` passes of the text adjoint over the rows G, fp32 accumulation."""
    ids, pos, types = geo["ids"].long(), geo["pos"].long(), geo["types"].long()
    g = G.float()
    out = {k: (torch.zeros_like(start[k]) if mutant == "overwrite" else start[k].clone()) for k in T.TABLES}
    for _ in range(times):
        keep = torch.ones(geo["n"], dtype=torch.bool)
        if mutant == "duplicate_of_id0_dropped":
            keep[torch.nonzero(ids == 0)[77]] = False
        if mutant == "last_write_wins":
            out["word"][ids] = out["word"][ids] + g                      # index_put without accumulate: one term per table row survives
        else:
            out["word"].index_add_(0, ids[keep], g[keep])
        p = torch.arange(geo["n"]) % geo["L"] if mutant == "pos_ids_from_arange" else pos
        gp = torch.zeros_like(out["pos"]).index_add_(0, p, g)
        if mutant == "pos_shifted_one_row":
            gp[:geo["L"]] = torch.roll(gp[:geo["L"]], 1, 0)
        out["pos"] += gp
        tot, one = g.sum(0), (g * types[:, None].float()).sum(0)
        r0, r1 = (1, 0) if mutant == "type_rows_swapped" else (0, 1)
        out["typ"][r1] += one
        out["typ"][r0] += tot if mutant == "type_row0_gets_total" else tot - one
    return out


def starts(D, main):
    st = T.text_starts(D)
    return {k: (st[k] if main else torch.zeros_like(st[k])) for k in T.TABLES}


# ------------------------------------------------------------------------------------------------ the text case itself
def test_text_case_has_the_rows_the_suite_is_about():
    c = RR.text_case()
    assert sum(RR.TEXT_LENS) == int(c["rows"].numel()) == 171 and c["ids"].shape == (RR.TEXT_M, RR.TEXT_L) == (9, 24)
    for form in FORMS:
        geo = T.geometry(form)
        ids, types = geo["ids"].long(), geo["types"].long()
        counts = torch.bincount(ids, minlength=RR.TEXT_V)
        assert int(counts[0]) >= 130, f"{form}: id 0 on {int(counts[0])} rows: no segment of more than two 64-row chunks"
        assert int((counts == 1).sum()) >= 10 and int((counts == 0).sum()) >= 10 and int(ids.max()) < RR.TEXT_V
        assert min(int((types == 0).sum()), int((types == 1).sum())) * 3 >= geo["n"], f"{form}: a token type covers less than a third of the rows"
        assert int(geo["pos"].max()) == RR.TEXT_L - 1 < RR.TEXT_P
    pad = torch.ones(216, dtype=torch.bool)
    pad[c["rows"]] = False
    assert bool((c["ids"].view(-1)[pad] == 0).all()) and int(pad.sum()) == 45
    assert torch.equal(c["ids"].view(-1)[c["rows"]], c["ids_rows"]) and torch.equal(c["pos_padded"][c["rows"]], c["pos_rows"])


# ------------------------------------------------------------------------------------------------ accepted, exact, not vacuous
@pytest.mark.parametrize("kind", T.KINDS)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dtype,D", CASES, ids=IDS)
def test_model_of_the_text_adjoints_is_accepted(dtype, D, form, kind):
    """Fresh buffers with one pass and pre-filled buffers with two passes, as the GPU file runs them.  Granule gradients: the
    reference marks every element bit-determined (so atomic and ordered sums must both BE the fp64 sum).  Random gradients:
    the fp64 value itself passes, i.e. the bound alone is not vacuous."""
    geo = T.geometry(form)
    G = T.upstream(kind, (geo["n"], D), dtype)
    for main, times in ((False, 1), (True, 2)):
        st = starts(D, main)
        refs = T.check_text_grads(model_text_adjoint(st, geo, G, times), st, geo, G, f"{form} {kind}", exact=kind == "granule", times=times)
        for k, (v, d, ex) in refs.items():
            if kind == "granule":
                assert bool(ex.all()) and float(d.max()) == 0.0
            else:
                touched = v != st[k].double()
                assert float(ex[touched].float().mean()) < 0.5, "random gradients are meant to exercise the bound, not equality"
                RR.check(f"{k} table grad", v.float(), (v, d, ex), dtype=f32, nonvacuous=True)
            if k != "typ":                                              # rows nobody addresses keep their bits
                idx = geo["ids"] if k == "word" else geo["pos"]
                quiet = torch.ones(v.shape[0], dtype=torch.bool)
                quiet[idx.long()] = False
                assert int(quiet.sum()) >= 10 and bool(ex[quiet].all()) and torch.equal(v[quiet], st[k].double()[quiet])


def test_sums_of_stored_dx_are_checked_like_any_rows():
    """The fused form sums the dx its LayerNorm backward stored: bf16 / fp32 values that sit on no common granule.  The same check
    takes them as exact terms; here a stand-in (random rows) shows the model accepted and a dropped duplicate rejected."""
    geo = T.geometry("ln")
    dx = RR.values((geo["n"], 520), 5, 0.3, bf16)
    st = starts(520, True)
    T.check_text_grads(model_text_adjoint(st, geo, dx), st, geo, dx, "stored dx")
    with pytest.raises(AssertionError):
        T.check_text_grads(model_text_adjoint(st, geo, dx, mutant="duplicate_of_id0_dropped"), st, geo, dx, "stored dx")


# ------------------------------------------------------------------------------------------------ mutants
@pytest.mark.parametrize("kind", T.KINDS)
@pytest.mark.parametrize("mutant", sorted(TEXT_MUTANTS))
@pytest.mark.parametrize("dtype,D", CASES, ids=IDS)
def test_text_adjoint_mutant_is_rejected(dtype, D, mutant, kind):
    for form in TEXT_MUTANTS[mutant]:
        geo = T.geometry(form)
        G = T.upstream(kind, (geo["n"], D), dtype)
        st = starts(D, True)
        table = {"duplicate_of_id0_dropped": "word", "last_write_wins": "word", "pos_shifted_one_row": "pos", "pos_ids_from_arange": "pos",
                 "type_rows_swapped": "typ", "type_row0_gets_total": "typ", "overwrite": "word"}[mutant]
        got = model_text_adjoint(st, geo, G, mutant=mutant)
        good = model_text_adjoint(st, geo, G)
        for k in T.TABLES:
            if k != table and mutant != "overwrite":
                assert torch.equal(got[k], good[k])
        with pytest.raises(AssertionError, match=f"{table} table grad"):
            T.check_text_grads(got, st, geo, G, f"{form} {mutant}", exact=kind == "granule")


# ------------------------------------------------------------------------------------------------ ViT
def vit_case(kind, pad):
    o = T.vit_operands(bf16, 14, 28)
    I, npatch, D, K = o["I"], o["npatch"], o["D"], o["K"]
    kp = 640 if pad else K
    G = T.upstream(kind, (I * (npatch + 1), D), bf16, k=2)
    cols = RR.reference_patchify(torch.zeros(I * npatch, kp, dtype=bf16), o["img"], 14)[0].to(bf16)
    dpatch = G.view(I, npatch + 1, D)[:, 1:].reshape(I * npatch, D).contiguous()
    return o, G, cols, dpatch, kp


def model_vit_weight_grad(start_w, dpatch, cols, K, mutant=None):
    """(accumulator before, after, gradient buffer after) of the padded or unpadded weight gradient, fp32 accumulation."""
    D, kp = dpatch.shape[1], cols.shape[1]
    before = start_w.view(D, K).clone() if kp == K else torch.zeros(D, kp)
    after = before + dpatch.float().t() @ cols.float()
    if mutant == "pad_column_leak":
        after[5, K + 7] = 2.0 ** -20
    if kp == K:
        return before, after, after.clone()
    gw = after[:, :K].clone() if mutant == "overwrite" else start_w.view(D, K) + after[:, :K]
    return before, after, gw


@pytest.mark.parametrize("kind", T.KINDS)
@pytest.mark.parametrize("pad", (True, False), ids=("k-padded", "any-shape"))
def test_vit_weight_gradient_model_and_mutants(pad, kind):
    o, G, cols, dpatch, kp = vit_case(kind, pad)
    st = T.vit_starts(o)
    K = o["K"]
    def run(mutant=None):
        before, after, gw = model_vit_weight_grad(st["w"], dpatch, cols, K, mutant)
        T.check_vit_weight_grad(before, after, dpatch, cols, gw, st["w"], K, 1, str(mutant))

    run()
    if pad:
        assert float(cols[:, K:].abs().sum()) == 0.0
        for mutant, why in (("pad_column_leak", "leaked into its padding|over their bound"), ("overwrite", "vit weight grad join")):
            with pytest.raises(AssertionError, match=why):
                run(mutant)


@pytest.mark.parametrize("kind", T.KINDS)
def test_vit_row_sums_model_and_overwrite_mutant(kind):
    """Bias, [CLS] and position gradients: sums over images (and patches) onto pre-filled buffers; granule gradients determine
    their bits; a buffer that is overwritten instead of added to is rejected."""
    o, G, _, dpatch, _ = vit_case(kind, True)
    I, npatch, D = o["I"], o["npatch"], o["D"]
    st = T.vit_starts(o)
    G3 = G.double().view(I, npatch + 1, D)
    for name, start, terms in (("vit bias grad", st["b"], dpatch.double()), ("vit cls grad", st["cls"], G3[:, 0]),
                               ("vit pos grad", st["pos"], G3.reshape(I, (npatch + 1) * D))):
        total = terms.float().sum(0).view(start.shape)
        T.check_total(name, start + total, start, terms, name, exact=kind == "granule")
        with pytest.raises(AssertionError):
            T.check_total(name, total, start, terms, name + " overwritten")


def test_fused_patch_embedding_reference_allows_one_rounding_and_no_more():
    """reference_patch_embed: the correctly rounded fp64 value passes; the three-launch arithmetic (the projection rounded to bf16
    before the position add: two roundings) does not, at these operands."""
    o = T.vit_operands(bf16, 16, 32)
    ref = RR.reference_patch_embed(o["img"], 16, o["w"], o["b"], o["cls"], o["pos"])
    RR.check("vit_patch_embed", ref[0].to(bf16), ref)
    I, npatch, D, K = o["I"], o["npatch"], o["D"], o["K"]
    cols = RR.reference_patchify(torch.zeros(I * npatch, K, dtype=bf16), o["img"], 16)[0]
    patches = (cols @ o["w"].double().view(D, K).t() + o["b"].double()).to(bf16)
    two = RR.reference_assemble(torch.zeros(I * (npatch + 1), D, dtype=bf16), patches, o["cls"].view(-1), o["pos"].view(npatch + 1, D), I, npatch, npatch + 1, 0)[0].to(bf16)
    with pytest.raises(AssertionError):
        RR.check("vit_patch_embed", two, ref)


# ------------------------------------------------------------------------------------------------ dropout
@pytest.mark.parametrize("dtype,D", CASES, ids=IDS)
def test_dropout_model_and_next_seed_mutant(dtype, D):
    rows, p, seed = 37, T.P_DROP, 0x1234567890ABCDEF & 0x7FFFFFFFFFFFFFFF
    x, G = RR.values((rows, D), T.SEED + 61, 1.0, dtype), RR.values((rows, D), T.SEED + 62, 1.0, dtype)

    def model(t, s):
        return (t.float() * GR.drop_scale(rows, D, p, s).float()).to(dtype)

    T.check_dropout("dropout forward", model(x, seed), x, p, seed, "model")
    T.check_dropout("dropout adjoint", model(G, seed), G, p, seed, "model")
    next_seed = (seed + 0x9E3779B97F4A7C15) & 0x7FFFFFFFFFFFFFFF
    with pytest.raises(AssertionError):
        T.check_dropout("dropout adjoint", model(G, next_seed), G, p, seed, "the backward mask of the next site")
