"""The embedding front ends of multimodaldiscussiontransformer_amd/engine.py on a bare Tape, forward and adjoint:
bert_embeddings, bert_embeddings_rows, bert_embeddings_ln_rows (with _embed_rows_grads / _type_emb_grad behind them),
vit_embeddings in its three forms with the _k_padded cache, and the thin dropout / layernorm ops that follow them.

The reference restates every form with plain torch indexing on fp64 CPU tensors.  Copies and gathers must be bit-equal;
table gradients, fp32 sums over rows, are compared with the fp64 sums under the any-order bound of
tests/rowops_reference.py (never vacuous: median bound / |ref| <= 2^-7); GEMMs with tests/gemm_reference.py from the
operands they read; LayerNorm with tests/layernorm_reference.py.  Every adjoint runs with two kinds of upstream gradient:
granule gradients (multiples of 1/16: every partial sum in every order is an fp32 number, so every table gradient is
bit-determined — asserted on the reference — and atomic and deterministic mode must both equal the fp64 sum) and random
gradients (the bound; deterministic mode reproduces its bits and launches no float atomics).  Gradients differ from row to
row, so a row permutation in an adjoint changes the result.

Shapes.  Text: D = 256 in fp32 and 520 in bf16 (the CASES of tests/test_engine_rows_gpu.py), 97 word rows, 40 position
rows, 2 types, M = 9 comments of L = 24 tokens (216 padded rows) and the ragged view of the 171 valid tokens
(rowops_reference.text_case: id 0 on 130 valid tokens and on all padding, twelve ids exactly once, 37 table rows never
referenced).  ViT: I = 3 images of 32 x 32 (16-pixel patches, 12 patch rows) and 28 x 28 (14-pixel patches, K = 588 padded
to 640), D = 128.  tests/test_engine_embeddings_reference_cpu.py proves at these shapes that the checks accept a plain
torch model of the adjoints and reject its mutants."""
import contextlib
import gc

import pytest
import torch

import tests.gemm_reference as GR
import tests.layernorm_reference as LR
import tests.rowops_reference as RR
from tests.rowops_reference import bf16, f32
from tests.test_engine_rows_gpu import CASES, IDS, check_sum, same

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEED = 8642
EPS = 1e-12                      # HF BertEmbeddings LayerNorm
P_DROP = 0.1
FORMS = ("padded", "ragged", "ln")
KINDS = ("granule", "random")
TABLES = ("word", "pos", "typ")
VIT_D, VIT_I = 128, 3
WORST = {}                       # GEMM checks of this file: worst err / bound (RR.WORST and LR.WORST keep the others)


@pytest.fixture(scope="module")
def E():
    from multimodaldiscussiontransformer_amd import engine
    assert torch.cuda.is_available(), "GPU tests need a device"
    return engine


@pytest.fixture(scope="module")
def ops():
    from multimodaldiscussiontransformer_amd import ops as o
    return o


def dev(t):
    return t.to(DEV).contiguous()


def i32(t):
    return t.to(torch.int32).to(DEV).contiguous()


@contextlib.contextmanager
def mode(E, deterministic):
    was = E.deterministic()
    E.set_deterministic(deterministic)
    try:
        yield
    finally:
        E.set_deterministic(was)


# ------------------------------------------------------------------------------------------------ operands (CPU; shared with the CPU companion)
def text_tables(dtype, D):
    return dict(word=RR.values((RR.TEXT_V, D), SEED + 1, 1.0, dtype), pos=RR.values((RR.TEXT_P, D), SEED + 2, 0.5, dtype),
                typ=RR.values((2, D), SEED + 3, 0.25, dtype), gamma=(1.0 + 0.25 * RR.gen((D,), SEED + 4, 1.0, f32)).to(dtype),
                beta=RR.gen((D,), SEED + 5, 0.5, dtype))


def text_starts(D):
    """What the main_grad buffers hold before the step: k / 16 with |k| <= 144, on the granule of the granule gradients."""
    return dict(word=RR.granule_rows(RR.TEXT_V, D, SEED + 11, f32, r=144), pos=RR.granule_rows(RR.TEXT_P, D, SEED + 12, f32, r=144),
                typ=RR.granule_rows(2, D, SEED + 13, f32, r=144), gamma=RR.granule_rows(1, D, SEED + 14, f32, r=144).view(-1),
                beta=RR.granule_rows(1, D, SEED + 15, f32, r=144).view(-1))


def upstream(kind, shape, dtype, k=0):
    """Granule gradients (k / 16, |k| <= 16) or random ones; both differ from row to row."""
    if kind == "granule":
        return RR.granule_rows(shape[0], shape[1], SEED + 21 + k, dtype)
    return RR.values(shape, SEED + 21 + k, 1.0, dtype)


def geometry(form):
    """Per row of the form: word id, token type and position id (the padded form takes its position from the column)."""
    c = RR.text_case()
    if form == "padded":
        return dict(n=c["M"] * c["L"], M=c["M"], L=c["L"], ids=c["ids"].view(-1), types=c["types"].view(-1), pos=c["pos_padded"])
    return dict(n=int(c["rows"].numel()), M=c["M"], L=c["L"], ids=c["ids_rows"], types=c["types_rows"], pos=c["pos_rows"])


# ------------------------------------------------------------------------------------------------ the checks (the CPU companion runs them on a torch model)
def check_text_grads(grads, start, geo, terms, what, exact=False, times=1):
    """The three table gradients (fp32 CPU buffers, None: frozen) after ``times`` passes that each added the rows ``terms``
    [n, D] onto ``start``: word and position tables against reference_scatter_add (rows nobody addresses keep their bits: the
    padded form's position rows L.. among them), the type table against reference_type_split.  ``exact``: these inputs must make
    every element bit-determined, so the result IS the fp64 sum whatever the order of the adds."""
    def rep(t):
        return torch.cat([t] * times)

    n = geo["n"] * times
    assert terms.shape[0] == geo["n"]
    T, ids, pos, types = rep(terms), rep(geo["ids"]), rep(geo["pos"]), rep(geo["types"])
    refs = {}
    if grads.get("word") is not None:
        refs["word"] = RR.reference_scatter_add(start["word"], ids, T, n)
    if grads.get("pos") is not None:
        refs["pos"] = RR.reference_scatter_add(start["pos"], pos, T, n)
    if grads.get("typ") is not None:
        refs["typ"] = RR.reference_type_split(start["typ"], types, T)
    for k, ref in refs.items():
        if exact:
            assert bool(ref[2].all()), f"{what}: these inputs do not determine the bits of the {k} gradient"
        RR.check(f"{k} table grad", grads[k], ref, what=f"{what} {k}", dtype=f32, nonvacuous=True)
    return refs


def check_total(name, got, start, terms64, what, exact=False):
    """An fp32 gradient buffer against start + Σ over dim 0 of terms64 in any order (check_sum with the old content as one more term)."""
    all_terms = torch.cat([start.double().reshape(1, -1), terms64.reshape(terms64.shape[0], -1)])
    if exact:
        assert bool((RR._sum_err(all_terms, torch.zeros_like(all_terms), 0) == 0).all()), f"{what}: these inputs do not determine the bits of {name}"
    check_sum(name, got.reshape(-1), all_terms, what=what)


def check_dropout(name, got, x, p, seed, what):
    """x keep / (1 - p) with the keep-bits of the CPU port for site ``seed``, counter row D + col: one fp32 product, one rounding."""
    v = x.double() * GR.drop_scale(x.shape[0], x.shape[1], p, seed)
    d = LR._rounded(torch.zeros_like(v), v, v.abs())
    RR.check(name, got, (v, d, d == 0), what=what)


def check_vit_weight_grad(before, after, dpatch, cols, gw, start_w, K, split_k, what):
    """The weight-gradient accumulator [D, kp] before and after its GEMM (dpatch^T cols, fp32, added to what was there) and the
    gradient buffer ``gw`` afterwards.  kp == K: the accumulator IS the buffer, pre-filled.  kp > K: a fresh zero buffer whose
    columns K.. must stay exactly zero and whose first K columns join the pre-filled gradient with one correctly rounded add."""
    D, kp = after.shape
    acc0 = start_w.view(D, K) if kp == K else torch.zeros(D, kp)
    assert torch.equal(before, acc0), f"{what}: the accumulator did not start from {'the pre-filled gradient' if kp == K else 'zero'}"
    ref = GR.reference(dpatch, cols, trans_a=True, trans_b=True, epilogue=GR.EPI_ATOMIC, c_old=before, split_k=split_k)
    gemm_check("patch weight grad", after, ref, f32, what + " weight gradient")
    if kp == K:
        assert torch.equal(gw.view(D, K), after), f"{what}: the gradient buffer is not the accumulator"
        return
    assert float(after[:, K:].abs().max()) == 0.0, f"{what}: the weight gradient leaked into its padding columns"
    RR.check("vit weight grad join", gw.view(D, K), RR.reference_row_axpby(start_w.view(D, K), D, a=after[:, :K].contiguous(), accumulate=True),
             what=what + " pre-filled + accumulator")


def gemm_check(name, out, ref, dtype, what):
    v, d = ref["out"]
    ratio = float(((out.double() - v).abs() / GR.bound(v, d, dtype).clamp(min=1e-300)).max())
    WORST[name] = max(WORST.get(name, 0.0), ratio if ratio == ratio else float("inf"))
    GR.check({"out": out}, ref, {"out": dtype}, what=what)


# ------------------------------------------------------------------------------------------------ text: running a form
def spy_reductions(E, monkeypatch):
    """Every gradient reduction the text adjoints launch, in order: (entry, target, source tensor)."""
    calls = []
    real_sc, real_cs, real_ax = E.scatter_add, E.colsum, E.ops.row_axpby

    def scatter_add(table, idx, src, nrows):
        calls.append(("scatter_add", table.shape[0], src))
        return real_sc(table, idx, src, nrows)

    def colsum(x, out=None, row_weight=None):
        calls.append(("colsum", "fresh" if out is None else "into", x))
        return real_cs(x, out=out, row_weight=row_weight)

    def row_axpby(dst, nrows, **kw):
        calls.append(("row_axpby", dst.shape[0], None))
        return real_ax(dst, nrows, **kw)

    monkeypatch.setattr(E, "scatter_add", scatter_add)
    monkeypatch.setattr(E, "colsum", colsum)
    monkeypatch.setattr(E.ops, "row_axpby", row_axpby)
    return calls


def text_forward(E, tape, form, geo, P):
    ids, types, pos = i32(geo["ids"]), i32(geo["types"]), i32(geo["pos"])
    if form == "padded":
        return E.bert_embeddings(tape, ids.view(geo["M"], geo["L"]), types.view(geo["M"], geo["L"]), P["word"], P["pos"], P["typ"])
    if form == "ragged":
        return E.bert_embeddings_rows(tape, ids, types, pos, P["word"], P["pos"], P["typ"])
    return E.bert_embeddings_ln_rows(tape, ids, types, pos, P["word"], P["pos"], P["typ"], P["gamma"], P["beta"], EPS)


def run_text(E, ops, calls, form, dtype, D, G, main=False, frozen=(), times=1):
    """``times`` forward + backward passes of ``form`` on ONE tape with the upstream gradient G; → the output, the table (and
    LayerNorm) gradient buffers as they are afterwards, what they held before, the rows the reductions summed in each pass,
    the reductions launched and the float-atomic launches of the adjoints."""
    geo, tabs, st = geometry(form), text_tables(dtype, D), text_starts(D)
    P = {k: torch.nn.Parameter(dev(t), requires_grad=k not in frozen) for k, t in tabs.items()}
    if main:
        for k, p in P.items():
            if p.requires_grad:
                p.main_grad = dev(st[k])
    tape = E.Tape(use_main_grad=main)
    del calls[:]
    atomics, summed = 0, []
    for _ in range(times):
        mark = len(calls)
        o = text_forward(E, tape, form, geo, P)
        assert len(calls) == mark, "a forward pass launched a gradient reduction"
        o.grad = dev(G)
        ops.float_atomic_launches(reset=True)
        tape.backward()
        atomics += ops.float_atomic_launches(reset=True)
        srcs = [c[2] for c in calls[mark:] if c[2] is not None]
        assert srcs and all(s.data_ptr() == srcs[0].data_ptr() and s.numel() == geo["n"] * D for s in srcs), "the reductions read different rows"
        summed.append(srcs[0].reshape(geo["n"], D).cpu())
    torch.cuda.synchronize()
    names = TABLES + (("gamma", "beta") if form == "ln" else ())
    grads = {}
    for k in names:
        if P[k].requires_grad:
            grads[k] = (P[k].main_grad if main else tape.tmp_grads[id(P[k])]).cpu()
        else:
            assert id(P[k]) not in tape.tmp_grads and not hasattr(P[k], "main_grad"), f"a frozen table ({k}) has a gradient buffer"
            grads[k] = None
    start = {k: (st[k] if main else torch.zeros_like(st[k])) for k in names}
    return dict(out=o.data.cpu(), grads=grads, start=start, summed=summed, calls=list(calls), atomics=atomics, geo=geo, tabs=tabs, tape=tape)


def targets(form, name):
    """The reductions that write the gradient of table ``name`` in ``form``."""
    if name == "word":
        return {("scatter_add", RR.TEXT_V)}
    if name == "pos":
        return {("colsum", "into")} if form == "padded" else {("scatter_add", RR.TEXT_P)}
    return {("colsum", "fresh"), ("row_axpby", 2)}


def check_text_run(res, form, dtype, G, what, exact, times=1, ln_stats=None):
    """One run_text result against the references.  Padded / ragged: the rows summed are the upstream gradient itself.  The
    fused form: the rows summed are the dx the LayerNorm backward stored — checked against the LayerNorm reference, then taken
    as exact terms of the table sums; its dgamma / dbeta accumulate over the passes."""
    if form != "ln":
        for s in res["summed"]:
            assert torch.equal(s, G), f"{what}: the reductions did not read the upstream gradient"
        check_text_grads(res["grads"], res["start"], res["geo"], G, what, exact=exact, times=times)
        return
    xs, mean, rstd = ln_stats
    for s in res["summed"][1:]:
        assert torch.equal(s, res["summed"][0]), f"{what}: dx differs between two passes over the same operands"

    def rep(t):
        return torch.cat([t] * times)

    ref = LR.reference_bwd(rep(G), rep(xs), res["tabs"]["gamma"], rep(mean), rep(rstd), dgamma0=res["start"]["gamma"], dbeta0=res["start"]["beta"])
    got = {"dx": rep(res["summed"][0])}
    for k, n in (("gamma", "dgamma"), ("beta", "dbeta")):
        if res["grads"][k] is not None:
            got[n] = res["grads"][k]
    LR.check(got, ref, {"dx": dtype}, what=what)
    if exact and res["grads"]["beta"] is not None:                              # Σ of granule rows: bit-determined
        assert float(ref["dbeta"][1].max()) == 0.0 and torch.equal(res["grads"]["beta"].double(), ref["dbeta"][0]), f"{what}: dbeta"
    check_text_grads(res["grads"], res["start"], res["geo"], res["summed"][0], what + " (stored dx)", times=times)


def ln_forward_stats(E, ops, dtype, D):
    """xs, mean, rstd that ops.bert_embed_ln_rows stores for the text case (host copies): the operands of the fused adjoint."""
    geo, tabs = geometry("ln"), text_tables(dtype, D)
    y, mean, rstd, xs = ops.bert_embed_ln_rows(i32(geo["ids"]), i32(geo["types"]), i32(geo["pos"]), *(dev(tabs[k]) for k in ("word", "pos", "typ", "gamma", "beta")), EPS)
    return xs.cpu(), mean.cpu(), rstd.cpu()


# ------------------------------------------------------------------------------------------------ text: forward
@pytest.mark.parametrize("form", ("padded", "ragged"))
@pytest.mark.parametrize("dtype,D", CASES, ids=IDS)
def test_bert_embeddings_forward(E, dtype, D, form):
    geo, tabs = geometry(form), text_tables(dtype, D)
    P = {k: torch.nn.Parameter(dev(t)) for k, t in tabs.items()}
    o = text_forward(E, E.Tape(), form, geo, P)
    ref = RR.reference_embed(torch.zeros(geo["n"], D, dtype=dtype), tabs["word"], tabs["pos"], tabs["typ"], geo["ids"], geo["types"], geo["pos"],
                             torch.arange(geo["n"]))
    RR.check("bert_embed forward", o.data.cpu(), ref, what=f"bert_embeddings {form} forward")


class LnSpy:
    """Keeps what ops.bert_embed_ln_rows and ops.layernorm_fwd returned (the real kernels run)."""

    def __init__(self, ops, monkeypatch):
        self.fused, self.plain = [], []
        real_f, real_p = ops.bert_embed_ln_rows, ops.layernorm_fwd

        def bert_embed_ln_rows(*a, **kw):
            r = real_f(*a, **kw)
            self.fused.append(r)
            return r

        def layernorm_fwd(*a, **kw):
            r = real_p(*a, **kw)
            self.plain.append(r)
            return r

        monkeypatch.setattr(ops, "bert_embed_ln_rows", bert_embed_ln_rows)
        monkeypatch.setattr(ops, "layernorm_fwd", layernorm_fwd)


@pytest.mark.parametrize("dtype,D", CASES, ids=IDS)
def test_bert_embeddings_ln_rows_forward_has_the_bits_of_the_two_ops(E, ops, monkeypatch, dtype, D):
    """y, mean, rstd and the kept sum of the fused op equal layernorm(bert_embeddings_rows(...)) on the same tape bit for bit, and
    are within the bounds of the fp64 value: the sum of reference_embed, the LayerNorm of reference_fwd on the stored sum."""
    geo, tabs = geometry("ln"), text_tables(dtype, D)
    P = {k: torch.nn.Parameter(dev(t)) for k, t in tabs.items()}
    spy = LnSpy(ops, monkeypatch)
    tape = E.Tape()
    fused = text_forward(E, tape, "ln", geo, P)
    rows = text_forward(E, tape, "ragged", geo, P)
    two = E.layernorm(tape, rows, P["gamma"], P["beta"], EPS)
    (y, mean, rstd, xs), = spy.fused
    (y2, mean2, rstd2), = spy.plain
    assert fused.data is y and two.data is y2 and len(tape.ops) == 3
    assert torch.equal(xs, rows.data), "the kept sum is not the rows bert_embeddings_rows writes"
    assert torch.equal(y, y2) and torch.equal(mean, mean2) and torch.equal(rstd, rstd2), "the fused op does not have the bits of the two ops"
    ref = RR.reference_embed(torch.zeros(geo["n"], D, dtype=dtype), tabs["word"], tabs["pos"], tabs["typ"], geo["ids"], geo["types"], geo["pos"],
                             torch.arange(geo["n"]))
    RR.check("bert_embed forward", xs.cpu(), ref, what="bert_embeddings_ln_rows kept sum")
    LR.check({"y": y.cpu(), "mean": mean.cpu(), "rstd": rstd.cpu()}, LR.reference_fwd(xs.cpu(), tabs["gamma"], tabs["beta"], EPS),
             {"y": dtype, "mean": f32, "rstd": f32}, what="bert_embeddings_ln_rows")


@pytest.mark.parametrize("dtype,D", CASES, ids=IDS)
def test_bert_embeddings_ln_rows_on_an_inference_tape(E, ops, monkeypatch, dtype, D):
    geo, tabs = geometry("ln"), text_tables(dtype, D)
    P = {k: torch.nn.Parameter(dev(t)) for k, t in tabs.items()}
    spy = LnSpy(ops, monkeypatch)
    train = text_forward(E, E.Tape(), "ln", geo, P)
    tape = E.Tape(inference=True)
    infer = text_forward(E, tape, "ln", geo, P)
    assert torch.equal(train.data, infer.data), "the inference tape's output differs from the training tape's"
    assert spy.fused[0][3] is not None and spy.fused[1][3] is None, "the summed rows are kept exactly when a backward pass will read them"
    assert tape.ops == [] and tape.tmp_grads == {}


# ------------------------------------------------------------------------------------------------ text: adjoints
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dtype,D", CASES, ids=IDS)
def test_text_adjoint_in_both_modes(E, ops, monkeypatch, dtype, D, form, kind):
    """Fresh gradient buffers, one pass; main_grad buffers pre-filled with granule values, two passes on one tape (the result adds
    to what was there, twice).  Atomic mode, then deterministic mode: the same checks, no float-atomic launch, granule results
    equal to the atomic mode's bit for bit, random results bit-identical across two runs."""
    calls = spy_reductions(E, monkeypatch)
    geo = geometry(form)
    G = upstream(kind, (geo["n"], D), dtype)
    exact = kind == "granule"
    stats = ln_forward_stats(E, ops, dtype, D) if form == "ln" else None
    runs = {}
    for det in (False, True):
        with mode(E, det):
            fresh = run_text(E, ops, calls, form, dtype, D, G)
            twice = run_text(E, ops, calls, form, dtype, D, G, main=True, times=2)
            again = run_text(E, ops, calls, form, dtype, D, G, main=True, times=2) if det else None
        what = f"{form} {kind} {'deterministic' if det else 'atomic'}"
        check_text_run(fresh, form, dtype, G, what + " fresh", exact, ln_stats=stats)
        check_text_run(twice, form, dtype, G, what + " pre-filled, two passes", exact, times=2, ln_stats=stats)
        for r in (fresh, twice):
            assert (r["atomics"] == 0) == det, f"{what}: {r['atomics']} float-atomic launches in the adjoint"
            for name in TABLES:
                assert targets(form, name) <= {c[:2] for c in r["calls"]}, f"{what}: the {name} gradient took another path than this test means to check"
        if det:
            for k, g in twice["grads"].items():
                assert torch.equal(g, again["grads"][k]), f"{what}: {k} gradient differs between two deterministic runs"
        runs[det] = (fresh, twice)
    for a, d in zip(runs[False], runs[True]):
        assert torch.equal(a["summed"][0], d["summed"][0]), "the rows summed differ between the modes"
        for k in a["grads"]:
            if exact and (form != "ln" or k == "beta"):
                assert torch.equal(a["grads"][k], d["grads"][k]), f"{form} granule: {k} gradient differs between atomic and deterministic mode"


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dtype,D", CASES, ids=IDS)
def test_text_adjoint_with_one_table_frozen(E, ops, monkeypatch, dtype, D, form):
    """word / pos / typ frozen alone, in both modes: the frozen table gets no buffer and no launch, the other two keep the bits
    they have with nothing frozen (granule gradients: bit-determined) and stay within the bounds (random gradients)."""
    calls = spy_reductions(E, monkeypatch)
    geo = geometry(form)
    stats = ln_forward_stats(E, ops, dtype, D) if form == "ln" else None
    for kind in KINDS:
        G = upstream(kind, (geo["n"], D), dtype, k=1)
        for det in (False, True):
            with mode(E, det):
                free = run_text(E, ops, calls, form, dtype, D, G, main=True)
                frozen = {name: run_text(E, ops, calls, form, dtype, D, G, main=True, frozen=(name,)) for name in TABLES}
            for name, r in frozen.items():
                what = f"{form} {kind} {'deterministic' if det else 'atomic'} {name} frozen"
                launched = {c[:2] for c in r["calls"]}
                assert not (targets(form, name) & launched), f"{what}: a launch targets the frozen table"
                assert r["grads"][name] is None
                check_text_run(r, form, dtype, G, what, kind == "granule", ln_stats=stats)
                for other in TABLES:
                    if other == name:
                        continue
                    assert targets(form, other) <= launched
                    if det or (kind == "granule" and form != "ln"):
                        assert torch.equal(r["grads"][other], free["grads"][other]), f"{what}: the {other} gradient changed its bits"
                assert (r["atomics"] == 0) == det


# ------------------------------------------------------------------------------------------------ ViT
def vit_operands(dtype, patch, HW, seed=0):
    g = HW // patch
    npatch, K, D = g * g, 3 * patch * patch, VIT_D
    s = SEED + 100 * seed
    return dict(img=RR.values((VIT_I, 3, HW, HW), s + 41, 2.0, f32), w=RR.values((D, 3, patch, patch), s + 42, 2.0 * GR.b_scale(K), dtype),
                b=RR.values((D,), s + 43, 0.3, dtype), cls=RR.values((1, 1, D), s + 44, 1.0, dtype),
                pos=RR.values((1, npatch + 1, D), s + 45, 0.5, dtype), patch=patch, npatch=npatch, K=K, D=D, I=VIT_I, dtype=dtype)


def vit_starts(o):
    return dict(w=RR.granule_rows(o["D"], o["K"], SEED + 51, f32, r=144).view(o["w"].shape), b=RR.granule_rows(1, o["D"], SEED + 52, f32, r=144).view(-1),
                cls=RR.granule_rows(1, o["D"], SEED + 53, f32, r=144).view(1, 1, -1), pos=RR.granule_rows(o["npatch"] + 1, o["D"], SEED + 54, f32, r=144)[None])


class VitSpy:
    """Wraps the launches of vit_embeddings (the real kernels run) and keeps what they read and wrote."""

    def __init__(self, E, ops, monkeypatch):
        from multimodaldiscussiontransformer_amd import _lib as L
        self.fused, self.patchify, self.assemble, self.gemms, self.wgrads, self.colsums = [], [], [], [], [], []
        real = {n: getattr(ops, n) for n in ("vit_patch_embed", "vit_patchify", "vit_assemble", "gemm")}
        real_wg, real_cs = E.wgrad_gemm, E.colsum

        def vit_patch_embed(*a, **kw):
            self.fused.append(1)
            return real["vit_patch_embed"](*a, **kw)

        def vit_patchify(*a, **kw):
            cols = real["vit_patchify"](*a, **kw)
            self.patchify.append(cols)
            return cols

        def vit_assemble(patches, *a, **kw):
            self.assemble.append(patches)
            return real["vit_assemble"](patches, *a, **kw)

        def gemm(a, b, **kw):
            out = real["gemm"](a, b, **kw)
            self.gemms.append(dict(a=a, b=b, out=out, kw=kw, route=L.last_route()))
            return out

        def wgrad_gemm(dy, x, out, asum=None):
            before = out.detach().cpu().clone()
            real_wg(dy, x, out, asum=asum)
            route = L.last_route()
            torch.cuda.synchronize()
            self.wgrads.append(dict(dy=dy.cpu(), x=x, before=before, after=out.detach().cpu().clone(), route=route))

        def colsum(x, out=None, row_weight=None):
            self.colsums.append(x)
            return real_cs(x, out=out, row_weight=row_weight)

        for n, f in (("vit_patch_embed", vit_patch_embed), ("vit_patchify", vit_patchify), ("vit_assemble", vit_assemble), ("gemm", gemm)):
            monkeypatch.setattr(ops, n, f)
        monkeypatch.setattr(E, "wgrad_gemm", wgrad_gemm)
        monkeypatch.setattr(E, "colsum", colsum)

    def counts(self):
        return len(self.fused), len(self.patchify), len(self.gemms), len(self.assemble)


def vit_params(o, frozen=(), main=False):
    P = {k: torch.nn.Parameter(dev(o[k]), requires_grad=k not in frozen) for k in ("w", "b", "cls", "pos")}
    if main:
        for k, t in vit_starts(o).items():
            if P[k].requires_grad:
                P[k].main_grad = dev(t)
    return P


def vit_forward(E, tape, o, P):
    return E.vit_embeddings(tape, dev(o["img"]), P["w"], P["b"], P["cls"], P["pos"], o["patch"])


def check_vit_three_launches(spy, o, tokens, kp, what, weight=None):
    """The gathered matrix exact with exactly zero pad columns, the projection within the GEMM bound on the operands it read
    (the second one the weight, zero-padded to ``kp`` columns), the assembly within its one add."""
    dtype, K, D, I, npatch = o["dtype"], o["K"], o["D"], o["I"], o["npatch"]
    w = (o["w"] if weight is None else weight).view(D, K)
    cols, g = spy.patchify[-1], spy.gemms[-1]
    assert tuple(cols.shape) == (I * npatch, kp), f"{what}: gathered matrix {tuple(cols.shape)}"
    RR.check("vit_patchify", cols.cpu(), RR.reference_patchify(torch.zeros(I * npatch, kp, dtype=dtype), o["img"], o["patch"]), what=what)
    assert g["a"] is cols and tuple(g["b"].shape) == (D, kp)
    b = g["b"].detach().cpu()
    assert torch.equal(b[:, :K], w) and float(b[:, K:].abs().sum()) == 0.0, f"{what}: the GEMM's weight operand is not the weight, zero-padded"
    patches = g["out"].cpu()
    gemm_check("patch projection", patches, GR.reference(cols.cpu(), b, epilogue=GR.EPI_BIAS, bias=g["kw"]["bias"].cpu()), dtype, what)
    assert spy.assemble[-1] is g["out"]
    RR.check("vit_assemble", tokens.cpu(), RR.reference_assemble(torch.zeros(I * (npatch + 1), D, dtype=dtype), patches, o["cls"].view(-1),
                                                                 o["pos"].view(npatch + 1, D), I, npatch, npatch + 1, 0), what=what)


@pytest.mark.parametrize("dtype", (bf16, f32), ids=("bf16", "f32"))
def test_vit_16px_routes_and_forward_values(E, ops, monkeypatch, dtype):
    """16-pixel patches.  A trainable projection: three launches.  A frozen projection (weight and bias) or an inference tape:
    one fused launch in bf16, whose tokens stay within ONE rounding of the fp64 value on the bf16-rounded operands; fp32
    parameters are never fused."""
    o = vit_operands(dtype, 16, 32)
    spy = VitSpy(E, ops, monkeypatch)
    tok = vit_forward(E, E.Tape(), o, vit_params(o))
    assert spy.counts() == (0, 1, 1, 1), f"trainable projection: launches {spy.counts()}"
    check_vit_three_launches(spy, o, tok.data, o["K"], f"vit 16 px {dtype} trainable")
    for name, tape, P in (("frozen projection", E.Tape(), vit_params(o, frozen=("w", "b"))), ("inference tape", E.Tape(inference=True), vit_params(o))):
        before = spy.counts()
        tok = vit_forward(E, tape, o, P)
        delta = tuple(a - b for a, b in zip(spy.counts(), before))
        if dtype == bf16:
            assert delta == (1, 0, 0, 0), f"{name}: launches {delta}, expected the fused one alone"
            RR.check("vit_patch_embed", tok.data.cpu(), RR.reference_patch_embed(o["img"], 16, o["w"], o["b"], o["cls"], o["pos"]), what=f"vit 16 px fused, {name}")
        else:
            assert delta == (0, 1, 1, 1), f"{name}, fp32 parameters: launches {delta}"
            check_vit_three_launches(spy, o, tok.data, o["K"], f"vit 16 px fp32 {name}")
    # only the bias trainable: its gradient needs the patch rows of g, not the gathered matrix, but the op is not fused
    before = spy.counts()
    vit_forward(E, E.Tape(), o, vit_params(o, frozen=("w",)))
    assert tuple(a - b for a, b in zip(spy.counts(), before)) == (0, 1, 1, 1)


@pytest.mark.parametrize("pad", (True, False), ids=("k-padded", "any-shape"))
def test_vit_14px_routes_and_forward_values(E, ops, monkeypatch, pad):
    """14-pixel patches, bf16: K = 588.  PATCH_K_PAD on: gathered matrix and weight zero-padded to 640, a tile kernel runs; off: 588
    columns on the any-shape kernel.  fp32 parameters are never padded."""
    monkeypatch.setattr(E, "PATCH_K_PAD", pad)
    spy = VitSpy(E, ops, monkeypatch)
    o = vit_operands(bf16, 14, 28)
    tok = vit_forward(E, E.Tape(), o, vit_params(o))
    assert spy.counts() == (0, 1, 1, 1)
    check_vit_three_launches(spy, o, tok.data, 640 if pad else 588, f"vit 14 px pad={pad}")
    assert (spy.gemms[-1]["route"] == "generic") == (not pad), f"pad={pad}: the projection ran on {spy.gemms[-1]['route']}"
    o32 = vit_operands(f32, 14, 28)
    tok = vit_forward(E, E.Tape(), o32, vit_params(o32))
    check_vit_three_launches(spy, o32, tok.data, 588, "vit 14 px fp32")
    assert spy.gemms[-1]["route"] == "generic"


VIT_ADJ = [(bf16, 16, 32, True), (f32, 16, 32, True), (bf16, 14, 28, True), (bf16, 14, 28, False)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype,patch,HW,pad", VIT_ADJ, ids=("bf16-16px", "f32-16px", "bf16-14px-padded", "bf16-14px-any-shape"))
def test_vit_adjoint_in_both_modes(E, ops, monkeypatch, dtype, patch, HW, pad, kind):
    """All four parameters trainable, main_grad buffers pre-filled with granule values.  The gathered dpatch is an exact copy of
    the patch rows of g; the weight-gradient GEMM is within its bound on the operands it read (trans_a, trans_b, the engine's
    split_k, the old accumulator); with padding the accumulator is a fresh [D, 640] buffer whose columns 588.. stay exactly
    zero and whose first 588 columns join the pre-filled gradient with one more (correctly rounded) add; bias, [CLS] and position
    gradients are fp32 sums of the recorded terms — bit-determined for granule gradients, in both modes."""
    monkeypatch.setattr(E, "PATCH_K_PAD", pad)
    spy = VitSpy(E, ops, monkeypatch)
    o = vit_operands(dtype, patch, HW)
    I, npatch, D, K = o["I"], o["npatch"], o["D"], o["K"]
    kp = 640 if (pad and K == 588) else K
    G = upstream(kind, (I * (npatch + 1), D), dtype, k=2)
    G3 = G.double().view(I, npatch + 1, D)
    st = vit_starts(o)
    results = {}
    for det in (False, True):
        what = f"vit {patch} px {dtype} pad={pad} {kind} {'deterministic' if det else 'atomic'}"
        runs = []
        for _ in range(2 if det else 1):
            P = vit_params(o, main=True)
            tape = E.Tape(use_main_grad=True)
            with mode(E, det):
                tok = vit_forward(E, tape, o, P)
                cols = spy.patchify[-1]
                tok.grad = dev(G)
                n_wg, n_cs = len(spy.wgrads), len(spy.colsums)
                ops.float_atomic_launches(reset=True)
                tape.backward()
                atomics = ops.float_atomic_launches(reset=True)
            torch.cuda.synchronize()
            assert (atomics == 0) == det, f"{what}: {atomics} float-atomic launches"
            runs.append({k: p.main_grad.cpu() for k, p in P.items()})
        (wg,) = spy.wgrads[n_wg:]
        assert len(spy.colsums) - n_cs == 3 and tuple(cols.shape) == (I * npatch, kp)
        same(wg["dy"], G3[:, 1:].reshape(I * npatch, D), what + " dpatch")
        assert wg["x"] is cols, f"{what}: the weight gradient did not contract over the gathered matrix of the forward"
        same(spy.colsums[n_cs], G3[:, 1:].reshape(I * npatch, D), what + " rows of the bias sum")
        got = runs[-1]
        check_vit_weight_grad(wg["before"], wg["after"], wg["dy"], cols.cpu(), got["w"], st["w"], K, E._split_k(D, kp, I * npatch), what)
        if kp != K:
            assert wg["route"] != "generic", f"{what}: the padded weight gradient ran on the any-shape kernel"
        exact = kind == "granule"
        check_total("vit bias grad", got["b"], st["b"], G3[:, 1:].reshape(I * npatch, D), what + " bias", exact)
        check_total("vit cls grad", got["cls"], st["cls"], G3[:, 0], what + " [CLS]", exact)
        check_total("vit pos grad", got["pos"], st["pos"], G3.reshape(I, (npatch + 1) * D), what + " position", exact)
        if det:
            for k in got:
                assert torch.equal(runs[0][k], runs[1][k]), f"{what}: {k} gradient differs between two deterministic runs"
        results[det] = got
    if kind == "granule":
        for k in ("b", "cls", "pos"):
            assert torch.equal(results[False][k], results[True][k]), f"vit granule: {k} gradient differs between atomic and deterministic mode"


def test_vit_adjoint_with_a_frozen_projection_weight(E, ops, monkeypatch):
    """Weight frozen, bias trainable (14 px, padded): no weight-gradient GEMM runs, the bias still sums the gathered patch rows."""
    spy = VitSpy(E, ops, monkeypatch)
    o = vit_operands(bf16, 14, 28)
    I, npatch, D = o["I"], o["npatch"], o["D"]
    G = upstream("granule", (I * (npatch + 1), D), bf16, k=3)
    P = vit_params(o, frozen=("w",))
    tape = E.Tape()
    tok = vit_forward(E, tape, o, P)
    tok.grad = dev(G)
    tape.backward()
    torch.cuda.synchronize()
    assert spy.wgrads == [] and id(P["w"]) not in tape.tmp_grads
    same(spy.colsums[0], G.double().view(I, npatch + 1, D)[:, 1:].reshape(I * npatch, D), "dpatch")
    check_total("vit bias grad", tape.tmp_grads[id(P["b"])].cpu(), torch.zeros(D), G.double().view(I, npatch + 1, D)[:, 1:].reshape(I * npatch, D), "bias, weight frozen", True)


def test_k_padded_cache_follows_the_weight(E, ops, monkeypatch):
    """Two forwards reuse one padded copy; an in-place write under no_grad, and a .data write followed by weights_changed(),
    refresh it and the tokens follow; a new parameter never gets the copy of a deleted one."""
    monkeypatch.setattr(E, "PATCH_K_PAD", True)
    spy = VitSpy(E, ops, monkeypatch)
    o = vit_operands(bf16, 14, 28)
    D, K = o["D"], o["K"]
    P = vit_params(o)

    def forward(weight, what):
        tok = vit_forward(E, E.Tape(inference=True), o, P)
        check_vit_three_launches(spy, o, tok.data, 640, what, weight=weight)
        return spy.gemms[-1]["b"]

    first = forward(o["w"], "first forward")
    second = forward(o["w"], "second forward")
    assert first.data_ptr() == second.data_ptr() and first is second, "the second forward padded the weight again"
    w2 = vit_operands(bf16, 14, 28, seed=1)["w"]
    with torch.no_grad():
        P["w"].copy_(dev(w2))
    third = forward(w2, "after an in-place write under no_grad")
    assert third is not first
    w3 = vit_operands(bf16, 14, 28, seed=2)["w"]
    version = P["w"]._version
    P["w"].data.copy_(dev(w3))
    assert P["w"]._version == version, "a .data write is meant to be invisible to torch's version counter here"
    E.weights_changed()
    fourth = forward(w3, "after a .data write and weights_changed()")
    assert fourth is not third
    # a deleted parameter's copy must not serve its successor, whatever id() and address the successor gets
    reused = 0
    for k in range(4):
        w_new = vit_operands(bf16, 14, 28, seed=3 + k)["w"]
        old_id, old_ptr = id(P["w"]), P["w"].data_ptr()
        del P["w"]
        gc.collect()
        P["w"] = torch.nn.Parameter(dev(w_new))
        reused += int(id(P["w"]) == old_id or P["w"].data_ptr() == old_ptr)
        forward(w_new, f"parameter {k} created after its predecessor was deleted")
    print(f"\n_k_padded: {reused} of 4 successors reused the id or the address of the deleted parameter")


# ------------------------------------------------------------------------------------------------ dropout, layernorm
@pytest.mark.parametrize("dtype,D", CASES, ids=IDS)
def test_dropout_forward_and_adjoint_share_the_site_seed(E, ops, monkeypatch, dtype, D):
    rows = 37
    x, G = RR.values((rows, D), SEED + 61, 1.0, dtype), RR.values((rows, D), SEED + 62, 1.0, dtype)
    seeds = []
    real = ops.dropout
    monkeypatch.setattr(ops, "dropout", lambda t, p, seed, out=None: (seeds.append((p, seed)), real(t, p, seed, out=out))[1])
    torch.manual_seed(1234)
    tape = E.Tape()
    tape.next_seed()                                                             # an earlier site: this op must take the NEXT seed
    xv = E.Var(dev(x))
    o = E.dropout(tape, xv, P_DROP)
    seed = (tape._seed_base + 0x9E3779B97F4A7C15 * 2) & 0x7FFFFFFFFFFFFFFF
    assert tape._seed_ctr == 2 and seeds == [(P_DROP, seed)], "the op did not take the tape's next site seed"
    check_dropout("dropout forward", o.data.cpu(), x, P_DROP, seed, "engine.dropout forward")
    assert torch.equal(o.data, real(dev(x), P_DROP, seed)), "the op's output is not that of ops.dropout with the site seed"
    kept = float((o.data != 0).float().mean())
    assert abs(kept - (1 - P_DROP)) < 0.02, f"{kept:.3f} of the elements kept at p = {P_DROP}"
    o.grad = dev(G)
    tape.backward()
    assert seeds == [(P_DROP, seed)] * 2, "the backward did not use the forward's site seed"
    check_dropout("dropout adjoint", xv.grad.cpu(), G, P_DROP, seed, "engine.dropout adjoint")
    assert torch.equal(xv.grad, real(dev(G), P_DROP, seed))


def test_dropout_with_p_zero_is_the_identity_and_takes_no_seed(E):
    torch.manual_seed(99)
    tape = E.Tape()
    first = tape.next_seed()
    xv = E.Var(dev(RR.values((3, 256), SEED, 1.0, f32)))
    assert E.dropout(tape, xv, 0.0) is xv and tape._seed_ctr == 1 and tape.ops == []
    after = tape.next_seed()
    torch.manual_seed(99)
    other = E.Tape()
    assert (other.next_seed(), other.next_seed()) == (first, after), "a p = 0 site moved the seeds of the sites behind it"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype,D", CASES, ids=IDS)
def test_layernorm_op_forward_and_adjoint(E, ops, monkeypatch, dtype, D, kind):
    """engine.layernorm on 171 rows: forward within the reference bounds; adjoint (dx, and dgamma / dbeta accumulated onto pre-filled
    main_grad buffers) within them in both modes, dx with the same bits in both, dbeta bit-determined for granule gradients."""
    rows = 171
    tabs, st = text_tables(dtype, D), text_starts(D)
    x, G = RR.values((rows, D), SEED + 71, 2.0, dtype), upstream(kind, (rows, D), dtype, k=4)
    spy = LnSpy(ops, monkeypatch)
    dxs = {}
    for det in (False, True):
        what = f"engine.layernorm {kind} {'deterministic' if det else 'atomic'}"
        P = {k: torch.nn.Parameter(dev(tabs[k])) for k in ("gamma", "beta")}
        for k, p in P.items():
            p.main_grad = dev(st[k])
        tape = E.Tape(use_main_grad=True)
        xv = E.Var(dev(x))
        with mode(E, det):
            o = E.layernorm(tape, xv, P["gamma"], P["beta"], EPS)
            y, mean, rstd = spy.plain[-1]
            assert o.data is y
            LR.check({"y": y.cpu(), "mean": mean.cpu(), "rstd": rstd.cpu()}, LR.reference_fwd(x, tabs["gamma"], tabs["beta"], EPS),
                     {"y": dtype, "mean": f32, "rstd": f32}, what=what)
            o.grad = dev(G)
            ops.float_atomic_launches(reset=True)
            tape.backward()
            assert (ops.float_atomic_launches(reset=True) == 0) == det
        ref = LR.reference_bwd(G, x, tabs["gamma"], mean.cpu(), rstd.cpu(), dgamma0=st["gamma"], dbeta0=st["beta"])
        got = {"dx": xv.grad.cpu(), "dgamma": P["gamma"].main_grad.cpu(), "dbeta": P["beta"].main_grad.cpu()}
        LR.check(got, ref, {"dx": dtype}, what=what)
        if kind == "granule":
            assert float(ref["dbeta"][1].max()) == 0.0 and torch.equal(got["dbeta"].double(), ref["dbeta"][0]), f"{what}: dbeta is not the exact sum"
        dxs[det] = got["dx"]
    assert torch.equal(dxs[False], dxs[True]), "dx differs between atomic and deterministic mode"


def test_report_worst_error_over_bound():
    """Not a check of its own: prints the worst err / bound each checked quantity reached in this run (pytest -s, or the log)."""
    worst = dict(RR.WORST)
    worst.update({f"layernorm {k}": v for k, v in LR.WORST.items()})
    worst.update(WORST)
    print("\nengine embeddings worst err/bound: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
    assert all(v <= 1.0 for v in worst.values())
