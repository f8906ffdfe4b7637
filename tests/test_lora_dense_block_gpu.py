"""engine.transformer_block with low-rank adapters on the attention output projection, fc1 and fc2 (BlockParams.lora_o / lora_fc1 /
lora_fc2), on the cases of tests/test_engine_block_gpu.py (D 128, 2 heads of 64, F 192; ragged lengths (20, 7, 13), or 3 x 20 rows
with a key mask where keep_rows needs whole sequences), post-LN and pre-LN, dropout off and on:
 (a) Bt = 0 on out and fc2: output and dx are bit-identical to the plain block;
 (b) fp32, random adapters on each site alone and on all six targets: output, dx and the base gradients equal those of the block
     run with the merged matrices W + s Bt^T A, and dA = s Bt dW, dBt = s A dW^T in fp64 from that block's dW — the project's fp32
     gate, 1e-3 of max(1, largest |reference|).  The fc1 site is held to this gate at Bt = 0 too (the fused GELU epilogue works
     from the fp32 accumulator, the adapter path from the stored pre-activation);
 (c) bf16 against the fp32 run of the same adapted block: relative L2 <= BF16_GRAD_REL_L2 per tensor;
 (d) keep_rows with q_limit, an input that wants no gradient, the fc1 bias gradient under an fc2 adapter, every other activation
     with an fc1 adapter, deterministic mode (two runs bit-identical, no float atomics from the adapters), frozen adapters and
     inference, the fp8 refusal, and exactly four dropout seeds per block."""
import pytest
import torch

from tests.rowops_reference import bf16, f32
from tests.test_engine_block_gpu import dev, host, make_case
from tests.test_real_shapes_gpu import BF16_GRAD_REL_L2

pytestmark = pytest.mark.gpu

BASE = ("qkv_w", "qkv_b", "o_w", "o_b", "ln1_w", "ln1_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b", "ln2_w", "ln2_b")
RANK, SCALE = 8, 2.0
SITES = {"out": ("lora_o", "o_w"), "fc1": ("lora_fc1", "fc1_w"), "fc2": ("lora_fc2", "fc2_w")}      # site -> (BlockParams field, base weight)
QKV = (0, 1, 2)
PLACE = pytest.mark.parametrize("pre_ln", (False, True), ids=("bert_post_ln", "vit_pre_ln"))
DROP = pytest.mark.parametrize("drop", (False, True), ids=("nodrop", "drop"))


@pytest.fixture(scope="module")
def E():
    from multimodaldiscussiontransformer_amd import engine
    return engine


@pytest.fixture
def restore_mode(E):
    was = E.deterministic()
    yield
    E.set_deterministic(was)


def adapters(cfg, sites, dtype, zero_b=(), qkv=False, seed=91, b_std=0.05):
    """{site: (A [r, in], Bt [r, out])} on the host, A as add_lora draws it (U(-1/sqrt in, 1/sqrt in)), Bt random (zero for the
    sites of ``zero_b``); with ``qkv`` also "qkv": (A, Bt) [3 r, D] for the three thirds of the fused projection."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for site in sites:
        w = cfg["params"][SITES[site][1]]
        A = ((torch.rand(RANK, w.shape[1], generator=g) * 2 - 1) / w.shape[1] ** 0.5).to(dtype)
        Bt = (torch.zeros(RANK, w.shape[0]) if site in zero_b else torch.randn(RANK, w.shape[0], generator=g) * b_std).to(dtype)
        out[site] = (A, Bt)
    if qkv:
        D = cfg["D"]
        out["qkv"] = (((torch.rand(3 * RANK, D, generator=g) * 2 - 1) / D ** 0.5).to(dtype), (torch.randn(3 * RANK, D, generator=g) * 0.05).to(dtype))
    return out


def merged(cfg, ad):
    """The base weights with s Bt^T A folded in, fp64, rounded once to the parameters' dtype."""
    D = cfg["D"]
    w = {}
    for site, (A, Bt) in ad.items():
        if site == "qkv":
            m = cfg["params"]["qkv_w"].double().clone()
            for c in QKV:
                rows = slice(c * RANK, (c + 1) * RANK)
                m[c * D:(c + 1) * D] += SCALE * Bt[rows].double().t() @ A[rows].double()
            w["qkv_w"] = m.to(cfg["dtype"])
        else:
            name = SITES[site][1]
            w[name] = (cfg["params"][name].double() + SCALE * Bt.double().t() @ A.double()).to(cfg["dtype"])
    return w


def run(E, cfg, ad=None, weights=None, frozen_adapters=False):
    """One forward + backward of the block.  ``ad``: adapters() or None; ``weights``: replaces base weights of the case."""
    sp = cfg["spec"]
    weights = weights or {}
    P = {n: torch.nn.Parameter(dev(weights.get(n, cfg["params"][n]))) for n in BASE}
    extra, order = {}, []
    for site, (A, Bt) in (ad or {}).items():
        a, b = (torch.nn.Parameter(dev(t), requires_grad=not frozen_adapters) for t in (A, Bt))
        P[site + "_A"], P[site + "_Bt"] = a, b
        if site == "qkv":
            extra.update(lora_A=a, lora_Bt=b, lora_cols=QKV, lora_scale=SCALE)
        else:
            extra[SITES[site][0]] = E.LoraSlot(a, b, SCALE)
    for site in ("qkv", "out", "fc1", "fc2"):           # BlockParams.all(): the QKV pair, then o, fc1, fc2 where present
        if ad and site in ad:
            order += [P[site + "_A"], P[site + "_Bt"]]
    BP = E.BlockParams(**{n: P[n] for n in BASE}, **extra)
    spec = E.AttnSpec(nseq=sp["nseq"], S=sp["S"], H=sp["H"], seq_stride=sp["seq_stride"], pos_stride=sp["pos_stride"],
                      key_mask=None if sp.get("key_mask") is None else dev(sp["key_mask"]),
                      seq_offsets=None if sp.get("seq_offsets") is None else dev(sp["seq_offsets"]), q_limit=sp["q_limit"])
    reported = []
    tape = E.Tape(on_params_ready=reported.append, inference=cfg["inference"])
    torch.manual_seed(cfg["torch_seed"])
    xv = E.Var(dev(cfg["x"]), needs_grad=cfg["x_needs_grad"])
    keep = None if cfg["keep_rows"] is None else dev(cfg["keep_rows"].to(torch.int32))
    o = E.transformer_block(tape, xv, BP, spec, pre_ln=cfg["pre_ln"], eps=cfg["eps"], p_hidden=cfg["p_hidden"], p_attn=cfg["p_attn"],
                            p_act=cfg["p_act"], keep_rows=keep, act=cfg["act"])
    assert tape._seed_ctr == 4, "the adapters add no dropout site: the block takes exactly four seeds"
    if cfg["inference"]:
        assert tape.ops == []
        return dict(y=host(o.data))
    o.grad = dev(cfg["cot"])
    tape.backward()
    torch.cuda.synchronize()
    assert len(reported) == 1 and len(reported[0]) == 12 + len(order)
    assert all(a is b for a, b in zip(reported[0][12:], order))
    return dict(y=host(o.data), dx=host(xv.grad), grads={n: host(tape.tmp_grads.get(id(p))) for n, p in P.items()}, tape=tape)


def close_fp32(got, want, what):
    err = float((got.double() - want.double()).abs().max())
    lim = 1e-3 * max(1.0, float(want.double().abs().max()))
    assert err <= lim, f"{what}: |err| {err:.3e} over {lim:.3e}"


def rel_l2(got, want):
    return float((got.double() - want.double()).norm() / want.double().norm().clamp(min=1e-30))


def adapter_grads_from_dw(cfg, ad, grads):
    """{name: fp64} dA = s Bt dW, dBt = s A dW^T from the merged block's weight gradients."""
    D, out = cfg["D"], {}
    for site, (A, Bt) in ad.items():
        if site == "qkv":
            dA, dBt = torch.zeros_like(A, dtype=torch.float64), torch.zeros_like(Bt, dtype=torch.float64)
            for c in QKV:
                rows, dW = slice(c * RANK, (c + 1) * RANK), grads["qkv_w"][c * D:(c + 1) * D].double()
                dA[rows], dBt[rows] = SCALE * Bt[rows].double() @ dW, SCALE * A[rows].double() @ dW.t()
        else:
            dW = grads[SITES[site][1]].double()
            dA, dBt = SCALE * Bt.double() @ dW, SCALE * A.double() @ dW.t()
        out[site + "_A"], out[site + "_Bt"] = dA, dBt
    return out


def against_merged(E, cfg, ad, names=BASE):
    got = run(E, cfg, ad)
    mg = run(E, cfg, weights=merged(cfg, ad))
    close_fp32(got["y"], mg["y"], "output")
    if cfg["x_needs_grad"]:
        close_fp32(got["dx"], mg["dx"], "dx")
    else:
        assert got["dx"] is None and mg["dx"] is None
    for n in names:
        close_fp32(got["grads"][n], mg["grads"][n], n)
    for n, want in adapter_grads_from_dw(cfg, ad, mg["grads"]).items():
        close_fp32(got["grads"][n], want, n)
        assert float(want.abs().max()) > 1e-2, n          # the comparison is not one of zeros
    return got, mg


@PLACE
@DROP
@pytest.mark.parametrize("dtype", (bf16, f32), ids=("bf16", "fp32"))
def test_zero_b_on_out_and_fc2_is_bit_identical_to_the_plain_block(E, dtype, pre_ln, drop):
    cfg = make_case("Sr", dtype, pre_ln, drop=drop)
    ad = adapters(cfg, ("out", "fc2"), dtype, zero_b=("out", "fc2"))
    plain, got = run(E, cfg), run(E, cfg, ad)
    assert torch.equal(plain["y"], got["y"]) and torch.equal(plain["dx"], got["dx"])
    for site in ("out", "fc2"):
        assert float(got["grads"][site + "_A"].abs().max()) == 0.0         # dt = s g Bt^T = 0
        assert float(got["grads"][site + "_Bt"].abs().max()) > 0.0         # and Bt does learn from the first step


@PLACE
@DROP
def test_zero_b_on_fc1_meets_the_fp32_gate(E, pre_ln, drop):
    cfg = make_case("Sr", f32, pre_ln, drop=drop)
    ad = adapters(cfg, ("fc1",), f32, zero_b=("fc1",))
    plain, got = run(E, cfg), run(E, cfg, ad)
    close_fp32(got["y"], plain["y"], "output")
    close_fp32(got["dx"], plain["dx"], "dx")
    for n in BASE:
        close_fp32(got["grads"][n], plain["grads"][n], n)


@PLACE
@DROP
@pytest.mark.parametrize("sites", (("out",), ("fc1",), ("fc2",), ("out", "fc1", "fc2")), ids=("out", "fc1", "fc2", "all"))
def test_fp32_equals_the_merged_block(E, pre_ln, drop, sites):
    cfg = make_case("Sr", f32, pre_ln, drop=drop)
    against_merged(E, cfg, adapters(cfg, sites, f32, qkv=len(sites) == 3))


@PLACE
@DROP
def test_bf16_against_fp32(E, pre_ln, drop):
    cfg16 = make_case("Sr", bf16, pre_ln, drop=drop)
    ad = adapters(cfg16, ("out", "fc1", "fc2"), bf16, qkv=True)
    cfg32 = dict(cfg16, dtype=f32, params={n: t.float() for n, t in cfg16["params"].items()}, x=cfg16["x"].float(), cot=cfg16["cot"].float())
    lo = run(E, cfg16, ad)
    hi = run(E, cfg32, {k: (a.float(), b.float()) for k, (a, b) in ad.items()})
    worst = {"y": rel_l2(lo["y"], hi["y"]), "dx": rel_l2(lo["dx"], hi["dx"])}
    worst.update({n: rel_l2(lo["grads"][n], hi["grads"][n]) for n in lo["grads"]})
    print({k: f"{v:.2e}" for k, v in worst.items()})
    over = {k: v for k, v in worst.items() if not v <= BF16_GRAD_REL_L2}
    assert not over, f"relative L2 over {BF16_GRAD_REL_L2}: {over}"


@PLACE
@pytest.mark.parametrize("dtype", (bf16, f32), ids=("bf16", "fp32"))
def test_keep_rows(E, dtype, pre_ln):
    cfg = make_case("S", f32, pre_ln, keep=True, drop=True)
    ad = adapters(cfg, ("out", "fc1", "fc2"), f32)
    if dtype == f32:
        got, _ = against_merged(E, cfg, ad)
        assert got["y"].shape[0] == 6
    else:
        c16 = make_case("S", bf16, pre_ln, keep=True, drop=True)
        ad16 = {k: (a.to(bf16), b.to(bf16)) for k, (a, b) in ad.items()}
        lo = run(E, c16, ad16)
        c32 = dict(c16, dtype=f32, params={n: t.float() for n, t in c16["params"].items()}, x=c16["x"].float(), cot=c16["cot"].float())
        hi = run(E, c32, {k: (a.float(), b.float()) for k, (a, b) in ad16.items()})
        for n in [s + w for s in ad for w in ("_A", "_Bt")]:
            assert rel_l2(lo["grads"][n], hi["grads"][n]) <= BF16_GRAD_REL_L2, n
        assert rel_l2(lo["y"], hi["y"]) <= BF16_GRAD_REL_L2 and rel_l2(lo["dx"], hi["dx"]) <= BF16_GRAD_REL_L2


@PLACE
def test_input_without_gradient(E, pre_ln):
    cfg = make_case("Sr", f32, pre_ln, x_needs_grad=False, drop=False)
    against_merged(E, cfg, adapters(cfg, ("out", "fc1", "fc2"), f32))


@PLACE
@DROP
def test_fc1_bias_gradient_under_an_fc2_adapter(E, pre_ln, drop):
    """bf16, default mode: the plain block sums fc1_b's gradient in the d_fc2 GEMM's epilogue, before the adapter's share of du
    exists.  With an fc2 adapter it has to be the column sum of the complete du."""
    cfg16 = make_case("Sr", bf16, pre_ln, drop=drop)
    ad = adapters(cfg16, ("fc2",), bf16, b_std=0.5)          # s Bt^T A about as large as fc2_w itself
    cfg32 = dict(cfg16, dtype=f32, params={n: t.float() for n, t in cfg16["params"].items()}, x=cfg16["x"].float(), cot=cfg16["cot"].float())
    lo = run(E, cfg16, ad)
    hi = run(E, cfg32, {k: (a.float(), b.float()) for k, (a, b) in ad.items()})
    mg = run(E, cfg32, weights=merged(cfg32, {k: (a.float(), b.float()) for k, (a, b) in ad.items()}))
    close_fp32(hi["grads"]["fc1_b"], mg["grads"]["fc1_b"], "fc1_b fp32")
    plain = run(E, cfg32)
    assert rel_l2(plain["grads"]["fc1_b"], mg["grads"]["fc1_b"]) > 4 * BF16_GRAD_REL_L2       # the adapter's share is not negligible
    assert rel_l2(lo["grads"]["fc1_b"], hi["grads"]["fc1_b"]) <= BF16_GRAD_REL_L2


@PLACE
@pytest.mark.parametrize("act", ("relu", "gelu_accurate", "tanh", "linear"))
def test_other_activations_with_an_fc1_adapter(E, pre_ln, act):
    cfg = make_case("Sr", f32, pre_ln, drop=True, act=act)
    against_merged(E, cfg, adapters(cfg, ("fc1", "fc2"), f32))


@PLACE
def test_deterministic_mode_repeats_bit_for_bit(E, ops_mod, pre_ln, restore_mode):
    E.set_deterministic(True)
    cfg = make_case("Sr", bf16, pre_ln, drop=True)
    ad = adapters(cfg, ("out", "fc1", "fc2"), bf16, qkv=True)
    before = ops_mod.float_atomic_launches()
    a, b = run(E, cfg, ad), run(E, cfg, ad)
    assert ops_mod.float_atomic_launches() == before
    assert torch.equal(a["y"], b["y"]) and torch.equal(a["dx"], b["dx"])
    for n in a["grads"]:
        assert torch.equal(a["grads"][n], b["grads"][n]), n


@pytest.fixture(scope="module")
def ops_mod():
    from multimodaldiscussiontransformer_amd import ops
    return ops


def test_frozen_adapters_and_inference_keep_nothing(E):
    cfg = make_case("Sr", bf16, False, drop=False)
    ad = adapters(cfg, ("out", "fc1", "fc2"), bf16)
    got = run(E, cfg, ad, frozen_adapters=True)
    tape = got["tape"]
    assert all(got["grads"][s + w] is None for s in ad for w in ("_A", "_Bt")) and got["dx"] is not None
    assert len(tape.tmp_grads) == 12                     # the base parameters' buffers and nothing else
    inf = run(E, make_case("Sr", bf16, False, drop=False, inference=True), ad)
    assert torch.equal(inf["y"], got["y"])


@pytest.mark.parametrize("site", tuple(SITES))
def test_fp8_on_a_block_with_a_dense_adapter_is_refused(E, monkeypatch, site):
    from multimodaldiscussiontransformer_amd import fp8 as F8
    cfg = make_case("Sr", bf16, False, drop=False)
    A, Bt = adapters(cfg, (site,), bf16)[site]
    P = {n: torch.nn.Parameter(dev(cfg["params"][n])) for n in BASE}
    BP = E.BlockParams(**P, **{SITES[site][0]: E.LoraSlot(torch.nn.Parameter(dev(A)), torch.nn.Parameter(dev(Bt)), SCALE)})
    sp = cfg["spec"]
    spec = E.AttnSpec(nseq=sp["nseq"], S=sp["S"], H=sp["H"], seq_offsets=dev(sp["seq_offsets"]))
    monkeypatch.setattr(F8, "ACTIVE", object())              # any state: the block refuses before it asks it anything
    with pytest.raises(NotImplementedError, match="adapters"):
        E.transformer_block(E.Tape(), E.Var(dev(cfg["x"])), BP, spec, pre_ln=False, eps=cfg["eps"])
