"""engine.transformer_block with low-rank adapters on its QKV projection, on one BERT-shaped (post-LN) and one ViT-shaped (pre-LN)
block at D 128 / 2 heads of 64 (the cases of tests/test_engine_block_gpu.py: ragged lengths (20, 7, 13), or 3 x 20 rows with a key
mask where keep_rows needs whole sequences), dropout off and on:
 (a) Bt = 0: output and dx are bit-identical to the same block without adapters;
 (b) fp32, random adapters: output, dx and the base parameters' gradients equal those of the block run with the merged matrix
     W_j + s Bt_j^T A_j, and dA, dBt equal s Bt_j dW_j and s A_j dW_j^T computed in fp64 from that block's dW — the project's fp32
     gate, 1e-3 of max(1, largest |reference|);
 (c) bf16 against the fp32 run of the same adapted block: relative L2 <= 5e-2 per tensor, the project's bf16 gate;
 (d) keep_rows with q_limit, and a block whose input wants no gradient (the first block behind frozen embeddings);
and the refusal of fp8 GEMMs on an adapted block."""
import pytest
import torch

from tests.rowops_reference import bf16, f32
from tests.test_engine_block_gpu import dev, host, make_case
from tests.test_real_shapes_gpu import BF16_GRAD_REL_L2

pytestmark = pytest.mark.gpu

BASE = ("qkv_w", "qkv_b", "o_w", "o_b", "ln1_w", "ln1_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b", "ln2_w", "ln2_b")
RANK, SCALE = 8, 2.0
PLACE = pytest.mark.parametrize("pre_ln", (False, True), ids=("bert_post_ln", "vit_pre_ln"))
DROP = pytest.mark.parametrize("drop", (False, True), ids=("nodrop", "drop"))


@pytest.fixture(scope="module")
def E():
    from multimodaldiscussiontransformer_amd import engine
    return engine


def adapters(D, cols, dtype, zero_b=False, seed=77):
    """(A, Bt) [|J| r, D] on the host: A as add_lora draws it (U(-1/sqrt D, 1/sqrt D)), Bt random or zero."""
    g = torch.Generator().manual_seed(seed)
    n = len(cols) * RANK
    A = ((torch.rand(n, D, generator=g) * 2 - 1) / D ** 0.5).to(dtype)
    Bt = (torch.zeros(n, D) if zero_b else torch.randn(n, D, generator=g) * 0.05).to(dtype)
    return A, Bt


def merged_qkv(cfg, A, Bt, cols):
    """W with s Bt_j^T A_j added to third c_j, fp64, rounded once to the parameters' dtype."""
    D = cfg["D"]
    w = cfg["params"]["qkv_w"].double().clone()
    for j, c in enumerate(cols):
        rows = slice(j * RANK, (j + 1) * RANK)
        w[c * D:(c + 1) * D] += SCALE * Bt[rows].double().t() @ A[rows].double()
    return w.to(cfg["dtype"])


def run(E, cfg, lora=None, qkv_w=None):
    """One forward + backward of the block.  ``lora``: (A, Bt, cols) or None; ``qkv_w``: replaces the case's projection."""
    sp = cfg["spec"]
    P = {n: torch.nn.Parameter(dev(cfg["params"][n] if (n != "qkv_w" or qkv_w is None) else qkv_w)) for n in BASE}
    extra = {}
    if lora is not None:
        A, Bt, cols = lora
        P["lora_A"], P["lora_Bt"] = torch.nn.Parameter(dev(A)), torch.nn.Parameter(dev(Bt))
        extra = dict(lora_A=P["lora_A"], lora_Bt=P["lora_Bt"], lora_cols=tuple(cols), lora_scale=SCALE)
    BP = E.BlockParams(**{n: P[n] for n in BASE}, **extra)
    spec = E.AttnSpec(nseq=sp["nseq"], S=sp["S"], H=sp["H"], seq_stride=sp["seq_stride"], pos_stride=sp["pos_stride"],
                      key_mask=None if sp.get("key_mask") is None else dev(sp["key_mask"]),
                      seq_offsets=None if sp.get("seq_offsets") is None else dev(sp["seq_offsets"]), q_limit=sp["q_limit"])
    reported = []
    tape = E.Tape(on_params_ready=reported.append)
    torch.manual_seed(cfg["torch_seed"])
    xv = E.Var(dev(cfg["x"]), needs_grad=cfg["x_needs_grad"])
    keep = None if cfg["keep_rows"] is None else dev(cfg["keep_rows"].to(torch.int32))
    o = E.transformer_block(tape, xv, BP, spec, pre_ln=cfg["pre_ln"], eps=cfg["eps"], p_hidden=cfg["p_hidden"], p_attn=cfg["p_attn"],
                            p_act=cfg["p_act"], keep_rows=keep)
    assert tape._seed_ctr == 4, "the adapters add no dropout site: the block takes exactly four seeds"
    o.grad = dev(cfg["cot"])
    tape.backward()
    torch.cuda.synchronize()
    assert len(reported) == 1 and len(reported[0]) == (14 if lora is not None else 12)
    if lora is not None:
        assert reported[0][12] is P["lora_A"] and reported[0][13] is P["lora_Bt"]
    return dict(y=host(o.data), dx=host(xv.grad), grads={n: host(tape.tmp_grads.get(id(p))) for n, p in P.items()})


def close_fp32(got, want, what):
    err = float((got.double() - want.double()).abs().max())
    lim = 1e-3 * max(1.0, float(want.double().abs().max()))
    assert err <= lim, f"{what}: |err| {err:.3e} over {lim:.3e}"


def rel_l2(got, want):
    return float((got.double() - want.double()).norm() / want.double().norm().clamp(min=1e-30))


def adapter_grads_from_dw(dW, A, Bt, cols, D):
    """dA = s Bt_j dW_j, dBt = s A_j dW_j^T in fp64 from the merged block's dW [3 D, D]."""
    dA, dBt = torch.zeros_like(A, dtype=torch.float64), torch.zeros_like(Bt, dtype=torch.float64)
    for j, c in enumerate(cols):
        rows, dWj = slice(j * RANK, (j + 1) * RANK), dW[c * D:(c + 1) * D].double()
        dA[rows] = SCALE * Bt[rows].double() @ dWj
        dBt[rows] = SCALE * A[rows].double() @ dWj.t()
    return dA, dBt


@PLACE
@DROP
@pytest.mark.parametrize("dtype", (bf16, f32), ids=("bf16", "fp32"))
def test_zero_b_is_bit_identical_to_the_plain_block(E, dtype, pre_ln, drop):
    cfg = make_case("Sr", dtype, pre_ln, drop=drop)
    A, Bt = adapters(cfg["D"], (0, 2), dtype, zero_b=True)
    plain, ad = run(E, cfg), run(E, cfg, lora=(A, Bt, (0, 2)))
    assert torch.equal(plain["y"], ad["y"]) and torch.equal(plain["dx"], ad["dx"])
    assert float(ad["grads"]["lora_A"].abs().max()) == 0.0          # dt = s dqkv Bt^T = 0
    assert float(ad["grads"]["lora_Bt"].abs().max()) > 0.0          # and Bt does learn from the first step


@PLACE
@DROP
@pytest.mark.parametrize("cols", ((0, 2), (1,), (0, 1, 2)), ids=("qv", "k", "qkv"))
def test_fp32_equals_the_merged_block(E, pre_ln, drop, cols):
    cfg = make_case("Sr", f32, pre_ln, drop=drop)
    A, Bt = adapters(cfg["D"], cols, f32)
    ad = run(E, cfg, lora=(A, Bt, cols))
    mg = run(E, cfg, qkv_w=merged_qkv(cfg, A, Bt, cols))
    close_fp32(ad["y"], mg["y"], "output")
    close_fp32(ad["dx"], mg["dx"], "dx")
    for n in BASE:
        close_fp32(ad["grads"][n], mg["grads"][n], n)
    dA, dBt = adapter_grads_from_dw(mg["grads"]["qkv_w"], A, Bt, cols, cfg["D"])
    close_fp32(ad["grads"]["lora_A"], dA, "dA")
    close_fp32(ad["grads"]["lora_Bt"], dBt, "dBt")
    assert float(dA.abs().max()) > 1e-2 and float(dBt.abs().max()) > 1e-2      # the comparison is not one of zeros


@PLACE
@DROP
def test_bf16_against_fp32(E, pre_ln, drop):
    cfg16 = make_case("Sr", bf16, pre_ln, drop=drop)
    A, Bt = adapters(cfg16["D"], (0, 2), bf16)
    cfg32 = dict(cfg16, dtype=f32, params={n: t.float() for n, t in cfg16["params"].items()}, x=cfg16["x"].float(), cot=cfg16["cot"].float())
    lo = run(E, cfg16, lora=(A, Bt, (0, 2)))
    hi = run(E, cfg32, lora=(A.float(), Bt.float(), (0, 2)))
    worst = {"y": rel_l2(lo["y"], hi["y"]), "dx": rel_l2(lo["dx"], hi["dx"])}
    worst.update({n: rel_l2(lo["grads"][n], hi["grads"][n]) for n in BASE + ("lora_A", "lora_Bt")})
    print({k: f"{v:.2e}" for k, v in worst.items()})
    over = {k: v for k, v in worst.items() if not v <= BF16_GRAD_REL_L2}
    assert not over, f"relative L2 over {BF16_GRAD_REL_L2}: {over}"


@PLACE
@pytest.mark.parametrize("dtype", (bf16, f32), ids=("bf16", "fp32"))
def test_keep_rows(E, dtype, pre_ln):
    cfg = make_case("S", f32, pre_ln, keep=True, drop=False)
    A, Bt = adapters(cfg["D"], (0, 2), f32)
    if dtype == f32:
        mg = run(E, cfg, qkv_w=merged_qkv(cfg, A, Bt, (0, 2)))
        dA, dBt = adapter_grads_from_dw(mg["grads"]["qkv_w"], A, Bt, (0, 2), cfg["D"])
        ad = run(E, cfg, lora=(A, Bt, (0, 2)))
        assert ad["y"].shape[0] == 6
        for got, want, what in ((ad["y"], mg["y"], "output"), (ad["dx"], mg["dx"], "dx"), (ad["grads"]["lora_A"], dA, "dA"),
                                (ad["grads"]["lora_Bt"], dBt, "dBt"), (ad["grads"]["o_w"], mg["grads"]["o_w"], "o_w")):
            close_fp32(got, want, what)
    else:
        c16 = make_case("S", bf16, pre_ln, keep=True, drop=False)
        ad = run(E, c16, lora=(A.to(bf16), Bt.to(bf16), (0, 2)))
        c32 = dict(c16, dtype=f32, params={n: t.float() for n, t in c16["params"].items()}, x=c16["x"].float(), cot=c16["cot"].float())
        hi = run(E, c32, lora=(A.to(bf16).float(), Bt.to(bf16).float(), (0, 2)))
        for n in ("lora_A", "lora_Bt"):
            assert rel_l2(ad["grads"][n], hi["grads"][n]) <= BF16_GRAD_REL_L2, n
        assert rel_l2(ad["y"], hi["y"]) <= BF16_GRAD_REL_L2 and rel_l2(ad["dx"], hi["dx"]) <= BF16_GRAD_REL_L2


@PLACE
def test_input_without_gradient(E, pre_ln):
    """The first block behind frozen embeddings: no dx is made, the adapters' gradients are the same."""
    cfg = make_case("Sr", f32, pre_ln, x_needs_grad=False, drop=False)
    A, Bt = adapters(cfg["D"], (0, 2), f32)
    ad = run(E, cfg, lora=(A, Bt, (0, 2)))
    mg = run(E, cfg, qkv_w=merged_qkv(cfg, A, Bt, (0, 2)))
    assert ad["dx"] is None and mg["dx"] is None
    dA, dBt = adapter_grads_from_dw(mg["grads"]["qkv_w"], A, Bt, (0, 2), cfg["D"])
    close_fp32(ad["grads"]["lora_A"], dA, "dA")
    close_fp32(ad["grads"]["lora_Bt"], dBt, "dBt")
    close_fp32(ad["y"], mg["y"], "output")


def test_frozen_adapters_and_inference_keep_nothing(E):
    cfg = make_case("Sr", bf16, False, drop=False)
    A, Bt = adapters(cfg["D"], (0, 2), bf16)
    sp = cfg["spec"]
    P = {n: torch.nn.Parameter(dev(cfg["params"][n])) for n in BASE}
    la, lb = torch.nn.Parameter(dev(A), requires_grad=False), torch.nn.Parameter(dev(Bt), requires_grad=False)
    BP = E.BlockParams(**P, lora_A=la, lora_Bt=lb, lora_cols=(0, 2), lora_scale=SCALE)
    spec = E.AttnSpec(nseq=sp["nseq"], S=sp["S"], H=sp["H"], seq_offsets=dev(sp["seq_offsets"]))
    tape = E.Tape()
    xv = E.Var(dev(cfg["x"]))
    o = E.transformer_block(tape, xv, BP, spec, pre_ln=False, eps=cfg["eps"])
    o.grad = dev(cfg["cot"])
    tape.backward()
    assert id(la) not in tape.tmp_grads and id(lb) not in tape.tmp_grads and xv.grad is not None      # frozen adapters: no buffers, dx still flows
    inf = E.Tape(inference=True)
    o2 = E.transformer_block(inf, E.Var(dev(cfg["x"])), BP, spec, pre_ln=False, eps=cfg["eps"])
    assert inf.ops == [] and torch.equal(o2.data, o.data)


def test_fp8_on_an_adapted_block_is_refused(E, monkeypatch):
    from multimodaldiscussiontransformer_amd import fp8 as F8
    cfg = make_case("Sr", bf16, False, drop=False)
    A, Bt = adapters(cfg["D"], (0, 2), bf16)
    P = {n: torch.nn.Parameter(dev(cfg["params"][n])) for n in BASE}
    BP = E.BlockParams(**P, lora_A=torch.nn.Parameter(dev(A)), lora_Bt=torch.nn.Parameter(dev(Bt)), lora_cols=(0, 2), lora_scale=SCALE)
    sp = cfg["spec"]
    spec = E.AttnSpec(nseq=sp["nseq"], S=sp["S"], H=sp["H"], seq_offsets=dev(sp["seq_offsets"]))
    monkeypatch.setattr(F8, "ACTIVE", object())              # any state: the block refuses before it asks it anything
    with pytest.raises(NotImplementedError, match="adapters"):
        E.transformer_block(E.Tape(), E.Var(dev(cfg["x"])), BP, spec, pre_ln=False, eps=cfg["eps"])
