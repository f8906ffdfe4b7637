"""Activation recomputation at the level of one block (engine.transformer_block ``recompute`` = "none" / "ffn" / "block"), on the
cases of tests/test_engine_block_gpu.py with dropout on (p_hidden 0.25, p_attn 0.25, p_act 0.5).

The forward has no float atomics and the dropout masks are functions of the four site seeds, so a replayed forward writes the
bits the first pass wrote.  In deterministic mode the adjoint has no float atomics either: output, input gradient and every
parameter gradient are compared as integers across the three policies.  In the default mode the output is still bit-identical and
the gradients differ by the order of the fp32 atomics only: the allowance tests/test_deterministic_step_gpu.py
(test_switch_leaves_no_state_behind) grants two default runs, atol 2e-5 max(1, |g|max), rtol 1e-4.  bf16 at 8192 rows is held to
the same allowance: the gradient buffers are fp32 there too, their addends are products of bit-identical bf16 operands, each
split-K slab is summed in a fixed order inside its tile, and only the order in which the at most 8 slabs (and the column-sum
partials that ride on them) land varies — a few fp32 roundings of the partial sums, well inside 2e-5 of the largest element.

A spy on ops.attention_fwd, ops.gemm and ops.layernorm_fwd shows that the recomputation happens, and only where the policy says."""
import pytest
import torch

from tests.rowops_reference import bf16, f32
from tests.test_engine_block_gpu import dev, device_spec, make_case
from tests.test_lora_dense_block_gpu import QKV, SCALE, SITES, adapters

pytestmark = pytest.mark.gpu

POLICIES = ("none", "ffn", "block")
BASE = ("qkv_w", "qkv_b", "o_w", "o_b", "ln1_w", "ln1_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b", "ln2_w", "ln2_b")
DT = pytest.mark.parametrize("dtype", (f32, bf16), ids=("fp32", "bf16"))
PLACE = pytest.mark.parametrize("pre_ln", (False, True), ids=("post", "pre"))
LORA = pytest.mark.parametrize("lora", (False, True), ids=("plain", "lora6"))


@pytest.fixture
def engine():
    from multimodaldiscussiontransformer_amd import engine as E
    from multimodaldiscussiontransformer_amd import fp8
    was_det, was_policy = E.deterministic(), E.recompute()
    yield E
    fp8.ACTIVE = None
    E.set_deterministic(was_det)
    E.set_recompute(was_policy)


def build(E, cfg, lora):
    """Device parameters of the case → (name -> Parameter, BlockParams, AttnSpec)"""
    P = {n: torch.nn.Parameter(dev(t)) for n, t in cfg["params"].items()}
    extra = {}
    if lora:                    # rank 8 on all six targets, B random (a zero B would hide the adapters' t from the comparison)
        for site, (A, Bt) in adapters(cfg, ("out", "fc1", "fc2"), cfg["dtype"], qkv=True).items():
            a, b = torch.nn.Parameter(dev(A)), torch.nn.Parameter(dev(Bt))
            P[site + "_A"], P[site + "_Bt"] = a, b
            if site == "qkv":
                extra.update(lora_A=a, lora_Bt=b, lora_cols=QKV, lora_scale=SCALE)
            else:
                extra[SITES[site][0]] = E.LoraSlot(a, b, SCALE)
    return P, E.BlockParams(**{n: P[n] for n in BASE}, **extra), device_spec(E, cfg, P)


def run(E, cfg, policy, *, lora=False, inference=False, built=None, between=None, hook=None):
    """One forward + backward of the block recorded under ``policy`` → device copies of output, dx and the gradient buffers.
    ``built``: called with the parameters before the forward; ``between``: called after the forward, before the backward."""
    P, BP, spec = build(E, cfg, lora)
    if built is not None:
        built(P)
    tape = E.Tape(inference=inference)
    if hook is not None:
        tape.on_params_ready = lambda params: hook(tape, P, BP, params)
    torch.manual_seed(cfg["torch_seed"])
    xv = E.Var(dev(cfg["x"]), needs_grad=cfg["x_needs_grad"])
    keep = None if cfg["keep_rows"] is None else dev(cfg["keep_rows"].to(torch.int32))
    o = E.transformer_block(tape, xv, BP, spec, pre_ln=cfg["pre_ln"], eps=cfg["eps"], p_hidden=cfg["p_hidden"], p_attn=cfg["p_attn"],
                            p_act=cfg["p_act"], keep_rows=keep, act=cfg["act"], recompute=policy)
    res = dict(y=o.data.clone(), seed_ctr=tape._seed_ctr, seed_base=tape._seed_base)
    if inference:
        assert tape.ops == []
        torch.cuda.synchronize()
        return res
    if between is not None:
        between()
    o.grad = dev(cfg["cot"])
    tape.backward()
    torch.cuda.synchronize()
    res.update(dx=None if xv.grad is None else xv.grad.clone(), grads={n: tape.tmp_grads.get(id(p)) for n, p in P.items()})
    return res


def same(a, b):
    """bit equality, as integers (tests/test_deterministic_step_gpu.py _same)"""
    if a is None or b is None:
        return a is None and b is None
    view = torch.int32 if a.dtype == torch.float32 else torch.int16
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(view), b.view(view))


def assert_same_bits(ref, got, what):
    assert same(ref["y"], got["y"]), f"{what}: output bits differ"
    assert same(ref["dx"], got["dx"]), f"{what}: dx bits differ"
    assert set(ref["grads"]) == set(got["grads"])
    for n, g in ref["grads"].items():
        assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, f"{what}: {n} has no gradient to compare"
        assert same(g, got["grads"][n]), f"{what}: {n}: {int((g != got['grads'][n]).sum())} gradient elements differ"


def compare_policies(E, cfg, lora):
    ref = run(E, cfg, "none", lora=lora)
    assert (ref["dx"] is not None) == cfg["x_needs_grad"]
    for policy in ("ffn", "block"):
        assert_same_bits(ref, run(E, cfg, policy, lora=lora), f"{policy} against none")
    return ref


# ------------------------------------------------------------------------------------------------ deterministic mode: bits
@DT
@PLACE
@LORA
@pytest.mark.parametrize("act", ("gelu", "relu"))
@pytest.mark.parametrize("keep", (False, True), ids=("allrows", "keeprows"))
@pytest.mark.parametrize("x_grad", (True, False), ids=("dx", "nodx"))
def test_policies_give_the_same_bits(engine, dtype, pre_ln, lora, act, keep, x_grad):
    engine.set_deterministic(True)
    cfg = make_case("S", dtype, pre_ln, keep=keep, act=act, x_needs_grad=x_grad, deterministic=True)
    ref = compare_policies(engine, cfg, lora)
    # another seed gives other bits: the comparison is not vacuous
    other = run(engine, dict(cfg, torch_seed=cfg["torch_seed"] + 1), "block", lora=lora)
    assert not same(ref["y"], other["y"])


@DT
@PLACE
@pytest.mark.parametrize("shape,act,lora", (("Sr", "gelu", False), ("Sr", "relu", True), ("G", "relu", False), ("R8192", "gelu", False),
                                            ("R8192", "gelu", True)))
def test_policies_give_the_same_bits_other_shapes(engine, dtype, pre_ln, shape, act, lora):
    """ragged lengths 20 / 7 / 13 with length bins; the graph layer's time-major structural-bias spec; 8192 rows"""
    engine.set_deterministic(True)
    compare_policies(engine, make_case(shape, dtype, pre_ln, act=act, deterministic=True), lora)


# ------------------------------------------------------------------------------------------------ default mode
@PLACE
@pytest.mark.parametrize("shape,dtype", (("S", f32), ("R8192", f32), ("R8192", bf16)), ids=("S-fp32", "R8192-fp32", "R8192-bf16"))
def test_default_mode_output_bits_and_gradient_allowance(engine, pre_ln, shape, dtype):
    """R8192 in bf16 is the first size at which the dense bias gradients ride on the weight-gradient GEMMs (engine.dyd_rides)."""
    engine.set_deterministic(False)
    cfg = make_case(shape, dtype, pre_ln)
    ref = run(engine, cfg, "none")
    for policy in ("ffn", "block"):
        got = run(engine, cfg, policy)
        assert same(ref["y"], got["y"]), f"{policy}: output bits differ"
        assert same(ref["dx"], got["dx"]), f"{policy}: dx comes from GEMMs and LayerNorm rows only, no atomics"
        for n, g in ref["grads"].items():
            scale = max(1.0, float(g.abs().max()))
            torch.testing.assert_close(got["grads"][n], g, atol=2e-5 * scale, rtol=1e-4, msg=lambda m: f"{policy}: {n}: {m}")


# ------------------------------------------------------------------------------------------------ what is launched
class Spy:
    """Counts ops.attention_fwd / layernorm_fwd calls and the forward-form (no transposition flag) ops.gemm calls per weight."""

    def __init__(self, ops, mp, P):
        self.counts = dict(attention_fwd=0, layernorm_fwd=0, qkv_w=0, o_w=0, fc1_w=0, fc2_w=0)
        ptr = {P[n].data_ptr(): n for n in ("qkv_w", "o_w", "fc1_w", "fc2_w")}
        real = {n: getattr(ops, n) for n in ("attention_fwd", "layernorm_fwd", "gemm")}

        def counted(name):
            def f(*a, **k):
                self.counts[name] += 1
                return real[name](*a, **k)
            return f

        def gemm(a, b, *rest, **k):
            if not k.get("trans_a") and not k.get("trans_b") and not rest and b.data_ptr() in ptr:
                self.counts[ptr[b.data_ptr()]] += 1
            return real["gemm"](a, b, *rest, **k)

        mp.setattr(ops, "attention_fwd", counted("attention_fwd"))
        mp.setattr(ops, "layernorm_fwd", counted("layernorm_fwd"))
        mp.setattr(ops, "gemm", gemm)


def spied(E, monkeypatch, cfg, policy, inference=False):
    """→ (the spy's counts, the on_params_ready calls as (parameter list matches BlockParams.all(), gradient snapshot))"""
    from multimodaldiscussiontransformer_amd import ops
    calls = []

    def hook(tape, P, BP, params):
        torch.cuda.synchronize()
        calls.append((len(params) == len(BP.all()) and all(a is b for a, b in zip(params, BP.all())),
                      {n: tape.tmp_grads[id(p)].clone() for n, p in P.items()}))

    spies = []
    with monkeypatch.context() as mp:
        res = run(E, cfg, policy, inference=inference, built=lambda P: spies.append(Spy(ops, mp, P)), hook=hook)
    return spies[0].counts, calls, res


@PLACE
def test_recomputation_happens_and_only_there(engine, monkeypatch, pre_ln):
    engine.set_deterministic(False)
    cfg = make_case("S", f32, pre_ln)
    counts = {}
    for policy in POLICIES:
        counts[policy], calls, res = spied(engine, monkeypatch, cfg, policy)
        # once per block, with the block's parameter list, after the last gradient write: what the hook saw is what is there at the end
        assert len(calls) == 1 and calls[0][0], f"{policy}: on_params_ready calls {[c[0] for c in calls]}"
        for n, g in res["grads"].items():
            assert same(calls[0][1][n], g), f"{policy}: {n} was written after on_params_ready"
    none, ffn, block = (counts[p] for p in POLICIES)
    assert none == dict(attention_fwd=1, layernorm_fwd=2, qkv_w=1, o_w=1, fc1_w=1, fc2_w=1), none
    assert block == {k: 2 * v for k, v in none.items()}, block
    assert ffn == dict(none, fc1_w=2), ffn


def test_an_inference_tape_ignores_the_policy(engine, monkeypatch):
    cfg = make_case("S", f32, False)
    seen = [spied(engine, monkeypatch, cfg, policy, inference=True) for policy in POLICIES]
    assert seen[0][0] == seen[1][0] == seen[2][0] == dict(attention_fwd=1, layernorm_fwd=2, qkv_w=1, o_w=1, fc1_w=1, fc2_w=1)
    assert same(seen[0][2]["y"], seen[1][2]["y"]) and same(seen[0][2]["y"], seen[2][2]["y"])


# ------------------------------------------------------------------------------------------------ capture, seeds, refusals
def test_policy_is_captured_when_the_block_is_recorded(engine, monkeypatch):
    """The process-wide switch flips between forward and backward: the replay still happens, with the recorded policy's result."""
    engine.set_deterministic(True)
    cfg = make_case("S", bf16, False, deterministic=True)
    engine.set_recompute("block")
    ref = run(engine, cfg, engine.recompute())
    assert engine.recompute() == "block"
    from multimodaldiscussiontransformer_amd import ops
    n_attn = []
    real = ops.attention_fwd
    monkeypatch.setattr(ops, "attention_fwd", lambda *a, **k: (n_attn.append(1), real(*a, **k))[1])
    got = run(engine, cfg, engine.recompute(), between=lambda: engine.set_recompute("none"))
    assert engine.recompute() == "none"
    assert len(n_attn) == 2, "the adjoint recorded under 'block' did not replay the forward"
    assert_same_bits(ref, got, "policy switched before backward")


@PLACE
def test_seed_counter_is_the_same_under_every_policy(engine, pre_ln):
    cfg = make_case("S", f32, pre_ln)
    seen = [run(engine, cfg, policy) for policy in POLICIES]
    assert [r["seed_ctr"] for r in seen] == [4, 4, 4]
    assert seen[0]["seed_base"] == seen[1]["seed_base"] == seen[2]["seed_base"]


def test_refusals(engine):
    from multimodaldiscussiontransformer_amd import fp8
    from tests.test_deterministic_step_gpu import _model
    assert engine.recompute() in POLICIES
    was = engine.recompute()
    with pytest.raises(ValueError, match="bogus"):
        engine.set_recompute("bogus")
    assert engine.recompute() == was
    cfg = make_case("S", bf16, False)
    with pytest.raises(ValueError, match="bogus"):
        run(engine, cfg, "bogus")
    _, _, model, _, _ = _model(torch.bfloat16)
    engine.set_recompute("none")
    assert model.enable_fp8() is fp8.ACTIVE is not None
    try:
        for policy in ("ffn", "block"):
            with pytest.raises(NotImplementedError, match="amax"):
                engine.set_recompute(policy)
            assert engine.recompute() == "none"
            with pytest.raises(NotImplementedError, match="amax"):       # a block reached with both
                run(engine, cfg, policy)
        engine.set_recompute("none")                                      # switching it off is never refused
    finally:
        model.enable_fp8(False)
    assert fp8.ACTIVE is None
    for policy in ("ffn", "block"):
        engine.set_recompute(policy)
        with pytest.raises(NotImplementedError, match="amax"):
            model.enable_fp8()
        assert engine.recompute() == policy and fp8.ACTIVE is None
