"""Activation recomputation at the level of a training step and of the launcher: the Tiny model of oracle.cases.tiny_hparams("A")
(text and images, 4 + 4 layers, D = 768) with dropout 0.1, built as tests/test_deterministic_step_gpu.py builds it.

Deterministic mode: loss and the whole fp32 gradient arena are bit-identical under "none", "ffn" and "block", in fp32 and bf16 and
with rank-8 adapters on all six targets.  Default mode (the two-stream tape; the fixture has images, so image-branch replays run on
the side stream): loss bits are equal and the arena is within the allowance test_switch_leaves_no_state_behind grants two default
runs (atol 2e-5 max(1, |g|max), rtol 1e-4).  The launcher's --checkpoint-activations / --checkpoint-policy reproduce the run
without them bit for bit under --deterministic, and leave the process-wide policy as they found it."""
import pytest
import torch

from tests.test_deterministic_step_gpu import P_DROP, _launcher_argv, _model, _same, _step

pytestmark = pytest.mark.gpu

POLICIES = ("none", "ffn", "block")


@pytest.fixture
def engine():
    from multimodaldiscussiontransformer_amd import engine as E
    from multimodaldiscussiontransformer_amd import fp8
    was_det, was_policy = E.deterministic(), E.recompute()
    yield E
    fp8.ACTIVE = None
    E.set_deterministic(was_det)
    E.set_recompute(was_policy)


def _steps(engine, model, crit, sample, policies=POLICIES, seed=1234):
    out = {}
    for policy in policies:
        engine.set_recompute(policy)
        out[policy] = _step(model, crit, sample, seed=seed)
    engine.set_recompute("none")
    return out


def _assert_arena_bits(runs):
    loss0, grad0 = runs["none"]
    assert bool(torch.isfinite(grad0).all()) and float(grad0.abs().max()) > 0
    for policy in ("ffn", "block"):
        loss, grad = runs[policy]
        assert _same(loss, loss0), f"{policy}: loss bits differ"
        assert _same(grad, grad0), f"{policy}: {int((grad != grad0).sum())} of {grad0.numel()} gradient elements differ"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_deterministic_step_has_the_same_bits_under_every_policy(engine, dtype):
    _, _, model, crit, sample = _model(dtype)
    engine.set_deterministic(True)
    runs = _steps(engine, model, crit, sample)
    _assert_arena_bits(runs)
    # another seed is another step: the comparison above is not vacuous
    engine.set_recompute("block")
    _, other = _step(model, crit, sample, seed=99)
    assert not _same(other, runs["none"][1])


def test_default_step_two_streams(engine):
    _, _, model, crit, sample = _model(torch.float32)
    assert not engine.deterministic()
    runs = _steps(engine, model, crit, sample)
    loss0, grad0 = runs["none"]
    scale = max(1.0, float(grad0.abs().max()))
    for policy in ("ffn", "block"):
        assert _same(runs[policy][0], loss0), f"{policy}: loss bits differ (the forward has no atomics)"
        torch.testing.assert_close(runs[policy][1], grad0, atol=2e-5 * scale, rtol=1e-4)
    engine.set_recompute("block")
    first = runs["block"][1]
    for rep in range(2):            # with the one above: three runs from one seed
        loss, grad = _step(model, crit, sample)
        assert _same(loss, loss0), f"block, repetition {rep + 1}: loss bits differ"
        torch.testing.assert_close(grad, first, atol=2e-5 * scale, rtol=1e-4)


def test_deterministic_step_with_adapters(engine):
    from multimodaldiscussiontransformer_amd.criterions import GraphPredictionNodeCrossEntropy
    from multimodaldiscussiontransformer_amd.data.packer import pack_batch
    from multimodaldiscussiontransformer_amd.models import GraphormerModel
    from oracle import cases
    from tests.util_model import fill_hash_weights, model_args
    hp = cases.tiny_hparams("A")
    trees = cases.tiny_trees("A", hp)
    model = GraphormerModel.build_model(model_args(hp, dropout=P_DROP, attention_dropout=P_DROP, act_dropout=P_DROP), task=None)
    model = fill_hash_weights(model)
    assert model.add_lora(8, targets="all") > 0
    g = torch.Generator().manual_seed(3)
    for n, p in model.named_parameters():           # B = 0 as add_lora leaves it would hide the adapters' t from the comparison
        if n.endswith("lora_Bt"):
            p.data.copy_(torch.randn(p.shape, generator=g) * 0.02)
    model = model.cuda().to(torch.bfloat16).train()
    model.prepare_main_grads()
    crit = GraphPredictionNodeCrossEntropy(None, positive_weight=hp.pos_weight, negative_weight=hp.neg_weight)
    sample = {"nsamples": len(trees), "net_input": {"batched_data": pack_batch(trees, 5).batched_data}}
    engine.set_deterministic(True)
    _assert_arena_bits(_steps(engine, model, crit, sample))


def _launch(train, tmp_path, name, extra):
    hist = train.main(_launcher_argv(tmp_path / name) + extra)
    sd = torch.load(tmp_path / name / "checkpoint_last.pt", weights_only=False)
    model = train.main.last_run["model"]
    n_blocks = sum(len(b) for b in model.pretrained_blocks())          # everything is trainable in this run: every one is covered
    return [h["loss"] for h in hist], sd["model"], set(sd["cfg"]["model"]), n_blocks


def test_launcher_flags_reproduce_the_plain_run(engine, tmp_path, capsys):
    from multimodaldiscussiontransformer_amd import train
    plain = _launch(train, tmp_path, "plain", [])
    assert "activation recomputation" not in capsys.readouterr().err
    for name, extra, policy in (("block", ["--checkpoint-activations"], "block"),
                                ("ffn", ["--checkpoint-activations", "--checkpoint-policy", "ffn"], "ffn")):
        seen = []
        real = engine.transformer_block

        def spy(*a, **k):
            seen.append(k.get("recompute", "none"))
            return real(*a, **k)

        engine.transformer_block = spy
        try:
            got = _launch(train, tmp_path, name, extra)
        finally:
            engine.transformer_block = real
        assert engine.recompute() == "none", "the launcher left the process-wide policy on"
        assert policy in seen, f"no block was recorded under {policy}"
        err = capsys.readouterr().err
        assert f"policy {policy}" in err and f" {got[3]} pretrained" in err and got[3] > 0, err[-400:]
        assert seen.count(policy) >= got[3], f"{seen.count(policy)} blocks recorded under {policy}, {got[3]} expected per forward"
        assert len(plain[0]) == 3 and got[0] == plain[0], (plain[0], got[0])
        assert set(got[1]) == set(plain[1])
        for k, t in plain[1].items():
            assert _same(t, got[1][k]) if t.dtype in (torch.float32, torch.bfloat16) else torch.equal(t, got[1][k]), k
        assert got[2] == plain[2], f"the flag changed the entries of the checkpoint's cfg: {got[2] ^ plain[2]}"
    # the policy is restored when main ends in a SystemExit raised after it was set
    with pytest.raises(SystemExit, match="does not exist"):
        train.main(_launcher_argv(tmp_path / "x") + ["--checkpoint-activations", "--restore-file", str(tmp_path / "no_such.pt")])
    assert engine.recompute() == "none"
