"""Activation recomputation, what needs no device: the process-wide policy and its environment default, the launcher's flag
validation, and that the policy is no property of the model (same state-dict keys, same parser defaults)."""
import os
import subprocess
import sys

import pytest
import torch

from oracle import cases
from tests.util_model import model_args


@pytest.fixture
def engine():
    from multimodaldiscussiontransformer_amd import engine as E
    was = E.recompute()
    yield E
    E.set_recompute(was)


def test_environment_sets_the_default():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "from multimodaldiscussiontransformer_amd import engine; print(engine.recompute())"
    for val, want in ((None, "none"), ("none", "none"), ("ffn", "ffn"), ("block", "block")):
        env = {k: v for k, v in os.environ.items() if k != "MDT_RECOMPUTE"}
        if val is not None:
            env["MDT_RECOMPUTE"] = val
        r = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip() == want, (val, r.stdout, r.stderr[-300:])
    r = subprocess.run([sys.executable, "-c", code], cwd=root, env=dict(os.environ, MDT_RECOMPUTE="everything"), capture_output=True, text=True)
    assert r.returncode != 0 and "ValueError" in r.stderr and "everything" in r.stderr, r.stderr[-300:]


def test_policy_switch(engine):
    for policy in ("ffn", "block", "none"):
        engine.set_recompute(policy)
        assert engine.recompute() == policy
    engine.set_recompute("ffn")
    for bad in ("bogus", "", None, "Block", True):
        with pytest.raises(ValueError, match="none, ffn, block"):
            engine.set_recompute(bad)
        assert engine.recompute() == "ffn"


@pytest.mark.parametrize("flags,msg", [
    (["--checkpoint-policy", "ffn"], "--checkpoint-policy without --checkpoint-activations"),
    (["--checkpoint-policy", "block"], "--checkpoint-policy without --checkpoint-activations"),
    (["--checkpoint-activations", "--fp8"], "--checkpoint-activations with --fp8.*amax"),
    (["--checkpoint-activations", "--checkpoint-policy", "ffn", "--fp8"], "--checkpoint-activations with --fp8.*amax"),
    (["--checkpoint-activations", "--offload-activations"], "unsupported FairSeq flag.*--offload-activations"),
])
def test_launcher_refuses_bad_flags(engine, flags, msg):
    from multimodaldiscussiontransformer_amd import train
    with pytest.raises(SystemExit, match=msg):
        train.main(["--dataset-name", "synthetic", "--max-update", "1"] + flags)
    assert engine.recompute() == "none"


def test_parser_knows_the_flags():
    from multimodaldiscussiontransformer_amd import train
    a = train.build_parser().parse_args([])
    assert a.checkpoint_activations is False and a.checkpoint_policy is None
    b = train.build_parser().parse_args(["--checkpoint-activations", "--checkpoint-policy", "ffn"])
    assert b.checkpoint_activations is True and b.checkpoint_policy == "ffn"
    with pytest.raises(SystemExit):
        train.build_parser().parse_args(["--checkpoint-activations", "--checkpoint-policy", "none"])


def test_state_dict_keys_do_not_depend_on_the_policy(engine):
    from multimodaldiscussiontransformer_amd.models import GraphormerModel
    keys = {}
    for policy in ("none", "ffn", "block"):
        engine.set_recompute(policy)
        torch.manual_seed(5)
        sd = GraphormerModel.build_model(model_args(cases.tiny_hparams("A")), task=None).state_dict()
        keys[policy] = {k: (tuple(v.shape), v.dtype) for k, v in sd.items()}
    assert keys["none"] and keys["ffn"] == keys["none"] and keys["block"] == keys["none"]
