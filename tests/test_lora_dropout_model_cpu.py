"""--lora-dropout and add_lora(dropout=...), module structure only (CPU): the flag's parsing and refusals, the ``lora_dropout``
checkpoint-cfg key present only when the flag is given and > 0, the range check of add_lora, where the probability is stored,
that blocks hand it to the engine in training mode only, and that it adds no parameter and no state-dict key."""
import pytest
import torch

from oracle import cases
from tests.util_model import model_args


def _build(**over):
    from multimodaldiscussiontransformer_amd.models import GraphormerModel
    torch.manual_seed(5)
    return GraphormerModel.build_model(model_args(cases.tiny_hparams("A"), **over), task=None)


def test_launcher_flag():
    from multimodaldiscussiontransformer_amd import train
    a = train.build_parser().parse_args(["--lora-rank", "16", "--lora-dropout", "0.05"])
    assert a.lora_dropout == 0.05
    assert train.build_parser().parse_args([]).lora_dropout is None


@pytest.mark.parametrize("flags,msg", [
    (["--lora-dropout", "0.1"], "--lora-dropout without --lora-rank"),
    (["--lora-rank", "8", "--lora-dropout", "1"], r"--lora-dropout must be in \[0, 1\)"),
    (["--lora-rank", "8", "--lora-dropout", "-0.1"], r"--lora-dropout must be in \[0, 1\)"),
    (["--lora-rank", "8", "--lora-dropout", "nan"], r"--lora-dropout must be in \[0, 1\)"),
    (["--lora-rank", "8", "--lora-dropout", "0.1", "--fp8"], "--fp8 with --lora-rank"),
])
def test_launcher_refuses_bad_flags(flags, msg):
    from multimodaldiscussiontransformer_amd import train
    with pytest.raises(SystemExit, match=msg):
        train.main(["--dataset-name", "synthetic", "--max-update", "1"] + flags)


@pytest.mark.parametrize("flags,want", [([], None), (["--lora-dropout", "0"], None), (["--lora-dropout", "0.1"], 0.1)])
def test_cfg_key_only_when_set(monkeypatch, flags, want):
    """The launcher's argument namespace is the checkpoint's cfg: it is caught where the model is built from it."""
    from multimodaldiscussiontransformer_amd import train
    from multimodaldiscussiontransformer_amd.registry import TASK_REGISTRY
    seen = {}

    class Stop(Exception):
        pass

    def build_model(self, args):
        seen.update(vars(args))
        raise Stop

    monkeypatch.setattr(TASK_REGISTRY["node_prediction"][0], "build_model", build_model)
    monkeypatch.setattr(torch.cuda, "set_device", lambda *_: None)
    with pytest.raises(Stop):
        train.main(["--task", "node_prediction", "--dataset-name", "synthetic", "--max-update", "1", "--lora-rank", "8"] + flags)
    assert seen["lora_rank"] == 8
    assert ("lora_dropout" in seen) == (want is not None)
    if want is not None:
        assert seen["lora_dropout"] == want
    seen.clear()
    with pytest.raises(Stop):                             # a run without adapters: the cfg it always wrote
        train.main(["--task", "node_prediction", "--dataset-name", "synthetic", "--max-update", "1"])
    assert not any(k.startswith("lora_") for k in seen)


@pytest.mark.parametrize("p", [1.0, -0.1, 1.5, float("nan")])
def test_add_lora_range_check(p):
    model = _build()
    with pytest.raises(ValueError, match=r"dropout .* is not in \[0, 1\)"):
        model.add_lora(8, targets="all", dropout=p)
    assert not model.lora_modules() and not model.lora_dense_modules()          # refused before anything was added


def test_add_lora_stores_the_probability_and_blocks_pass_it_in_training_only():
    plain, model = _build(), _build()
    plain.add_lora(8, targets="all")
    model.add_lora(8, targets="all", dropout=0.1)
    assert sorted(plain.state_dict()) == sorted(model.state_dict())               # no parameter, no key
    assert [n for n, _ in plain.named_parameters()] == [n for n, _ in model.named_parameters()]
    prefix, fusion = model.pretrained_blocks()
    model.train()
    for b in prefix + fusion:
        assert b.lora_dropout_p == 0.1 and b.drop_kwargs()["p_lora"] == 0.1
    for b in sum(plain.pretrained_blocks(), []):
        assert b.lora_dropout_p == 0.0 and "p_lora" not in b.drop_kwargs()       # the keywords of a block without the feature
    model.eval()
    assert all("p_lora" not in b.drop_kwargs() for b in prefix + fusion)
    model.train()
    assert model.merge_lora() > 0
    assert all(b.lora_dropout_p == 0.0 for b in prefix + fusion)
    assert sorted(model.state_dict()) == sorted(_build().state_dict())


def test_frozen_prefixes_get_no_probability():
    model = _build(freeze_initial_encoders=True)
    model.add_lora(8, targets="q,v", dropout=0.2)
    prefix, fusion = model.pretrained_blocks()
    assert all(b.lora_dropout_p == 0.0 for b in prefix) and all(b.lora_dropout_p == 0.2 for b in fusion)


def test_build_model_reads_the_cfg_key():
    model = _build(lora_rank=8, lora_targets="all", lora_dropout=0.1)
    assert all(b.lora_dropout_p == 0.1 for b in sum(model.pretrained_blocks(), []))
    model = _build(lora_rank=8, lora_targets="all")
    assert all(b.lora_dropout_p == 0.0 for b in sum(model.pretrained_blocks(), []))
