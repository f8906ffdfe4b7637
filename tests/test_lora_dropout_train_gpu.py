"""The launcher with --lora-rank 8 --lora-dropout 0.1 on the tiny --bert-config / --vit-config shapes of
tests/test_lora_train_gpu.py: the adapters move and every frozen tensor keeps its bits; a checkpoint carries ``lora_dropout`` and
resumes bit for bit; --deterministic runs repeat bit for bit; --checkpoint-activations with either policy reproduces the loss
bit for bit (the site seeds are drawn outside the recomputed region); in eval mode the probability is not applied; --save-merged
still writes a plain checkpoint that loads into a model built without adapters."""
import argparse
import math

import pytest
import torch

from tests.test_lora_train_gpu import argv as lora_argv
from tests.test_lora_train_gpu import masters

pytestmark = pytest.mark.gpu

ALL = ["--lora-targets", "all"]


def argv(extra, dropout="0", p="0.1"):
    return lora_argv(["--lora-dropout", p] + extra, dropout=dropout)


def test_adapters_train_and_frozen_tensors_keep_their_bits(capsys):
    from multimodaldiscussiontransformer_amd import train
    train.main(argv(["--max-update", "1", "--no-save"] + ALL, dropout="0.1"))
    one = {n: p.detach().clone() for n, p in train.main.last_run["model"].named_parameters()}
    err = capsys.readouterr().err
    assert "--lora-rank 8:" in err and "dropout 0.1" in err
    hist = train.main(argv(["--max-update", "12", "--no-save"] + ALL, dropout="0.1"))
    model = train.main.last_run["model"]
    assert len(hist) == 12 and all(math.isfinite(h["loss"]) for h in hist)
    prefix, fusion = model.pretrained_blocks()
    assert all(b.lora_dropout_p == 0.1 and b.drop_kwargs()["p_lora"] == 0.1 for b in prefix + fusion)
    ids = model.encoder_layer_ids()
    n_frozen = n_adapters = 0
    for n, p in model.named_parameters():
        if id(p) in ids and "lora_" not in n:
            assert not p.requires_grad
            assert torch.equal(p.detach().view(torch.int16), one[n].view(torch.int16)), f"{n}: a frozen tensor changed"
            n_frozen += 1
        elif "lora_" in n:
            assert p.requires_grad and float(p.detach().float().abs().max()) > 0 and not torch.equal(p.detach(), one[n]), f"{n} did not move"
            n_adapters += 1
    assert n_adapters == 2 * (len(model.lora_modules()) + len(model.lora_dense_modules())) and n_adapters >= 16 and n_frozen > 20


def test_the_masks_change_the_run():
    from multimodaldiscussiontransformer_amd import train
    """B = 0 at the first update, so the loss is that of the run without the flag — but dB = s tᵀ g reads t = dropout(x) Aᵀ, so
    the gradient arena already differs (the bf16 loss of these tiny runs is too coarse to show the masks within a few updates)."""
    a = train.main(argv(["--max-update", "1", "--no-save", "--deterministic"] + ALL))
    ga = train.main.last_run["model"].main_grad_flat.clone()
    b = train.main(lora_argv(["--max-update", "1", "--no-save", "--deterministic"] + ALL))
    gb = train.main.last_run["model"].main_grad_flat.clone()
    assert a[0]["loss"] == b[0]["loss"]
    assert ga.shape == gb.shape and float(ga.abs().max()) > 0 and not torch.equal(ga, gb)


def test_checkpoint_resume_is_bit_for_bit(tmp_path):
    from multimodaldiscussiontransformer_amd import train
    full = train.main(argv(["--max-update", "8", "--no-save", "--deterministic"] + ALL))
    want = masters(train.main.last_run)
    d = tmp_path / "ck"
    train.main(argv(["--max-update", "4", "--save-dir", str(d), "--deterministic"] + ALL))
    ck = d / "checkpoint_last.pt"
    st = torch.load(ck, weights_only=False)
    assert st["cfg"]["model"]["lora_rank"] == 8 and st["cfg"]["model"]["lora_dropout"] == 0.1
    assert not any("dropout" in k for k in st["model"])                   # no state-dict key
    second = train.main(argv(["--max-update", "8", "--restore-file", str(ck), "--no-save", "--deterministic"] + ALL))
    assert [h["num_updates"] for h in second] == [5, 6, 7, 8]
    assert [h["loss"] for h in second] == [h["loss"] for h in full[4:]]
    got = masters(train.main.last_run)
    for n in want:
        assert torch.equal(want[n].view(torch.uint8), got[n].view(torch.uint8)), f"{n} differs after the resume"


def test_deterministic_runs_repeat_and_recompute_reproduces_the_loss():
    from multimodaldiscussiontransformer_amd import ops, train
    runs = []
    for extra in ([], [], ["--checkpoint-activations", "--checkpoint-policy", "ffn"], ["--checkpoint-activations", "--checkpoint-policy", "block"]):
        before = ops.float_atomic_launches()
        hist = train.main(argv(["--max-update", "3", "--no-save", "--deterministic"] + ALL + extra, dropout="0.1"))
        assert ops.float_atomic_launches() == before
        runs.append(([h["loss"] for h in hist], train.main.last_run["model"].main_grad_flat.clone()))
    assert float(runs[0][1].abs().max()) > 0
    for losses, grads in runs[1:]:
        assert losses == runs[0][0]
        assert torch.equal(grads.view(torch.int32), runs[0][1].view(torch.int32))


def test_eval_mode_does_not_drop():
    from multimodaldiscussiontransformer_amd import train
    train.main(argv(["--max-update", "3", "--no-save"] + ALL, p="0.3"))
    run = train.main.last_run
    model = run["model"]
    prefix, fusion = model.pretrained_blocks()
    blocks = prefix + fusion
    assert all(b.lora_dropout_p == 0.3 for b in blocks)
    model.eval()
    assert all("p_lora" not in b.drop_kwargs() for b in blocks)
    batches = list(run["valid_batches"]())
    with torch.no_grad():
        with_p = [model(pb.batched_data)[0].clone() for pb in batches]
        for b in blocks:
            b.lora_dropout_p = 0.0
        without = [model(pb.batched_data)[0].clone() for pb in batches]
    model.train()
    assert with_p and all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(with_p, without))


def test_save_merged_still_loads_into_a_plain_model(tmp_path):
    from multimodaldiscussiontransformer_amd import checkpoint as ckpt
    from multimodaldiscussiontransformer_amd import train
    from multimodaldiscussiontransformer_amd.registry import TASK_REGISTRY
    merged = tmp_path / "merged.pt"
    train.main(argv(["--max-update", "4", "--no-save", "--save-merged", str(merged)] + ALL))
    st = torch.load(merged, weights_only=False)
    cfg = st["cfg"]["model"]
    assert not any(k.startswith("lora_") for k in cfg) and not any("lora_" in k for k in st["model"])
    a = argparse.Namespace(**{k: v for k, v in cfg.items() if k != "_name"})
    task_cls, task_cfg_cls = TASK_REGISTRY[a.task]
    task = task_cls.setup_task(task_cfg_cls(**{k: getattr(a, k) for k in task_cfg_cls.__dataclass_fields__}))
    plain = task.build_model(a).cuda().bfloat16()
    assert not plain.lora_modules() and not plain.lora_dense_modules()
    info = ckpt.load_checkpoint(str(merged), plain, allow_missing_prefixes=("node_encoder_stack.",))
    assert not info["unexpected"]
