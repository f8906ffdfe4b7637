"""The launcher with --lora-rank 8 --lora-targets all on the tiny shapes of tests/test_lora_train_gpu.py: a dozen updates make the
loss fall, move every adapter (QKV, attention output, fc1, fc2) and leave every frozen tensor's bits alone; a checkpoint carries
the PEFT keys of the dense layers and resumes bit for bit; --save-merged writes a plain checkpoint whose model reproduces the
adapted model's eval logits within the bf16 gate."""
import argparse
import math

import pytest
import torch

from tests.test_lora_train_gpu import argv, masters
from tests.test_real_shapes_gpu import BF16_GRAD_REL_L2

pytestmark = pytest.mark.gpu

ALL = ["--lora-targets", "all"]


def test_adapters_train_and_frozen_tensors_keep_their_bits(capsys):
    from multimodaldiscussiontransformer_amd import train
    train.main(argv(ALL + ["--max-update", "1", "--no-save"], dropout="0.1"))
    one = {n: p.detach().clone() for n, p in train.main.last_run["model"].named_parameters()}
    err = capsys.readouterr().err
    assert "adapted QKV projections and" in err and "adapted dense layers" in err and "targets q,k,v,out,fc1,fc2" in err
    hist = train.main(argv(ALL + ["--max-update", "12", "--no-save"], dropout="0.1"))
    model = train.main.last_run["model"]
    assert len(hist) == 12 and all(math.isfinite(h["loss"]) for h in hist)
    assert sum(h["loss"] for h in hist[-3:]) < sum(h["loss"] for h in hist[:3]), [h["loss"] for h in hist]
    ids = model.encoder_layer_ids()
    n_frozen = n_adapters = n_other = 0
    for n, p in model.named_parameters():
        if id(p) in ids and "lora_" not in n:
            assert not p.requires_grad and not hasattr(p, "main_grad"), n
            assert torch.equal(p.detach().view(torch.int16), one[n].view(torch.int16)), f"{n}: a frozen tensor changed"
            n_frozen += 1
        elif "lora_" in n:
            assert p.requires_grad and float(p.detach().float().abs().max()) > 0 and not torch.equal(p.detach(), one[n]), f"{n} did not move"
            n_adapters += 1
        elif p.requires_grad and not torch.equal(p.detach(), one[n]):
            n_other += 1
    dense = model.lora_dense_modules()
    assert len(dense) == 3 * len(model.lora_modules()) and n_adapters == 2 * (len(dense) + len(model.lora_modules()))
    assert n_frozen > 20 and n_other > 0               # the non-pretrained parts (graph stack, poolers, head) train as before


def test_checkpoint_resume_is_bit_for_bit(tmp_path):
    """dropout off, as in tests/test_lora_train_gpu.py: a checkpoint does not carry the generator the dropout seeds come from"""
    from multimodaldiscussiontransformer_amd import train
    full = train.main(argv(ALL + ["--max-update", "6", "--no-save", "--deterministic"]))
    want = masters(train.main.last_run)
    d = tmp_path / "ck"
    train.main(argv(ALL + ["--max-update", "3", "--save-dir", str(d), "--deterministic"]))
    ck = d / "checkpoint_last.pt"
    st = torch.load(ck, weights_only=False)
    assert st["cfg"]["model"]["lora_rank"] == 8 and st["cfg"]["model"]["lora_targets"] == "q,k,v,out,fc1,fc2"
    keys = [k for k in st["model"] if ".dense.lora_" in k]
    assert keys and all(k.endswith((".dense.lora_A.weight", ".dense.lora_B.weight")) for k in keys)
    for part in ("attention.output.dense", "intermediate.dense", ".output.dense"):
        assert any(part in k and float(st["model"][k].abs().max()) > 0 for k in keys if k.endswith(".lora_B.weight")), part
    second = train.main(argv(ALL + ["--max-update", "6", "--restore-file", str(ck), "--no-save", "--deterministic"]))
    assert [h["num_updates"] for h in second] == [4, 5, 6]
    assert [h["loss"] for h in second] == [h["loss"] for h in full[3:]]
    got = masters(train.main.last_run)
    for n in want:
        assert torch.equal(want[n].view(torch.uint8), got[n].view(torch.uint8)), f"{n} differs after the resume"


def test_save_merged_gives_a_plain_checkpoint(tmp_path):
    from multimodaldiscussiontransformer_amd import checkpoint as ckpt
    from multimodaldiscussiontransformer_amd import train
    from multimodaldiscussiontransformer_amd.models import GraphormerModel
    from multimodaldiscussiontransformer_amd.registry import TASK_REGISTRY
    merged = tmp_path / "merged.pt"
    train.main(argv(ALL + ["--max-update", "6", "--no-save", "--save-merged", str(merged)]))
    run = train.main.last_run
    adapted = run["model"]
    st = torch.load(merged, weights_only=False)
    cfg = st["cfg"]["model"]
    assert not any(k.startswith("lora_") or k == "save_merged" for k in cfg) and not any("lora_" in k for k in st["model"])
    a = argparse.Namespace(**{k: v for k, v in cfg.items() if k != "_name"})
    task_cls, task_cfg_cls = TASK_REGISTRY[a.task]          # built as the launcher builds it: the task attaches its classifier list
    task = task_cls.setup_task(task_cfg_cls(**{k: getattr(a, k) for k in task_cfg_cls.__dataclass_fields__}))
    plain = task.build_model(a).cuda().bfloat16()
    assert isinstance(plain, GraphormerModel) and not plain.lora_modules() and not plain.lora_dense_modules()
    info = ckpt.load_checkpoint(str(merged), plain, allow_missing_prefixes=("node_encoder_stack.",))
    assert not info["unexpected"]
    assert all(float(m.lora_Bt.detach().float().abs().max()) > 0 for m in adapted.lora_dense_modules())       # there was something to merge
    adapted.eval()
    plain.eval()
    with torch.no_grad():
        for pb in run["valid_batches"]():
            lo, _ = adapted(pb.batched_data)
            lp, _ = plain(pb.batched_data)
            rel = float((lp.double() - lo.double()).norm() / lo.double().norm())
            print(f"merged vs adapted logits: relative L2 {rel:.3e}")
            assert rel <= BF16_GRAD_REL_L2
    adapted.train()
