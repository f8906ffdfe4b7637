"""The launcher with --lora-rank on the tiny --bert-config / --vit-config shapes of tests/test_train_gpu.py: a dozen updates move
the loss and the adapters and leave every frozen tensor's bits alone; a checkpoint resumes bit for bit; --deterministic runs
repeat bit for bit (loss and gradient arena); --save-merged writes a plain checkpoint whose model reproduces the adapted
model's eval logits; --fp8 with adapters exits with the message."""
import argparse
import math

import pytest
import torch

from tests.test_real_shapes_gpu import BF16_GRAD_REL_L2

pytestmark = pytest.mark.gpu


def argv(extra, dropout="0"):
    return ["--task", "node_prediction", "--arch", "multi_graphormer_base", "--criterion", "node_cross_entropy",
            "--dataset-name", "synthetic", "--batch-size", "8", "--lr", "2e-3", "--end-learning-rate", "1e-5",
            "--warmup-updates", "2", "--total-num-update", "12", "--encoder-embed-dim", "128", "--encoder-ffn-embed-dim", "128",
            "--encoder-attention-heads", "2", "--num_fusion_layers", "0", "--num_bottleneck_tokens", "2",
            "--attention-dropout", dropout, "--act-dropout", dropout, "--dropout", dropout, "--spatial-pos-max", "5", "--log-interval", "1",
            "--synthetic-nodes", "6", "--synthetic-seq-len", "12", "--synthetic-batches", "4", "--synthetic-image-frac", "0.5", "--seed", "5",
            "--bf16", "--lora-rank", "8",
            "--bert-config", '{"dim": 128, "layers": 2, "heads": 2, "intermediate": 128, "vocab": 512, "max_pos": 64}',
            "--vit-config", '{"dim": 128, "layers": 2, "heads": 2, "intermediate": 128, "image_size": 32, "patch": 16}'] + extra


def masters(run):
    """{name: fp32 master (or the parameter itself)} of the last run's model."""
    opt = run["optimizer"]
    out = {}
    for n, p in run["model"].named_parameters():
        st = opt.state.get(id(p), {})
        out[n] = (st["master"] if "master" in st else p.data).detach().clone()
    return out


def test_adapters_train_and_frozen_tensors_keep_their_bits(capsys):
    from multimodaldiscussiontransformer_amd import train
    train.main(argv(["--max-update", "1", "--no-save"], dropout="0.1"))
    one = {n: p.detach().clone() for n, p in train.main.last_run["model"].named_parameters()}
    err = capsys.readouterr().err
    assert "--lora-rank 8:" in err and "adapted QKV projections" in err and "trainable" in err and "frozen" in err
    hist = train.main(argv(["--max-update", "12", "--no-save"], dropout="0.1"))
    model = train.main.last_run["model"]
    assert len(hist) == 12 and all(math.isfinite(h["loss"]) for h in hist)
    assert sum(h["loss"] for h in hist[-3:]) < sum(h["loss"] for h in hist[:3]), [h["loss"] for h in hist]
    ids = model.encoder_layer_ids()
    n_frozen = n_adapters = 0
    for n, p in model.named_parameters():
        if id(p) in ids and "lora_" not in n:
            assert not p.requires_grad and not hasattr(p, "main_grad"), n
            assert torch.equal(p.detach().view(torch.int16), one[n].view(torch.int16)), f"{n}: a frozen tensor changed"
            n_frozen += 1
        elif "lora_" in n:
            assert p.requires_grad and float(p.detach().float().abs().max()) > 0 and not torch.equal(p.detach(), one[n]), f"{n} did not move"
            n_adapters += 1
    assert n_adapters == 2 * len(model.lora_modules()) and n_adapters >= 4 and n_frozen > 20


def test_checkpoint_resume_is_bit_for_bit(tmp_path):
    from multimodaldiscussiontransformer_amd import train
    full = train.main(argv(["--max-update", "8", "--no-save", "--deterministic"]))
    want = masters(train.main.last_run)
    d = tmp_path / "ck"
    train.main(argv(["--max-update", "4", "--save-dir", str(d), "--deterministic"]))
    ck = d / "checkpoint_last.pt"
    st = torch.load(ck, weights_only=False)
    assert st["cfg"]["model"]["lora_rank"] == 8 and st["cfg"]["model"]["lora_alpha"] == 16.0 and st["cfg"]["model"]["lora_targets"] == "q,v"
    keys = [k for k in st["model"] if ".lora_" in k]
    assert keys and all(k.endswith((".lora_A.weight", ".lora_B.weight")) for k in keys)
    assert any(float(st["model"][k].abs().max()) > 0 for k in keys if k.endswith(".lora_B.weight"))
    second = train.main(argv(["--max-update", "8", "--restore-file", str(ck), "--no-save", "--deterministic"]))
    assert [h["num_updates"] for h in second] == [5, 6, 7, 8]
    assert [h["loss"] for h in second] == [h["loss"] for h in full[4:]]
    got = masters(train.main.last_run)
    for n in want:
        assert torch.equal(want[n].view(torch.uint8), got[n].view(torch.uint8)), f"{n} differs after the resume"


def test_deterministic_runs_repeat(tmp_path):
    from multimodaldiscussiontransformer_amd import ops, train
    runs = []
    for _ in range(2):
        before = ops.float_atomic_launches()
        hist = train.main(argv(["--max-update", "3", "--no-save", "--deterministic"], dropout="0.1"))
        assert ops.float_atomic_launches() == before
        runs.append(([h["loss"] for h in hist], train.main.last_run["model"].main_grad_flat.clone()))
    assert runs[0][0] == runs[1][0]
    assert float(runs[0][1].abs().max()) > 0 and torch.equal(runs[0][1].view(torch.int32), runs[1][1].view(torch.int32))


def test_save_merged_gives_a_plain_checkpoint(tmp_path):
    from multimodaldiscussiontransformer_amd import checkpoint as ckpt
    from multimodaldiscussiontransformer_amd import train
    from multimodaldiscussiontransformer_amd.models import GraphormerModel
    merged = tmp_path / "merged.pt"
    train.main(argv(["--max-update", "6", "--no-save", "--save-merged", str(merged)]))
    run = train.main.last_run
    adapted = run["model"]
    st = torch.load(merged, weights_only=False)
    cfg = st["cfg"]["model"]
    assert not any(k.startswith("lora_") or k == "save_merged" for k in cfg) and not any("lora_" in k for k in st["model"])
    a = argparse.Namespace(**{k: v for k, v in cfg.items() if k != "_name"})
    from multimodaldiscussiontransformer_amd.registry import TASK_REGISTRY
    task_cls, task_cfg_cls = TASK_REGISTRY[a.task]          # built as the launcher builds it: the task attaches its classifier list
    task = task_cls.setup_task(task_cfg_cls(**{k: getattr(a, k) for k in task_cfg_cls.__dataclass_fields__}))
    plain = task.build_model(a).cuda().bfloat16()
    assert isinstance(plain, GraphormerModel) and not plain.lora_modules()
    info = ckpt.load_checkpoint(str(merged), plain, allow_missing_prefixes=("node_encoder_stack.",))
    assert not info["unexpected"]
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
    assert all(float(m.lora_Bt.detach().float().abs().max()) > 0 for m in adapted.lora_modules())       # there was something to merge


def test_fp8_with_adapters_exits():
    from multimodaldiscussiontransformer_amd import train
    with pytest.raises(SystemExit, match="--fp8 with --lora-rank"):
        train.main(argv(["--max-update", "1", "--no-save", "--fp8"]))
