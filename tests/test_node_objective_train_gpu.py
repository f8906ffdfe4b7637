"""The launcher with --label-smoothing / --focal-gamma on the toy shapes of tests/test_train_gpu.py: every log line carries a
finite loss and nll_loss, the validation line valid_nll_loss; a checkpoint records the two values and resumes the uninterrupted
run — with the flags repeated and with none on the command line; --deterministic runs print identical lines; and a run without
the flags has exactly the log keys and the checkpoint cfg it always had."""
import contextlib
import io
import json
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

OBJ = ["--label-smoothing", "0.1", "--focal-gamma", "2"]
TRAIN_KEYS = ["loss", "accuracy", "recall", "precision", "f1", "num_updates", "lr", "gnorm", "clip", "skipped_updates", "wall"]
VALID_KEYS = ["valid_loss", "valid_accuracy", "valid_recall", "valid_precision", "valid_f1", "valid_counters", "num_updates", "subset",
              "valid_best_loss"]


def argv(extra):
    return ["--task", "node_prediction", "--arch", "multi_graphormer_base", "--criterion", "node_cross_entropy",
            "--dataset-name", "synthetic", "--batch-size", "8", "--update-freq", "2", "--lr", "5e-4", "--end-learning-rate", "1e-5",
            "--warmup-updates", "2", "--total-num-update", "6", "--encoder-embed-dim", "128", "--encoder-ffn-embed-dim", "128",
            "--encoder-attention-heads", "2", "--num_fusion_layers", "0", "--num_bottleneck_tokens", "2",
            "--attention-dropout", "0", "--act-dropout", "0", "--dropout", "0", "--spatial-pos-max", "5", "--log-interval", "1",
            "--positive-weight", "1.5", "--negative-weight", "1",
            "--synthetic-nodes", "6", "--synthetic-seq-len", "12", "--synthetic-batches", "5", "--seed", "5", "--deterministic",
            "--bert-config", '{"dim": 128, "layers": 2, "heads": 2, "intermediate": 128, "vocab": 512, "max_pos": 64}',
            "--vit-config", '{"dim": 128, "layers": 2, "heads": 2, "intermediate": 128, "image_size": 32, "patch": 16}'] + extra


def run(extra):
    """→ (history, the JSON lines printed, stderr)."""
    from multimodaldiscussiontransformer_amd import train
    out, err = io.StringIO(), io.StringIO()
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        hist = train.main(argv(extra))
    return hist, [json.loads(line) for line in out.getvalue().splitlines() if line.startswith("{")], err.getvalue()


def values(lines):
    return [{k: v for k, v in h.items() if k != "wall"} for h in lines]


def valid_lines(printed):
    return [p for p in printed if "valid_loss" in p]


@pytest.fixture(scope="module")
def full():
    """Six uninterrupted updates with the objective on."""
    return run(OBJ + ["--max-update", "6", "--no-save"])


def test_every_line_has_loss_and_nll_loss(full):
    hist, printed, _ = full
    assert len(hist) == 6
    for h in hist:
        assert list(h) == TRAIN_KEYS[:1] + ["nll_loss"] + TRAIN_KEYS[1:]
        assert math.isfinite(h["loss"]) and math.isfinite(h["nll_loss"]) and h["nll_loss"] > 0 and h["loss"] != h["nll_loss"]
    assert [p for p in printed if "valid_loss" not in p] == hist
    (v,) = valid_lines(printed)
    assert list(v) == VALID_KEYS[:1] + ["valid_nll_loss"] + VALID_KEYS[1:]
    assert math.isfinite(v["valid_nll_loss"]) and v["valid_best_loss"] == v["valid_loss"] != v["valid_nll_loss"]
    assert v["valid_counters"]["nll_loss"] / v["valid_counters"]["sample_size"] == v["valid_nll_loss"]


def test_deterministic_runs_print_identical_lines(full):
    hist, printed, _ = run(OBJ + ["--max-update", "6", "--no-save"])
    assert values(hist) == values(full[0]) and valid_lines(printed) == valid_lines(full[1])


def test_checkpoint_records_the_objective_and_resumes_it(full, tmp_path):
    d = tmp_path / "ck"
    first, _, _ = run(OBJ + ["--max-update", "3", "--save-dir", str(d)])
    assert values(first) == values(full[0][:3])
    ck = d / "checkpoint_last.pt"
    cfg = torch.load(ck, weights_only=False)["cfg"]["model"]
    assert abs(cfg["label_smoothing"] - 0.1) < 1e-12 and cfg["focal_gamma"] == 2.0
    for flags in (OBJ, []):            # repeated on the command line, and left to the checkpoint's cfg
        second, printed, err = run(flags + ["--max-update", "6", "--restore-file", str(ck), "--no-save"])
        assert [h["num_updates"] for h in second] == [4, 5, 6]
        assert values(second) == values(full[0][3:]), flags
        assert valid_lines(printed) == valid_lines(full[1])
        assert ("continuing with them" in err) == (not flags)
    # a flag on the command line, 0 included, overrides the checkpoint's objective
    off, _, _ = run(["--label-smoothing", "0", "--max-update", "4", "--restore-file", str(ck), "--no-save"])
    assert len(off) == 1 and list(off[0]) == TRAIN_KEYS


def test_run_without_the_flags_is_todays(tmp_path):
    from multimodaldiscussiontransformer_amd import train
    d = tmp_path / "ck"
    hist, printed, _ = run(["--max-update", "2", "--save-dir", str(d)])
    assert len(hist) == 2 and all(list(h) == TRAIN_KEYS for h in hist)
    (v,) = valid_lines(printed)
    assert list(v) == VALID_KEYS
    assert list(v["valid_counters"]) == ["loss", "sample_size", "ncorrect", "num_positive_correct", "total_positive", "num_pred_positive"]
    cfg = torch.load(d / "checkpoint_last.pt", weights_only=False)["cfg"]["model"]
    assert "label_smoothing" not in cfg and "focal_gamma" not in cfg and cfg["positive_weight"] == 1.5
    crit = train.main.last_run["criterion"]
    assert crit.label_smoothing == 0.0 and crit.focal_gamma == 0.0


def test_launcher_refuses_what_the_kernel_would():
    for flags in (["--label-smoothing", "1"], ["--label-smoothing", "-0.1"], ["--label-smoothing", "nan"], ["--focal-gamma", "-1"],
                  ["--focal-gamma", "inf"], ["--focal-gamma", "nan"]):
        with pytest.raises(SystemExit, match="--label-smoothing must be in"):
            run(flags + ["--max-update", "1", "--no-save"])
    from multimodaldiscussiontransformer_amd import train
    with pytest.raises(SystemExit, match="only node_cross_entropy"):
        train.main([a if a != "node_cross_entropy" else "contrastive_loss" for a in argv(["--focal-gamma", "2", "--max-update", "1", "--no-save"])])
