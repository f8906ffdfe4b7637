#!/usr/bin/env python3
"""What activation recomputation (engine.set_recompute, the launcher's --checkpoint-activations / --checkpoint-policy) costs in
time and buys in memory, measured in ONE process on ONE model with a shared warm-up and interleaved arms (none, ffn, block, none,
ffn, block, ...): the policy is a process-wide switch read when a block is recorded, so the arms differ in nothing else.

The workload is bench.py --config base (32 trees x 64 comments, image-frac 0.25; tools/lora_ab.py's batches and model) in bf16 with
dropout on.  Every step gets a freshly packed batch, so the per-batch index vectors are derived inside the step as in training.
Forward + backward are timed by HIP events; torch.cuda.max_memory_allocated() is read over the same step after
reset_peak_memory_stats().  Every timed stage runs under a watchdog of its own (--limit seconds: the process is ended, nothing
more is started on the device) and ends in a device synchronise.  One JSON line per policy goes to stdout and to --out.

    python tools/recompute_ab.py [--steps 8] [--warmup 2] [--limit 120] [--out profiles/recompute_ab_mi355x.jsonl]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from lora_ab import Stage, spread, timed_ms  # noqa: E402

POLICIES = ("none", "ffn", "block")


def host_trees(n):
    """The trees of ``n`` bench.py --config base batches (its generator, its seeds) and the args of its model."""
    import bench
    import numpy as np
    cfg = bench.CONFIGS["base"]
    a = argparse.Namespace(config="base", num_fusion_layers=cfg["layers"] // 2 - 1, dropout=0.4, attention_dropout=0.3, act_dropout=0.3,
                           freeze_initial_encoders=False)
    per_tree_img = int(round(0.25 * cfg["nodes"]))
    pool = np.random.Generator(np.random.PCG64(99)).standard_normal((per_tree_img * 6 + 64, 3, cfg["image"], cfg["image"]), dtype=np.float32)
    trees = [bench.trees_for_rank(i, 0, 1, trees_per_gpu=cfg["trees"], nodes=cfg["nodes"], image_frac=0.25, image_size=cfg["image"],
                                  patch=cfg["patch"], shape=cfg["shape"], image_pool=pool) for i in range(n)]
    return trees, bench.base_args(a)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=120, help="seconds a timed stage may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recompute_ab_mi355x.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("[recompute_ab] no GPU: nothing is measured without one")
    torch.cuda.set_device(0)
    from multimodaldiscussiontransformer_amd import engine
    from multimodaldiscussiontransformer_amd.criterions import GraphPredictionNodeCrossEntropy
    from multimodaldiscussiontransformer_amd.data.packer import pack_batch
    from multimodaldiscussiontransformer_amd.models import GraphormerModel
    trees, margs = host_trees(2)
    with Stage(max(a.limit, 300)):                                 # building mDT-base on the host takes its time
        torch.manual_seed(1234)
        model = GraphormerModel.build_model(argparse.Namespace(**vars(margs)), task=None).cuda().bfloat16().train()
        model.prepare_main_grads()
    crit = GraphPredictionNodeCrossEntropy(None, positive_weight=1.5, negative_weight=1.0)
    covered = sum(len(b) for b in model.pretrained_blocks())
    was = engine.recompute()

    def step(policy, i):
        """→ (ms of forward + backward, peak bytes allocated over them, loss) on a batch packed for this step alone"""
        pb = pack_batch(trees[i % len(trees)], spatial_pos_max=5)
        engine.set_recompute(policy)
        torch.manual_seed(1000 + i)                                # the same dropout masks for the three arms of a round
        model.zero_main_grads()
        out = {}

        def run():
            loss, _, _ = crit(model, {"nsamples": pb.B, "net_input": {"batched_data": pb.batched_data}})
            loss.backward()
            out["loss"] = loss.detach()

        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        ms = timed_ms(run)
        return ms, torch.cuda.max_memory_allocated(), float(out["loss"])

    res = {p: dict(ms=[], peak=[], loss=[]) for p in POLICIES}
    try:
        for i in range(a.warmup):                                  # shared warm-up: every arm's routes, the allocator's pools
            for policy in POLICIES:
                with Stage(a.limit):
                    step(policy, i)
        for i in range(a.steps):                                   # interleaved arms, one step per stage
            for policy in POLICIES:
                with Stage(a.limit):
                    ms, peak, loss = step(policy, a.warmup + i)
                res[policy]["ms"].append(ms)
                res[policy]["peak"].append(peak)
                res[policy]["loss"].append(loss)
    finally:
        engine.set_recompute(was)
    base_ms, base_peak = spread(res["none"]["ms"])["median"], max(res["none"]["peak"])
    lines = []
    for policy in POLICIES:
        r = res[policy]
        ms, peak = spread(r["ms"]), max(r["peak"])
        lines.append({"tool": "recompute_ab", "policy": policy, "device": torch.cuda.get_device_name(0),
                      "workload": "bench.py --config base (32 trees x 64 comments, image-frac 0.25), bf16, dropout on, a freshly packed "
                                  "batch per step, forward + backward",
                      "blocks_covered": 0 if policy == "none" else covered, "steps": a.steps, "warmup": a.warmup, "fwd_bwd_ms": ms,
                      "ms_over_none": round(ms["median"] / base_ms, 4), "peak_bytes": peak, "peak_gib": round(peak / 2 ** 30, 3),
                      "peak_over_none": round(peak / base_peak, 4), "same_loss_as_none": r["loss"] == res["none"]["loss"]})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            print(json.dumps(line), flush=True)
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
