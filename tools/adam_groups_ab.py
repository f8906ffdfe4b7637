#!/usr/bin/env python3
"""What parameter groups cost in the optimiser: the multi-tensor Adam launch over the REAL parameter table of bench.py's --config base
(BASELINE.json configs[1]: mDT-base, bf16 with fp32 masters, 432 tensors), timed with device events in one process, the arms
interleaved round by round (tools/ema_ab.py's method):

    plain         mdt_adam_step_multi                              30 B per element
    groups        mdt_adam_step_multi_groups, the records GraphormerModel.optimizer_groups gives for
                  --encoder-lr-scale 0.5 --encoder-layer-decay 0.75 --no-decay-bias-norm: + 8 B per TENSOR
    three         what the one grouped launch replaces: three optimisers without groups over the same tensors split three ways
                  (pretrained blocks / other matrices / vectors), one mdt_adam_step_multi each
    parent        (--parent-lib FILE) mdt_adam_step_multi of another build of the library on the same table

Every arm runs an update on the same tensors (timing does not depend on the values).  Prints one JSON line: per arm the median / min
/ max in microseconds over --reps rounds; the spread of `plain` (max - min over median) is the run-to-run noise a difference has to
exceed.  --out FILE also writes the line there.

    python tools/adam_groups_ab.py [--reps 30] [--warmup 5] [--parent-lib path/to/other/libmdt_hip.so] [--out profiles/adam_groups_ab_mi355x.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parent-lib", default="", help="libmdt_hip.so of another build (the parent commit's): its plain launch is timed too")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from ema_ab import base_model_args
    from multimodaldiscussiontransformer_amd._lib import _SIGS, check, lib, ptr, stream
    from multimodaldiscussiontransformer_amd.models import GraphormerModel
    from multimodaldiscussiontransformer_amd.optim import FusedAdam
    if not torch.cuda.is_available():
        raise SystemExit("[adam_groups_ab] no GPU: nothing is measured without one")
    torch.manual_seed(1234)
    model = GraphormerModel.build_model(base_model_args(), task=None).cuda().bfloat16().train()
    model.prepare_main_grads()
    model.main_grad_flat.normal_(0.0, 1e-3)
    held = [p for p in model.parameters() if hasattr(p, "main_grad")]
    groups = [dict(g, params=[p for p in g["params"] if hasattr(p, "main_grad")])
              for g in model.optimizer_groups(encoder_lr_scale=0.5, encoder_layer_decay=0.75, no_decay_bias_norm=True, weight_decay=0.01)]
    grouped = FusedAdam([g for g in groups if g["params"]], lr=3e-5, weight_decay=0.01)
    plain_opt = FusedAdam(held, lr=3e-5, weight_decay=0.01)
    ids = model.encoder_layer_ids()
    split = [[p for p in held if id(p) in ids and p.ndim > 1], [p for p in held if id(p) not in ids and p.ndim > 1], [p for p in held if p.ndim <= 1]]
    three = [FusedAdam(ps, lr=3e-5, weight_decay=0.01) for ps in split if ps]
    tabs_plain, tabs_grouped, tabs_three = plain_opt._tables(), grouped._tables(), [o._tables() for o in three]
    assert sum(len(t.params) for t in tabs_grouped.values()) == len(held) == sum(len(t.params) for t in tabs_plain.values())
    assert all(t.groups is not None for t in tabs_grouped.values()) and all(t.groups is None for t in tabs_plain.values())
    elements = sum(p.numel() for p in held)
    hyper = (3e-5, 0.9, 0.999, 1e-8)
    step = [0]

    def run_plain(tabs, which=lib):
        for dtype, t in tabs.items():
            check(which.mdt_adam_step_multi(stream(), 0 if dtype == torch.float32 else 1, t.n, ptr(t.rec), ptr(t.first), t.total, *hyper, 0.01,
                                            step[0], None), "mdt_adam_step_multi")

    def run_groups():
        for dtype, t in tabs_grouped.items():
            check(lib.mdt_adam_step_multi_groups(stream(), 0 if dtype == torch.float32 else 1, t.n, ptr(t.rec), ptr(t.first), t.total, *hyper,
                                                 step[0], ptr(t.groups), None, None, None, 0.0), "mdt_adam_step_multi_groups")

    def run_three():
        for tabs in tabs_three:
            run_plain(tabs)

    arms = {"plain": lambda: run_plain(tabs_plain), "groups": run_groups, "three": run_three}
    if a.parent_lib:
        other = C.CDLL(os.path.abspath(a.parent_lib))
        other.mdt_adam_step_multi.argtypes, other.mdt_adam_step_multi.restype = _SIGS["mdt_adam_step_multi"]
        arms["parent"] = lambda: run_plain(tabs_plain, other)
    times = {k: [] for k in arms}
    for r in range(a.warmup + a.reps):
        for name, fn in arms.items():
            step[0] += 1
            beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            beg.record()
            fn()
            end.record()
            end.synchronize()
            if r >= a.warmup:
                times[name].append(beg.elapsed_time(end) * 1e3)
    out = {"tool": "adam_groups_ab", "config": "base", "dtype": "bf16", "tensors": len(held), "elements": elements, "reps": a.reps,
           "distinct_groups": len(grouped.param_groups), "three_way_split_tensors": [len(ps) for ps in split]}
    for name in arms:
        t = times[name]
        med = statistics.median(t)
        out[name] = {"us_median": round(med, 1), "us_min": round(min(t), 1), "us_max": round(max(t), 1),
                     "GBps_at_median": round(elements * 30 / med / 1e3, 1)}
    p = out["plain"]
    out["plain_spread"] = round((p["us_max"] - p["us_min"]) / p["us_median"], 4)
    out["groups_over_plain"] = round(out["groups"]["us_median"] / p["us_median"], 4)
    out["three_over_groups"] = round(out["three"]["us_median"] / out["groups"]["us_median"], 4)
    if "parent" in out:
        out["plain_over_parent"] = round(p["us_median"] / out["parent"]["us_median"], 4)
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
