#!/usr/bin/env python3
"""What the weight average (--store-ema) costs in the optimiser: the multi-tensor Adam launch over the REAL parameter table of
bench.py's --config base (BASELINE.json configs[1]: mDT-base, bf16 with fp32 masters), timed with device events in one process, the
arms interleaved round by round:

    plain         mdt_adam_step_multi                      30 B per element (grad 4, m 8, v 8, master 8, bf16 parameter 2)
    ema           mdt_adam_step_multi_ema                  + 8 B (the average read and written)
    plain+lerp    the plain launch, then torch._foreach_lerp_(averages, masters, 1 - d): the unfused alternative, + 12 B
    parent        (--parent-lib FILE) mdt_adam_step_multi of another build of the library on the same table

Every arm runs the same update on the same tensors (the state drifts identically: timing does not depend on the values).  Prints one
JSON line: per arm the median / min / max in microseconds over --reps rounds and the GB/s of its bytes at the median; the spread of
`plain` (max - min over median) is the run-to-run noise a difference has to exceed.

    python tools/ema_ab.py [--reps 30] [--warmup 5] [--parent-lib path/to/other/libmdt_hip.so]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def base_model_args():
    """bench.py base_args for --config base (BERT-base + ViT-B/16 split 6 + 6, 5 fusion layers, D 768)."""
    return SimpleNamespace(
        num_atoms=512 * 9, num_in_degree=512, num_out_degree=512, num_edges=512 * 3, num_spatial=512, num_edge_dis=128,
        edge_type="multi_hop", multi_hop_max_dist=5, num_bottleneck_tokens=4, num_fusion_layers=5, num_fusion_stack=1, num_graph_stack=1,
        encoder_layers=4, encoder_embed_dim=768, encoder_ffn_embed_dim=768, encoder_attention_heads=12, dropout=0.0, attention_dropout=0.0,
        act_dropout=0.0, encoder_normalize_before=True, pre_layernorm=False, apply_graphormer_init=False, activation_fn="gelu",
        freeze_initial_encoders=False, share_encoder_input_output_embed=False, max_nodes=10000, num_classes=1,
        bert_config=dict(dim=768, layers=12, heads=12, intermediate=3072),
        vit_config=dict(dim=768, layers=12, heads=12, intermediate=3072, image_size=224, patch=16))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--decay", type=float, default=0.9999)
    ap.add_argument("--parent-lib", default="", help="libmdt_hip.so of another build (the parent commit's): its plain launch is timed too")
    a = ap.parse_args()
    import torch
    from multimodaldiscussiontransformer_amd._lib import check, lib, ptr, stream
    from multimodaldiscussiontransformer_amd.models import GraphormerModel
    from multimodaldiscussiontransformer_amd.optim import FusedAdam
    if not torch.cuda.is_available():
        raise SystemExit("[ema_ab] no GPU: nothing is measured without one")
    torch.manual_seed(1234)
    model = GraphormerModel.build_model(base_model_args(), task=None).cuda().bfloat16().train()
    model.prepare_main_grads()
    opt = FusedAdam([p for p in model.parameters() if hasattr(p, "main_grad")], lr=3e-5, weight_decay=0.01, ema_decay=a.decay)
    model.main_grad_flat.normal_(0.0, 1e-3)
    tables = opt._tables()
    covered = sum(len(t.params) for t in tables.values())
    assert covered == len(opt.params), f"{len(opt.params) - covered} parameters are outside the multi-tensor table"
    elements = sum(p.numel() for p in opt.params)
    masters = [opt.state[id(p)]["master"] for p in opt.params]
    emas = [opt.state[id(p)]["ema"] for p in opt.params]
    hyper = (3e-5, 0.9, 0.999, 1e-8, 0.01)
    step = [0]

    def head(dtype, t):
        return (stream(), 0 if dtype == torch.float32 else 1, t.n, ptr(t.rec), ptr(t.first), t.total, *hyper, step[0])

    def plain(which=lib):
        for dtype, t in tables.items():
            check(which.mdt_adam_step_multi(*head(dtype, t), None), "mdt_adam_step_multi")

    def ema():
        for dtype, t in tables.items():
            check(lib.mdt_adam_step_multi_ema(*head(dtype, t), None, ptr(t.ema_ptrs), a.decay), "mdt_adam_step_multi_ema")

    def plain_lerp():
        plain()
        torch._foreach_lerp_(emas, masters, 1.0 - a.decay)

    arms = {"plain": (plain, 30), "ema": (ema, 38), "plain+lerp": (plain_lerp, 42)}
    if a.parent_lib:
        other = C.CDLL(os.path.abspath(a.parent_lib))
        from multimodaldiscussiontransformer_amd._lib import _SIGS
        other.mdt_adam_step_multi.argtypes, other.mdt_adam_step_multi.restype = _SIGS["mdt_adam_step_multi"]
        arms["parent"] = (lambda: plain(other), 30)
    times = {k: [] for k in arms}
    for r in range(a.warmup + a.reps):
        for name, (fn, _) in arms.items():
            step[0] += 1
            beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            beg.record()
            fn()
            end.record()
            end.synchronize()
            if r >= a.warmup:
                times[name].append(beg.elapsed_time(end) * 1e3)
    out = {"tool": "ema_ab", "config": "base", "dtype": "bf16", "tensors": len(opt.params), "elements": elements, "reps": a.reps, "decay": a.decay}
    for name, (_, bytes_per) in arms.items():
        t = times[name]
        med = statistics.median(t)
        out[name] = {"us_median": round(med, 1), "us_min": round(min(t), 1), "us_max": round(max(t), 1), "bytes_per_element": bytes_per,
                     "GBps_at_median": round(elements * bytes_per / med / 1e3, 1)}
    p = out["plain"]
    out["plain_spread"] = round((p["us_max"] - p["us_min"]) / p["us_median"], 4)
    out["ema_over_plain"] = round(out["ema"]["us_median"] / p["us_median"], 4)
    out["lerp_over_plain"] = round(out["plain+lerp"]["us_median"] / p["us_median"], 4)
    if "parent" in out:
        out["plain_over_parent"] = round(p["us_median"] / out["parent"]["us_median"], 4)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
