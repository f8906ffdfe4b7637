#!/usr/bin/env python3
"""What low-rank adapters (--lora-rank) cost and buy, measured in ONE process with a shared warm-up and alternating arms
(tools/ordered_ab.py's idea, in-process: the arms differ in the model, not in an environment switch).  Every timed stage runs under
a watchdog of its own (--limit seconds: the process is ended, nothing more is started on the device) and ends in a device
synchronise.  Prints JSON lines.

  (i)  kernels   at the bench workload's block shapes (token rows R of the text and of the image branch of one bench.py --config base
                 batch, D 768, rank 16, targets q,v): ops.lora_down / lora_up_add / lora_wgrad against the same products composed
                 from ops.gemm / engine.wgrad_gemm, each kernel next to its traffic floor (bytes moved once / the streaming rate
                 --stream-rate-tbs, e.g. what tools/probes/dram_locality_probe prints on that box; without it a device copy is timed here)
  (ii) step      the same workload in bf16, three models side by side: full fine-tuning, the pretrained stacks frozen without
                 adapters (the ceiling of what freezing buys) and add_lora(16); forward + backward and the Adam step timed apart

    python tools/lora_ab.py [--part kernels|step|both] [--rounds 5] [--iters 20] [--steps 6] [--warmup 3] [--limit 120] [--stream-rate-tbs X]
"""
import argparse
import faulthandler
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


class Stage:
    """A timed stage under its own limit: a stage that does not end within ``limit`` seconds ends the process."""

    def __init__(self, limit):
        self.limit = limit

    def __enter__(self):
        faulthandler.dump_traceback_later(self.limit, exit=True)

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        faulthandler.cancel_dump_traceback_later()


def timed_ms(fn, iters=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def spread(xs):
    return dict(median=round(statistics.median(xs), 4), min=round(min(xs), 4), max=round(max(xs), 4), n=len(xs))


def bench_batches(n=2):
    """``n`` packed batches of the bench.py --config base workload (its generator, its seeds) and the args of its model."""
    import bench
    from multimodaldiscussiontransformer_amd.data.packer import pack_batch
    cfg = bench.CONFIGS["base"]
    a = argparse.Namespace(config="base", num_fusion_layers=cfg["layers"] // 2 - 1, dropout=0.4, attention_dropout=0.3, act_dropout=0.3,
                           freeze_initial_encoders=False)
    per_tree_img = int(round(0.25 * cfg["nodes"]))
    pool = np.random.Generator(np.random.PCG64(99)).standard_normal((per_tree_img * 6 + 64, 3, cfg["image"], cfg["image"]), dtype=np.float32)
    out = []
    for i in range(n):
        trees = bench.trees_for_rank(i, 0, 1, trees_per_gpu=cfg["trees"], nodes=cfg["nodes"], image_frac=0.25, image_size=cfg["image"],
                                     patch=cfg["patch"], shape=cfg["shape"], image_pool=pool)
        out.append(pack_batch(trees, spatial_pos_max=5))
    return out, bench.base_args(a)


# ------------------------------------------------------------------------------------------------ (i) kernels
def kernel_part(a, shapes):
    from multimodaldiscussiontransformer_amd import engine, ops
    D, r, nj, s = 768, 16, 2, 2.0
    n = nj * r
    cols = (0, 2)
    rate = a.stream_rate_tbs
    if rate is None:
        with Stage(a.limit):
            src_, dst_ = torch.empty(1 << 29, dtype=torch.uint8, device="cuda"), torch.empty(1 << 29, dtype=torch.uint8, device="cuda")
            dst_.copy_(src_)
            ms = min(timed_ms(lambda: dst_.copy_(src_), 5) for _ in range(3))
            rate = 2 * (1 << 29) / (ms * 1e-3) / 1e12
            del src_, dst_
        print(json.dumps({"tool": "lora_ab", "part": "stream_rate", "source": "device copy of 512 MiB timed here (read + write bytes)",
                          "tb_per_s": round(rate, 3)}), flush=True)
    for branch, R in shapes.items():
        g = torch.Generator(device="cuda").manual_seed(1)
        rnd = lambda *shape, sc=1.0: ((torch.rand(*shape, generator=g, device="cuda") * 2 - 1) * sc).to(torch.bfloat16)      # noqa: E731
        src, qkv, dqkv, dx = rnd(R, D), rnd(R, 3 * D), rnd(R, 3 * D, sc=0.1), rnd(R, D, sc=0.1)
        A, Bt = rnd(n, D, sc=D ** -0.5), rnd(n, D, sc=0.05)
        t, dt = torch.empty(R, n, dtype=torch.bfloat16, device="cuda"), torch.empty(R, n, dtype=torch.bfloat16, device="cuda")
        gA, gBt = torch.zeros(n, D, device="cuda"), torch.zeros(n, D, device="cuda")
        ws = engine.ordered_workspace(ops.lib.mdt_lora_wgrad_workspace_bytes(R, n, D), "cuda")
        sl = lambda x, j: x[:, j * r:(j + 1) * r]                 # noqa: E731
        third = lambda x, c: x[:, c * D:(c + 1) * D]              # noqa: E731
        B2 = 2                                                    # bytes per bf16 element
        single = {      # one launch each: (new kernel, composition of the parent's ops, bytes every operand moves once)
            "down t=src A^T (n 32)": (lambda: ops.lora_down(src, A, out=t), lambda: ops.gemm(src, A, out=t), (R * D + R * n) * B2),
            "up_add qkv_j+=s t_j Bt_j (n 16)": (lambda: ops.lora_up_add(sl(t, 0), Bt[:r], third(qkv, 0), alpha=s),
                                                 lambda: ops.gemm(sl(t, 0), Bt[:r], trans_b=True, out=third(qkv, 0), epilogue=ops.EPI_ACCUM, alpha=s),
                                                 (2 * R * D + R * r) * B2),
            "wgrad dBt_j+=s t_j^T dqkv_j (n 16)": (lambda: ops.lora_wgrad(sl(t, 0), third(dqkv, 0), gBt[:r], alpha=s, ws=ws),
                                                    lambda: engine.wgrad_gemm(sl(t, 0), third(dqkv, 0), gBt[:r]), (R * D + R * r) * B2),
            "down dt_j=s dqkv_j Bt_j^T (n 16)": (lambda: ops.lora_down(third(dqkv, 0), Bt[:r], out=sl(dt, 0), alpha=s),
                                                  lambda: ops.gemm(third(dqkv, 0), Bt[:r], out=sl(dt, 0), alpha=s), (R * D + R * r) * B2),
            "wgrad dA+=dt^T src (n 32)": (lambda: ops.lora_wgrad(dt, src, gA, ws=ws), lambda: engine.wgrad_gemm(dt, src, gA), (R * D + R * n) * B2),
            "up_add dx+=dt A (n 32)": (lambda: ops.lora_up_add(dt, A, dx), lambda: ops.gemm(dt, A, trans_b=True, out=dx, epilogue=ops.EPI_ACCUM),
                                        (2 * R * D + R * n) * B2),
        }

        def fwd(new):
            k = 0 if new else 1
            single["down t=src A^T (n 32)"][k]()
            for j, c in enumerate(cols):
                if new:
                    ops.lora_up_add(sl(t, j), Bt[j * r:(j + 1) * r], third(qkv, c), alpha=s)
                else:
                    ops.gemm(sl(t, j), Bt[j * r:(j + 1) * r], trans_b=True, out=third(qkv, c), epilogue=ops.EPI_ACCUM, alpha=s)

        def bwd(new):
            for j, c in enumerate(cols):
                rows = slice(j * r, (j + 1) * r)
                if new:
                    ops.lora_wgrad(sl(t, j), third(dqkv, c), gBt[rows], alpha=s, ws=ws)
                    ops.lora_down(third(dqkv, c), Bt[rows], out=sl(dt, j), alpha=s)
                else:
                    engine.wgrad_gemm(sl(t, j), third(dqkv, c), gBt[rows])
                    ops.gemm(third(dqkv, c), Bt[rows], out=sl(dt, j), alpha=s)
            single["wgrad dA+=dt^T src (n 32)"][0 if new else 1]()
            single["up_add dx+=dt A (n 32)"][0 if new else 1]()

        arms = {name: (f[0], f[1]) for name, f in single.items()}
        arms["forward (3 launches)"] = (lambda: fwd(True), lambda: fwd(False))
        arms["backward (6 launches)"] = (lambda: bwd(True), lambda: bwd(False))
        for name, (new, old) in arms.items():
            res = {"new": [], "composed": []}
            try:
                with Stage(a.limit):
                    new(), old()                                   # shared warm-up: both arms' code objects and routes
                for _ in range(a.rounds):                          # alternating arms
                    for arm, fn in (("new", new), ("composed", old)):
                        with Stage(a.limit):
                            res[arm].append(timed_ms(fn, a.iters))
            except Exception as e:  # noqa: BLE001  (an argument refusal of the comparator is a result, not a fault)
                print(json.dumps({"tool": "lora_ab", "part": "kernels", "branch": branch, "R": R, "kernel": name, "error": str(e)[:300]}), flush=True)
                continue
            line = {"tool": "lora_ab", "part": "kernels", "branch": branch, "R": R, "D": D, "rank": r, "kernel": name, "iters": a.iters,
                    "new_ms": spread(res["new"]), "composed_ms": spread(res["composed"]),
                    "new_over_composed": round(statistics.median(res["new"]) / statistics.median(res["composed"]), 3)}
            if name in single:
                nbytes = single[name][2]
                line.update(bytes_moved_once=nbytes, floor_ms=round(nbytes / (rate * 1e12) * 1e3, 4),
                            new_over_floor=round(statistics.median(res["new"]) / (nbytes / (rate * 1e12) * 1e3), 2))
            print(json.dumps(line), flush=True)
        del src, qkv, dqkv, dx, t, dt


# ------------------------------------------------------------------------------------------------ (ii) step
def step_part(a, batches, margs):
    from multimodaldiscussiontransformer_amd.criterions import GraphPredictionNodeCrossEntropy
    from multimodaldiscussiontransformer_amd.ddp import DataParallel
    from multimodaldiscussiontransformer_amd.models import GraphormerModel
    from multimodaldiscussiontransformer_amd.optim import FusedAdam
    crit = GraphPredictionNodeCrossEntropy(None, positive_weight=1.5, negative_weight=1.0)
    scal = torch.zeros(6, dtype=torch.float32, device="cuda")

    def make(kind):
        torch.manual_seed(1234)
        m = GraphormerModel.build_model(argparse.Namespace(**vars(margs)), task=None)
        if kind == "frozen":
            ids = m.encoder_layer_ids()
            for p in m.parameters():
                if id(p) in ids:
                    p.requires_grad = False
        elif kind == "lora16":
            m.add_lora(16)
        m = m.cuda().bfloat16().train()
        dp = DataParallel(m)
        opt = FusedAdam([p for p in m.parameters() if hasattr(p, "main_grad")], lr=3e-5, weight_decay=0.01)
        n_train = sum(p.numel() for p in m.parameters() if p.requires_grad)
        return dict(model=m, dp=dp, opt=opt, trainable=n_train, fwdbwd=[], adam=[])

    def fwdbwd(arm, pb):
        arm["dp"].zero_grad()
        loss, sample_size, log = crit(arm["model"], {"nsamples": pb.B, "net_input": {"batched_data": pb.batched_data}})
        loss.backward()
        scal[0] = loss.detach().float()
        scal[1].fill_(float(sample_size))
        arm["gscale"] = arm["dp"].finish_backward(scal, fold_scale=True)

    arms = {}
    for kind in ("full", "frozen", "lora16"):
        with Stage(max(a.limit, 300)):                             # building mDT-base on the host takes its time
            arms[kind] = make(kind)
    for i in range(a.warmup):                                      # shared warm-up
        for arm in arms.values():
            with Stage(a.limit):
                fwdbwd(arm, batches[i % len(batches)])
                arm["opt"].step(grad_scale=arm["gscale"])
    for i in range(a.steps):                                       # alternating arms, one step per stage
        for arm in arms.values():
            pb = batches[i % len(batches)]
            with Stage(a.limit):
                arm["fwdbwd"].append(timed_ms(lambda: fwdbwd(arm, pb)))
            with Stage(a.limit):
                arm["adam"].append(timed_ms(lambda: arm["opt"].step(grad_scale=arm["gscale"])))
    out = {k: dict(trainable_elements=v["trainable"], fwd_bwd_ms=spread(v["fwdbwd"]), adam_ms=spread(v["adam"])) for k, v in arms.items()}
    med = lambda k, w: out[k][w]["median"]      # noqa: E731
    print(json.dumps({"tool": "lora_ab", "part": "step", "workload": "bench.py --config base (32 trees x 64 comments, image-frac 0.25), bf16, resident batches",
                      "steps": a.steps, "warmup": a.warmup, "arms": out,
                      "freezing_buys_fwd_bwd_ms": round(med("full", "fwd_bwd_ms") - med("frozen", "fwd_bwd_ms"), 3),
                      "adapters_cost_over_frozen_fwd_bwd_ms": round(med("lora16", "fwd_bwd_ms") - med("frozen", "fwd_bwd_ms"), 3),
                      "lora16_over_full_step": round((med("lora16", "fwd_bwd_ms") + med("lora16", "adam_ms")) /
                                                     (med("full", "fwd_bwd_ms") + med("full", "adam_ms")), 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--part", default="both", choices=["kernels", "step", "both"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=120, help="seconds a timed stage may take")
    ap.add_argument("--stream-rate-tbs", type=float, default=None, help="streaming rate of the box in TB/s (tools/probes/dram_locality_probe)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("[lora_ab] no GPU: nothing is measured without one")
    torch.cuda.set_device(0)
    batches, margs = bench_batches(2)
    pb = batches[0]
    nb = margs.num_bottleneck_tokens
    shapes = {"text": int(pb.text_mask.sum()) + nb * pb.M, "image": pb.I * ((224 // 16) ** 2 + 1 + nb)}
    if a.part in ("kernels", "both"):
        kernel_part(a, shapes)
    if a.part in ("step", "both"):
        step_part(a, batches, margs)


if __name__ == "__main__":
    main()
