#!/usr/bin/env python3
"""What the adapters on the attention output projection, fc1 and fc2 cost, measured in ONE process with a shared warm-up and
alternating arms (tools/lora_ab.py's frame, whose Stage / timed_ms / bench_batches this reuses).  Prints JSON lines.

  (i)  kernels   at the bench workload's block shapes (token rows R of the text and of the image branch of one bench.py --config base
                 batch, D 768, F 3072, rank 16): each epilogue form of the up-projection against the same result composed from
                 the entry points that existed before it, and next to its traffic floor (bytes every operand moves once / the
                 streaming rate, --stream-rate-tbs or a device copy timed here)
                   fc1     ops.lora_up_act                 vs  ops.lora_up_add into pre + ops.act_fwd          (6 B vs 10 B per element of [R, F])
                   o, fc2  the fused GEMM + ops.lora_up_add_drop  vs  an unfused GEMM + ops.lora_up_add + ops.dropout + the residual add
                   mul     ops.lora_up_add_mul             vs  ops.lora_up_add into a zeroed scratch tensor, times u, added to du
  (ii) step      forward + backward of the bench step in bf16 with add_lora(16) on q,v against all six targets

    python tools/lora_dense_ab.py [--part kernels|step|both] [--rounds 5] [--iters 20] [--steps 6] [--warmup 3] [--limit 120] [--stream-rate-tbs X]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from lora_ab import Stage, bench_batches, spread, timed_ms  # noqa: E402

TOOL = "lora_dense_ab"


def stream_rate(a):
    if a.stream_rate_tbs is not None:
        return a.stream_rate_tbs
    with Stage(a.limit):
        src_, dst_ = torch.empty(1 << 29, dtype=torch.uint8, device="cuda"), torch.empty(1 << 29, dtype=torch.uint8, device="cuda")
        dst_.copy_(src_)
        ms = min(timed_ms(lambda: dst_.copy_(src_), 5) for _ in range(3))
    rate = 2 * (1 << 29) / (ms * 1e-3) / 1e12
    print(json.dumps({"tool": TOOL, "part": "stream_rate", "source": "device copy of 512 MiB timed here (read + write bytes)",
                      "tb_per_s": round(rate, 3)}), flush=True)
    return rate


# ------------------------------------------------------------------------------------------------ (i) kernels
def kernel_part(a, shapes):
    from multimodaldiscussiontransformer_amd import ops
    D, F, r, s, p, seed = 768, 3072, 16, 2.0, 0.4, 1234
    rate = stream_rate(a)
    B2 = 2
    for branch, R in shapes.items():
        g = torch.Generator(device="cuda").manual_seed(1)
        rnd = lambda *shape, sc=1.0: ((torch.rand(*shape, generator=g, device="cuda") * 2 - 1) * sc).to(torch.bfloat16)      # noqa: E731
        h, res = rnd(R, F), rnd(R, D)
        pre, u, du = rnd(R, F), rnd(R, F), rnd(R, F, sc=0.1)
        w2, b2 = rnd(D, F, sc=F ** -0.5), rnd(D, sc=0.1)
        t = rnd(R, r)
        BtF, BtD, A_F = rnd(r, F, sc=0.05), rnd(r, D, sc=0.05), rnd(r, F, sc=F ** -0.5)
        y = torch.empty(R, D, dtype=torch.bfloat16, device="cuda")
        hbuf, ubuf = torch.empty_like(pre), torch.empty_like(pre)
        scratch = pre.clone()

        def act_new():
            ops.lora_up_act(t, BtF, pre, "gelu", alpha=s, drop_p=0.3, drop_seed=seed, out=hbuf, u=ubuf)

        def act_old():                       # the sum is rounded to bf16 on its way through memory
            hbuf.copy_(pre)
            ops.lora_up_add(t, BtF, hbuf, alpha=s)
            ops.act_fwd(hbuf, "gelu", drop_p=0.3, drop_seed=seed, out=hbuf, u=ubuf)

        def act_old_inplace():               # without the copy that keeps pre: what an engine that owns pre would run
            ops.lora_up_add(t, BtF, scratch, alpha=s)
            ops.act_fwd(scratch, "gelu", drop_p=0.3, drop_seed=seed, out=scratch, u=ubuf)

        def fc2_new():
            ops.gemm(h, w2, bias=b2, residual=res, drop_p=p, drop_seed=seed, out=y)
            ops.lora_up_add_drop(t, BtD, y, alpha=s, drop_p=p, drop_seed=seed)

        def fc2_old():
            ops.gemm(h, w2, bias=b2, out=y)
            ops.lora_up_add(t, BtD, y, alpha=s)
            ops.dropout(y, p, seed, out=y)
            y.add_(res)

        def drop_new():
            ops.lora_up_add_drop(t, BtD, y, alpha=s, drop_p=p, drop_seed=seed)

        def mul_new():
            ops.lora_up_add_mul(t, A_F, du, u, alpha=1.0)

        def mul_old():
            scratch.zero_()
            ops.lora_up_add(t, A_F, scratch)
            du.addcmul_(scratch, u)

        arms = {
            "fc1: up_act (gelu, p 0.3) vs copy + up_add + act_fwd": (act_new, act_old, (3 * R * F + R * r) * B2),
            "fc1: up_act vs up_add + act_fwd in place": (act_new, act_old_inplace, (3 * R * F + R * r) * B2),
            "fc2: fused GEMM + up_add_drop vs GEMM + up_add + dropout + residual": (fc2_new, fc2_old, None),
            "o / fc2 epilogue alone: up_add_drop [R, D]": (drop_new, None, (2 * R * D + R * r) * B2),
            "fc2 backward: up_add_mul vs zero + up_add + addcmul": (mul_new, mul_old, (3 * R * F + R * r) * B2),
        }
        for name, (new, old, nbytes) in arms.items():
            res_ms = {"new": [], "composed": []}
            with Stage(a.limit):
                new()
                if old:
                    old()
            for _ in range(a.rounds):
                for arm, fn in (("new", new), ("composed", old)):
                    if fn is None:
                        continue
                    with Stage(a.limit):
                        res_ms[arm].append(timed_ms(fn, a.iters))
            line = {"tool": TOOL, "part": "kernels", "branch": branch, "R": R, "D": D, "F": F, "rank": r, "kernel": name, "iters": a.iters,
                    "new_ms": spread(res_ms["new"])}
            if old:
                line.update(composed_ms=spread(res_ms["composed"]),
                            new_over_composed=round(statistics.median(res_ms["new"]) / statistics.median(res_ms["composed"]), 3))
            if nbytes:
                floor = nbytes / (rate * 1e12) * 1e3
                line.update(bytes_moved_once=nbytes, floor_ms=round(floor, 4), new_over_floor=round(statistics.median(res_ms["new"]) / floor, 2))
            print(json.dumps(line), flush=True)
        del h, res, pre, u, du, hbuf, ubuf, scratch, y


# ------------------------------------------------------------------------------------------------ (ii) step
def step_part(a, batches, margs):
    from multimodaldiscussiontransformer_amd.criterions import GraphPredictionNodeCrossEntropy
    from multimodaldiscussiontransformer_amd.ddp import DataParallel
    from multimodaldiscussiontransformer_amd.models import GraphormerModel
    crit = GraphPredictionNodeCrossEntropy(None, positive_weight=1.5, negative_weight=1.0)
    scal = torch.zeros(6, dtype=torch.float32, device="cuda")

    def make(targets):
        torch.manual_seed(1234)
        m = GraphormerModel.build_model(argparse.Namespace(**vars(margs)), task=None)
        m.add_lora(16, targets=targets)
        m = m.cuda().bfloat16().train()
        return dict(model=m, dp=DataParallel(m), trainable=sum(p.numel() for p in m.parameters() if p.requires_grad), fwdbwd=[])

    def fwdbwd(arm, pb):
        arm["dp"].zero_grad()
        loss, sample_size, log = crit(arm["model"], {"nsamples": pb.B, "net_input": {"batched_data": pb.batched_data}})
        loss.backward()
        scal[0] = loss.detach().float()
        scal[1].fill_(float(sample_size))
        arm["dp"].finish_backward(scal, fold_scale=True)

    arms = {}
    for kind, targets in (("q,v", "q,v"), ("all", "all")):
        with Stage(max(a.limit, 300)):
            arms[kind] = make(targets)
    for i in range(a.warmup):
        for arm in arms.values():
            with Stage(a.limit):
                fwdbwd(arm, batches[i % len(batches)])
    for i in range(a.steps):
        for arm in arms.values():
            pb = batches[i % len(batches)]
            with Stage(a.limit):
                arm["fwdbwd"].append(timed_ms(lambda: fwdbwd(arm, pb)))
    out = {k: dict(trainable_elements=v["trainable"], fwd_bwd_ms=spread(v["fwdbwd"])) for k, v in arms.items()}
    print(json.dumps({"tool": TOOL, "part": "step", "workload": "bench.py --config base (32 trees x 64 comments, image-frac 0.25), bf16, resident batches, add_lora(16)",
                      "steps": a.steps, "warmup": a.warmup, "arms": out,
                      "all_over_qv_fwd_bwd": round(out["all"]["fwd_bwd_ms"]["median"] / out["q,v"]["fwd_bwd_ms"]["median"], 3)}), flush=True)


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
        raise SystemExit("[lora_dense_ab] no GPU: nothing is measured without one")
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
