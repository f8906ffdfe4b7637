#!/usr/bin/env python3
"""What adapter-input dropout (--lora-dropout) costs inside the adapter kernels, measured on tools/lora_ab.py's frame: ONE process,
a shared warm-up, alternating arms, device events, every timed stage under a watchdog of its own.  Prints JSON lines and appends
them to --out (default profiles/lora_dropout_ab_mi355x.jsonl).

  (i)  kernels   at the bench workload's block shapes (token rows R of the text and of the image branch of one bench.py --config base
                 batch, D 768, F 3072, rank 16, p 0.1), for each masked kernel three arms:
                   (a) masked     ops.lora_down_drop / lora_wgrad_drop / lora_up_add_mul_drop
                   (b) plain      ops.lora_down / lora_wgrad / lora_up_add_mul: (a) - (b) is the price of the mask
                   (c) composed   what exists without the feature: ops.dropout of the wide operand into a scratch tensor, then the
                                  plain kernel — one more read and one more write of that operand, and a copy to keep for backward
                 each next to its traffic floor (bytes every operand moves once / the rate of a device copy timed in this call).
                 Before timing, (a) is checked against the fp64 reference within the kernel tests' bound, and (c) against the same
                 reference with the bound widened by the one rounding of x / (1 - p) to bf16 that only (c) makes.
  (ii) step      forward + backward of the bench step with add_lora(16, targets="all") at dropout 0 and at 0.1, with the peak
                 allocated memory of both

    python tools/lora_dropout_ab.py [--part kernels|step|both] [--rounds 5] [--iters 10] [--steps 5] [--warmup 2] [--limit 120]
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

TOOL = "lora_dropout_ab"
OUT = None


def emit(line):
    text = json.dumps(dict(tool=TOOL, **line))
    print(text, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(text + "\n")


def copy_rate(limit):
    with Stage(limit):
        src, dst = torch.empty(1 << 29, dtype=torch.uint8, device="cuda"), torch.empty(1 << 29, dtype=torch.uint8, device="cuda")
        dst.copy_(src)
        ms = min(timed_ms(lambda: dst.copy_(src), 5) for _ in range(3))
    rate = 2 * (1 << 29) / (ms * 1e-3) / 1e12
    emit({"part": "stream_rate", "source": "device copy of 512 MiB timed in this call (read + write bytes)", "tb_per_s": round(rate, 3)})
    return rate


# ------------------------------------------------------------------------------------------------ (i) kernels
def agreement(ops, kind, got_a, got_c, t, x, w, aux, y0, p, seed, alpha):
    """(a) within the kernel tests' bound of the fp64 reference; (c) within that bound widened by its operand rounding.  On the device
    in fp64: the mask is ops.dropout_mask's, the error model tests/lora_reference.py's."""
    import tests.gemm_reference as GR
    import tests.lora_dropout_reference as LDR
    import tests.lora_reference as LR
    R, W = x.shape if kind != "up_mul" else y0.shape
    keep = ops.dropout_mask(R * W, p, seed).reshape(R, W) != 0
    f = LDR.factor(alpha, p)
    if kind == "up_mul":
        sc = keep.double() * GR.drop_params(p)[1]
        v, d = LDR.up_add_mul_drop(t, w, y0, aux, alpha, sc)
        extra = 2.0 ** -8 * (v - y0.double()).abs()                # (c) rounds s * aux to bf16: half an ulp, at most 2^-8 of the term
        dt = torch.bfloat16
    else:
        xm = torch.where(keep, x.double(), torch.zeros((), dtype=torch.float64, device=x.device))
        if kind == "down":
            v, d = LR.down(xm, w, f)
            extra = 2.0 ** -8 * f * (xm.abs() @ w.double().abs().t())
            dt = torch.bfloat16
        else:
            v, d = LR.wgrad(t, xm, y0, f)
            extra = 2.0 ** -8 * f * (t.double().abs().t() @ xm.abs())
            dt = torch.float32
    ra = float(((got_a.double() - v).abs() / LR.bound(v, d, dt).clamp(min=1e-300)).max())
    rc = float(((got_c.double() - v).abs() / LR.bound(v, d + extra, dt).clamp(min=1e-300)).max())
    return dict(a_worst_err_over_bound=round(ra, 3), a_within_bound=ra <= 1.0, c_worst_err_over_widened_bound=round(rc, 3), c_within_widened_bound=rc <= 1.0)


def kernel_part(a, shapes, rate):
    from multimodaldiscussiontransformer_amd import engine, ops
    D, F, n, p, seed = 768, 3072, 16, 0.1, 0x5EED0D0
    B2 = 2
    for branch, R in shapes.items():
        g = torch.Generator(device="cuda").manual_seed(1)
        rnd = lambda *shape, sc=1.0: ((torch.rand(*shape, generator=g, device="cuda") * 2 - 1) * sc).to(torch.bfloat16)      # noqa: E731
        for W in (D, F):
            x, scratch = rnd(R, W), torch.empty(R, W, dtype=torch.bfloat16, device="cuda")
            A = rnd(n, W, sc=W ** -0.5)
            t, dt_ = torch.empty(R, n, dtype=torch.bfloat16, device="cuda"), rnd(R, n, sc=0.1)
            gA = torch.zeros(n, W, device="cuda")
            ws = engine.ordered_workspace(ops.lib.mdt_lora_wgrad_workspace_bytes(R, n, W), "cuda")
            cases = {
                "down": dict(name=f"down t=drop(x) A^T (K {W}, n {n})", bytes=(R * W + R * n) * B2,
                             a=lambda: ops.lora_down_drop(x, A, out=t, drop_p=p, drop_seed=seed), b=lambda: ops.lora_down(x, A, out=t),
                             c=lambda: (ops.dropout(x, p, seed, out=scratch), ops.lora_down(scratch, A, out=t)), out=lambda: t.clone()),
                "wgrad": dict(name=f"wgrad dA+=dt^T drop(x) (N {W}, n {n})", bytes=(R * W + R * n) * B2,
                              a=lambda: ops.lora_wgrad_drop(dt_, x, gA, drop_p=p, drop_seed=seed, ws=ws), b=lambda: ops.lora_wgrad(dt_, x, gA, ws=ws),
                              c=lambda: (ops.dropout(x, p, seed, out=scratch), ops.lora_wgrad(dt_, scratch, gA, ws=ws)), out=lambda: gA.clone()),
            }
            if W == F:      # fc2's share of du: the only site whose dx takes the multiply by u
                du, u = rnd(R, W, sc=0.1), rnd(R, W)
                cases["up_mul"] = dict(name=f"up_add_mul du+=(s o (dt A)) u (N {W}, n {n})", bytes=(3 * R * W + R * n) * B2,
                                       a=lambda: ops.lora_up_add_mul_drop(dt_, A, du, u, drop_p=p, drop_seed=seed), b=lambda: ops.lora_up_add_mul(dt_, A, du, u),
                                       c=lambda: (ops.dropout(u, p, seed, out=scratch), ops.lora_up_add_mul(dt_, A, du, scratch)), out=lambda: du.clone())
            for kind, c in cases.items():
                line = {"part": "kernels", "branch": branch, "R": R, "width": W, "rank": n, "p": p, "kernel": c["name"], "iters": a.iters}
                try:
                    with Stage(max(a.limit, 300)):                 # the agreement check holds fp64 copies of the wide operand
                        acc = du if kind == "up_mul" else gA if kind == "wgrad" else None
                        y0 = None if acc is None else acc.clone()
                        outs = []
                        for arm in ("a", "c"):
                            if acc is not None:
                                acc.copy_(y0)
                            c[arm]()
                            outs.append(c["out"]())
                        line.update(agreement(ops, kind, outs[0], outs[1], dt_, x, A, u if kind == "up_mul" else None, y0, p, seed, 1.0))
                        del outs
                        c["b"]()                                   # shared warm-up: all three arms have run
                    res = {"a": [], "b": [], "c": []}
                    for _ in range(a.rounds):                      # alternating arms
                        for arm in res:
                            with Stage(a.limit):
                                res[arm].append(timed_ms(c[arm], a.iters))
                except Exception as e:  # noqa: BLE001
                    emit(dict(line, error=str(e)[:300]))
                    continue
                med = {k: statistics.median(v) for k, v in res.items()}
                floor = c["bytes"] / (rate * 1e12) * 1e3
                emit(dict(line, masked_ms=spread(res["a"]), plain_ms=spread(res["b"]), composed_ms=spread(res["c"]), bytes_moved_once=c["bytes"],
                          floor_ms=round(floor, 4), masked_over_floor=round(med["a"] / floor, 2), plain_over_floor=round(med["b"] / floor, 2),
                          mask_price_ms=round(med["a"] - med["b"], 4), masked_over_plain=round(med["a"] / med["b"], 3),
                          masked_over_composed=round(med["a"] / med["c"], 3)))
            del x, scratch, t, dt_, gA, ws, cases
            torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ (ii) step
def step_part(a, batches, margs):
    from multimodaldiscussiontransformer_amd.criterions import GraphPredictionNodeCrossEntropy
    from multimodaldiscussiontransformer_amd.ddp import DataParallel
    from multimodaldiscussiontransformer_amd.models import GraphormerModel
    crit = GraphPredictionNodeCrossEntropy(None, positive_weight=1.5, negative_weight=1.0)
    scal = torch.zeros(6, dtype=torch.float32, device="cuda")

    def make(p):
        torch.manual_seed(1234)
        m = GraphormerModel.build_model(argparse.Namespace(**vars(margs)), task=None)
        m.add_lora(16, targets="all", dropout=p)
        m = m.cuda().bfloat16().train()
        return dict(model=m, dp=DataParallel(m), fwdbwd=[], peak=[])

    def fwdbwd(arm, pb):
        arm["dp"].zero_grad()
        loss, sample_size, _ = crit(arm["model"], {"nsamples": pb.B, "net_input": {"batched_data": pb.batched_data}})
        loss.backward()
        scal[0] = loss.detach().float()
        scal[1].fill_(float(sample_size))
        arm["dp"].finish_backward(scal, fold_scale=True)

    arms = {}
    for name, p in (("dropout_0", 0.0), ("dropout_0.1", 0.1)):
        with Stage(max(a.limit, 300)):
            arms[name] = make(p)
    for i in range(a.warmup):
        for arm in arms.values():
            with Stage(a.limit):
                fwdbwd(arm, batches[i % len(batches)])
    for i in range(a.steps):
        for arm in arms.values():
            pb = batches[i % len(batches)]
            with Stage(a.limit):
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                arm["fwdbwd"].append(timed_ms(lambda: fwdbwd(arm, pb)))
                arm["peak"].append(torch.cuda.max_memory_allocated() / 2 ** 30)
    out = {k: dict(fwd_bwd_ms=spread(v["fwdbwd"]), peak_allocated_gib=round(max(v["peak"]), 3)) for k, v in arms.items()}
    emit({"part": "step", "workload": "bench.py --config base (32 trees x 64 comments, image-frac 0.25), bf16, add_lora(16, targets=all), forward + backward, "
          "both models resident", "steps": a.steps, "warmup": a.warmup, "arms": out,
          "dropout_cost_fwd_bwd_ms": round(out["dropout_0.1"]["fwd_bwd_ms"]["median"] - out["dropout_0"]["fwd_bwd_ms"]["median"], 3),
          "peak_growth_gib": round(out["dropout_0.1"]["peak_allocated_gib"] - out["dropout_0"]["peak_allocated_gib"], 3)})


def main():
    global OUT
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--part", default="both", choices=["kernels", "step", "both"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=120, help="seconds a timed stage may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lora_dropout_ab_mi355x.jsonl"), help="file the JSON lines are appended to ('' for none)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit(f"[{TOOL}] no GPU: nothing is measured without one")
    OUT = a.out or None
    torch.cuda.set_device(0)
    batches, margs = bench_batches(2)
    pb = batches[0]
    nb = margs.num_bottleneck_tokens
    shapes = {"text": int(pb.text_mask.sum()) + nb * pb.M, "image": pb.I * ((224 // 16) ** 2 + 1 + nb)}
    if a.part in ("kernels", "both"):
        kernel_part(a, shapes, copy_rate(a.limit))
    if a.part in ("step", "both"):
        step_part(a, batches, margs)


if __name__ == "__main__":
    main()
