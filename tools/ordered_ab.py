#!/usr/bin/env python3
"""What deterministic (ordered) mode costs: the bench workload timed in the default mode and with MDT_DETERMINISTIC=1, in
one call.  Each arm is a fresh `bench.py --gpus 1` process (the switch is read when the engine is imported; bench.py itself
is not touched) under its own time limit; a failed or overrunning arm ends the tool — nothing more is started on the device.
Prints the two result lines' timings and their ratio as one JSON line.

    python tools/ordered_ab.py [--steps 8] [--warmup 3] [--limit 420] [-- extra bench.py flags]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_arm(name, env_over, steps, warmup, limit, extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)] + extra
    env = dict(os.environ, **env_over)
    try:
        r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"[ordered_ab] arm {name}: no result within {limit} s — stopping")
    if r.returncode != 0:
        raise SystemExit(f"[ordered_ab] arm {name}: bench.py exited with {r.returncode} — stopping\n{r.stderr[-2000:]}")
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{") and '"metric"' in ln]
    if not lines:
        raise SystemExit(f"[ordered_ab] arm {name}: no result line\n{r.stdout[-1000:]}")
    out = json.loads(lines[-1])
    if out.get("value") is None:
        raise SystemExit(f"[ordered_ab] arm {name}: bench.py reported no value: {lines[-1][:500]}")
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=420, help="seconds each arm may take")
    ap.add_argument("extra", nargs="*", help="further bench.py flags (after --)")
    a = ap.parse_args()
    arms = {}
    for name, env in (("default", {"MDT_DETERMINISTIC": "0"}), ("ordered", {"MDT_DETERMINISTIC": "1"})):
        o = run_arm(name, env, a.steps, a.warmup, a.limit, a.extra)
        arms[name] = {k: o.get(k) for k in ("value", "unit", "ms_per_step", "ms_per_step_median", "dtype")}
        print(f"[ordered_ab] {name}: {arms[name]}", file=sys.stderr, flush=True)
    d, o = arms["default"], arms["ordered"]
    print(json.dumps({"tool": "ordered_ab", "steps": a.steps, "warmup": a.warmup, "default": d, "ordered": o,
                      "ordered_over_default_ms_per_step": round(o["ms_per_step_median"] / d["ms_per_step_median"], 3)}), flush=True)


if __name__ == "__main__":
    main()
