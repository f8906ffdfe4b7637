"""bench.py's one JSON line — the contract the driver reads — at toy sizes, for every configuration it offers: the N = 1 form
(`python bench.py`), the shipped launch (`--config launch`: micro-batches, frozen prefix, fused Adam), mDT-large shapes, fp8 operands.
The numbers mean nothing at these sizes; the fields, their types and the legs that must have run under --full (roofline from live
HIP events, cpu_baseline from the oracle, the numerics self-check) do, and so do a plain run's outputs (--dump-outputs)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(*extra, timeout=420):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--trees", "2", "--nodes", "8", *extra],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.parametrize("extra,dtype", [((), "bf16"), (("--config", "launch"), "bf16"), (("--config", "large"), "bf16"), (("--dtype", "fp8", "--no-selfcheck"), "fp8")])      # the self-check's fp8 gates are calibrated at the full size
def test_bench_line_contract(extra, dtype):
    d = run_bench(*extra, "--full", "--no-cpu-baseline")
    assert d["metric"] == "discussion-tree comments/sec fwd+bwd" and d["unit"] == "comments/s" and d["higher_is_better"] is True
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["scaling"] == "weak" and d["data"] == "synthetic"
    assert d["vs_baseline"] is None and d["dtype"] == dtype
    assert d["value"] > 0 and d["ms_per_step"] > 0
    assert abs(d["value"] - d["config"]["comments_per_step_per_gpu"] / d["ms_per_step"] * 1e3) <= 0.02 * d["value"]
    assert isinstance(d["config"]["workload"], str) and "model" not in d["config"]
    rf = d["roofline"]
    assert rf["bound"] == "mfma" and rf["unit"] == "TFLOP/s" and rf["peak"] in (2500.0, 5000.0)
    assert rf["achieved"] > 0 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3 and rf["launches"] > 0
    if "--no-selfcheck" not in extra:
        assert d["selfcheck"]["kernels"] == "passed"


def test_bench_cpu_baseline_leg_runs_the_oracle():
    d = run_bench("--full", "--trees", "1", "--nodes", "4")
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["unit"] == "comments/s" and cb["value"] > 0 and cb["cores"] >= 1 and "oracle" in cb["sample"]


# with the optimizer the run is ONE step: after four Adam updates at this toy size, 79 of the 4 M sampled gradient
# elements differed between two runs by up to 2 % of the largest (the atomics' reordered sums, carried on by the updates)
@pytest.mark.parametrize("extra,steps", [((), 3), (("--config", "launch", "--warmup", "0"), 1)])
def test_bench_plain_run_dumps_the_last_steps_outputs(tmp_path, extra, steps):
    """A plain run times --steps steps and leaves the --full legs out; --dump-outputs writes the last timed step's results
    (with the optimizer: also the updated parameters), float32 / float64 and 64 MB at most, and a second run with the same
    arguments computes the same values (fixed trees, weights and dropout seeds; split-K atomics reorder fp32 sums)."""
    runs = []
    for k in range(2):
        d = run_bench(*extra, "--steps", str(steps), "--dump-outputs", str(tmp_path / str(k)))
        assert d["steps"] == steps and d["ms_per_step"] > 0 and d["value"] > 0
        assert not {"roofline", "selfcheck", "cpu_baseline", "host_issue_ms_per_step"} & set(d)
        runs.append({f[:-4]: np.load(tmp_path / str(k) / f) for f in os.listdir(tmp_path / str(k))})
    a, b = runs
    names = {"scalars", "grad_scale", "grad_norms", "grad_sample"} | ({"param_norms", "param_sample"} if extra else set())
    assert set(a) == set(b) == names
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    for n in names:
        assert a[n].dtype in (np.float32, np.float64) and a[n].shape == b[n].shape and np.isfinite(a[n]).all(), n
        np.testing.assert_allclose(a[n], b[n], rtol=1e-3, atol=1e-3 * float(np.abs(a[n]).max()), err_msg=n)
    assert a["scalars"].shape == (6,) and np.isclose(a["grad_scale"][0], 1.0 / max(a["scalars"][1], 1.0), rtol=1e-6)
    assert a["grad_norms"].max() > 0
