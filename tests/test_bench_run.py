"""
bench.py end to end on one GPU, on the 70k-vertex config (the headline workload's code path, a smaller system): the plain run prints
the headline line and nothing that takes runs of its own; --full adds the roofline, the per-launch table, the constructor repeats, the
CPU baselines and the forward error against the fp64 oracle.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKLOAD = "cfg2_bunny70k"
KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
        "data", "config", "roofline", "cpu_baseline")


def run_bench(*extra):
    env = dict(os.environ)
    for name in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "LS_DIST_LOOPBACK"):
        env.pop(name, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--workload", WORKLOAD, *extra]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    for key in KEYS:
        assert key in d, key
    assert d["metric"] == "from_differential_solves_per_sec" and d["unit"] == "solves/s" and d["n_gpus"] == 1
    assert d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["ms_per_step"] > 0 and abs(d["value"] - 1e3 / d["ms_per_step"]) <= 1e-6 * d["value"]
    assert WORKLOAD in d["config"]["workload"] and d["config"]["method"] == "nested-dissection"
    return d


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_x(tmp_path):
    from largesteps import synthetic
    d = run_bench("--dump-outputs", str(tmp_path))
    assert d["roofline"] is None and d["cpu_baseline"] is None
    c = d["config"]
    assert c["factor_seconds"] > 0 and c["assemble_ms"] > 0
    for moved in ("tolerance", "launches", "assemble", "to_differential", "factor_seconds_steady", "rel_residual"):
        assert moved not in c, moved
    # u = M v: the solution the timed steps returned is v
    v, _, _ = synthetic.config_mesh(WORKLOAD)
    x = np.load(tmp_path / "x.npy")
    assert x.dtype == np.float32 and x.shape == v.shape
    assert np.abs(x - v).max() <= 1e-4 * np.abs(v).max()


@pytest.mark.gpu
def test_full_run_adds_roofline_baselines_and_oracle_parity():
    d = run_bench("--full")
    c = d["config"]
    tol = c["tolerance"]
    assert tol["measured"] is not None and tol["met"] is True, tol
    assert c["launches"] and all(row["us"] > 0 for row in c["launches"])
    assert c["factor_seconds_steady"] is not None and len(c["factor_seconds_cycles"]) == 6
    assert c["assemble"]["us_per_call"] > 0 and c["to_differential"]["us_per_call"] > 0
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and abs(r["frac"] - r["achieved"] / r["peak"]) <= 1e-9
    b = d["cpu_baseline"]
    assert b["value"] > 0 and b["cores"] == 1
    assert set(b["extra"]) == {"B2_reference_cg_cpu_cfg2", "B3_torch_cg_hip_device"}
