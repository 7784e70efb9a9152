"""
bench.py as a plain run (no --full): exactly --steps timed steps, the headline keys, none of the checks / baselines / extra passes
that live behind --full, and --dump-outputs: the arrays of the last timed step as float64 .npy files, the same from run to run.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus")
BEHIND_FULL = ("cpu_baseline", "vs_cpu_baseline", "shard_pass", "full_config", "vcor_fit", "parity_ok", "parity_maxabs",
               "parity_stages_ok", "parity_freivalds_maxabs")


def _bench(args, override):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    if override:
        env["DMK_BENCH_OVERRIDE"] = json.dumps(override)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
@pytest.mark.parametrize("workload,override,names", [
    ("C3", {"mesh": [3, 2, 2], "nlo": 24, "naux": 16, "nval": 8, "spin": 2},
     ("ew", "occ", "mu", "sigma", "rho_R", "basis", "C_ao_emb", "eri", "H1", "JK_core", "rdm1_emb")),
    ("C1", None, ("ew", "occ", "mu", "sigma", "rho_R", "basis"))])
def test_plain_run_and_dump_outputs(tmp_path, workload, override, names):
    runs = []
    for tag in ("a", "b"):
        d = str(tmp_path / tag)
        res = _bench(["--gpus", "1", "--steps", "3", "--warmup", "2", "--workload", workload, "--dump-outputs", d], override)
        for key in HEADLINE:
            assert key in res, key
        for key in BEHIND_FULL:
            assert key not in res, key
        assert res["steps"] == 3 and res["warmup"] == 2 and res["n_gpus"] == 1 and res["dtype"] == "f64"
        assert res["ms_per_step"] > 0 and res["value"] > 0
        listed = res["dump_outputs"]
        for name in names:
            assert name in listed, name
        assert sorted(os.listdir(d)) == sorted(n + ".npy" for n in listed)
        arrays = {n: np.load(os.path.join(d, n + ".npy"), allow_pickle=False) for n in listed}
        for n, x in arrays.items():
            assert x.dtype == np.float64 and list(x.shape) == listed[n]["shape"] and np.isfinite(x).all(), n
        assert sum(x.nbytes for x in arrays.values()) <= 64 * 1024 * 1024
        runs.append(arrays)
    if override:                      # spin 2, nemb = nlo + nval: every pair row of the small ERI is written
        nemb = override["nlo"] + override["nval"]
        npair = nemb * (nemb + 1) // 2
        assert runs[0]["eri"].shape == (3, npair, npair) and np.abs(runs[0]["eri"]).max() > 0
    # seeded inputs: the second run computes the same arrays (to the rounding of a different summation order at most)
    for n in runs[0]:
        scale = max(1.0, np.abs(runs[0][n]).max())
        assert runs[0][n].shape == runs[1][n].shape and np.abs(runs[0][n] - runs[1][n]).max() <= 1e-10 * scale, n
