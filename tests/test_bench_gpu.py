"""bench.py as a command on the GPU: a plain run reports the headline figure
only and --dump-outputs writes the calls of its last timed step.

One short run of C1 (BASELINE configs[0], the smallest config): the dumped
arrays must be the C oracle's calls at the benchmark's thresholds (0.1 / 5),
element for element, in float64; the result line carries the contract fields
and none of the measurements that --full adds.
"""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import depth_util as du

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("single_batch_ms_per_step", "roofline", "roofline_timed", "roofline_hbm", "cpu_baseline", "e2e")


@pytest.mark.timeout(300)
def test_plain_run_dumps_the_last_step(pkg, tmp_path):
    out = tmp_path / "dump"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--config", "c1", "--steps", "5",
           "--warmup", "1", "--dump-outputs", str(out)]
    p = subprocess.run(cmd, env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-4000:]
    rec = json.loads(lines[0])
    bench = importlib.import_module("bench")
    assert rec["metric"] == bench.METRIC and rec["unit"] == "aligned bases/s" and rec["dtype"] == "u8"
    assert rec["higher_is_better"] is True and rec["n_gpus"] == 1 and rec["steps"] == 5 and rec["full"] is False
    assert rec["value"] > 0 and rec["ms_per_step"] > 0
    # value = aligned bases of the timed steps / their wall time, ms_per_step = that wall time / steps
    per_step = rec["config"]["aligned_bases_per_step"]
    assert abs(rec["value"] * rec["ms_per_step"] * 1e-3 - per_step) <= 1e-9 * per_step
    assert not [k for k in FULL_ONLY if k in rec]

    samples, _ = bench.shard_samples(pkg, "c1", 0, 1)
    exp = [du.derive(f, 0.1, 5.0) for f in du.oracle_many(samples, -1.0, 1.0)]
    md = np.load(out / "max_depth.npy")
    assert md.dtype == np.float64 and md.shape == (len(samples),)
    written = md.nbytes
    for s, e in enumerate(exp):
        got = {"max_depth": int(md[s])}
        for f in bench.DUMP_FIELDS:
            a = np.load(out / f"sample{s}_{f}.npy")
            assert a.dtype == np.float64
            assert np.array_equal(a, np.floor(a))
            got[f] = a.astype(np.int64)
            written += a.nbytes
        du.compare(got, e, ("bench dump c1", s))
    assert len(exp[0]["base"]) > 0
    assert rec["dump_outputs"]["bytes"] == written <= bench.DUMP_MAX_BYTES
    assert not [f for f in os.listdir(out) if f.endswith("_rows.npy")]  # C1 fits: nothing sampled
