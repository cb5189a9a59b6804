"""bench.py --dump-outputs on the GPU: a plain run (no --full) writes what its last timed step returned, and those records
are the oracle's for the frames of the synthetic stream at the checked batch positions."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from oracle import check
from rtvqa_amd.engine import FRAME_DTYPE, PLANE_DTYPE

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _records(d, B):
    """the dumped fields back into the engine's record arrays (every field is exact in float64)"""
    c = np.zeros(B, FRAME_DTYPE)
    for f in FRAME_DTYPE.names:
        c[f] = np.load(os.path.join(d, "complexity_%s.npy" % f))
    q = np.zeros((B, 3), PLANE_DTYPE)
    for f in PLANE_DTYPE.names:
        q[f] = np.load(os.path.join(d, "quality_%s.npy" % f))
    return q, c


def test_plain_bench_dumps_the_last_timed_step(tmp_path):
    B = 8
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "VQA_BENCH_DEVICE")}
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--batch", str(B), "--steps", "2", "--warmup", "1",
           "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2500:])
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["kernels"] == {} and "verified" not in line and "cpu_baseline" not in line   # the legs of --full
    q, c = _records(str(tmp_path), B)
    for j in (0, 1, B - 1):
        _, exp = bench._expect_item(("natural", 0, 1080, 1920, B, j, True, "sad", "gauss", False, "block8"))
        assert check.compare(exp, c[j], q[j], "gauss") == [], j
