#!/usr/bin/env python3
"""k_sig against k_align_cross (radius 0) and k_sigstats_accum on the same resident 64 x 1080p 4:2:0 clips, at 8 and 10 bits, and the
cross stage (k_sig_diag, k_sig_best) on random signatures, in one process:

    python scripts/sync_rate.py [--out FILE]

Two streams of 64 frames each (noise over the depth's range: the kernels are integer arithmetic with no data-dependent path).
Kernel times are vqa_profile_read's (HIP events): 4 warm-up calls, then the median of 24 calls per kernel id.  The cross stage
runs at (4096, 4096) and (65536, 65536) signatures; its larger size takes 6 calls after 1 warm-up.

Prints one JSON document with ms per kernel id and, for k_sig, the bytes of the model "plane 0 read once" - frames x H x W x bytes
per sample - and the rate they give against the 8 TB/s roof and the 6.29 TB/s a float4 copy measures on this part."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rtvqa_amd
from rtvqa_amd.engine import yuv_planes

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the JSON document here")
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--frames", type=int, default=64)
ap.add_argument("--reps", type=int, default=24)
ap.add_argument("--cross", type=int, nargs="*", default=[4096, 65536], help="the signatures of either side of a cross")
args = ap.parse_args()
H, W, NF, REPS, WARM = args.height, args.width, args.frames, args.reps, 4
HBM_ROOF_TBS, HBM_COPY_TBS = 8.0, 6.29
SAMPLES = H * W * 3 // 2
out = {"geometry": [H, W], "frames": NF, "hbm_roof_tb_s": HBM_ROOF_TBS, "hbm_copy_tb_s": HBM_COPY_TBS}


def clip(depth, rng):
    """NF frames out of a few distinct ones, shuffled"""
    base = rng.integers(0, 1 << depth, (4, SAMPLES)).astype(np.uint16 if depth > 8 else np.uint8)
    return np.concatenate([base] * (NF // 4))[rng.permutation(NF)]


def timed(eng, ids, fn, reps=REPS, warm=WARM):
    times = {k: [] for k in ids}
    for r in range(warm + reps):
        fn(r)
        prof = eng.profile_read(reset=True)
        if r >= warm:
            for k in ids:
                times[k].append(prof[k][0])
    return {k: dict(median_ms=float(np.median(v)), min_ms=min(v), max_ms=max(v)) for k, v in times.items()}


with rtvqa_amd.Engine(0) as eng:
    for depth in (8, 10):
        planes = yuv_planes(H, W, "420", depth)
        model_bytes = 1.0 * NF * H * W * (2 if depth > 8 else 1)
        rng = np.random.default_rng(depth)
        ref, dist = eng.upload(clip(depth, rng)), eng.upload(clip(depth, rng))
        eng.profile(True)
        eng.profile_read(reset=True)
        got = {"model_bytes": model_bytes}
        t = timed(eng, ("k_sig",), lambda r: eng.signature(ref, planes))["k_sig"]
        tbs = model_bytes / (t["median_ms"] * 1e-3) / 1e12
        t.update(model_tb_s=tbs, share_of_roof=tbs / HBM_ROOF_TBS, share_of_copy_rate=tbs / HBM_COPY_TBS)
        got["k_sig"] = t
        got.update(timed(eng, ("k_align_cross",), lambda r: eng.align(ref, dist, planes, radius=0)))
        got.update(timed(eng, ("k_sigstats_accum",), lambda r: eng.sigstats(ref, planes)))
        eng.profile(False)
        out["%dbit" % depth] = got
        for c in (ref, dist):
            c._owner.free()
        del ref, dist
    out["k_sig_10bit_over_8bit"] = out["10bit"]["k_sig"]["median_ms"] / out["8bit"]["k_sig"]["median_ms"]
    eng.profile(True)
    eng.profile_read(reset=True)
    for n in args.cross:
        rng = np.random.default_rng(n)
        d, r = (rng.integers(0, 256, (n, 256)).astype(np.uint8) for _ in range(2))
        big = n > 16384
        got = timed(eng, ("k_sig_diag", "k_sig_best"), lambda _r: eng.sig_cross(d, r), reps=6 if big else REPS, warm=1 if big else WARM)
        got["pairs"] = float(n) * n
        got["macs"] = 256.0 * n * n
        out["cross_%d" % n] = got
    eng.profile(False)
    out["bound"] = "not attributed"   # no counter run was made
print(json.dumps(out, indent=1))
if args.out:
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
