#!/usr/bin/env python3
"""k_shift at radius 1, 4, 7, 8 and 16 against k_align_cross and k_psnr_hvs on the same resident 64 x 1080p 4:2:0 clips, at 8 and
10 bits, in one process:

    python scripts/shift_rate.py [--out FILE]

Two streams of 64 frames each (noise over the depth's range: the kernel is integer arithmetic with no data-dependent path), the
distorted one unrelated to the reference.  Kernel times are vqa_profile_read's (HIP events): 4 warm-up calls, then the median of
24 calls per kernel id.  The working set of one call (2 x 199 MB at 8 bits) exceeds the 256 MiB Infinity Cache.

Prints one JSON document with ms per kernel id and, for k_shift, the bytes of the model "plane 0 of both streams read once" -
2 x frames x H x W x bytes per sample - and the rate they give against the 8 TB/s roof and the 6.29 TB/s a float4 copy measures
on this part; k_shift over k_align_cross (radius 8) at every radius, and the time at 10 bits over the time at 8."""
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
args = ap.parse_args()
H, W, NF, REPS, WARM = args.height, args.width, args.frames, args.reps, 4
HBM_ROOF_TBS, HBM_COPY_TBS = 8.0, 6.29
SAMPLES = H * W * 3 // 2
RADII = (1, 4, 7, 8, 16)
out = {"geometry": [H, W], "frames": NF, "hbm_roof_tb_s": HBM_ROOF_TBS, "hbm_copy_tb_s": HBM_COPY_TBS}


def clip(depth, rng):
    """NF frames out of a few distinct ones, shuffled"""
    base = rng.integers(0, 1 << depth, (4, SAMPLES)).astype(np.uint16 if depth > 8 else np.uint8)
    return np.concatenate([base] * (NF // 4))[rng.permutation(NF)]


def timed(eng, ids, fn):
    times = {k: [] for k in ids}
    for r in range(WARM + REPS):
        fn(r)
        prof = eng.profile_read(reset=True)
        if r >= WARM:
            for k in ids:
                times[k].append(prof[k][0])
    return {k: dict(median_ms=float(np.median(v)), min_ms=min(v), max_ms=max(v)) for k, v in times.items()}


with rtvqa_amd.Engine(0) as eng:
    for depth in (8, 10):
        planes = yuv_planes(H, W, "420", depth)
        model_bytes = 2.0 * NF * H * W * (2 if depth > 8 else 1)
        rng = np.random.default_rng(depth)
        ref, dist = eng.upload(clip(depth, rng)), eng.upload(clip(depth, rng))
        eng.profile(True)
        eng.profile_read(reset=True)
        got = {"model_bytes": model_bytes}
        got.update(timed(eng, ("k_align_cross",), lambda r: eng.align(ref, dist, planes, radius=8)))
        got.update(timed(eng, ("k_psnr_hvs",), lambda r: eng.psnr_hvs(ref, dist, planes)))
        for radius in RADII:
            t = timed(eng, ("k_shift",), lambda r: eng.shift(ref, dist, planes, radius=radius))["k_shift"]
            tbs = model_bytes / (t["median_ms"] * 1e-3) / 1e12
            t.update(model_tb_s=tbs, share_of_roof=tbs / HBM_ROOF_TBS, share_of_copy_rate=tbs / HBM_COPY_TBS,
                     over_k_align_cross=t["median_ms"] / got["k_align_cross"]["median_ms"],
                     over_k_psnr_hvs=t["median_ms"] / got["k_psnr_hvs"]["median_ms"])
            got["k_shift_r%d" % radius] = t
        eng.profile(False)
        out["%dbit" % depth] = got
        for c in (ref, dist):
            c._owner.free()
        del ref, dist
    for radius in RADII:
        out["r%d_10bit_over_8bit" % radius] = (out["10bit"]["k_shift_r%d" % radius]["median_ms"] /
                                               out["8bit"]["k_shift_r%d" % radius]["median_ms"])
    out["bound"] = "not attributed"   # no counter run was made
print(json.dumps(out, indent=1))
if args.out:
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
