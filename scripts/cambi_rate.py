#!/usr/bin/env python3
"""The CAMBI kernels against k_gmsd and k_motion_sad on the same resident 64 x 1080p 4:2:0 clips, at 8 and 10 bits in one process:

    python scripts/cambi_rate.py [--out FILE] [--reps N]

Three contents per depth: a staircase (bands of 60 columns, steps of one level of the depth: the worst case, nearly every
sample is masked and walks its 65 x 65 window), natural texture (a smooth field with +-2 levels of noise: the mask is nearly
empty) and uniform noise (the mask is empty).  Four frames repeat through each clip.  Kernel times are vqa_profile_read's (HIP
events): 1 warm-up call, then the median of --reps (24) calls, a call being the launches of a 4:2:0 frame list (luma; the two
chroma planes).  k_gmsd compares the clip with itself, k_motion_sad walks it.
Prints one JSON document: per content and depth the milliseconds of the four CAMBI kernel ids, each id's share of their total,
the masked samples of all scales together, k_cambi_contrast's ns per masked sample, and the two yardsticks."""
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
ap.add_argument("--reps", type=int, default=24)
args = ap.parse_args()
H, W, NF, REPS, WARM = 1080, 1920, 64, args.reps, 1
IDS = ("k_cambi_mask", "k_cambi_decimate", "k_cambi_contrast", "k_cambi_topk")


def plane(kind, h, w, depth, rng):
    y, x = np.mgrid[0:h, 0:w]
    mid = 1 << (depth - 1)
    if kind == "staircase":
        return mid + x // 60 + (y // 270)
    if kind == "natural":
        return np.rint(mid + 0.3 * mid * np.sin(x / 37.0) * np.cos(y / 29.0)).astype(np.int64) + rng.integers(-2, 3, (h, w))
    return rng.integers(0, 1 << depth, (h, w))


def frame(kind, depth, rng):
    return np.concatenate([plane(kind, h, w, depth, rng).ravel() for h, w in ((H, W), (H // 2, W // 2), (H // 2, W // 2))])


out = {}
with rtvqa_amd.Engine(0) as eng:
    for depth in (8, 10):
        planes = yuv_planes(H, W, "420", depth)
        dt = np.uint16 if depth > 8 else np.uint8
        for kind in ("staircase", "natural", "noise"):
            rng = np.random.default_rng(depth)
            base = np.stack([frame(kind, depth, rng) for _ in range(4)]).astype(dt)
            clip = eng.upload(np.concatenate([base] * (NF // 4)))
            eng.profile(True)
            rec = eng.cambi(clip, planes)
            masked = int(rec["masked"].sum())
            eng.profile_read(reset=True)
            calls = (("cambi", IDS, lambda: eng.cambi(clip, planes)), ("k_gmsd", ("k_gmsd",), lambda: eng.gmsd(clip, clip, planes)),
                     ("k_motion_sad", ("k_motion_sad",), lambda: eng.motion(clip, planes)))
            row = {"masked_samples": masked, "cambi_luma_frame0": float(rec["cambi"][0, 0])}
            for name, ids, fn in calls:
                times = {k: [] for k in ids}
                for r in range(WARM + REPS):
                    fn()
                    prof = eng.profile_read(reset=True)
                    if r >= WARM:
                        for k in ids:
                            times[k].append(prof[k][0])
                for k in ids:
                    row[k + "_ms"] = float(np.median(times[k]))
            total = sum(row[k + "_ms"] for k in IDS)
            row["cambi_total_ms"] = total
            for k in IDS:
                row[k + "_share"] = row[k + "_ms"] / total
            row["contrast_ns_per_masked_sample"] = row["k_cambi_contrast_ms"] * 1e6 / masked if masked else None
            out["%s_%dbit" % (kind, depth)] = row
            print("%s %d bits: %s" % (kind, depth, json.dumps(row)), flush=True)
            eng.profile(False)
            del clip
print(json.dumps(out, indent=1))
if args.out:
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
