#!/usr/bin/env python3
"""The six FSIM kernel ids against k_mdsi_map and k_gmsd on the same resident 64 x 1080p 4:2:0 clips, at 8 and 10 bits, in one
process:

    python scripts/fsim_rate.py [--out FILE]

Per depth two noise clips alternate, the one compared with the other, so that the working set (2 x 199 MB at 8 bits) exceeds the
256 MiB Infinity Cache.  Kernel times are vqa_profile_read's (HIP events): 4 warm-up calls, then the median of 24 calls, per kernel
id (a 1080p batch of 64 goes out in sub-slices of 3 frames, whose entries of one id are added).  Prints one JSON document with ms
per kernel id and, for k_fsim_dft, the flops of its model - per image 4 hd wd^2 (the real row transform) + 8 hd^2 wd (the column
transform) + 16 * 8 hd wd (hd + wd) (the sixteen inverses), every complex multiply-add as 8 flops - and the rate they give.  No
fp64 matrix peak is quoted: none has been measured here."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rtvqa_amd
from rtvqa_amd.engine import mdsi_factor, yuv_planes

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the JSON document here")
args = ap.parse_args()
H, W, NF, REPS, WARM = 1080, 1920, 64, 24, 4
F = mdsi_factor(H, W)
HD, WD = -(-H // F), -(-W // F)
FLOPS = 2.0 * NF * (4.0 * HD * WD * WD + 8.0 * HD * HD * WD + 128.0 * HD * WD * (HD + WD))
IDS = ("k_fsim_luma", "k_fsim_dft", "k_fsim_energy", "k_fsim_median", "k_fsim_pc", "k_fsim_pool")
out = {"factor": F, "grid": [HD, WD], "dft_model_flops": FLOPS}
with rtvqa_amd.Engine(0) as eng:
    for depth in (8, 10):
        planes = yuv_planes(H, W, "420", depth)
        samples = H * W * 3 // 2
        rng = np.random.default_rng(depth)
        dt = np.uint16 if depth > 8 else np.uint8
        clips = []
        for k in range(2):
            base = rng.integers(0, 1 << depth, (4, samples)).astype(dt)
            clips.append(eng.upload(np.concatenate([base] * (NF // 4))[rng.permutation(NF)]))
        eng.profile(True)
        calls = (("fsim", IDS, lambda r: eng.fsim(clips[r % 2], clips[1 - r % 2], planes)),
                 ("mdsi", ("k_mdsi_map",), lambda r: eng.mdsi(clips[r % 2], clips[1 - r % 2], planes)),
                 ("gmsd", ("k_gmsd",), lambda r: eng.gmsd(clips[r % 2], clips[1 - r % 2], planes)))
        for name, ids, fn in calls:
            times = {k: [] for k in ids}
            for r in range(WARM + REPS):
                fn(r)
                prof = eng.profile_read(reset=True)
                if r >= WARM:
                    for k in ids:
                        times[k].append(prof[k][0])
            for k in ids:
                t = sorted(times[k])
                out["%s_%dbit" % (k, depth)] = dict(median_ms=float(np.median(t)), min_ms=t[0], max_ms=t[-1])
            if name == "fsim":
                med = sum(out["%s_%dbit" % (k, depth)]["median_ms"] for k in ids)
                dft = out["k_fsim_dft_%dbit" % depth]["median_ms"]
                out["fsim_%dbit" % depth] = dict(median_ms=med, ms_per_frame_pair=med / NF, dft_tflops=FLOPS / (dft * 1e-3) / 1e12)
        eng.profile(False)
        del clips
print(json.dumps(out, indent=1))
if args.out:
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
