#!/usr/bin/env python3
"""k_mdsi_map and k_mdsi_dev against k_gmsd and k_ciede on the same resident 64 x 1080p clips in one process - 4:2:0 at 8 and 10
bits, packed bgr24 at 8 (k_gmsd and k_ciede on the same bgr24 clips too):

    python scripts/mdsi_rate.py [--out FILE]

Per layout two noise clips alternate, the one compared with the other, so that the working set (2 x 199 MB at 4:2:0, 8 bits)
exceeds the 256 MiB Infinity Cache.  Kernel times are vqa_profile_read's (HIP events): 4 warm-up calls, then the median of 24
calls.  Prints one JSON document with ms per kernel id and, for MDSI, the bytes of its model - one read of every sample of both
streams plus 8 bytes per downsampled sample for the map of g (written once, read once) - and the byte rate against the
8.0 TB/s HBM roof."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rtvqa_amd
from rtvqa_amd.engine import bgr_planes, mdsi_factor, yuv_planes

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the JSON document here")
args = ap.parse_args()
H, W, NF, REPS, WARM = 1080, 1920, 64, 24, 4
F = mdsi_factor(H, W)
MAP = -(-H // F) * -(-W // F)
out = {"factor": F, "map_samples": MAP}
with rtvqa_amd.Engine(0) as eng:
    for tag, depth, planes, samples in (("yuv420p", 8, yuv_planes(H, W, "420", 8), H * W * 3 // 2),
                                        ("yuv420p10le", 10, yuv_planes(H, W, "420", 10), H * W * 3 // 2),
                                        ("bgr24", 8, bgr_planes(H, W), H * W * 3)):
        rng = np.random.default_rng(depth + len(tag))
        dt = np.uint16 if depth > 8 else np.uint8
        clips = []
        for k in range(2):
            base = rng.integers(0, 1 << depth, (4, samples)).astype(dt)
            clips.append(eng.upload(np.concatenate([base] * (NF // 4))[rng.permutation(NF)]))
        eng.profile(True)
        calls = (("mdsi", ("k_mdsi_map", "k_mdsi_dev"), lambda r: eng.mdsi(clips[r % 2], clips[1 - r % 2], planes)),
                 ("gmsd", ("k_gmsd",), lambda r: eng.gmsd(clips[r % 2], clips[1 - r % 2], planes)),
                 ("ciede", ("k_ciede",), lambda r: eng.ciede(clips[r % 2], clips[1 - r % 2], planes)))
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
                out["%s_%s" % (k, tag)] = dict(median_ms=float(np.median(t)), min_ms=t[0], max_ms=t[-1])
            if name == "mdsi":
                med = sum(out["%s_%s" % (k, tag)]["median_ms"] for k in ids)
                nbytes = 2.0 * NF * samples * np.dtype(dt).itemsize + 8.0 * NF * MAP
                out["mdsi_%s" % tag] = dict(median_ms=med, model_bytes=nbytes, tb_per_s=nbytes / (med * 1e-3) / 1e12,
                                            share_of_8p0=nbytes / (med * 1e-3) / 8.0e12)
        eng.profile(False)
        del clips
print(json.dumps(out, indent=1))
if args.out:
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
