#!/usr/bin/env python3
"""k_artifacts against k_siti and k_gmsd on the same resident 64 x 1080p 4:2:0 clips, at 8 and 10 bits, on natural content and on
noise, in one process:

    python scripts/artifacts_rate.py [--out FILE]

Per depth and content two clips alternate - k_gmsd compares the one with the other, k_artifacts and k_siti walk one of them -,
so that the working set (2 x 199 MB at 8 bits) exceeds the 256 MiB Infinity Cache.  Kernel times are vqa_profile_read's (HIP
events): 4 warm-up calls, then the median of 24 calls.  A call is two launches of a 4:2:0 frame list (the luma and the two chroma
planes), timed together.  The byte model is one read of every sample of the stream, against the 8.0 TB/s HBM roof and the
6.29 TB/s a copy reaches; its floor is what DESIGN.md 4n states for the same clip.  Prints one JSON document."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rtvqa_amd
from rtvqa_amd import synth
from rtvqa_amd.engine import yuv_planes
from rtvqa_amd.frames import bgr_to_yuv420p

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the JSON document here")
args = ap.parse_args()
REPS, WARM = 24, 4
out = {}


def measure(eng, name, kernel, fn, nbytes, launches):
    times = []
    for r in range(WARM + REPS):
        fn(r)
        prof = eng.profile_read(reset=True)
        assert prof[kernel][1] == launches, prof
        if r >= WARM:
            times.append(prof[kernel][0])
    times.sort()
    med = float(np.median(times))
    out[name] = dict(median_ms=med, min_ms=times[0], max_ms=times[-1], model_bytes=nbytes, floor_ms=nbytes / 8.0e12 * 1e3,
                     tb_per_s=nbytes / (med * 1e-3) / 1e12, share_of_8p0=nbytes / (med * 1e-3) / 8.0e12,
                     share_of_6p29=nbytes / (med * 1e-3) / 6.29e12)


def base_frames(kind, depth, samples, rng, h, w):
    """four different frames [4, samples]"""
    dt = np.uint16 if depth > 8 else np.uint8
    if kind == "noise":
        return rng.integers(0, 1 << depth, (4, samples)).astype(dt)
    y = bgr_to_yuv420p(synth.s_natural(4, h, w, seed=int(rng.integers(1, 1000)))).astype(dt)
    if depth > 8:
        y = y * (1 << (depth - 8)) + rng.integers(0, 1 << (depth - 8), y.shape).astype(dt)
    return y


with rtvqa_amd.Engine(0) as eng:
    h, w, nf = 1080, 1920, 64
    for depth in (8, 10):
        planes = yuv_planes(h, w, "420", depth)
        samples = h * w * 3 // 2
        bps = 2 if depth > 8 else 1
        for kind in ("natural", "noise"):
            rng = np.random.default_rng(depth + (7 if kind == "noise" else 0))
            clips = []
            for k in range(2):
                base = base_frames(kind, depth, samples, rng, h, w)
                clips.append(eng.upload(np.concatenate([base] * (nf // 4))[rng.permutation(nf)]))
            eng.profile(True)
            tag = "%dp_%dbit_%s" % (h, depth, kind)
            measure(eng, "k_artifacts_" + tag, "k_artifacts", lambda r: eng.artifacts(clips[r % 2], planes),
                    1.0 * nf * samples * bps, 2)
            measure(eng, "k_siti_" + tag, "k_siti", lambda r: eng.siti(clips[r % 2], planes), 2.0 * nf * samples * bps, 2)
            measure(eng, "k_gmsd_" + tag, "k_gmsd", lambda r: eng.gmsd(clips[r % 2], clips[1 - r % 2], planes),
                    2.0 * nf * samples * bps, 2)
            eng.profile(False)
            del clips
print(json.dumps(out, indent=1))
if args.out:
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
