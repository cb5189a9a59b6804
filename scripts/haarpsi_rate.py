#!/usr/bin/env python3
"""k_haarpsi against k_gmsd and k_siti on the same resident 64 x 1080p 4:2:0 clips, at 8 and 10 bits in one process:

    python scripts/haarpsi_rate.py [--out FILE]

Per depth two noise clips alternate - k_haarpsi and k_gmsd compare the one with the other, k_siti walks one of them -, so that
the working set (2 x 199 MB at 8 bits) exceeds the 256 MiB Infinity Cache.  Kernel times are vqa_profile_read's (HIP events): 4
warm-up calls, then the median of 24 calls, a call being the two launches of a 4:2:0 frame list (luma; the two chroma planes).
Prints one JSON document with ms, the bytes of the two-reads-per-sample model (for k_haarpsi and k_gmsd: one read of either
image) and the byte rate against the 8.0 TB/s HBM roof and the 6.29 TB/s a copy reaches."""
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
args = ap.parse_args()
H, W, NF, REPS, WARM = 1080, 1920, 64, 24, 4
out = {}
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
        calls = (("k_haarpsi", lambda r: eng.haarpsi(clips[r % 2], clips[1 - r % 2], planes)),
                 ("k_gmsd", lambda r: eng.gmsd(clips[r % 2], clips[1 - r % 2], planes)),
                 ("k_siti", lambda r: eng.siti(clips[r % 2], planes)))
        for name, fn in calls:
            times = []
            for r in range(WARM + REPS):
                fn(r)
                ms, cnt = eng.profile_read(reset=True)[name]
                assert cnt == 2
                if r >= WARM:
                    times.append(ms)
            times.sort()
            med = float(np.median(times))
            nbytes = 2.0 * NF * samples * np.dtype(dt).itemsize      # two reads per sample
            out["%s_%dbit" % (name, depth)] = dict(median_ms=med, min_ms=times[0], max_ms=times[-1], model_bytes=nbytes,
                                                   tb_per_s=nbytes / (med * 1e-3) / 1e12, share_of_8p0=nbytes / (med * 1e-3) / 8.0e12,
                                                   share_of_6p29=nbytes / (med * 1e-3) / 6.29e12)
        eng.profile(False)
        del clips
print(json.dumps(out, indent=1))
if args.out:
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
