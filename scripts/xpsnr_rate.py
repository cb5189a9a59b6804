#!/usr/bin/env python3
"""k_xpsnr_act + k_xpsnr_sse against k_siti and k_gmsd on the same resident 64 x 1080p 4:2:0 clips, at 8 and 10 bits in one
process, and one 2160p figure for the 2 x 2 path (bv = 2):

    python scripts/xpsnr_rate.py [--out FILE]

Per depth two noise clips alternate - XPSNR and k_gmsd compare the one with the other, k_siti walks one of them -, so that the
working set (2 x 199 MB at 8 bits) exceeds the 256 MiB Infinity Cache.  Kernel times are vqa_profile_read's (HIP events): 4
warm-up calls, then the median of 24 calls.  An XPSNR call is three launches of a 4:2:0 frame list (the luma activity; the
luma's and the two chroma planes' squared error); its byte model is two luma reads (the frame and the one before it) plus one
read of every sample of both streams.  Prints one JSON document with ms, the model's bytes and the byte rate against the
8.0 TB/s HBM roof and the 6.29 TB/s a copy reaches."""
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
REPS, WARM = 24, 4
out = {}


def measure(eng, name, kernels, fn, nbytes, launches):
    times = []
    for r in range(WARM + REPS):
        fn(r)
        prof = eng.profile_read(reset=True)
        assert sum(prof[k][1] for k in kernels) == launches, prof
        if r >= WARM:
            times.append(sum(prof[k][0] for k in kernels))
    times.sort()
    med = float(np.median(times))
    out[name] = dict(median_ms=med, min_ms=times[0], max_ms=times[-1], model_bytes=nbytes, tb_per_s=nbytes / (med * 1e-3) / 1e12,
                     share_of_8p0=nbytes / (med * 1e-3) / 8.0e12, share_of_6p29=nbytes / (med * 1e-3) / 6.29e12)


with rtvqa_amd.Engine(0) as eng:
    for (h, w, nf), depths in (((1080, 1920, 64), (8, 10)), ((2160, 3840, 16), (8,))):
        for depth in depths:
            planes = yuv_planes(h, w, "420", depth)
            samples = h * w * 3 // 2
            rng = np.random.default_rng(depth)
            dt = np.uint16 if depth > 8 else np.uint8
            bps = np.dtype(dt).itemsize
            clips = []
            for k in range(2):
                base = rng.integers(0, 1 << depth, (4, samples)).astype(dt)
                clips.append(eng.upload(np.concatenate([base] * (nf // 4))[rng.permutation(nf)]))
            eng.profile(True)
            tag = "%dp_%dbit" % (h, depth)
            measure(eng, "xpsnr_" + tag, ("k_xpsnr_act", "k_xpsnr_sse"), lambda r: eng.xpsnr(clips[r % 2], clips[1 - r % 2], planes),
                    (2.0 * h * w + 2.0 * samples) * nf * bps, 3)
            if h == 1080:
                measure(eng, "k_siti_" + tag, ("k_siti",), lambda r: eng.siti(clips[r % 2], planes), 2.0 * nf * samples * bps, 2)
                measure(eng, "k_gmsd_" + tag, ("k_gmsd",), lambda r: eng.gmsd(clips[r % 2], clips[1 - r % 2], planes),
                        2.0 * nf * samples * bps, 2)
            eng.profile(False)
            del clips
print(json.dumps(out, indent=1))
if args.out:
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
