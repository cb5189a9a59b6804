#!/usr/bin/env python3
"""k_vca_blocks + k_vca_sum against k_siti and k_gmsd on the same resident 64 x 1080p 4:2:0 clips, at 8 and 10 bits in one
process:

    python scripts/vca_rate.py [--out FILE]

Per depth two noise clips alternate - k_gmsd compares the one with the other, VCA and k_siti walk one of them -, so that the
working set (2 x 199 MB at 8 bits) exceeds the 256 MiB Infinity Cache.  Kernel times are vqa_profile_read's (HIP events): 4
warm-up calls, then the median of 24 calls.  A VCA call is three launches of a 4:2:0 frame list (k_vca_blocks for the luma and
for the two chroma planes, k_vca_sum once), timed together.  Two models: bytes - every sample of the stream read exactly once -
against the 8.0 TB/s HBM roof and the 6.29 TB/s a copy reaches, and flops - two 32 x 32 x 32 products, 131072 flop, per block -
against the 157.3 TF fp32 matrix peak.  Prints one JSON document."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rtvqa_amd
from rtvqa_amd.engine import vca_grid, yuv_planes

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the JSON document here")
args = ap.parse_args()
REPS, WARM = 24, 4
PEAK_FP32_MATRIX = 157.3e12
out = {}


def measure(eng, name, kernels, fn, nbytes, launches, flop=None):
    times, parts = [], []
    for r in range(WARM + REPS):
        fn(r)
        prof = eng.profile_read(reset=True)
        assert sum(prof[k][1] for k in kernels) == launches, prof
        if r >= WARM:
            times.append(sum(prof[k][0] for k in kernels))
            parts.append([prof[k][0] for k in kernels])
    times.sort()
    med = float(np.median(times))
    out[name] = dict(median_ms=med, min_ms=times[0], max_ms=times[-1], model_bytes=nbytes, tb_per_s=nbytes / (med * 1e-3) / 1e12,
                     share_of_8p0=nbytes / (med * 1e-3) / 8.0e12, share_of_6p29=nbytes / (med * 1e-3) / 6.29e12,
                     per_kernel_median_ms=dict(zip(kernels, np.median(np.array(parts), axis=0).tolist())))
    if flop is not None:
        out[name].update(model_flop=flop, tflops=flop / (med * 1e-3) / 1e12, share_of_fp32_matrix_peak=flop / (med * 1e-3) / PEAK_FP32_MATRIX,
                         floor_ms_bytes=nbytes / 8.0e12 * 1e3, floor_ms_matrix=flop / PEAK_FP32_MATRIX * 1e3)


with rtvqa_amd.Engine(0) as eng:
    h, w, nf = 1080, 1920, 64
    for depth in (8, 10):
        planes = yuv_planes(h, w, "420", depth)
        samples = h * w * 3 // 2
        blocks = sum(gx * gy for gx, gy in (vca_grid(p[0], p[1]) for p in planes))
        rng = np.random.default_rng(depth)
        dt = np.uint16 if depth > 8 else np.uint8
        bps = np.dtype(dt).itemsize
        clips = []
        for k in range(2):
            base = rng.integers(0, 1 << depth, (4, samples)).astype(dt)
            clips.append(eng.upload(np.concatenate([base] * (nf // 4))[rng.permutation(nf)]))
        eng.profile(True)
        tag = "%dp_%dbit" % (h, depth)
        measure(eng, "vca_" + tag, ("k_vca_blocks", "k_vca_sum"), lambda r: eng.vca(clips[r % 2], planes),
                1.0 * nf * samples * bps, 3, flop=131072.0 * blocks * nf)
        measure(eng, "k_siti_" + tag, ("k_siti",), lambda r: eng.siti(clips[r % 2], planes), 2.0 * nf * samples * bps, 2)
        measure(eng, "k_gmsd_" + tag, ("k_gmsd",), lambda r: eng.gmsd(clips[r % 2], clips[1 - r % 2], planes),
                2.0 * nf * samples * bps, 2)
        eng.profile(False)
        del clips
print(json.dumps(out, indent=1))
if args.out:
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
