#!/usr/bin/env python3
"""k_pu21_encode and k_pu21_ssim against k_itp and k_psnr_hvs on the same resident 64 x 1080p 4:2:0 clips, in one process:

    python scripts/pu21_rate.py [--out FILE]

10 bits under PQ and under HLG, and 8 bits under PQ.  Per format two noise clips alternate - every kernel compares the one with
the other.  Unrelated noise is the worst case for k_pu21_encode, as for k_itp: no pixel pair is equal, so none skips the second
chain.  Kernel times are vqa_profile_read's (HIP events): 4 warm-up calls, then the median of 24 calls, per kernel id (a 1080p
batch of 64 goes out in four sub-slices of 16 frames, so a call is four launches of either kernel; their times are added).
Prints one JSON document with ms, ns per pixel pair, and the bytes of a stated model against the 8.0 TB/s HBM roof:
  k_pu21_encode   one read of every sample of both streams, plus the write of the two maps (8 bytes a luma sample)
  k_pu21_ssim     one read of the two maps (8 bytes a luma sample); the apron's re-reads are left to the caches
The shares say how far from the byte roof the kernels run; what bounds them instead is not measured here."""
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
SUBSLICES = -(-NF // max(1, (1 << 28) // (8 * H * W)))    # 64 frames at 16 a sub-slice: 4
out = {}
with rtvqa_amd.Engine(0) as eng:
    for depth in (10, 8):
        planes = yuv_planes(H, W, "420", depth)
        samples = H * W * 3 // 2
        rng = np.random.default_rng(depth)
        dt = np.uint16 if depth > 8 else np.uint8
        clips = []
        for k in range(2):
            base = rng.integers(0, 1 << depth, (4, samples)).astype(dt)
            clips.append(eng.upload(np.concatenate([base] * (NF // 4))[rng.permutation(NF)]))
        eng.profile(True)
        calls = [(("k_pu21_encode", "k_pu21_ssim"), "pq", lambda r: eng.pu21(clips[r % 2], clips[1 - r % 2], planes, transfer="pq"))]
        if depth == 10:
            calls.append((("k_pu21_encode", "k_pu21_ssim"), "hlg",
                          lambda r: eng.pu21(clips[r % 2], clips[1 - r % 2], planes, transfer="hlg")))
        calls += [(("k_itp",), "pq", lambda r: eng.itp(clips[r % 2], clips[1 - r % 2], planes, transfer="pq")),
                  (("k_psnr_hvs",), None, lambda r: eng.psnr_hvs(clips[r % 2], clips[1 - r % 2], planes))]
        for names, tf, fn in calls:
            times = {name: [] for name in names}
            for r in range(WARM + REPS):
                fn(r)
                prof = eng.profile_read(reset=True)
                for name in names:
                    ms, cnt = prof[name]
                    assert cnt == (SUBSLICES if name.startswith("k_pu21") else 2 if name == "k_psnr_hvs" else 1), (name, cnt)
                    if r >= WARM:
                        times[name].append(ms)
            src_bytes = 2.0 * NF * samples * np.dtype(dt).itemsize      # either image once
            map_bytes = 8.0 * NF * H * W
            for name in names:
                t = sorted(times[name])
                med = float(np.median(t))
                nbytes = {"k_pu21_encode": src_bytes + map_bytes, "k_pu21_ssim": map_bytes}.get(name, src_bytes)
                out["%s%s_%dbit" % (name, "_" + tf if tf else "", depth)] = dict(
                    median_ms=med, min_ms=t[0], max_ms=t[-1], launches_per_call=SUBSLICES if name.startswith("k_pu21") else None,
                    model_bytes=nbytes, tb_per_s=nbytes / (med * 1e-3) / 1e12, share_of_8p0=nbytes / (med * 1e-3) / 8.0e12,
                    ns_per_pixel_pair=med * 1e6 / (NF * H * W))
        eng.profile(False)
        del clips
print(json.dumps(out, indent=1))
if args.out:
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
