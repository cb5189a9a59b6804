#!/usr/bin/env python3
"""k_ciede against k_psnr_hvs and k_motion_sad on the same resident 64 x 1080p clips, in one process:

    python scripts/ciede_rate.py [--out FILE]

4:2:0 at 8 and 10 bits, plus packed bgr24 at 8 bits (k_ciede only: the sample-by-sample path).  Per format two noise clips
alternate - k_ciede and k_psnr_hvs compare the one with the other, k_motion_sad walks one of them.  Unrelated noise is the worst
case for k_ciede: no pixel pair is equal, so none takes the exact-zero shortcut.  Kernel times are vqa_profile_read's (HIP
events): 4 warm-up calls, then the median of 24 calls.  Prints one JSON document with ms, the bytes of the one-read-per-sample
model and their rate against the 8.0 TB/s HBM roof, and - k_ciede is bound by arithmetic, not bytes - the share of the vector
ALU's issue rate the kernel's static instruction count explains: VALU_PER_PIXEL vector instructions per pixel
pair, TRANS_PER_PIXEL of them hardware transcendentals (v_rcp / v_sqrt / v_exp / v_log), counted in the compiled loop body of
the 4:2:0 kernel; 1024 SIMDs at 2.4 GHz issue a wave64 instruction in 2 cycles, a transcendental in 8."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rtvqa_amd
from rtvqa_amd.engine import bgr_planes, yuv_planes

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the JSON document here")
args = ap.parse_args()
H, W, NF, REPS, WARM = 1080, 1920, 64, 24, 4
VALU_PER_PIXEL, TRANS_PER_PIXEL = 2542, 74
SIMDS, CLOCK, CYC_VALU, CYC_TRANS = 1024, 2.4e9, 2, 8
out = {}
with rtvqa_amd.Engine(0) as eng:
    for fmt, depth in (("yuv420p", 8), ("yuv420p10le", 10), ("bgr24", 8)):
        yuv = fmt != "bgr24"
        planes = yuv_planes(H, W, "420", depth) if yuv else bgr_planes(H, W)
        samples = H * W * 3 // 2 if yuv else H * W * 3
        rng = np.random.default_rng(depth + len(fmt))
        dt = np.uint16 if depth > 8 else np.uint8
        clips = []
        for k in range(2):
            base = rng.integers(0, 1 << depth, (4, samples)).astype(dt)
            clips.append(eng.upload(np.concatenate([base] * (NF // 4))[rng.permutation(NF)]))
        eng.profile(True)
        calls = [("k_ciede", 1, lambda r: eng.ciede(clips[r % 2], clips[1 - r % 2], planes))]
        if yuv:
            calls += [("k_psnr_hvs", 2, lambda r: eng.psnr_hvs(clips[r % 2], clips[1 - r % 2], planes)),
                      ("k_motion_sad", 2, lambda r: eng.motion(clips[r % 2], planes))]
        for name, launches, fn in calls:
            times = []
            for r in range(WARM + REPS):
                fn(r)
                ms, cnt = eng.profile_read(reset=True)[name]
                assert cnt == launches
                if r >= WARM:
                    times.append(ms)
            times.sort()
            med = float(np.median(times))
            nbytes = 2.0 * NF * samples * np.dtype(dt).itemsize      # either image once (k_motion_sad: two reads per sample)
            rec = dict(median_ms=med, min_ms=times[0], max_ms=times[-1], model_bytes=nbytes,
                       tb_per_s=nbytes / (med * 1e-3) / 1e12, share_of_8p0=nbytes / (med * 1e-3) / 8.0e12)
            if name == "k_ciede":
                waves = NF * H * W / 64.0
                cyc = waves * ((VALU_PER_PIXEL - TRANS_PER_PIXEL) * CYC_VALU + TRANS_PER_PIXEL * CYC_TRANS)
                rec.update(valu_model_ms=cyc / (SIMDS * CLOCK) * 1e3, share_of_valu_issue=cyc / (SIMDS * CLOCK) / (med * 1e-3),
                           share_of_transcendental_issue=waves * TRANS_PER_PIXEL * CYC_TRANS / (SIMDS * CLOCK) / (med * 1e-3),
                           ns_per_pixel=med * 1e6 / (NF * H * W))
            out["%s_%s" % (name, fmt)] = rec
        eng.profile(False)
        del clips
print(json.dumps(out, indent=1))
if args.out:
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
