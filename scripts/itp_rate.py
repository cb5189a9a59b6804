#!/usr/bin/env python3
"""k_itp against k_ciede and k_psnr_hvs on the same resident 64 x 1080p 4:2:0 clips, in one process:

    python scripts/itp_rate.py [--out FILE]

10 bits under PQ and under HLG, and 8 bits under PQ.  Per format two noise clips alternate - every kernel compares the one with
the other.  Unrelated noise is the worst case for k_itp, as for k_ciede: no pixel pair is equal, so none takes the exact-zero
shortcut.  Kernel times are vqa_profile_read's (HIP events): 4 warm-up calls, then the median of 24 calls.  Prints one JSON
document with ms, ns per pixel pair, the bytes of the one-read-per-sample model and their rate against the 8.0 TB/s HBM roof,
and - k_itp is bound by arithmetic, not bytes - A MODEL, not a measurement, of the vector ALU's share:
VALU_PER_PAIR vector instructions per pixel pair, F64_PER_PAIR of them double-precision (v_fma_f64, v_mul_f64, v_add_f64 and
the like), counted in the compiled loop body of the 10-bit 4:2:0 kernel along the path a PQ pixel pair takes (both colours, three
channels each, through the four pow sites); 1024 SIMDs at 2.4 GHz issue a wave64 fp64 instruction in 4 cycles (16 lanes, full
rate: 78.6 TFLOP/s of FMA) and any other vector instruction in 2 (a modelling simplification: transcendentals are slower, and
there are few).  No counter run stands behind the share."""
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
# the instructions one pixel pair executes, from the basic blocks of k_itp<uint16_t, YUV2020, *, true> as compiled: the pixel
# loop's head, twice (the image start, three rounds of the EOTF loop, three of the inverse loop), the difference.  HLG takes the
# exp branch of every channel here (the upper bound)
VALU_PER_PAIR = {"pq": 4830, "hlg": 3370}
F64_PER_PAIR = {"pq": 4010, "hlg": 2750}
SIMDS, CLOCK, CYC_F64, CYC_VALU = 1024, 2.4e9, 4, 2
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
        calls = [("k_itp", "pq", lambda r: eng.itp(clips[r % 2], clips[1 - r % 2], planes, transfer="pq"))]
        if depth == 10:
            calls.append(("k_itp", "hlg", lambda r: eng.itp(clips[r % 2], clips[1 - r % 2], planes, transfer="hlg")))
        calls += [("k_ciede", None, lambda r: eng.ciede(clips[r % 2], clips[1 - r % 2], planes)),
                  ("k_psnr_hvs", None, lambda r: eng.psnr_hvs(clips[r % 2], clips[1 - r % 2], planes))]
        for name, tf, fn in calls:
            times = []
            for r in range(WARM + REPS):
                fn(r)
                ms, cnt = eng.profile_read(reset=True)[name]
                assert cnt == (2 if name == "k_psnr_hvs" else 1)
                if r >= WARM:
                    times.append(ms)
            times.sort()
            med = float(np.median(times))
            nbytes = 2.0 * NF * samples * np.dtype(dt).itemsize      # either image once
            rec = dict(median_ms=med, min_ms=times[0], max_ms=times[-1], model_bytes=nbytes,
                       tb_per_s=nbytes / (med * 1e-3) / 1e12, share_of_8p0=nbytes / (med * 1e-3) / 8.0e12)
            if name == "k_itp":
                waves = NF * H * W / 64.0
                f64, valu = F64_PER_PAIR[tf], VALU_PER_PAIR[tf]
                cyc = waves * (f64 * CYC_F64 + (valu - f64) * CYC_VALU)
                rec.update(model_valu_ms=cyc / (SIMDS * CLOCK) * 1e3, model_share_of_valu_issue=cyc / (SIMDS * CLOCK) / (med * 1e-3),
                           ns_per_pixel_pair=med * 1e6 / (NF * H * W))
            out["%s%s_%dbit" % (name, "_" + tf if tf else "", depth)] = rec
        eng.profile(False)
        del clips
print(json.dumps(out, indent=1))
if args.out:
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
