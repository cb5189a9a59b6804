#!/usr/bin/env python3
"""k_scale against k_gmsd and k_siti on resident 64-frame 4:2:0 clips, in one process:

    python scripts/scale_rate.py [--out FILE]

1280 x 720 -> 1920 x 1080 at 8 and 10 bits, bicubic and lanczos, and 640 x 360 -> 1920 x 1080 at 8 bits, bicubic; then k_gmsd and
k_siti on the 1920 x 1080 clips the resampler wrote.  Two noise source clips alternate per case.  Kernel times are
vqa_profile_read's (HIP events, the launches of the plane groups of one call added): 4 warm-up calls, then the median of 24.
Prints one JSON document with ms per case, the bytes of the model "source read once, destination written once" and the share of
8 TB/s they give."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rtvqa_amd
from rtvqa_amd.engine import planes_span, yuv_planes

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the JSON document here")
args = ap.parse_args()
NF, REPS, WARM, ROOF = 64, 24, 4, 8e12
OH, OW = 1080, 1920
CASES = ((720, 1280, 8, "bicubic"), (720, 1280, 8, "lanczos"), (720, 1280, 10, "bicubic"), (720, 1280, 10, "lanczos"),
         (360, 640, 8, "bicubic"))
out = {}


def median_ms(eng, ids, fn):
    times = []
    for r in range(WARM + REPS):
        fn(r)
        prof = eng.profile_read(reset=True)
        if r >= WARM:
            times.append(sum(prof[k][0] for k in ids))
    t = sorted(times)
    return dict(median_ms=float(np.median(t)), min_ms=t[0], max_ms=t[-1])


with rtvqa_amd.Engine(0) as eng:
    eng.profile(True)
    for h, w, depth, filt in CASES:
        planes, out_planes = yuv_planes(h, w, "420", depth), yuv_planes(OH, OW, "420", depth)
        dt = np.uint16 if depth > 8 else np.uint8
        rng = np.random.default_rng(depth + h)
        clips = []
        for k in range(2):
            base = rng.integers(0, 1 << depth, (4, planes_span(planes) // dt().itemsize)).astype(dt)
            clips.append(eng.upload(np.concatenate([base] * (NF // 4))[rng.permutation(NF)]))
        dst = eng.scale(clips[0], planes, out_planes, filt)
        name = "%dx%d_%dbit_%s" % (w, h, depth, filt)
        res = median_ms(eng, ("k_scale",), lambda r: eng.scale(clips[r % 2], planes, out_planes, filt, out=dst))
        model = NF * (planes_span(planes) + planes_span(out_planes))
        res.update(model_bytes=model, roof_share=model / (res["median_ms"] * 1e-3) / ROOF)
        out["k_scale_" + name] = res
        if filt == "bicubic" and h == 720:
            other = eng.scale(clips[1], planes, out_planes, "lanczos")
            out["k_gmsd_%dbit" % depth] = median_ms(eng, ("k_gmsd",), lambda r: eng.gmsd(dst, other, out_planes))
            out["k_siti_%dbit" % depth] = median_ms(eng, ("k_siti",), lambda r: eng.siti(dst, out_planes))
            other._owner.free()
        dst._owner.free()
        for c in clips:
            c._owner.free()
    eng.profile(False)
print(json.dumps(out, indent=1))
if args.out:
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
