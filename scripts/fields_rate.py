#!/usr/bin/env python3
"""The fields and weave kernels beside k_siti, k_sigstats_accum and a plain device-to-device copy, on 64 resident 1080p 4:2:0
frames at 8 and 10 bits, in one process:

    python scripts/fields_rate.py [--out FILE]

The fields and weave kernels have NO profiling id (enum vqa_kernel_id is closed), so every figure is the WALL CLOCK around
vqa_sync, submit, wait on resident frames: 4 warm-up calls, then the median of 24.  IT INCLUDES THE LAUNCHES and the host's
checks.  Timed the same way in the same session on the same clips: Engine.siti and (8 bits) Engine.sigstats over the luma plane
alone, and torch's device-to-device copy of the woven stream's bytes.

Prints one JSON document: ms per case, the bytes of the model - fields: every luma sample of the frame and of its predecessor
read once (two reads per sample, like k_siti and k_motion_sad); weave: every byte read once and written once - and the rate
they give against the 8 TB/s roof.  No counter run stands behind any attribution."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rtvqa_amd
from rtvqa_amd import fields as F
from rtvqa_amd.engine import yuv_planes

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the JSON document here")
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--frames", type=int, default=64)
ap.add_argument("--reps", type=int, default=24)
args = ap.parse_args()
H, W, NF, REPS, WARM = args.height, args.width, args.frames, args.reps, 4
HBM_ROOF_TBS = 8.0


def wall(sync, fn):
    t = []
    for r in range(WARM + REPS):
        sync()
        t0 = time.perf_counter()
        fn()
        if r >= WARM:
            t.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=float(np.median(t)), min_ms=min(t), max_ms=max(t))


def rated(t, model_bytes):
    tbs = model_bytes / (t["median_ms"] * 1e-3) / 1e12
    t.update(model_bytes=model_bytes, model_tb_s=tbs, share_of_roof=tbs / HBM_ROOF_TBS)
    return t


out = {"geometry": [H, W], "frames": NF, "hbm_roof_tb_s": HBM_ROOF_TBS,
       "timing": "wall clock around sync, submit, wait: launches and the host's checks included"}
with rtvqa_amd.Engine(0) as eng:
    import torch
    for depth in (8, 10):
        bps = 2 if depth > 8 else 1
        planes = yuv_planes(H, W, "420", depth)
        luma = [planes[0]]
        fb = sum(int(p[0]) * int(p[1]) for p in planes) * bps
        rng = np.random.default_rng(depth)
        src = eng.upload(rng.integers(0, 1 << depth, (NF, fb // bps)).astype(np.uint16 if depth > 8 else np.uint8))
        prev0 = src.frame(NF - 1)
        two_reads = 2.0 * NF * H * W * bps
        got = {"fields": rated(wall(eng.sync, lambda: eng.fields(src, planes, prev0)), two_reads),
               "siti_luma": rated(wall(eng.sync, lambda: eng.siti(src, luma, prev0)), two_reads)}
        if depth == 8:
            got["sigstats_luma"] = rated(wall(eng.sync, lambda: eng.sigstats(src, luma, prev0)), two_reads)
        got["fields_over_siti_ms"] = got["fields"]["median_ms"] / got["siti_luma"]["median_ms"]
        # 2:3 pulldown of the clip: 5 output frames for 4 source frames, every output byte read once and written once
        top, bottom = F.telecine_plan(NF)
        dst = eng.weave(src, planes, top, bottom)
        moved = 2.0 * len(top) * fb
        got["weave_pulldown"] = rated(wall(eng.sync, lambda: eng.weave(src, planes, top, bottom, out=dst)), moved)
        a = torch.randint(0, 255, (len(top) * fb,), dtype=torch.uint8, device="cuda:0")
        b = torch.empty_like(a)

        def d2d():
            b.copy_(a)
            torch.cuda.synchronize()
        got["d2d_copy_of_woven_bytes"] = rated(wall(torch.cuda.synchronize, d2d), moved)
        got["weave_over_d2d_copy_ms"] = got["weave_pulldown"]["median_ms"] / got["d2d_copy_of_woven_bytes"]["median_ms"]
        del a, b
        for f in (src, dst):
            f._owner.free()
        out["yuv420p%s" % ("" if depth == 8 else "10le")] = got
    out["bound"] = "not attributed"   # no counter run was made
print(json.dumps(out, indent=1))
if args.out:
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
