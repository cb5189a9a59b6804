#!/usr/bin/env python3
"""The conform kernels against a plain device-to-device copy of the same bytes and against k_scale, on resident 64 x 1080p 4:2:0
clips at 8 and 10 bits, in one process:

    python scripts/conform_rate.py [--out FILE]

Cases, each ONE stream of 64 frames into a resident destination: the identity copy; the crop of the shift (1, 3) - the window
1078 x 1916 at luma corner (1, 3), chroma corner (0, 1), so the luma rows start at an odd byte (8 bits) and the realign path
runs; that crop with a table; that crop with a full matrix (the patch kernel); the identity with a reversed frame index.

The conform kernels have NO profiling id (enum vqa_kernel_id is closed), so every figure is the WALL CLOCK around vqa_sync,
submit, wait on resident frames: 4 warm-up calls, then the median of 24.  IT INCLUDES THE LAUNCHES (two kernels at most, and the
copy of the index and the tables to the device) and the host's checks of the index and the tables.  Beside them, timed the same
way in the same session: torch's device-to-device copy of the identity case's bytes, and Engine.scale 720p -> 1080p bicubic (its
kernel time by id as well).

Prints one JSON document: ms per case, the bytes of the model "window read once, destination written once" - 2 x frames x window
samples x bytes per sample - and the rate they give against the 8 TB/s roof and the 6.29 TB/s a float4 copy measures on this
part.  No counter run stands behind any attribution."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rtvqa_amd
from rtvqa_amd.engine import yuv_planes

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the JSON document here")
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--frames", type=int, default=64)
ap.add_argument("--reps", type=int, default=24)
args = ap.parse_args()
H, W, NF, REPS, WARM = args.height, args.width, args.frames, args.reps, 4
HBM_ROOF_TBS, HBM_COPY_TBS = 8.0, 6.29


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
    t.update(model_bytes=model_bytes, model_tb_s=tbs, share_of_roof=tbs / HBM_ROOF_TBS, share_of_copy_rate=tbs / HBM_COPY_TBS)
    return t


def samples(planes):
    return sum(int(p[0]) * int(p[1]) for p in planes)


out = {"geometry": [H, W], "frames": NF, "hbm_roof_tb_s": HBM_ROOF_TBS, "hbm_copy_tb_s": HBM_COPY_TBS,
       "timing": "wall clock around sync, submit, wait: launches, the copy of index and tables and the host's checks included"}
with rtvqa_amd.Engine(0) as eng:
    import torch
    for depth in (8, 10):
        bps = 2 if depth > 8 else 1
        dt = np.uint16 if depth > 8 else np.uint8
        planes = yuv_planes(H, W, "420", depth)
        crop = yuv_planes(H - 2, W - 4, "420", depth)
        corner = [(1, 3), (0, 1), (0, 1)]
        rng = np.random.default_rng(depth)
        src = eng.upload(rng.integers(0, 1 << depth, (NF, samples(planes))).astype(dt))
        lut = rng.integers(0, 1 << depth, (3, 1 << depth)).astype(dt)
        matrix = np.array([[60000, 3000, -2000, 1 << 20], [-1500, 64000, 900, 1 << 18], [700, -2500, 66000, -(1 << 19)]], np.int64)
        whole = eng.conform(src, planes, planes)          # the destinations, allocated once
        part = eng.conform(src, planes, crop, corner)
        cases = {
            "identity": (planes, dict(out=whole)),
            "crop_1_3": (crop, dict(origin=corner, out=part)),
            "crop_table": (crop, dict(origin=corner, lut=lut, out=part)),
            "crop_matrix": (crop, dict(origin=corner, matrix=matrix, out=part)),
            "reversed_index": (planes, dict(index=np.arange(NF)[::-1].copy(), out=whole)),
        }
        got = {}
        for name, (out_planes, kw) in cases.items():
            t = wall(eng.sync, lambda: eng.conform(src, planes, out_planes, **kw))
            got[name] = rated(t, 2.0 * NF * samples(out_planes) * bps)
        # a plain device-to-device copy of the identity case's bytes, in the same session
        a = torch.randint(0, 255, (NF * samples(planes) * bps,), dtype=torch.uint8, device="cuda:0")
        b = torch.empty_like(a)

        def d2d():
            b.copy_(a)
            torch.cuda.synchronize()
        got["d2d_copy"] = rated(wall(torch.cuda.synchronize, d2d), 2.0 * a.numel())
        del a, b
        # the resampler, 720p -> 1080p bicubic: wall clock like the others, and its kernel time by id
        rung = yuv_planes(720, 1280, "420", depth)
        small = eng.upload(rng.integers(0, 1 << depth, (NF, samples(rung))).astype(dt))
        t = wall(eng.sync, lambda: eng.scale(small, rung, planes, "bicubic", out=whole))
        got["k_scale_720p_to_1080p"] = rated(t, 1.0 * NF * (samples(rung) + samples(planes)) * bps)
        eng.profile(True)
        eng.profile_read(reset=True)
        ks = []
        for r in range(WARM + REPS):
            eng.scale(small, rung, planes, "bicubic", out=whole)
            ms = eng.profile_read(reset=True)["k_scale"][0]
            if r >= WARM:
                ks.append(ms)
        eng.profile(False)
        got["k_scale_720p_to_1080p"]["kernel_ms_by_id"] = float(np.median(ks))
        for name in cases:
            got[name]["over_d2d_copy"] = got[name]["median_ms"] / (got["d2d_copy"]["median_ms"] * got[name]["model_bytes"]
                                                                   / got["d2d_copy"]["model_bytes"])
        for f in (src, small, whole, part):
            f._owner.free()
        out["depth_%d" % depth] = got
    out["bound"] = "not attributed"   # no counter run was made
print(json.dumps(out, indent=1))
if args.out:
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
