#!/usr/bin/env python3
"""The convert kernels against Engine.conform's identity copy and a plain device-to-device copy, on 64 resident 1080p frames,
in one process:

    python scripts/convert_rate.py [--out FILE]

Cases, each ONE stream of 64 frames into a resident destination: 4:2:0 8 -> 4:2:0 10 (depth only); 4:2:0 8 -> 4:2:2 10
`linear`; 4:2:2 10 -> 4:2:0 8 `linear`; 4:2:0 8 -> 4:4:4 8 `box`; the identity (4:2:0 8 -> 4:2:0 8).

The convert kernels have NO profiling id (enum vqa_kernel_id is closed), so every figure is the WALL CLOCK around vqa_sync,
submit, wait on resident frames: 4 warm-up calls, then the median of 24.  IT INCLUDES THE LAUNCHES (three kernels at most) and
the host's checks.  Beside them, timed the same way in the same session: Engine.conform's identity copy of the case's SOURCE
stream, and torch's device-to-device copy of the case's DESTINATION bytes.

Prints one JSON document: ms per case, its ratio to those two, the bytes of the model "source read once, destination written
once" and the rate they give against the 8 TB/s roof and the 6.29 TB/s a float4 copy measures on this part.  No counter run
stands behind any attribution."""
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
CASES = (
    # name, source (chroma, depth), destination (chroma, depth), (chroma filter, siting, range)
    ("420p8_to_420p10_depth_only", ("420", 8), ("420", 10), ("linear", "center", "limited")),
    ("420p8_to_422p10_linear", ("420", 8), ("422", 10), ("linear", "center", "limited")),
    ("422p10_to_420p8_linear", ("422", 10), ("420", 8), ("linear", "center", "limited")),
    ("420p8_to_444p8_box", ("420", 8), ("444", 8), ("box", "center", "limited")),
    ("identity_420p8", ("420", 8), ("420", 8), ("linear", "center", "limited")),
)


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


def frame_bytes(planes, depth):
    return sum(int(p[0]) * int(p[1]) for p in planes) * (2 if depth > 8 else 1)


out = {"geometry": [H, W], "frames": NF, "hbm_roof_tb_s": HBM_ROOF_TBS, "hbm_copy_tb_s": HBM_COPY_TBS,
       "timing": "wall clock around sync, submit, wait: launches and the host's checks included"}
with rtvqa_amd.Engine(0) as eng:
    import torch
    for name, (cs, ds), (cd, dd), opts in CASES:
        planes, out_planes = yuv_planes(H, W, cs, ds), yuv_planes(H, W, cd, dd)
        sb, db = frame_bytes(planes, ds), frame_bytes(out_planes, dd)
        rng = np.random.default_rng(ds)
        src = eng.upload(rng.integers(0, 1 << ds, (NF, sb // (2 if ds > 8 else 1))).astype(np.uint16 if ds > 8 else np.uint8))
        dst = eng.convert(src, planes, out_planes, *opts)          # the destination, allocated once
        got = rated(wall(eng.sync, lambda: eng.convert(src, planes, out_planes, *opts, out=dst)), 1.0 * NF * (sb + db))
        # Engine.conform's identity copy of the source stream, and a plain device-to-device copy of the destination's bytes
        same = eng.conform(src, planes, planes)
        conf = rated(wall(eng.sync, lambda: eng.conform(src, planes, planes, out=same)), 2.0 * NF * sb)
        a = torch.randint(0, 255, (NF * db,), dtype=torch.uint8, device="cuda:0")
        b = torch.empty_like(a)

        def d2d():
            b.copy_(a)
            torch.cuda.synchronize()
        copy = rated(wall(torch.cuda.synchronize, d2d), 2.0 * a.numel())
        del a, b
        got["conform_identity_of_source"], got["d2d_copy_of_destination"] = conf, copy
        got["over_conform_identity_ms"] = got["median_ms"] / conf["median_ms"]
        got["over_d2d_copy_ms"] = got["median_ms"] / copy["median_ms"]
        # the same two per byte of the model, so that streams of different sizes compare
        got["over_conform_identity_per_byte"] = conf["model_tb_s"] / got["model_tb_s"]
        got["over_d2d_copy_per_byte"] = copy["model_tb_s"] / got["model_tb_s"]
        for f in (src, dst, same):
            f._owner.free()
        out[name] = got
    out["bound"] = "not attributed"   # no counter run was made
print(json.dumps(out, indent=1))
if args.out:
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
