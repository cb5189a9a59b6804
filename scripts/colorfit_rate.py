#!/usr/bin/env python3
"""k_colorfit against k_ciede, k_light_accum and k_align_cross on the same resident 64 x 1080p 4:2:0 clips at 8 and 10 bits, in
one process:

    python scripts/colorfit_rate.py [--out FILE]

Three pairs of clips of 64 frames per stream and depth: noise over the whole range of the depth (every position its own bin),
natural content (the BGR test scene as limited-range Y'CbCr) against a slightly damaged copy, and a FLAT pair (every position of
a wave in one bin: the worst case for LDS atomics, which the kernel answers with one entry per wave).  Each pair is measured with
tables on and off.

k_colorfit has NO profiling id (enum vqa_kernel_id is closed), so its figure is the WALL CLOCK around vqa_sync, submit, wait on
resident frames: 4 warm-up calls, then the median of 24.  IT INCLUDES THE LAUNCHES (one memset, one kernel, one copy) AND THE COPY
OF THE WORDS to the host - 192 bytes per frame, 24 n_planes bins bytes of tables.  The three kernels it is compared with are timed
through their ids (vqa_profile_read, HIP events) in the same session on the same clips; their figures are kernel time alone, so
the ratios flatter them by the launch overhead.

Prints one JSON document: ms per measurement and, for k_colorfit, the bytes of the model "every sample of both streams read
once" - 2 x frames x H x W x 1.5 x bytes per sample - and the rate they give against the 8 TB/s roof and the 6.29 TB/s a float4
copy measures on this part; flat over noise with tables on.  No counter run stands behind any attribution."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rtvqa_amd
from rtvqa_amd import frames, synth
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
SAMPLES = H * W * 3 // 2


def clips(depth, rng):
    """-> {name: (ref, dist)} of four frames each"""
    dt = np.uint16 if depth > 8 else np.uint8
    s = 1 << (depth - 8)
    nat = frames.bgr_to_yuv420p(synth.s_natural(4, H, W, seed=7)).astype(np.int64) * s
    hurt = np.clip(nat * 219 // 255 + 16 * s + rng.integers(-s, s + 1, nat.shape), 0, (1 << depth) - 1)
    flat = np.zeros((4, SAMPLES), dt)
    flat[:, :H * W] = 125 * s
    flat[:, H * W:] = 128 * s
    return {"noise": (rng.integers(0, 1 << depth, (4, SAMPLES)).astype(dt), rng.integers(0, 1 << depth, (4, SAMPLES)).astype(dt)),
            "natural": (nat.astype(dt), hurt.astype(dt)), "flat": (flat, flat.copy())}


def wall(eng, fn):
    t = []
    for r in range(WARM + REPS):
        eng.sync()
        t0 = time.perf_counter()
        fn()
        if r >= WARM:
            t.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=float(np.median(t)), min_ms=min(t), max_ms=max(t))


def by_id(eng, ids, fn):
    times = {k: [] for k in ids}
    for r in range(WARM + REPS):
        fn()
        prof = eng.profile_read(reset=True)
        if r >= WARM:
            for k in ids:
                times[k].append(prof[k][0])
    return {k: dict(median_ms=float(np.median(v)), min_ms=min(v), max_ms=max(v)) for k, v in times.items()}


out = {"geometry": [H, W], "frames": NF, "hbm_roof_tb_s": HBM_ROOF_TBS, "hbm_copy_tb_s": HBM_COPY_TBS,
       "k_colorfit": "wall clock around sync, submit, wait: launches and the copy of the words included",
       "others": "kernel time by id (HIP events)"}
with rtvqa_amd.Engine(0) as eng:
    for depth in (8, 10):
        planes = yuv_planes(H, W, "420", depth)
        rng = np.random.default_rng(depth)
        bps = 2 if depth > 8 else 1
        model_bytes = 2.0 * NF * SAMPLES * bps
        order = rng.permutation(NF)
        table = eng.light_table("pq")
        got_depth = {"model_bytes": model_bytes}
        for name, (a, b) in clips(depth, rng).items():
            ref, dist = (eng.upload(np.concatenate([v] * (NF // 4))[order]) for v in (a, b))
            got = {}
            for tables in (False, True):
                t = wall(eng, lambda: eng.colorfit(ref, dist, planes, tables=tables))
                tbs = model_bytes / (t["median_ms"] * 1e-3) / 1e12
                t.update(model_tb_s=tbs, share_of_roof=tbs / HBM_ROOF_TBS, share_of_copy_rate=tbs / HBM_COPY_TBS,
                         ns_per_position=t["median_ms"] * 1e6 / (NF * H * W))
                got["k_colorfit_tables_on" if tables else "k_colorfit_tables_off"] = t
            eng.profile(True)
            eng.profile_read(reset=True)
            got.update(by_id(eng, ("k_ciede",), lambda: eng.ciede(ref, dist, planes)))
            got.update(by_id(eng, ("k_light_accum",), lambda: eng.light(ref, planes, table=table)))
            got.update(by_id(eng, ("k_align_cross",), lambda: eng.align(ref, dist, planes, radius=1)))
            eng.profile(False)
            got_depth[name] = got
            ref._owner.free()
            dist._owner.free()
        got_depth["flat_over_noise_tables_on"] = (got_depth["flat"]["k_colorfit_tables_on"]["median_ms"] /
                                                  got_depth["noise"]["k_colorfit_tables_on"]["median_ms"])
        out["depth_%d" % depth] = got_depth
    out["bound"] = "not attributed"   # no counter run was made
print(json.dumps(out, indent=1))
if args.out:
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
