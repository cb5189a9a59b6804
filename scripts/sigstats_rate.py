#!/usr/bin/env python3
"""k_sigstats_accum and k_sigstats_scan against k_siti and the gray + histogram kernel on the same resident 64 x 1080p clips, at 8
and 10 bits, in one process:

    python scripts/sigstats_rate.py [--out FILE]

Three contents per depth: natural (synth.s_natural as 4:2:0), noise over the depth's range, and a FLAT clip - every sample of a
plane in ONE bin, the worst case for histogram atomics.  Per content two clips alternate, so that the working set (2 x 199 MB at
8 bits) exceeds the 256 MiB Infinity Cache.  Kernel times are vqa_profile_read's (HIP events): 4 warm-up calls, then the median
of 24 calls, per kernel id (the entries of one id within a call are added).  The gray + histogram kernel reads packed BGR and
exists at 8 bits only: it is timed on BGR clips of the same three contents.

Prints one JSON document with ms per kernel id and, for the kernels that read a frame and its predecessor (k_sigstats_accum,
k_siti), the bytes of a two-reads-per-sample model - 2 x frames x samples x bytes per sample - and the rate they give against the
6.29 TB/s a float4 copy measures on this part."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rtvqa_amd
from rtvqa_amd import _native as N
from rtvqa_amd import synth
from rtvqa_amd.engine import yuv_planes
from rtvqa_amd.frames import bgr_to_yuv420p

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the JSON document here")
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--frames", type=int, default=64)
ap.add_argument("--reps", type=int, default=24)
args = ap.parse_args()
H, W, NF, REPS, WARM = args.height, args.width, args.frames, args.reps, 4
HBM_COPY_TBS = 6.29
SAMPLES = H * W * 3 // 2
out = {"geometry": [H, W], "frames": NF, "hbm_copy_tb_s": HBM_COPY_TBS}


def tile(base, rng):
    """NF frames out of a few distinct ones, shuffled"""
    return np.concatenate([base] * (NF // len(base)))[rng.permutation(NF)]


def yuv_clip(content, depth, rng, natural):
    dt = np.uint16 if depth > 8 else np.uint8
    if content == "noise":
        return tile(rng.integers(0, 1 << depth, (4, SAMPLES)).astype(dt), rng)
    if content == "flat":
        return np.full((NF, SAMPLES), 128 << (depth - 8), dt)
    base = bgr_to_yuv420p(natural).astype(dt)
    if depth > 8:
        base = base * (1 << (depth - 8)) + rng.integers(0, 1 << (depth - 8), base.shape).astype(dt)
    return tile(base, rng)


def bgr_clip(content, rng, natural):
    if content == "noise":
        return tile(rng.integers(0, 256, (4, H, W, 3)).astype(np.uint8), rng)
    if content == "flat":
        return np.full((NF, H, W, 3), 128, np.uint8)
    return tile(natural, rng)


def timed(eng, ids, fn):
    times = {k: [] for k in ids}
    for r in range(WARM + REPS):
        fn(r)
        prof = eng.profile_read(reset=True)
        if r >= WARM:
            for k in ids:
                times[k].append(prof[k][0])
    return {k: dict(median_ms=float(np.median(v)), min_ms=min(v), max_ms=max(v)) for k, v in times.items()}


with rtvqa_amd.Engine(0) as eng:
    natural = synth.s_natural(4, H, W, seed=5)
    for depth in (8, 10):
        planes = yuv_planes(H, W, "420", depth)
        model_bytes = 2.0 * NF * SAMPLES * (2 if depth > 8 else 1)
        for content in ("natural", "noise", "flat"):
            rng = np.random.default_rng(depth)
            clips = [eng.upload(yuv_clip(content, depth, rng, natural)) for _k in range(2)]
            eng.profile(True)
            eng.profile_read(reset=True)
            got = timed(eng, ("k_sigstats_accum", "k_sigstats_scan"), lambda r: eng.sigstats(clips[r % 2], planes))
            got.update(timed(eng, ("k_siti",), lambda r: eng.siti(clips[r % 2], planes)))
            eng.profile(False)
            for k in ("k_sigstats_accum", "k_siti"):
                tbs = model_bytes / (got[k]["median_ms"] * 1e-3) / 1e12
                got[k].update(model_tb_s=tbs, share_of_copy_rate=tbs / HBM_COPY_TBS)
            got["model_bytes"] = model_bytes
            out["%s_%dbit" % (content, depth)] = got
            for c in clips:
                c._owner.free()
            del clips
    for content in ("natural", "noise", "flat"):
        rng = np.random.default_rng(3)
        clips = [eng.upload(bgr_clip(content, rng, natural)) for _k in range(2)]
        params = eng.make_params()
        eng.profile(True)
        eng.profile_read(reset=True)
        got = timed(eng, ("k_bgr2gray_hist",), lambda r: eng.complexity(clips[r % 2], None, N.M_GRAY_HIST, params))
        eng.profile(False)
        got["read_bytes"] = float(NF * H * W * 3)
        got["k_bgr2gray_hist"]["read_tb_s"] = got["read_bytes"] / (got["k_bgr2gray_hist"]["median_ms"] * 1e-3) / 1e12
        out["%s_bgr24" % content] = got
        for c in clips:
            c._owner.free()
        del clips
print(json.dumps(out, indent=1))
if args.out:
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
