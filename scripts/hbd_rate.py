#!/usr/bin/env python3
"""ms per batch of 64 device-resident 1080p 4:2:0 frame pairs through vqa_quality_submit, 8-bit against 10-bit samples
(one depth and one SSIM mode per process; the job runs each under its own time limit):

    python scripts/hbd_rate.py --depth 10 --mode ffmpeg [--iters 20] [--batch 64]

Prints one JSON line: the wall time of a call (host clock around submit + wait, i.e. ending in a device synchronise), the
kernel time of the quality launches (HIP events around them, vqa_profile_*; a separate loop with the profiler on), the
algorithmic HBM bytes (ref + dist read once: 2 x 1.5 x W x H x bytes per sample per pair) and their share of the 8 TB/s
spec peak at the kernel time.  Inputs are seeded (synth.s_natural, widened to the depth); the output records' digest
lets two runs be compared."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
HBM_PEAK_GBS = 8000.0   # MI355X HBM3E spec peak


def frames_420(n, h, w, depth, seed):
    """n frame pairs [n, samples] of planar 4:2:0 at `depth` bits: the 8-bit conversion of synthetic BGR frames, shifted up
    and filled with seeded low bits above 8 bits"""
    from rtvqa_amd import synth
    from rtvqa_amd.frames import bgr_to_yuv420p
    ref = synth.s_natural(n, h, w, seed=seed)
    r8, d8 = bgr_to_yuv420p(ref), bgr_to_yuv420p(synth.distort(ref))
    if depth == 8:
        return r8, d8
    rng = np.random.default_rng(seed)
    lo = 1 << (depth - 8)
    r = (r8.astype(np.uint16) << (depth - 8)) + rng.integers(0, lo, r8.shape, dtype=np.uint16)
    d = (d8.astype(np.uint16) << (depth - 8)) + rng.integers(0, lo, d8.shape, dtype=np.uint16)
    return r, d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depth", type=int, default=10)
    ap.add_argument("--mode", choices=["gauss", "ffmpeg"], default="ffmpeg")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    a = ap.parse_args()
    import rtvqa_amd
    from rtvqa_amd import _native as N
    from rtvqa_amd.engine import yuv_planes
    h, w, B = 1080, 1920, a.batch
    mode = N.SSIM_GAUSS if a.mode == "gauss" else N.SSIM_FFMPEG
    planes = yuv_planes(h, w, "420", a.depth)
    r, d = frames_420(B, h, w, a.depth, seed=7)
    with rtvqa_amd.Engine(0) as eng:
        dr, dd = eng.upload(r), eng.upload(d)
        for _ in range(3):
            res = eng.quality(dr, dd, planes, mode)
        walls = []
        for _ in range(a.iters):
            t0 = time.perf_counter()
            eng.quality(dr, dd, planes, mode)
            walls.append((time.perf_counter() - t0) * 1e3)
        eng.profile(True)
        eng.profile_read(reset=True)
        for _ in range(a.iters):
            eng.quality(dr, dd, planes, mode)
        prof = eng.profile_read(reset=True)
        eng.profile(False)
    kname = "ssim_gauss" if a.mode == "gauss" else "ssim_ffmpeg"
    kms = sum(ms for k, (ms, _n) in prof.items() if kname in k) / a.iters
    nbytes = 2 * r.nbytes
    out = {"depth": a.depth, "mode": a.mode, "batch": B, "geometry": "%dx%d 4:2:0" % (w, h), "iters": a.iters,
           "wall_ms_median": round(float(np.median(walls)), 3), "wall_ms_min": round(float(np.min(walls)), 3),
           "kernel_ms": round(kms, 3), "alg_bytes": int(nbytes), "GBps_kernel": round(nbytes / kms / 1e6, 1),
           "frac_hbm": round(nbytes / kms / 1e6 / HBM_PEAK_GBS, 4), "profile": {k: [round(v[0], 3), v[1]] for k, v in prof.items()},
           "records_sha16": hashlib.sha256(res.tobytes()).hexdigest()[:16]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
