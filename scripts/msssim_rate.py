#!/usr/bin/env python3
"""ms per batch of 64 device-resident 1080p 4:2:0 frame pairs through vqa_quality_submit in three configurations, at one depth
per process:

    python scripts/msssim_rate.py --depth 8 [--parent-lib PATH] [--rounds 5] [--iters 10] [--batch 64]

  1. gauss mode on the PARENT commit's library (--parent-lib: a libvqa_hip.so built from the parent; skipped without it)
  2. gauss mode on this tree's library - within run-to-run noise of 1.: the single-scale kernel instances were not disturbed
  3. msssim mode on this tree's library

The configurations alternate round by round inside one process, on the same device buffers (both libraries are driven through
the C ABI of include/vqa.h, one ctx each).  Per configuration and round: the median wall time of a call (host clock around
submit + wait) and the kernel times of vqa_profile_read (HIP events; a separate loop with the profiler on): the pyramid
launch and the Gaussian launches - five per plane group in msssim mode, accounted together under k_ssim_gauss, so the cost
of levels 1..4 shows as the difference to gauss mode's single launch.  Prints one JSON line with every round, the spread
of each configuration over the rounds, the msssim / gauss ratio and the pyramid kernel's algorithmic bytes per second
(2 P b read + 2 x 0.332 P x 4 written per plane pair) against the 8 TB/s spec peak."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "scripts"))
HBM_PEAK_GBS = 8000.0


class Lib:
    """one build of the ABI with a ctx of its own"""

    def __init__(self, path, N):
        self.N = N
        self.lib = C.CDLL(path)
        for name, (res, args) in N.SIGNATURES.items():
            if hasattr(self.lib, name):
                fn = getattr(self.lib, name)
                fn.restype, fn.argtypes = res, args
        self.ctx = C.c_void_p()
        assert self.lib.vqa_create(0, C.byref(self.ctx)) == 0

    def upload(self, arr):
        p = C.c_void_p()
        assert self.lib.vqa_alloc_device(self.ctx, arr.nbytes, C.byref(p)) == 0
        assert self.lib.vqa_copy_h2d(self.ctx, p, arr.ctypes.data, arr.nbytes) == 0
        assert self.lib.vqa_sync(self.ctx) == 0
        return p

    def call(self, pr, pd, n, fb, descs, npl, mode, out):
        st = self.lib.vqa_quality_submit(self.ctx, pr, pd, self.N.VQA_MEM_DEVICE, n, fb, fb, descs, npl, mode)
        assert st == 0, st
        assert self.lib.vqa_quality_wait(self.ctx, out, n * npl) == 0

    def profile(self, ids):
        out = {}
        for k in ids:
            ms, cnt = C.c_double(0), C.c_int64(0)
            if self.lib.vqa_profile_read(self.ctx, k, C.byref(ms), C.byref(cnt), 1) == 0 and cnt.value:
                out[self.lib.vqa_kernel_name(k).decode()] = (ms.value, cnt.value)
        return out

    def close(self):
        self.lib.vqa_destroy(self.ctx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batch", type=int, default=64)
    a = ap.parse_args()
    from hbd_rate import frames_420
    from rtvqa_amd import _native as N
    from rtvqa_amd.engine import plane_descs, yuv_planes
    h, w, B = 1080, 1920, a.batch
    planes = yuv_planes(h, w, "420", a.depth)
    descs = plane_descs(planes)
    r, d = frames_420(B, h, w, a.depth, seed=7)
    fb = r.nbytes // B
    this = Lib(N.LIB_PATH, N)
    configs = [("gauss", this, N.SSIM_GAUSS), ("msssim", this, N.SSIM_MS)]
    libs = [this]
    if a.parent_lib:
        parent = Lib(a.parent_lib, N)
        libs.append(parent)
        configs.insert(0, ("gauss_parent", parent, N.SSIM_GAUSS))
    bufs = {id(L): (L.upload(r), L.upload(d)) for L in libs}
    out = (N.VqaPlaneMetrics * (B * 3))()
    ids = (N.K_SSIM_GAUSS, N.K_MS_PYRAMID)
    rounds = {name: [] for name, _L, _m in configs}
    for name, L, mode in configs:          # warm-up: scratch grown, clocks up
        for _ in range(3):
            L.call(*bufs[id(L)], B, fb, descs, 3, mode, out)
    for _ in range(a.rounds):
        for name, L, mode in configs:
            pr, pd = bufs[id(L)]
            walls = []
            for _ in range(a.iters):
                t0 = time.perf_counter()
                L.call(pr, pd, B, fb, descs, 3, mode, out)
                walls.append((time.perf_counter() - t0) * 1e3)
            L.lib.vqa_profile_enable(L.ctx, 1)
            L.profile(ids)
            for _ in range(a.iters):
                L.call(pr, pd, B, fb, descs, 3, mode, out)
            prof = L.profile(ids)
            L.lib.vqa_profile_enable(L.ctx, 0)
            rounds[name].append({"wall_ms": round(float(np.median(walls)), 3),
                                 "ssim_ms": round(prof.get("k_ssim_gauss", (0, 0))[0] / a.iters, 3),
                                 "pyramid_ms": round(prof.get("k_ms_pyramid", (0, 0))[0] / a.iters, 4),
                                 "launches": {k: v[1] // a.iters for k, v in prof.items()}})
    for L in libs:
        L.close()

    def spread(name, key):
        v = [x[key] for x in rounds[name]]
        return {"min": min(v), "median": round(float(np.median(v)), 4), "max": max(v)}
    summary = {name: {k: spread(name, k) for k in ("wall_ms", "ssim_ms", "pyramid_ms")} for name in rounds}
    P = sum(pw * ph for pw, ph, *_ in planes) * B
    bps = 2 if a.depth > 8 else 1
    pyr_bytes = 2 * P * bps + 2 * 0.332 * P * 4
    pyr_ms = summary["msssim"]["pyramid_ms"]["median"]
    res = {"depth": a.depth, "batch": B, "geometry": "%dx%d 4:2:0" % (w, h), "rounds": a.rounds, "iters": a.iters,
           "summary": summary,
           "msssim_over_gauss_kernel": round((summary["msssim"]["ssim_ms"]["median"] + pyr_ms) / summary["gauss"]["ssim_ms"]["median"], 4),
           "msssim_over_gauss_wall": round(summary["msssim"]["wall_ms"]["median"] / summary["gauss"]["wall_ms"]["median"], 4),
           "pyramid_alg_bytes": int(pyr_bytes), "pyramid_GBps": round(pyr_bytes / pyr_ms / 1e6, 1) if pyr_ms else None,
           "pyramid_frac_hbm": round(pyr_bytes / pyr_ms / 1e6 / HBM_PEAK_GBS, 4) if pyr_ms else None,
           "per_round": rounds}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
