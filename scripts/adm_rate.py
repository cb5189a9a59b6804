#!/usr/bin/env python3
"""ms per batch of 64 device-resident 1080p 4:2:0 frame pairs, at one depth per process:

    python scripts/adm_rate.py --depth 8 [--parent-lib PATH] [--rounds 5] [--iters 10] [--batch 64]

  1. gauss and msssim mode and VIF on the PARENT commit's library (--parent-lib: a libvqa_hip.so built from the parent; skipped
     without it)
  2. the same three on this tree's library - within run-to-run noise of 1.: the existing kernels were not disturbed
  3. ADM on four scales (vqa_adm_submit) on this tree's library

The configurations alternate round by round inside one process, on the same device buffers (both libraries are driven through
the C ABI of include/vqa.h, one ctx each).  Per configuration and round: the median wall time of a call (host clock around
submit + wait) and the kernel times of vqa_profile_read (HIP events; a separate loop with the profiler on).  Prints one JSON
line with every round, the spread of each configuration over the rounds, ADM against gauss, msssim and VIF, and ADM's byte and
FMA rates against the HBM roof (8 TB/s) and the fp32 vector peak (157.3 TFLOP/s = 78.6 T FMA/s) from the model in DESIGN.md 4e."""
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
FMA_PEAK = 78.6e12
HBM_PEAK = 8.0e12
# per level-0 sample.  Band samples: 1/4 + 1/16 + 1/64 + 1/256 of the plane.  FMAs per band sample: two images x
# (vertical pass, L and Hh at two input columns: 2 x 2 x 4, + horizontal pass, four bands x 4 taps) = 64; the decoupling adds
# about 60 flops and three divisions per band sample.  Bytes: both planes read once (2 b) + the a bands of scales 0..2 of both
# images written once and read once as fp32 (2 x 2 x 4 x (1/4 + 1/16 + 1/64))
BAND_SAMPLES = 1 / 4 + 1 / 16 + 1 / 64 + 1 / 256
FMA_PER_SAMPLE = 64 * BAND_SAMPLES


def bytes_per_sample(depth):
    return 2 * (2 if depth > 8 else 1) + 16 * (1 / 4 + 1 / 16 + 1 / 64)


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

    def call(self, pr, pd, n, fb, descs, npl, mode, out, vout, aout=None):
        N = self.N
        if mode == "adm":
            st = self.lib.vqa_adm_submit(self.ctx, pr, pd, N.VQA_MEM_DEVICE, n, fb, fb, descs, npl)
            assert st == 0, st
            assert self.lib.vqa_adm_wait(self.ctx, aout, n * npl) == 0
        elif mode == "vif":
            st = self.lib.vqa_vif_submit(self.ctx, pr, pd, N.VQA_MEM_DEVICE, n, fb, fb, descs, npl)
            assert st == 0, st
            assert self.lib.vqa_vif_wait(self.ctx, vout, n * npl) == 0
        else:
            st = self.lib.vqa_quality_submit(self.ctx, pr, pd, N.VQA_MEM_DEVICE, n, fb, fb, descs, npl, mode)
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
    configs = [("gauss", this, N.SSIM_GAUSS), ("msssim", this, N.SSIM_MS), ("vif", this, "vif"), ("adm", this, "adm")]
    libs = [this]
    if a.parent_lib:
        parent = Lib(a.parent_lib, N)
        libs.append(parent)
        configs = [("gauss_parent", parent, N.SSIM_GAUSS), ("msssim_parent", parent, N.SSIM_MS), ("vif_parent", parent, "vif")] + configs
    bufs = {id(L): (L.upload(r), L.upload(d)) for L in libs}
    out = (N.VqaPlaneMetrics * (B * 3))()
    vout = (N.VqaVifMetrics * (B * 3))()
    aout = (N.VqaAdmMetrics * (B * 3))()
    ids = (N.K_SSIM_GAUSS, N.K_MS_PYRAMID, N.K_VIF, N.K_VIF_DECIMATE, N.K_ADM, N.K_ADM_REDUCE)
    rounds = {name: [] for name, _L, _m in configs}
    for name, L, mode in configs:          # warm-up: scratch grown, clocks up
        for _ in range(3):
            L.call(*bufs[id(L)], B, fb, descs, 3, mode, out, vout, aout)
    for _ in range(a.rounds):
        for name, L, mode in configs:
            pr, pd = bufs[id(L)]
            walls = []
            for _ in range(a.iters):
                t0 = time.perf_counter()
                L.call(pr, pd, B, fb, descs, 3, mode, out, vout, aout)
                walls.append((time.perf_counter() - t0) * 1e3)
            L.lib.vqa_profile_enable(L.ctx, 1)
            L.profile(ids)
            for _ in range(a.iters):
                L.call(pr, pd, B, fb, descs, 3, mode, out, vout, aout)
            prof = L.profile(ids)
            L.lib.vqa_profile_enable(L.ctx, 0)
            rec = {"wall_ms": round(float(np.median(walls)), 3)}
            for k, v in prof.items():
                rec[k + "_ms"] = round(v[0] / a.iters, 4)
            rec["kernel_ms"] = round(sum(v[0] for v in prof.values()) / a.iters, 4)
            rec["launches"] = {k: v[1] // a.iters for k, v in prof.items()}
            rounds[name].append(rec)
    for L in libs:
        L.close()

    def spread(name, key):
        v = [x[key] for x in rounds[name] if key in x]
        return {"min": min(v), "median": round(float(np.median(v)), 4), "max": max(v)} if v else None
    keys = ("wall_ms", "kernel_ms", "k_ssim_gauss_ms", "k_ms_pyramid_ms", "k_vif_stats_ms", "k_vif_decimate_ms", "k_adm_scale_ms",
            "k_adm_reduce_ms")
    summary = {name: {k: s for k in keys for s in [spread(name, k)] if s} for name in rounds}
    P = sum(pw * ph for pw, ph, *_ in planes) * B
    adm_ms = summary["adm"]["kernel_ms"]["median"]
    res = {"depth": a.depth, "batch": B, "geometry": "%dx%d 4:2:0" % (w, h), "rounds": a.rounds, "iters": a.iters,
           "summary": summary,
           "adm_over_gauss_kernel": round(adm_ms / summary["gauss"]["kernel_ms"]["median"], 3),
           "adm_over_msssim_kernel": round(adm_ms / summary["msssim"]["kernel_ms"]["median"], 3),
           "adm_over_vif_kernel": round(adm_ms / summary["vif"]["kernel_ms"]["median"], 3),
           "adm_fma_per_sample": round(FMA_PER_SAMPLE, 2), "adm_bytes_per_sample": round(bytes_per_sample(a.depth), 2), "adm_samples": P,
           "adm_frac_fp32_peak": round(P * FMA_PER_SAMPLE / (adm_ms * 1e-3) / FMA_PEAK, 4),
           "adm_frac_hbm_peak": round(P * bytes_per_sample(a.depth) / (adm_ms * 1e-3) / HBM_PEAK, 4),
           "per_round": rounds}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
