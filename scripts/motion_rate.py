#!/usr/bin/env python3
"""ms per launch of VMAF's motion feature on 64 device-resident 1080p 4:2:0 reference frames, at one depth per process, with VIF
and ADM on the same clip beside it:

    python scripts/motion_rate.py --depth 8 [--rounds 5] [--iters 10] [--batch 64]

The configurations (vif, adm, motion) alternate round by round inside one process, on the same device buffers, driven through
the C ABI of include/vqa.h.  Motion gets prev0 = the clip's last frame, so all 64 frames are measured.  Per configuration and
round: the median wall time of a call (host clock around submit + wait) and the kernel times of vqa_profile_read (HIP events; a
separate loop with the profiler on).  Prints one JSON line with every round, the spread of each configuration over the rounds
and motion's byte rate against the HBM roof (8 TB/s) from the model in DESIGN.md 4f: every sample of the reference stream is
read twice (as the current frame of its own pair and as the previous frame of the next), nothing is written.  The apron is not
in the model: a 64 x 32 tile loads 68 x 36 samples of either frame, 1.2 times the tile, and what the neighbour tiles have just
read comes from L2."""
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
HBM_PEAK = 8.0e12
FMA_PEAK = 78.6e12
APRON = (68 * 36) / (64 * 32)
FMA_PER_SAMPLE = 2 * 10 * APRON     # two images, five taps in either pass; the vertical pass also covers the apron columns


def bytes_per_sample(depth):
    return 2 * (2 if depth > 8 else 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batch", type=int, default=64)
    a = ap.parse_args()
    from adm_rate import Lib
    from hbd_rate import frames_420
    from rtvqa_amd import _native as N
    from rtvqa_amd.engine import plane_descs, yuv_planes
    h, w, B = 1080, 1920, a.batch
    planes = yuv_planes(h, w, "420", a.depth)
    descs = plane_descs(planes)
    r, d = frames_420(B, h, w, a.depth, seed=7)
    fb = r.nbytes // B
    L = Lib(N.LIB_PATH, N)
    pr, pd = L.upload(r), L.upload(d)
    prev0 = C.c_void_p(pr.value + (B - 1) * fb)
    out = (N.VqaPlaneMetrics * (B * 3))()
    vout, aout, mout = (N.VqaVifMetrics * (B * 3))(), (N.VqaAdmMetrics * (B * 3))(), (N.VqaMotionMetrics * (B * 3))()

    def call(mode):
        if mode == "motion":
            st = L.lib.vqa_motion_submit(L.ctx, pr, prev0, N.VQA_MEM_DEVICE, B, fb, descs, 3)
            assert st == 0, st
            assert L.lib.vqa_motion_wait(L.ctx, mout, B * 3) == 0
        else:
            L.call(pr, pd, B, fb, descs, 3, mode, out, vout, aout)
    configs = ("vif", "adm", "motion")
    ids = (N.K_VIF, N.K_VIF_DECIMATE, N.K_ADM, N.K_ADM_REDUCE, N.K_MOTION)
    rounds = {name: [] for name in configs}
    for name in configs:          # warm-up: scratch grown, clocks up
        for _ in range(3):
            call(name)
    for _ in range(a.rounds):
        for name in configs:
            walls = []
            for _ in range(a.iters):
                t0 = time.perf_counter()
                call(name)
                walls.append((time.perf_counter() - t0) * 1e3)
            L.lib.vqa_profile_enable(L.ctx, 1)
            L.profile(ids)
            for _ in range(a.iters):
                call(name)
            prof = L.profile(ids)
            L.lib.vqa_profile_enable(L.ctx, 0)
            rec = {"wall_ms": round(float(np.median(walls)), 3)}
            for k, v in prof.items():
                rec[k + "_ms"] = round(v[0] / a.iters, 4)
            rec["kernel_ms"] = round(sum(v[0] for v in prof.values()) / a.iters, 4)
            rec["launches"] = {k: v[1] // a.iters for k, v in prof.items()}
            rounds[name].append(rec)
    motion_first = [float(mout[i].motion) for i in range(3)]
    L.close()

    def spread(name, key):
        v = [x[key] for x in rounds[name] if key in x]
        return {"min": min(v), "median": round(float(np.median(v)), 4), "max": max(v)} if v else None
    summary = {name: {k: s for k in ("wall_ms", "kernel_ms") for s in [spread(name, k)] if s} for name in rounds}
    P = sum(pw * ph for pw, ph, *_ in planes) * B
    ms = summary["motion"]["kernel_ms"]["median"]
    launches = rounds["motion"][0]["launches"].get("k_motion_sad", 0)
    res = {"depth": a.depth, "batch": B, "geometry": "%dx%d 4:2:0" % (w, h), "rounds": a.rounds, "iters": a.iters,
           "summary": summary, "motion_launches_per_batch": launches,
           "motion_ms_per_launch": round(ms / max(launches, 1), 4),
           "motion_over_vif_kernel": round(ms / summary["vif"]["kernel_ms"]["median"], 4),
           "motion_over_adm_kernel": round(ms / summary["adm"]["kernel_ms"]["median"], 4),
           "motion_bytes_per_sample": bytes_per_sample(a.depth), "motion_samples": P, "apron_factor": round(APRON, 3),
           "motion_frac_hbm_peak": round(P * bytes_per_sample(a.depth) / (ms * 1e-3) / HBM_PEAK, 4),
           "motion_frac_fp32_peak": round(P * FMA_PER_SAMPLE / (ms * 1e-3) / FMA_PEAK, 4),
           "motion_of_frame_0": motion_first, "per_round": rounds}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
