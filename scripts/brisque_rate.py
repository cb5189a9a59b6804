#!/usr/bin/env python3
"""The BRISQUE kernels against k_siti and k_gmsd on the same resident 64 x 1080p 4:2:0 clips, at 8 and 10 bits, on natural
content and on noise, in one process:

    python scripts/brisque_rate.py [--out FILE]

Per depth and content two clips alternate - k_gmsd compares the one with the other, the BRISQUE kernels and k_siti walk one of
them -, so that the working set (2 x 199 MB at 8 bits) exceeds the 256 MiB Infinity Cache.  Kernel times are vqa_profile_read's
(HIP events): 4 warm-up calls, then the median of 24 calls.  A call covers both plane groups of a 4:2:0 frame list (the luma and
the two chroma planes), timed together: 2 launches of k_brisque_half, 4 of k_brisque_mscn and of k_brisque_seam; "brisque" is
their sum per call; one set of calls serves all four figures.  k_brisque_seam reads strips, not planes: it gets a time and no
byte model.  The byte model of the three together: every sample read twice (k_brisque_half, scale 0 of k_brisque_mscn)
and the scale-1 plane, 8 bytes for every four samples, written once and read once; against the 8.0 TB/s HBM roof and the
6.29 TB/s a copy reaches.  Prints one JSON document."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rtvqa_amd
from rtvqa_amd import synth
from rtvqa_amd.engine import yuv_planes
from rtvqa_amd.frames import bgr_to_yuv420p

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the JSON document here")
args = ap.parse_args()
REPS, WARM = 24, 4
out = {}


def measure(eng, groups, fn):
    """groups: {name: ({kernel: launches per call}, model bytes or None)}.  One set of WARM + REPS calls of fn serves every
    group: a group's time per call is the sum of its kernels' times in that call"""
    times = {name: [] for name in groups}
    for r in range(WARM + REPS):
        fn(r)
        prof = eng.profile_read(reset=True)
        for name, (kernels, _nbytes) in groups.items():
            for kernel, cnt in kernels.items():
                assert prof[kernel][1] == cnt, prof
            if r >= WARM:
                times[name].append(sum(prof[kernel][0] for kernel in kernels))
    for name, (_kernels, nbytes) in groups.items():
        t = sorted(times[name])
        med = float(np.median(t))
        out[name] = dict(median_ms=med, min_ms=t[0], max_ms=t[-1])
        if nbytes is not None:
            out[name].update(model_bytes=nbytes, floor_ms=nbytes / 8.0e12 * 1e3, tb_per_s=nbytes / (med * 1e-3) / 1e12,
                             share_of_8p0=nbytes / (med * 1e-3) / 8.0e12, share_of_6p29=nbytes / (med * 1e-3) / 6.29e12)


def base_frames(kind, depth, samples, rng, h, w):
    """four different frames [4, samples]"""
    dt = np.uint16 if depth > 8 else np.uint8
    if kind == "noise":
        return rng.integers(0, 1 << depth, (4, samples)).astype(dt)
    y = bgr_to_yuv420p(synth.s_natural(4, h, w, seed=int(rng.integers(1, 1000)))).astype(dt)
    if depth > 8:
        y = y * (1 << (depth - 8)) + rng.integers(0, 1 << (depth - 8), y.shape).astype(dt)
    return y


with rtvqa_amd.Engine(0) as eng:
    h, w, nf = 1080, 1920, 64
    for depth in (8, 10):
        planes = yuv_planes(h, w, "420", depth)
        samples = h * w * 3 // 2
        bps = 2 if depth > 8 else 1
        for kind in ("natural", "noise"):
            rng = np.random.default_rng(depth + (7 if kind == "noise" else 0))
            clips = []
            for k in range(2):
                base = base_frames(kind, depth, samples, rng, h, w)
                clips.append(eng.upload(np.concatenate([base] * (nf // 4))[rng.permutation(nf)]))
            eng.profile(True)
            tag = "%dp_%dbit_%s" % (h, depth, kind)
            px = 1.0 * nf * samples
            measure(eng, {"brisque_" + tag: ({"k_brisque_half": 2, "k_brisque_mscn": 4, "k_brisque_seam": 4}, px * (2 * bps + 4)),
                          "k_brisque_half_" + tag: ({"k_brisque_half": 2}, px * (bps + 2)),
                          "k_brisque_mscn_" + tag: ({"k_brisque_mscn": 4}, px * (bps + 2)),
                          "k_brisque_seam_" + tag: ({"k_brisque_seam": 4}, None)},
                    lambda r: eng.brisque(clips[r % 2], planes))
            measure(eng, {"k_siti_" + tag: ({"k_siti": 2}, 2 * px * bps)}, lambda r: eng.siti(clips[r % 2], planes))
            measure(eng, {"k_gmsd_" + tag: ({"k_gmsd": 2}, 2 * px * bps)},
                    lambda r: eng.gmsd(clips[r % 2], clips[1 - r % 2], planes))
            eng.profile(False)
            del clips
print(json.dumps(out, indent=1))
if args.out:
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
