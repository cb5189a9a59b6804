#!/usr/bin/env python3
"""k_light_accum and k_light_scan against k_itp and k_sigstats_accum on the same resident 64 x 1080p 4:2:0 clips at 10 bits, in one
process:

    python scripts/light_rate.py [--out FILE]

Three clips of 64 frames each: noise over the whole 10-bit range (every pixel its own histogram bin and table line: the worst
case for the gathers), natural content (a BGR test scene turned into limited-range BT.2020 PQ Y'CbCr: smooth areas, runs of equal
bins) and a FLAT clip (every pixel of a wave in one bin: the worst case for LDS atomics, which the kernel answers with one add per
wave).  k_itp compares each clip with the noise clip (the noise clip with the natural one).  Kernel times are
vqa_profile_read's (HIP events): 4 warm-up calls, then the median of 24 calls per kernel id.  The working set of one call (398 MB) exceeds the 256 MiB Infinity Cache.

Prints one JSON document with ms per kernel id and clip and, for k_light_accum, the bytes of the model "every sample of the three
planes read once" - frames x H x W x 1.5 x 2 bytes; the 24 table bytes a pixel gathers are NOT in the model: the 512 KB table is
meant to stay in L2 - and the rate they give against the 8 TB/s roof and the 6.29 TB/s a float4 copy measures on this part; ns
per pixel; k_light_accum over k_itp and over k_sigstats_accum; flat and natural over noise.  No counter run stands behind any
attribution."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rtvqa_amd
from rtvqa_amd import synth
from rtvqa_amd.engine import yuv_planes

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the JSON document here")
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--frames", type=int, default=64)
ap.add_argument("--reps", type=int, default=24)
args = ap.parse_args()
H, W, NF, REPS, WARM, DEPTH = args.height, args.width, args.frames, args.reps, 4, 10
HBM_ROOF_TBS, HBM_COPY_TBS = 8.0, 6.29
SAMPLES = H * W * 3 // 2
M1, M2 = 2610.0 / 16384.0, 2523.0 / 4096.0 * 128.0
C1, C2, C3 = 3424.0 / 4096.0, 2413.0 / 4096.0 * 32.0, 2392.0 / 4096.0 * 32.0


def pq_signal(nits):
    y = np.power(nits / 10000.0, M1)
    return np.power((C1 + C2 * y) / (1.0 + C3 * y), M2)


def natural(rng):
    """four frames of the BGR test scene read as linear light up to 1000 cd/m2 -> limited-range BT.2020 PQ 4:2:0 at 10 bits"""
    bgr = synth.s_natural(4, H, W, seed=7).astype(np.float64) / 255.0
    e = pq_signal(1000.0 * bgr ** 2.4)
    b, g, r = e[..., 0], e[..., 1], e[..., 2]
    y = 0.2627 * r + 0.6780 * g + 0.0593 * b
    cb, cr = (b - y) / 1.8814, (r - y) / 1.4746
    out = np.zeros((4, SAMPLES), np.uint16)
    out[:, :H * W] = np.rint(876.0 * y + 64.0).reshape(4, -1)
    ch, cw = (H + 1) // 2, (W + 1) // 2
    out[:, H * W:H * W + ch * cw] = np.rint(896.0 * cb[:, ::2, ::2] + 512.0).reshape(4, -1)
    out[:, H * W + ch * cw:] = np.rint(896.0 * cr[:, ::2, ::2] + 512.0).reshape(4, -1)
    return out


def clips(rng):
    noise = rng.integers(0, 1 << DEPTH, (4, SAMPLES)).astype(np.uint16)
    flat = np.zeros((4, SAMPLES), np.uint16)
    flat[:, :H * W] = 500
    flat[:, H * W:] = 512
    return {"noise": noise, "natural": natural(rng), "flat": flat}


def timed(eng, ids, fn):
    times = {k: [] for k in ids}
    for r in range(WARM + REPS):
        fn(r)
        prof = eng.profile_read(reset=True)
        if r >= WARM:
            for k in ids:
                times[k].append(prof[k][0])
    return {k: dict(median_ms=float(np.median(v)), min_ms=min(v), max_ms=max(v)) for k, v in times.items()}


out = {"geometry": [H, W], "frames": NF, "depth": DEPTH, "hbm_roof_tb_s": HBM_ROOF_TBS, "hbm_copy_tb_s": HBM_COPY_TBS}
with rtvqa_amd.Engine(0) as eng:
    planes = yuv_planes(H, W, "420", DEPTH)
    rng = np.random.default_rng(DEPTH)
    model_bytes = 2.0 * NF * SAMPLES
    table = eng.light_table("pq")
    dev = {k: eng.upload(np.concatenate([v] * (NF // 4))[rng.permutation(NF)]) for k, v in clips(rng).items()}
    eng.profile(True)
    eng.profile_read(reset=True)
    for name, d in dev.items():
        got = {"model_bytes": model_bytes}
        got.update(timed(eng, ("k_light_accum", "k_light_scan"), lambda r: eng.light(d, planes, table=table)))
        other = dev["natural" if name == "noise" else "noise"]
        got.update(timed(eng, ("k_itp",), lambda r: eng.itp(d, other, planes)))
        got.update(timed(eng, ("k_sigstats_accum",), lambda r: eng.sigstats(d, planes)))
        t = got["k_light_accum"]
        tbs = model_bytes / (t["median_ms"] * 1e-3) / 1e12
        t.update(model_tb_s=tbs, share_of_roof=tbs / HBM_ROOF_TBS, share_of_copy_rate=tbs / HBM_COPY_TBS,
                 ns_per_pixel=t["median_ms"] * 1e6 / (NF * H * W), over_k_itp=t["median_ms"] / got["k_itp"]["median_ms"],
                 over_k_sigstats_accum=t["median_ms"] / got["k_sigstats_accum"]["median_ms"])
        out[name] = got
    eng.profile(False)
    for name in ("natural", "flat"):
        out["%s_over_noise" % name] = out[name]["k_light_accum"]["median_ms"] / out["noise"]["k_light_accum"]["median_ms"]
    out["bound"] = "not attributed"   # no counter run was made
print(json.dumps(out, indent=1))
if args.out:
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
