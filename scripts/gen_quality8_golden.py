#!/usr/bin/env python3
"""Writes tests/golden/quality8_records.json: the 8-bit quality records (sse, ssim as float.hex) of
test_gpu_parity.py::test_quality_bgr_and_yuv420p's inputs in both SSIM modes, as the GPU computes them.

The committed file was made at the commit before 9..16-bit samples were added; tests/test_gpu_quality_hbd.py compares
the current kernels against it bit for bit (the 8-bit path must not change).  Needs a GPU:

    python scripts/gen_quality8_golden.py [OUT.json]
"""
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def inputs():
    """(name, ref, dist, planes) exactly as test_quality_bgr_and_yuv420p builds them"""
    from rtvqa_amd import synth
    from rtvqa_amd.engine import bgr_planes, yuv420p_planes
    h, w = 72, 104
    ref = synth.s_natural(3, h, w, seed=9)
    dist = synth.distort(ref)
    yuv_r = np.random.default_rng(10).integers(0, 256, (2, h * w * 3 // 2), dtype=np.uint8)
    yuv_d = np.clip(yuv_r.astype(int) + np.random.default_rng(11).integers(-5, 6, yuv_r.shape), 0, 255).astype(np.uint8)
    return [("bgr24", ref, dist, bgr_planes(h, w)), ("yuv420p", yuv_r, yuv_d, yuv420p_planes(h, w))]


def records(engine):
    from rtvqa_amd import _native as N
    out = {}
    for name, ref, dist, planes in inputs():
        for mode_name, mode in (("gauss", N.SSIM_GAUSS), ("ffmpeg", N.SSIM_FFMPEG)):
            res = engine.quality(ref, dist, planes, mode)
            out["%s/%s" % (name, mode_name)] = {"sse": [[int(v) for v in row] for row in res["sse"]],
                                                "ssim": [[float(v).hex() for v in row] for row in res["ssim"]]}
    return out


def main():
    import rtvqa_amd
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "tests", "golden", "quality8_records.json")
    with rtvqa_amd.Engine(0) as eng:
        rec = records(eng)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    print("wrote", path)


if __name__ == "__main__":
    main()
