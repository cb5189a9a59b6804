"""The content of the slice-seam tests (tests/test_gpu_slices.py, tests/test_slices_host.py): a pool of 7 frame pairs built per
plane at the plane's own size from hostile_cases, repeated along the batch, and the index maps that say which records of such a
batch must be equal.  The C ABI cuts a plane batch into slices of 32768 frames (the lab build: VQA_QSLICE frames); 32768 % 7 = 1
and 3 % 7 = 3, so a seam never coincides with the pool's period and a record written to the wrong slot, or a seam frame
measured against the wrong predecessor, lands on a record of other content.  Integer-only and seeded; one module, so that the
host and the GPU tests see the same bytes."""
import numpy as np

import hostile_cases as K

NATURAL_SEEDS = (2, 3, 4, 13, 26)
# checker_inv: negative totals through the unsigned atomics; full_vs_zero: the accumulators' ends
POOL = tuple("natural%d" % s for s in NATURAL_SEEDS) + ("checker_inv", K.ENDS)
PERIOD = len(POOL)
assert PERIOD == 7 and 32768 % PERIOD == 1

METRICS = ("gauss", "ffmpeg", "ms", "vif", "adm", "motion", "siti", "psnr_hvs", "ciede", "gmsd", "cambi")
# Which metrics have a floating-point reference with a float32 run of its own (tests/test_slices_host.py asks it to stay within
# half the GPU bar on every entry compared with the reference).  The others are compared on every entry: vf_ssim against the C
# oracle's integer sums, the motion feature at a worst-case bound that holds for any in-range samples, SI/TI, GMSD's and CAMBI's
# words as integers.
FLOAT32_CHECKED = ("gauss", "ms", "vif", "adm", "psnr_hvs", "ciede")
# (entry, depth) left out of a metric's comparison with the reference, by name: what tests/test_slices_host.py finds unfair
# (its printout has the deviations; DESIGN.md section 3, "slice seam").  Every entry still takes part in every byte comparison.
EXCLUDED = {
    # all L against all 0 under the Gaussian window: SSIM = C1 / (L^2 + C1) ~ 1e-4, and the bar is relative to it
    "gauss": ((K.ENDS, 8), (K.ENDS, 10)),
    "ms": (), "vif": (), "adm": (), "psnr_hvs": (), "ciede": (),
}
MAX_EXCLUDED = 2               # of the seven entries, per metric and depth


# the layouts (chroma, h, w, depth) of tests/test_gpu_slices.py.  SMALL: through the lab library at VQA_QSLICE=3 - two geometry
# groups per slice, ceil-half chroma of an odd luma height (34 x 50), wider than one 64-sample tile; BIG: the shipped library at
# the shipped constant, n = 32771
SMALL = (("420", 67, 99, 8), ("420", 67, 99, 10))
SMALL_BGR = ("bgr", 67, 99, 8)                                # CIEDE2000's packed model
SMALL_MS = (("mono", 170, 161, 10), ("420", 322, 324, 8))     # MS-SSIM needs 161 x 161 on every plane
BIG = (("420", 32, 32, 8), ("mono", 16, 16, 10))
BIG_CIEDE = ("444", 16, 16, 10)                               # CIEDE2000 takes three planes
BIG_N = 32771
SMALL_NS = (3, 4, 8)           # at VQA_QSLICE=3: exactly one slice, one frame over, 3 + 3 + 2


def layouts_of(metric):
    """every layout on which section 3 compares `metric` with its reference"""
    if metric == "ms":
        return SMALL_MS
    if metric == "ciede":
        return SMALL + (SMALL_BGR, BIG[0], BIG_CIEDE)
    if metric == "cambi":
        return SMALL + (BIG[1],)
    return SMALL + BIG


def entry_pair(name, h, w, depth, k=0):
    """-> (ref, dist) int64 [h, w] of pool entry `name` for plane k of a layout"""
    if name.startswith("natural"):
        return K.natural_pair(h, w, depth, 10 * int(name[7:]) + k)
    return K.pair(name, h, w, depth, k)


def bgr_planes16(h, w, depth):
    """packed B, G, R as three planes (engine.bgr_planes, with the depth's sample size)"""
    bps = 2 if depth > 8 else 1
    return [(w, h, c * bps, 3 * w * bps, 3 * bps) + ((depth,) if depth > 8 else ()) for c in range(3)]


def layout_planes(chroma, h, w, depth):
    from rtvqa_amd.engine import yuv_planes
    return bgr_planes16(h, w, depth) if chroma == "bgr" else yuv_planes(h, w, chroma, depth)


def pool(chroma, h, w, depth):
    """the 7 frame pairs of a layout ("mono" | "420" | "444" | "bgr"): -> (ref, dist [7, samples] uint8 / uint16, planes)"""
    planes = layout_planes(chroma, h, w, depth)
    dt = np.uint16 if depth > 8 else np.uint8
    isz = np.dtype(dt).itemsize
    size = max(p[2] + (p[1] - 1) * p[3] + (p[0] - 1) * p[4] + isz for p in planes) // isz
    out = [np.zeros((PERIOD, size), dt), np.zeros((PERIOD, size), dt)]
    for e, name in enumerate(POOL):
        for k, p in enumerate(planes):
            pw, ph, off, rs, step = p[:5]
            pair = entry_pair(name, ph, pw, depth, k)
            for o, v in zip(out, pair):
                view = np.lib.stride_tricks.as_strided(o[e, off // isz:], shape=(ph, pw), strides=(rs, step))
                view[...] = v
    return out[0], out[1], planes


def batch(pool_frames, n):
    """frame i of the batch is pool entry i % 7: -> [n, samples], contiguous"""
    return np.ascontiguousarray(pool_frames[np.arange(n) % PERIOD])


def pair_source(i):
    """pair metrics and CAMBI: record i equals record pair_source(i)"""
    return i % PERIOD


def temporal_source(i):
    """the motion feature and SI/TI (frame i against frame i - 1): record i equals record temporal_source(i); records 0 .. 7 stand
    for themselves (record 0 has prev0 or no predecessor, record 7 has pool entry 6 before it), record i >= 8 equals record i - 7"""
    return i if i <= PERIOD else (i - 1) % PERIOD + 1


def pair_map(n):
    return np.arange(n) % PERIOD


def temporal_map(n):
    i = np.arange(n)
    return np.where(i <= PERIOD, i, (i - 1) % PERIOD + 1)


def ref_entries(metric, depth):
    """the pool indices whose records are compared with the metric's reference"""
    out = {e for e, d in EXCLUDED.get(metric, ()) if d == depth}
    return [k for k, name in enumerate(POOL) if name not in out]
