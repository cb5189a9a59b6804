"""The cases of the colour-registration tests (tests/test_gpu_colorfit.py): the smallest shapes at which the kernel can still go
wrong, and the clips that go with them.  A frame is [samples] of uint8 (depth 8) or uint16; a clip [n, samples].

  16 x 16      the smallest frame the kind takes (8 x 8 chroma at 4:2:0): one partial chunk
  17 x 19      odd both ways (h x w): ceil-half chroma, partial patches on both edges, never one load per row
  33 x 70      an odd height, a width that is no multiple of the 4-wide patch (but even: the halved planes take the one-load path
               only where their rows allow it)
  67 x 259     34 x 65 = 2210 patches: nine chunks of 256, so TWO workgroups per frame and two flushes into every word
  130 x 258    65 x 65 = 4225 patches: 17 chunks, three workgroups, the last of one partial chunk
"""
import numpy as np

import colorfit_reference as CR

SHAPES = ((16, 16), (17, 19), (33, 70), (67, 259), (130, 258))          # (h, w)
LAYOUTS = ("420", "422", "444", "bgr", "gray")
DEPTHS = (8, 10, 12, 16)
ODD_DEPTHS = (9, 15)            # at one shape
ODD_DEPTH_SHAPE = (17, 19)
COUNTS = (1, 3, 5)
_CACHE = {}


def planes_of(layout, h, w, depth):
    from rtvqa_amd.engine import yuv_planes
    if layout == "gray":
        return yuv_planes(h, w, "mono", depth)
    if layout != "bgr":
        return yuv_planes(h, w, layout, depth)
    bps = 2 if depth > 8 else 1
    return [(w, h, c * bps, 3 * w * bps, 3 * bps) + ((depth,) if depth > 8 else ()) for c in range(3)]


def samples_of(planes):
    bps = 2 if len(planes[0]) > 5 else 1
    return max(p[2] + (p[1] - 1) * p[3] + (p[0] - 1) * p[4] + bps for p in planes) // bps


def clip(layout, h, w, depth, n=5, seed=0):
    """n frame pairs, a different seed per frame -> (ref, dist, planes):
      0  uniform noise over the whole range of the sample type against other noise: at depths below 16 samples above the peak
         included (they are read as they are and land in the last bin)
      1  a FLAT pair at the largest sample (255, or 65535 in uint16 whatever the depth): the largest products, every position in
         one bin
      2  a ramp against noise over the legal range: runs of equal bins
      3  identical streams (noise)
      4  noise against noise again"""
    planes = planes_of(layout, h, w, depth)
    dt = np.uint16 if depth > 8 else np.uint8
    top = np.iinfo(dt).max
    peak = (1 << depth) - 1
    total = samples_of(planes)
    ref, dist = np.zeros((n, total), dt), np.zeros((n, total), dt)
    for i in range(n):
        rng = np.random.default_rng([seed, i, h, w, depth, LAYOUTS.index(layout)])
        kind = i % 5
        if kind in (0, 4):
            ref[i], dist[i] = rng.integers(0, top + 1, total), rng.integers(0, top + 1, total)
        elif kind == 1:
            ref[i], dist[i] = top, top
        elif kind == 2:
            ref[i] = ((np.arange(total) // 5) * (peak // 61 + 1)) % (peak + 1)
            dist[i] = rng.integers(0, peak + 1, total)
        else:
            ref[i] = rng.integers(0, peak + 1, total)
            dist[i] = ref[i]
    return ref, dist, planes


def matrix():
    out = [(shape, layout, depth) for shape in SHAPES for layout in LAYOUTS for depth in DEPTHS]
    return out + [(ODD_DEPTH_SHAPE, layout, depth) for layout in ("420", "gray") for depth in ODD_DEPTHS]


def matrix_ids():
    return ["%dx%d-%s-%d" % (s[1], s[0], layout, d) for s, layout, d in matrix()]


def reference(ref, dist, planes, depth, key=None):
    """the restatement's (records, {m: tables of the first m frames for m in COUNTS}), computed once per key and left unchanged"""
    if key is not None and key in _CACHE:
        return _CACHE[key]
    got = (CR.records(ref, dist, planes), {m: CR.tables(ref[:m], dist[:m], planes, depth) for m in COUNTS if m <= len(ref)})
    if key is not None:
        _CACHE[key] = got
    return got
