"""The cases of the light-level tests (tests/test_gpu_light.py, tests/test_light_host.py): the smallest shapes at which the kernel
can still go wrong, and the clips that go with them.  A frame is [samples] of uint8 (depth 8) or uint16; a clip [n, samples].

  16 x 16     one chunk of 32 patches, the smallest frame the kind takes (8 x 8 chroma at 4:2:0)
  17 x 19     odd both ways (h x w): ceil-half chroma, partial patches on both edges, never one load per row
  66 x 130    33 x 33 = 1089 patches: five chunks of 256, the last partial; several waves; a partial last patch column
"""
import numpy as np

import itp_reference as IR
import light_reference as LR

SHAPES = ((16, 16), (17, 19), (66, 130))          # (h, w)
CHROMAS = ("444", "422", "420", "bgr")
DEPTHS = (8, 10, 12, 16)
COUNTS = (1, 3)
_CACHE = {}


def planes_of(chroma, h, w, depth):
    from rtvqa_amd.engine import yuv_planes
    if chroma != "bgr":
        return yuv_planes(h, w, chroma, depth)
    bps = 2 if depth > 8 else 1
    return [(w, h, c * bps, 3 * w * bps, 3 * bps) + ((depth,) if depth > 8 else ()) for c in range(3)]


def model_of(chroma):
    return IR.BGR if chroma == "bgr" else IR.YUV2020


def samples_of(planes):
    bps = 2 if len(planes[0]) > 5 else 1
    return max(p[2] + (p[1] - 1) * p[3] + (p[0] - 1) * p[4] + bps for p in planes) // bps


def clip(chroma, h, w, depth, n=3, seed=0):
    """n frames: frame 0 noise over the whole sample range (illegal Y'CbCr combinations included: the clamp), frame 1 noise
    over the legal limited range, frame 2 a diagonal ramp (runs of equal bins), then noise again -> (frames, planes)"""
    planes = planes_of(chroma, h, w, depth)
    dt = np.uint16 if depth > 8 else np.uint8
    rng = np.random.default_rng([seed, h, w, depth, CHROMAS.index(chroma)])
    s, peak = 1 << (depth - 8), (1 << depth) - 1
    total = samples_of(planes)
    out = np.zeros((n, total), dt)
    for i in range(n):
        if i % 3 == 0:
            out[i] = rng.integers(0, peak + 1, total)
        elif i % 3 == 1:
            out[i] = rng.integers(16 * s, 236 * s, total)
        else:
            out[i] = ((np.arange(total) // 7) * (peak // 97 + 1) + 16 * s) % (peak + 1)
    return out, planes


def matrix():
    return [(shape, chroma, depth, full) for shape in SHAPES for chroma in CHROMAS for depth in DEPTHS
            for full in ((False, True) if chroma != "bgr" else (False,))]


def matrix_ids():
    return ["%dx%d-%s-%d-%s" % (s[1], s[0], c, d, "full" if f else "limited") for s, c, d, f in matrix()]


def reference(frames, planes, depth, model, full, table, m709, mp3, key=None):
    """the restatement's (record, histogram) of every frame, computed once per key and left unchanged"""
    if key is not None and key in _CACHE:
        return _CACHE[key]
    got = LR.records(frames, planes, depth, model, full, table, m709, mp3)
    if key is not None:
        _CACHE[key] = got
    return got


# the seam test: 32771 frames of 16 x 16 8-bit 4:2:0 drawn from a pool of 7
SEAM_FRAMES, SEAM_POOL = 32771, 7


def seam_pool():
    frames, planes = clip("420", 16, 16, 8, SEAM_POOL, seed=11)
    return frames, planes


def in_gamut_colours(name, n, seed):
    """n random colours inside gamut `name` as linear BT.2020 display light [n, 3]: a quarter any colour, a quarter with one
    channel at zero, a quarter pure primaries, a quarter any colour again, each scaled so that its largest component is
    1e-4 .. 1 of 1000 cd/m2 (log-uniform)"""
    rng = np.random.default_rng(seed)
    to2020 = np.linalg.inv(LR.gamut_double(name))
    rgb = rng.random((n, 3))
    kind = rng.integers(0, 4, n)
    one = np.where(kind == 1)[0]
    rgb[one, rng.integers(0, 3, len(one))] = 0.0
    pure = np.where(kind == 2)[0]
    rgb[pure] = 0.0
    rgb[pure, rng.integers(0, 3, len(pure))] = 1.0
    peak = 1000.0 * 10.0 ** rng.uniform(-4.0, 0.0, n)
    rgb = rgb / np.maximum(rgb.max(axis=1, keepdims=True), 1e-9) * peak[:, None]
    return rgb @ to2020.T
