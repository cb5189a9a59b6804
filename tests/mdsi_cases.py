"""The shapes, layouts and contents of the MDSI parity matrix, shared by tests/test_mdsi_host.py (is the integer pooling admitted
on them?) and tests/test_gpu_mdsi.py (the GPU against the restatements), so that both see the same samples.  Integer-only and
seeded.

Shapes (h, w), the smallest at which the kernels can still go wrong:
  16 x 16    f = 1  the minimum
  33 x 67    f = 1  odd sizes, odd chroma
  67 x 130   f = 1  past both seams of the kernel's 64 x 32 tile
  385 x 391  f = 2  both odd: a half-weight last row and column, windows that straddle 4:2:0 chroma samples
  640 x 644  f = 3  the rounding tie (Python's round would give 2); the first window starts at row -1; 640 = 3 * 213 + 1
  897 x 900  f = 4  the even window at -1 .. +2; 900 = 4 * 225, so the last window is cut on the right"""
import functools

import numpy as np

SMALL = ((16, 16), (33, 67), (67, 130))
LARGE = ((385, 391), (640, 644), (897, 900))
FACTORS = {(16, 16): 1, (33, 67): 1, (67, 130): 1, (385, 391): 2, (640, 644): 3, (897, 900): 4}
LAYOUTS = ("bgr24", "yuv444p", "yuv422p", "yuv420p", "gray")
DEPTHS = (8, 10, 16)
CONTENTS = ("natural", "noise", "texture_flat", "identical", "ends", "flat_zero", "flat_peak")
MODEL = {"bgr24": "bgr", "yuv444p": "yuv709", "yuv422p": "yuv709", "yuv420p": "yuv709", "gray": "gray"}
BAR_LIMIT = 1e-6       # no case's derived bar (mdsi_reference.derived_bar) may exceed this


def plane_sizes(layout, h, w):
    if layout == "gray":
        return [(h, w)]
    if layout in ("bgr24", "yuv444p"):
        return [(h, w)] * 3
    ch = (h + 1) // 2 if layout == "yuv420p" else h
    return [(h, w), (ch, (w + 1) // 2), (ch, (w + 1) // 2)]


def engine_planes(layout, h, w, depth=8):
    """the engine's plane tuples of one frame of the layout"""
    bps = 2 if depth > 8 else 1
    tail = (depth,) if depth > 8 else ()
    if layout == "bgr24":
        return [(w, h, c * bps, 3 * w * bps, 3 * bps) + tail for c in range(3)]
    out, off = [], 0
    for ph, pw in plane_sizes(layout, h, w):
        out.append((pw, ph, off, pw * bps, bps) + tail)
        off += pw * ph * bps
    return out


def _texture(h, w, peak, phase):
    y, x = np.mgrid[0:h, 0:w]
    base = 40.0 + 150.0 * (0.5 + 0.5 * np.sin(x / 9.0 + phase) * np.cos(y / 7.0 - phase)) + 30.0 * ((x // 11 + y // 13 + int(phase)) % 2)
    return np.clip(np.rint(base * peak / 255.0), 0, peak).astype(np.int64)


@functools.lru_cache(maxsize=None)
def pair(name, layout, h, w, depth=8, seed=0):
    """-> (ref, dist): two tuples of int64 planes of `depth` bits.  Cached: treat the arrays as read-only."""
    rng = np.random.default_rng(100000 * LAYOUTS.index(layout) + 1000 * h + w + 7 * depth + seed)
    peak, sizes = (1 << depth) - 1, plane_sizes(layout, h, w)
    mid = 128 << (depth - 8)
    if name == "natural":        # a smooth gradient with a few edges per plane, and +-12 levels (8-bit scale) of noise on the copy
        r = [_texture(ph, pw, peak, float(k)) for k, (ph, pw) in enumerate(sizes)]
        d = [np.clip(p + np.rint(rng.integers(-12, 13, p.shape) * (peak / 255.0)).astype(np.int64), 0, peak) for p in r]
    elif name == "noise":        # unrelated uniform noise over the full range in every plane
        r = [rng.integers(0, peak + 1, s).astype(np.int64) for s in sizes]
        d = [rng.integers(0, peak + 1, s).astype(np.int64) for s in sizes]
    elif name == "texture_flat":  # a textured reference against a flat distorted image: removed edges, GCS < 0
        r = [_texture(ph, pw, peak, float(k)) for k, (ph, pw) in enumerate(sizes)]
        d = [np.full(s, mid, np.int64) for s in sizes]
    elif name == "identical":
        r = [rng.integers(0, peak + 1, s).astype(np.int64) for s in sizes]
        d = [p.copy() for p in r]
    elif name == "ends":         # flat 0 against the flat maximum
        r, d = [np.zeros(s, np.int64) for s in sizes], [np.full(s, peak, np.int64) for s in sizes]
    elif name in ("flat_zero", "flat_peak"):
        v = 0 if name == "flat_zero" else peak
        r, d = [np.full(s, v, np.int64) for s in sizes], [np.full(s, v, np.int64) for s in sizes]
    else:
        raise KeyError(name)
    for p in r + d:
        p.setflags(write=False)
    return tuple(r), tuple(d)


def dtype_of(depth):
    return np.uint16 if depth > 8 else np.uint8


def pack(frames, layout, depth=8):
    """a list of frames (each a tuple of planes) -> [n, samples] array in the layout: planar, or packed B, G, R"""
    dt = dtype_of(depth)
    if layout == "bgr24":
        return np.stack([np.stack(f, axis=-1).astype(dt).reshape(-1) for f in frames])
    return np.stack([np.concatenate([p.astype(dt).reshape(-1) for p in f]) for f in frames])


def matrix():
    """(content, layout, shape, depth): every content in every layout on the small shapes at 8 bits; natural, noise and
    texture_flat in yuv420p and bgr24 at f = 2, 3, 4; every content at 10 and 16 bits in yuv420p and bgr24 on 33 x 67"""
    out = [(c, l, s, 8) for c in CONTENTS for l in LAYOUTS for s in SMALL]
    out += [(c, l, s, 8) for c in ("natural", "noise", "texture_flat") for l in ("yuv420p", "bgr24") for s in LARGE]
    out += [(c, l, (33, 67), dp) for c in CONTENTS for l in ("yuv420p", "bgr24") for dp in DEPTHS if dp != 8]
    return out


MATRIX_CASES = 7 * 5 * 3 + 3 * 2 * 3 + 7 * 2 * 2       # 151


def case_id(case):
    c, l, s, dp = case
    return "%s-%s-%dx%d-%d" % (c, l, s[0], s[1], dp)


SLICE_LAYOUTS = (("yuv420p", 33, 67, 8), ("bgr24", 33, 67, 10))
SLICE_FRAMES = 7


def slice_pool(layout, h, w, depth):
    """the seven distinct frame pairs of tests/test_gpu_mdsi_slices.py: natural, noise and texture_flat under changing seeds
    -> (ref frames, dist frames), each a list of plane tuples; tests/test_mdsi_host.py admits every one"""
    names = ("natural", "noise", "texture_flat", "noise", "natural", "noise", "natural")
    pairs = [pair(nm, layout, h, w, depth, seed=11 + k) for k, nm in enumerate(names)]
    return [p[0] for p in pairs], [p[1] for p in pairs]
