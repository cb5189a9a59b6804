"""The clips and hand-made planes the signal-statistics tests measure, in every layout of test_gpu_siti.py's grid."""
import numpy as np

import motion_cases as K

# geometry (h, w), depth, layout: test_gpu_siti.py's grid - the minimum, sizes that cross a tile's edge by one sample either way,
# every sample type and step
GRID = [((16, 16), 8, "gray"), ((33, 65), 8, "gray"), ((47, 35), 8, "gray"), ((66, 98), 8, "yuv420p"),
        ((64, 96), 10, "yuv420p10le"), ((40, 56), 12, "yuv444p12le"), ((50, 70), 16, "gray16le"), ((40, 56), 8, "bgr24")]
IDS = ["%dx%d-%s" % (g[0][0], g[0][1], g[2]) for g in GRID]
BARS = (3, 2, 2, 3)   # the dark rows at the top and the bottom, the dark columns at the left and the right of a boxed picture


def type_max(depth):
    """the largest value of the SAMPLE TYPE: above the peak for uint16 samples of less than 16 bits"""
    return 65535 if depth > 8 else 255


def noise(rng, h, w, depth):
    """the full range of the sample type: at depths 9 .. 15 this includes samples above the peak"""
    return rng.integers(0, type_max(depth) + 1, (h, w)).astype(np.int64)


def boxed(rng, h, w, depth, crop_level):
    """a letterboxed and pillarboxed picture whose bars sit exactly AT crop_level (dark: a sum equal to the limit is dark) and
    whose picture lies above it everywhere -> (samples, the box)"""
    t, b, l, r = BARS
    x = np.full((h, w), crop_level, np.int64)
    x[t:h - b, l:w - r] = rng.integers(crop_level + 1, (1 << depth), (h - t - b, w - l - r))
    return x, (t, h - b - 1, l, w - r - 1)


def plane_content(rng, h, w, depth, crop_level):
    """five frames of one plane: noise, noise, a boxed picture, the same again (a frame equal to its predecessor), noise"""
    bx, _ = boxed(rng, h, w, depth, crop_level)
    return np.stack([noise(rng, h, w, depth), noise(rng, h, w, depth), bx, bx.copy(), noise(rng, h, w, depth)])


def pack(layout, h, w, depth, per_plane):
    """per_plane(k, ph, pw) -> [n, ph, pw] samples of plane k; -> (frames [n, samples] ([n, h, w, 3] for bgr24), planes)"""
    planes = K.planes_of(layout, h, w)
    dt = np.uint16 if depth > 8 else np.uint8
    isz = np.dtype(dt).itemsize
    size = max(p[2] + (p[1] - 1) * p[3] + (p[0] - 1) * p[4] + isz for p in planes) // isz
    out = None
    for k, p in enumerate(planes):
        pw, ph, off, rs, step = p[:5]
        a = per_plane(k, ph, pw)
        if out is None:
            out = np.zeros((len(a), size), dt)
        for i in range(len(a)):
            view = np.lib.stride_tricks.as_strided(out[i, off // isz:], shape=(ph, pw), strides=(rs, step))
            view[...] = a[i]
    if layout == "bgr24":
        out = out.reshape(len(out), h, w, 3)
    return out, planes


def clip(layout, h, w, depth, seed, crop_level=None):
    """the five frames of plane_content in every plane of `layout`"""
    crop = (24 << (depth - 8)) if crop_level is None else crop_level
    rng = np.random.default_rng(seed)
    return pack(layout, h, w, depth, lambda k, ph, pw: plane_content(rng, ph, pw, depth, crop))


def mono(samples, depth):
    """[n, h, w] samples of one plane -> (frames [n, h w], planes)"""
    from rtvqa_amd.engine import gray_planes, mono_planes
    a = np.asarray(samples)
    n, h, w = a.shape
    return (a.astype(np.uint16 if depth > 8 else np.uint8).reshape(n, h * w),
            gray_planes(h, w) if depth == 8 else mono_planes(h, w, depth))


def two_level(h, w, count_a, a, b, seed=0):
    """a plane with exactly count_a samples of value a and the rest b, shuffled"""
    x = np.full(h * w, b, np.int64)
    x[:count_a] = a
    np.random.default_rng(seed).shuffle(x)
    return x.reshape(h, w)


def qc_clip(h=48, w=64, depth=8):
    """A short clip with a black frame, a frozen pair, a cut and bars, one plane [n, h, w]:
    0, 1     shot A, frame 1 a slightly changed frame 0
    2        black
    3, 4     shot A again, frame 4 equal to frame 3 (frozen)
    5, 6     shot B, far from shot A (the cut is at 5); frame 6 a slightly changed frame 5
    (the black frame is far from shot A too: scene_score marks frame 2, and not frame 3, whose mafd is close to frame 2's)
    Every frame but the black one carries the bars of BARS at crop_level's default."""
    s = 1 << (depth - 8)
    rng = np.random.default_rng(7)
    t, b, l, r = BARS

    def shot(lo, hi):
        x = np.full((h, w), 24 * s, np.int64)
        x[t:h - b, l:w - r] = rng.integers(lo * s, hi * s, (h - t - b, w - l - r))
        return x
    a0, b0 = shot(40, 90), shot(160, 230)
    a1, b1 = a0.copy(), b0.copy()
    a1[10:30, 10:50] += 3 * s   # sad = 2400 s: above freezedetect's 0.001 N (2^d - 1) = 783 s, far below a cut
    b1[20:40, 10:50] -= 3 * s
    black = np.full((h, w), 16 * s, np.int64)
    return np.stack([a0, a1, black, a0, a0.copy(), b0, b1]), (t, h - b - 1, l, w - r - 1)
