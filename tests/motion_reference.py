"""VMAF's motion feature in float64, written from the definition in include/vqa.h (vqa_motion_submit) - not from the kernel.

    samples   x = R / 2^(depth-8) - 128
    blur      5 taps (0.054488685, 0.244201342, 0.402619947, 0.244201342, 0.054488685), columns (vertical) first, then rows
    borders   index i < 0 reads -i; index i >= n reads 2n - i - 1
    motion[i] = sum |blur(x_i) - blur(x_{i-1})| / (h w), 0 for a frame with no predecessor
    motion2[i] = min(motion[i], motion[i+1]), motion2[last] = motion[last]
"""
import numpy as np

TAPS = (0.054488685, 0.244201342, 0.402619947, 0.244201342, 0.054488685)
MIN_DIM = 16


def border_index(i, n):
    if i < 0:
        i = -i
    if i >= n:
        i = 2 * n - i - 1
    return i


def samples(plane, depth=8):
    return np.asarray(plane, np.float64) / float(1 << (depth - 8)) - 128.0


def _pass(x, axis):
    n = x.shape[axis]
    out = np.zeros_like(x)
    for k, t in enumerate(TAPS):
        idx = [border_index(i + k - 2, n) for i in range(n)]
        out = out + t * np.take(x, idx, axis=axis)
    return out


def blur(x):
    """the vertical pass first, then the horizontal one"""
    return _pass(_pass(np.asarray(x, np.float64), 0), 1)


def blur_loops(x):
    """the same by plain loops (small planes: the tests check blur against it)"""
    x = np.asarray(x, np.float64)
    h, w = x.shape
    v = np.zeros((h, w))
    for i in range(h):
        for j in range(w):
            for k in range(5):
                v[i, j] += TAPS[k] * x[border_index(i + k - 2, h), j]
    out = np.zeros((h, w))
    for i in range(h):
        for j in range(w):
            for k in range(5):
                out[i, j] += TAPS[k] * v[i, border_index(j + k - 2, w)]
    return out


def sad(cur, prev, depth=8):
    """sum |blur(x_cur) - blur(x_prev)| over the plane"""
    cur, prev = np.asarray(cur), np.asarray(prev)
    if cur.shape != prev.shape or cur.ndim != 2:
        raise ValueError("two planes of one geometry")
    if min(cur.shape) < MIN_DIM:
        raise ValueError("planes of at least %d x %d" % (MIN_DIM, MIN_DIM))
    return float(np.abs(blur(samples(cur, depth)) - blur(samples(prev, depth))).sum())


def motion(planes, depth=8, prev0=None):
    """planes: [n, h, w] of one plane over a clip -> motion [n]; frame 0 is compared with prev0 (None: 0)"""
    planes = np.asarray(planes)
    n, h, w = planes.shape
    out = np.zeros(n)
    for i in range(n):
        prev = planes[i - 1] if i > 0 else prev0
        if prev is not None:
            out[i] = sad(planes[i], prev, depth) / (h * w)
    return out


def motion2(m):
    m = [float(v) for v in m]
    return np.array([min(m[i], m[i + 1]) if i + 1 < len(m) else m[i] for i in range(len(m))], np.float64)
