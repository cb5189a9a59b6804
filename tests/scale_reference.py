"""The resampler of vqa_scale_submit restated in NumPy (include/vqa.h states the definition): Pillow's Image.resize for 8-bit
images - the tables of precompute_coeffs in double, quantised once to 2^-22 as normalize_coeffs_8bpc does, the horizontal pass
clipped and stored at the sample type before the vertical pass reads it - carried to 9..16 bits with 64-bit sums.

tables(filter, n_in, n_out) builds the integer tables of one axis; resample(plane, out_h, out_w, depth, tabs_x, tabs_y) takes
the tables as an ARGUMENT, so a test can hand it the tables vqa_scale_tables built and does not depend on this machine's sin."""
import math

import numpy as np

PRECISION_BITS = 22
FILTERS = ("bilinear", "bicubic", "lanczos")
SUPPORT = {"bilinear": 1.0, "bicubic": 2.0, "lanczos": 3.0}


def _bilinear(x):
    x = -x if x < 0.0 else x
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic(x):
    a = -0.5
    x = -x if x < 0.0 else x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


_KERNEL = {"bilinear": _bilinear, "bicubic": _bicubic, "lanczos": _lanczos}


def ksize(filter, n_in, n_out):
    fs = max(n_in / n_out, 1.0)
    return 2 * int(math.ceil(SUPPORT[filter] * fs)) + 1


def tables(filter, n_in, n_out):
    """-> (k int32 [n_out, ksize], xmin int32 [n_out], count int32 [n_out]); the unused tail of a row of k is 0"""
    f = _KERNEL[filter]
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = SUPPORT[filter] * fs
    ks = 2 * int(math.ceil(support)) + 1
    k = np.zeros((n_out, ks), np.int32)
    xmin = np.zeros(n_out, np.int32)
    count = np.zeros(n_out, np.int32)
    ss = 1.0 / fs
    for x in range(n_out):
        c = (x + 0.5) * scale
        lo = max(0, int(c - support + 0.5))
        hi = min(n_in, int(c + support + 0.5))
        w = [f((j + lo - c + 0.5) * ss) for j in range(hi - lo)]
        ww = 0.0
        for v in w:
            ww += v
        for j, v in enumerate(w):
            v = v / ww if ww != 0.0 else v
            k[x, j] = int(v * (1 << PRECISION_BITS) - 0.5) if v < 0 else int(v * (1 << PRECISION_BITS) + 0.5)
        xmin[x], count[x] = lo, hi - lo
    return k, xmin, count


def _pass(a, tabs, peak):
    """the last axis of the int64 array `a` through one axis' tables"""
    k, xmin, count = tabs
    n_out, ks = k.shape
    idx = np.minimum(xmin[:, None] + np.arange(ks)[None, :], a.shape[-1] - 1)   # (k is 0 past count)
    acc = (a[..., idx] * k.astype(np.int64)).sum(axis=-1) + (1 << (PRECISION_BITS - 1))
    return np.clip(acc >> PRECISION_BITS, 0, peak)


def resample(plane, out_h, out_w, depth=8, tabs_x=None, tabs_y=None, filter="bicubic"):
    """plane [h, w] (or [.., h, w]) of uint8 / uint16 samples -> [.., out_h, out_w] of the same type.  tabs_x / tabs_y: the
    tables of the horizontal / vertical axis (None: built here from `filter`).  An axis whose size does not change is copied
    as it is; what leaves is clipped to the depth's peak."""
    plane = np.asarray(plane)
    h, w = plane.shape[-2:]
    peak = (1 << depth) - 1
    a = plane.astype(np.int64)
    if out_w != w:
        a = _pass(a, tabs_x if tabs_x is not None else tables(filter, w, out_w), peak)
    if out_h != h:
        t = tabs_y if tabs_y is not None else tables(filter, h, out_h)
        a = np.swapaxes(_pass(np.swapaxes(a, -1, -2), t, peak), -1, -2)
    return np.minimum(a, peak).astype(plane.dtype)


def pin_input(seed, index, h, w, content, depth=8):
    """the input plane of case `index` of tests/golden/scale_pins.json (scripts/gen_scale_pins.py records the seed)"""
    rng = np.random.default_rng([seed, index])
    peak = (1 << depth) - 1
    if content == "noise":
        a = rng.integers(0, peak + 1, (h, w))
    elif content == "midnoise":   # the middle half of the range: no pass can leave 0 .. peak (sum |k| < 2 per pass)
        a = rng.integers((peak + 1) // 4, 3 * (peak + 1) // 4, (h, w))
    else:   # "binary": 0 / peak in runs, so that the overshoot of bicubic and lanczos clips at both ends
        a = (rng.integers(0, 2, ((h + 2) // 3, (w + 2) // 3)).repeat(3, 0).repeat(3, 1)[:h, :w]) * peak
    return a.astype(np.uint16 if depth > 8 else np.uint8)
