"""include/vqa.h's definition of vqa_convert_submit, restated in NumPy int64 straight from its text: the relation per axis, the
taps (weights that sum to 4, the edge replicated), horizontal first and vertical second with no rounding in between, then the
depth / range step with the one rounding and the clip.  Nothing here is shared with the product."""
import numpy as np


def relation(n_s, n_d):
    if n_d == n_s:
        return "same"
    if n_s == (n_d + 1) >> 1:
        return "up"
    if n_d == (n_s + 1) >> 1:
        return "down"
    raise ValueError("no relation between %d and %d samples" % (n_s, n_d))


def taps(s, n_d, chroma, left, axis):
    """the taps of one axis, times 4: s int64, n_d output samples along `axis`; left: left-sited (LINEAR, horizontal only)"""
    n_s = s.shape[axis]
    rel = relation(n_s, n_d)
    x = np.arange(n_d)

    def at(i):
        return np.take(s, np.clip(i, 0, n_s - 1), axis=axis)

    def per_x(even, odd):
        shape = [1] * s.ndim
        shape[axis] = n_d
        return np.where((x & 1).reshape(shape) == 0, even, odd)

    if rel == "same":
        return 4 * s
    if rel == "up":
        if chroma == "box":
            return 4 * at(x >> 1)
        if left:
            return per_x(4 * at(x >> 1), 2 * at(x >> 1) + 2 * at((x >> 1) + 1))
        return per_x(3 * at(x >> 1) + at((x >> 1) - 1), 3 * at(x >> 1) + at((x >> 1) + 1))
    if chroma == "linear" and left:
        return at(2 * x - 1) + 2 * at(2 * x) + at(2 * x + 1)
    return 2 * at(2 * x) + 2 * at(2 * x + 1)


def round_v(v, ds, dd, range):
    """v, the exact value with denominator 16 -> the output code"""
    v = np.asarray(v, np.int64)
    ps, pd = (1 << ds) - 1, (1 << dd) - 1
    if range == "limited":
        if dd >= ds:
            out = ((v << (dd - ds)) + 8) >> 4
        else:
            out = (v + (1 << (3 + ds - dd))) >> (4 + ds - dd)
    else:
        out = (2 * v * pd + 16 * ps) // (32 * ps)
    return np.minimum(out, pd)


def convert_plane(s, dh, dw, ds, dd, chroma="linear", siting="center", range="limited"):
    """s: [.., h, w] samples of depth ds (read as they are) -> [.., dh, dw] int64 codes of depth dd"""
    s = np.asarray(s).astype(np.int64)
    hz = taps(s, dw, chroma, siting == "left", s.ndim - 1)
    v = taps(hz, dh, chroma, False, s.ndim - 2)     # the vertical axis is always centre-sited
    return round_v(v, ds, dd, range)


def _depth(planes):
    return (int(planes[0][5]) if len(planes[0]) > 5 else 0) or 8


def read_plane(frame, plane):
    """frame: uint8 [bytes] of one frame; plane: (w, h, offset, row_stride, pixel_step[, depth]) -> int64 [h, w]"""
    w, h, off, rs, step = (int(v) for v in plane[:5])
    bps = 2 if _depth([plane]) > 8 else 1
    idx = off + np.arange(h)[:, None] * rs + np.arange(w)[None, :] * step
    v = frame[idx].astype(np.int64)
    if bps == 2:
        v |= frame[idx + 1].astype(np.int64) << 8
    return v


def write_plane(frame, plane, values):
    w, h, off, rs, step = (int(v) for v in plane[:5])
    bps = 2 if _depth([plane]) > 8 else 1
    idx = off + np.arange(h)[:, None] * rs + np.arange(w)[None, :] * step
    frame[idx] = (values & 0xff).astype(np.uint8)
    if bps == 2:
        frame[idx + 1] = (values >> 8).astype(np.uint8)


def convert_frames(src, planes, dst, out_planes, chroma="linear", siting="center", range="limited"):
    """src: uint8 [n, source frame bytes]; dst: uint8 [n, destination frame bytes], written in place where a destination sample
    lies and nowhere else -> dst"""
    ds, dd = _depth(planes), _depth(out_planes)
    for j in np.arange(src.shape[0]):
        for a, b in zip(planes, out_planes):
            write_plane(dst[j], b, convert_plane(read_plane(src[j], a), int(b[1]), int(b[0]), ds, dd, chroma, siting, range))
    return dst


def convert_packed(frames, planes, out_planes, chroma="linear", siting="center", range="limited"):
    """frames: [n, samples] of the planes' sample type, tightly described by `planes` -> [n, samples of out_planes], zero where
    no sample lies (the layouts of the entry points have no such bytes)"""
    src = np.ascontiguousarray(frames)
    n = src.shape[0]
    bd = 2 if _depth(out_planes) > 8 else 1
    span = max(int(p[2]) + (int(p[1]) - 1) * int(p[3]) + (int(p[0]) - 1) * int(p[4]) + bd for p in out_planes)
    dst = np.zeros((n, span), np.uint8)
    convert_frames(src.view(np.uint8).reshape(n, -1), planes, dst, out_planes, chroma, siting, range)
    return dst.view(np.uint16 if bd == 2 else np.uint8)
