"""Colour registration restated in NumPy from the text of include/vqa.h (vqa_colorfit_submit): replicate the chroma to the luma
grid, then direct sums in int64 / Python integers, the tables by np.bincount.  It shares no code with the package.

A frame is a 1-D array of samples (uint8, or uint16 above 8 bits); a plane is (width, height, offset, row_stride, pixel_step[,
depth]) with offset and strides in bytes."""
import numpy as np

PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
FIELDS = ("count", "sum_r", "sum_d", "rr", "rd", "dd", "sse")


def grid(frame, plane, h, w):
    """plane `plane` of a frame on the h x w luma grid as int64: position (y, x) is the sample at (y >> sy, x >> sx)"""
    bps = frame.dtype.itemsize
    pw, ph, off, rs, step = (int(v) for v in plane[:5])
    assert off % bps == 0 and rs % bps == 0 and step % bps == 0
    assert pw in (w, (w + 1) // 2) and ph in (h, (h + 1) // 2)
    sy, sx = int(ph != h), int(pw != w)
    y = (np.arange(h) >> sy)[:, None]
    x = (np.arange(w) >> sx)[None, :]
    return frame[(off + y * rs + x * step) // bps].astype(np.int64)


def record(ref, dist, planes):
    """one frame pair -> dict of Python integers / lists of them, the fields of vqa_colorfit_metrics"""
    w, h = int(planes[0][0]), int(planes[0][1])
    r = [grid(ref, p, h, w) for p in planes]
    d = [grid(dist, p, h, w) for p in planes]
    n = len(planes)

    def total(a):
        return int(a.sum(dtype=np.int64))

    out = {"count": h * w, "sum_r": [0] * 3, "sum_d": [0] * 3, "rr": [0] * 6, "rd": [0] * 9, "dd": [0] * 3, "sse": [0] * 3}
    for i in range(n):
        out["sum_r"][i] = total(r[i])
        out["sum_d"][i] = total(d[i])
        out["dd"][i] = total(d[i] * d[i])
        out["sse"][i] = total((d[i] - r[i]) ** 2)
        for k in range(n):
            out["rd"][3 * i + k] = total(r[i] * d[k])
    for q, (i, j) in enumerate(PAIRS):
        if i < n and j < n:
            out["rr"][q] = total(r[i] * r[j])
    for i in range(n):   # the header's identity
        assert out["sse"][i] == out["dd"][i] - 2 * out["rd"][4 * i] + out["rr"][(0, 3, 5)[i]]
    return out


def records(ref, dist, planes):
    return [record(a, b, planes) for a, b in zip(ref, dist)]


def bins_of(depth):
    return 1 << min(depth, 10)


def tables(ref, dist, planes, depth):
    """all frames of a submit -> int64 [n_planes][bins][3]: count, sum_d, sum_dd per bin of the reference sample"""
    w, h = int(planes[0][0]), int(planes[0][1])
    bins, shift = bins_of(depth), max(depth - 10, 0)
    out = np.zeros((len(planes), bins, 3), np.int64)
    for a, b in zip(ref, dist):
        for p, plane in enumerate(planes):
            r, d = grid(a, plane, h, w).ravel(), grid(b, plane, h, w).ravel()
            at = np.minimum(r >> shift, bins - 1)
            out[p, :, 0] += np.bincount(at, minlength=bins)
            for col, wgt in ((1, d), (2, d * d)):
                s = np.bincount(at, weights=wgt.astype(np.float64), minlength=bins)
                assert s.max() < 2.0 ** 53   # integer sums below 2^53 are exact in float64
                out[p, :, col] += np.rint(s).astype(np.int64)
    return out
