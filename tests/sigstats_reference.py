"""A NumPy restatement of the signal statistics of include/vqa.h (vqa_sigstats_submit), written from the header's text.  It does
NOT share the kernels' method: the order statistics come from np.sort and indexing (no histogram), the counts from comparisons on
the samples, the box from sum(axis=..)."""
import numpy as np

INT_FIELDS = ("count", "sum", "sum_sq", "min", "max", "low", "median", "high", "or_mask", "and_mask", "bits_used", "below_black",
              "under", "over_luma", "over_chroma", "above_peak", "sad", "changed", "top", "bottom", "left", "right")
FIELDS = INT_FIELDS + ("mean", "stdev", "dif")
OFFSETS = (0, 8, 16, 24, 28, 32, 36, 40, 44, 48, 52, 56, 64, 72, 80, 88, 96, 104, 112, 116, 120, 124, 128, 136, 144)
SIZE = 152


def ranks(n):
    """k of low, median and high for a plane of n samples"""
    return (n + 9) // 10, (n + 1) // 2, (9 * n + 9) // 10


def defaults(depth):
    """(black_level, crop_level) where the caller gives none"""
    return 32 << (depth - 8), 24 << (depth - 8)


def box(x, crop_level):
    """(top, bottom, left, right): the first and last row and column that are not dark"""
    h, w = x.shape
    rows = np.nonzero(x.sum(axis=1) > crop_level * w)[0]
    cols = np.nonzero(x.sum(axis=0) > crop_level * h)[0]
    return (int(rows[0]) if len(rows) else h, int(rows[-1]) if len(rows) else -1,
            int(cols[0]) if len(cols) else w, int(cols[-1]) if len(cols) else -1)


def record(x, depth, prev=None, black_level=None, crop_level=None):
    """x, prev: [h, w] integer samples (prev: the same plane of the frame before, or None) -> dict of Python ints"""
    x = np.asarray(x).astype(np.int64)
    s = 1 << (depth - 8)
    black = 32 * s if black_level is None else black_level
    crop = 24 * s if crop_level is None else crop_level
    n = x.size
    srt = np.sort(x, axis=None)
    # the smallest v with C(v) >= k is the k-th smallest sample
    low, median, high = (int(srt[k - 1]) for k in ranks(n))
    orm = int(np.bitwise_or.reduce(x, axis=None))
    r = dict(count=n, sum=int(x.sum()), sum_sq=int((x * x).sum()), min=int(srt[0]), max=int(srt[-1]), low=low, median=median,
             high=high, or_mask=orm, and_mask=int(np.bitwise_and.reduce(x, axis=None)),
             bits_used=0 if orm == 0 else depth - (orm & -orm).bit_length() + 1,
             below_black=int((x < black).sum()), under=int((x < 16 * s).sum()), over_luma=int((x > 235 * s).sum()),
             over_chroma=int((x > 240 * s).sum()), above_peak=int((x > (1 << depth) - 1).sum()), sad=0, changed=0)
    if prev is not None:
        p = np.asarray(prev).astype(np.int64)
        r["sad"], r["changed"] = int(np.abs(x - p).sum()), int((x != p).sum())
    r["top"], r["bottom"], r["left"], r["right"] = box(x, crop)
    return r


def doubles(r):
    """(mean, stdev, dif) from a record's own words by the header's formula, in the order written"""
    n = np.float64(int(r["count"]))
    mean = np.float64(int(r["sum"])) / n
    var = np.float64(int(r["sum_sq"])) / n - mean * mean
    return float(mean), float(np.sqrt(var if var > 0.0 else np.float64(0.0))), float(np.float64(int(r["sad"])) / n)


def series(plane, depth, prev0=None, black_level=None, crop_level=None):
    """plane: [n, h, w] -> the n records, frame i against frame i - 1, frame 0 against prev0 ([h, w] or None)"""
    out = []
    for i in range(len(plane)):
        prev = plane[i - 1] if i > 0 else prev0
        out.append(record(plane[i], depth, prev, black_level, crop_level))
    return out


def profile(x):
    """(row sums [h], column sums [w]) as uint64"""
    x = np.asarray(x).astype(np.int64)
    return x.sum(axis=1).astype(np.uint64), x.sum(axis=0).astype(np.uint64)


def same_words(got, want):
    """the names of the integer words of a device record `got` that differ from the reference's dict `want`"""
    return [k for k in INT_FIELDS if int(got[k]) != want[k]]


def ulp_close(a, b, ulps=2):
    return abs(a - b) <= ulps * np.spacing(max(abs(a), abs(b)))
