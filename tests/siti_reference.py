"""ITU-T P.910 spatial and temporal information, restated in NumPy from the definition in include/vqa.h (vqa_siti_submit), from
int64 samples.  Two forms:

  sums / record   the definition as it is built: the integer sums through int64 / Python-int arithmetic (grad_fix =
                  sum rint(sqrt((double) q) 2^32) as Python ints), then the host formulas in float64.
  si_exact / ti_exact   an independent two-pass np.std in float64 with no quantisation: what the quantised form is measured
                  against (quantum_bar is the bound the definition derives for the gap)."""
import numpy as np

MIN_DIM = 16
FIX = 2.0 ** 32


def sobel_q(r):
    """[h, w] int64 samples -> q = gx^2 + gy^2 on the interior, [h-2, w-2] int64"""
    r = np.asarray(r, np.int64)
    if r.shape[0] < MIN_DIM or r.shape[1] < MIN_DIM:
        raise ValueError("planes below %d x %d are not measured" % (MIN_DIM, MIN_DIM))
    gx = (r[:-2, 2:] + 2 * r[1:-1, 2:] + r[2:, 2:]) - (r[:-2, :-2] + 2 * r[1:-1, :-2] + r[2:, :-2])
    gy = (r[2:, :-2] + 2 * r[2:, 1:-1] + r[2:, 2:]) - (r[:-2, :-2] + 2 * r[:-2, 1:-1] + r[:-2, 2:])
    return gx * gx + gy * gy


def sums(r, prev=None):
    """-> (grad_fix, grad_sq, diff_sum, diff_sq) as Python ints; the two diff sums are 0 without a predecessor"""
    q = sobel_q(r)
    assert int(q.max()) < 2 ** 38
    grad_sq = sum(int(v) for v in q.sum(axis=1))                       # row sums fit int64; the total as a Python int
    fix = np.rint(np.sqrt(q.astype(np.float64)) * FIX)                   # each below 2^51: exact in float64
    grad_fix = sum(int(v) for v in fix.astype(np.int64).sum(axis=1))
    if prev is None:
        return grad_fix, grad_sq, 0, 0
    d = np.asarray(r, np.int64) - np.asarray(prev, np.int64)
    return grad_fix, grad_sq, int(d.sum()), int((d * d).sum())


def results(grad_sum, grad_sq, diff_sum, diff_sq, h, w, depth=8):
    """the host formulas of include/vqa.h in float64 -> (si, ti); grad_sum is the double the record carries"""
    sc = 2.0 ** -(depth - 8)
    n_i, n_a = np.float64((h - 2) * (w - 2)), np.float64(h * w)
    m = np.float64(grad_sum) / n_i
    si = sc * np.sqrt(max(np.float64(grad_sq) / n_i - m * m, 0.0))
    md = np.float64(diff_sum) / n_a
    ti = sc * np.sqrt(max(np.float64(diff_sq) / n_a - md * md, 0.0))
    return float(si), float(ti)


def grad_sum_of(grad_fix):
    """the record's grad_sum from the integer total: (double) hi + (double) lo 2^-32"""
    return float(np.float64(grad_fix >> 32) + np.float64(grad_fix & 0xFFFFFFFF) * 2.0 ** -32)


def record(r, prev=None, depth=8):
    """-> dict(grad_fix, grad_sum, grad_sq, diff_sum, diff_sq, si, ti) of one plane"""
    h, w = np.asarray(r).shape
    grad_fix, grad_sq, diff_sum, diff_sq = sums(r, prev)
    gs = grad_sum_of(grad_fix)
    si, ti = results(gs, grad_sq, diff_sum, diff_sq, h, w, depth)
    return dict(grad_fix=grad_fix, grad_sum=gs, grad_sq=grad_sq, diff_sum=diff_sum, diff_sq=diff_sq, si=si, ti=ti)


def series(planes, depth=8, prev0=None):
    """[n, h, w] -> list of records, frame i against frame i - 1 (frame 0 against prev0 or nothing)"""
    out = []
    for i in range(len(planes)):
        prev = planes[i - 1] if i > 0 else prev0
        out.append(record(planes[i], prev, depth))
    return out


def si_exact(r, depth=8):
    """two-pass population standard deviation of the Sobel magnitude, float64, no quantisation; -> (si, mean, variance) with
    mean and variance on the raw sample scale"""
    g = np.sqrt(sobel_q(r).astype(np.float64))
    return float(np.std(g) * 2.0 ** -(depth - 8)), float(g.mean()), float(g.var())


def ti_exact(r, prev, depth=8):
    """two-pass population standard deviation of the frame difference, float64; -> (ti, mean, variance), mean and variance on
    the raw sample scale; all 0 without a predecessor"""
    if prev is None:
        return 0.0, 0.0, 0.0
    d = (np.asarray(r, np.int64) - np.asarray(prev, np.int64)).astype(np.float64)
    return float(np.std(d) * 2.0 ** -(depth - 8)), float(d.mean()), float(d.var())


def quantum_bar(m, var, depth=8, e=2.0 ** -32):
    """what an error e on the mean m can move si by (include/vqa.h: the variance moves by 2 m e + e^2), on the 8-bit scale,
    plus 1e-12 for the float64 arithmetic of either side"""
    return float((np.sqrt(var + 2.0 * m * e + e * e) - np.sqrt(var)) * 2.0 ** -(depth - 8) + 1e-12)
