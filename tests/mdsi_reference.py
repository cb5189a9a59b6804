"""MDSI (Nafchi, Shahkolaei, Hedjam and Cheriet 2016, the "sum" combination) restated twice from the definition in include/vqa.h
(vqa_mdsi_submit), in NumPy:

  mdsi_float      the definition in plain float64: colour conversion per pixel, box mean, channels, Prewitt of L_r, L_d and of the
                  fused image F = 0.5 (L_r + L_d) itself, similarities from the magnitudes, the complex quarter root, the mean
                  absolute deviation.  Nothing is quantised.
  mdsi_quantised  the device's form op for op: integer box sums and the 3 x 4 matrix, the stated order of every double
                  operation, g = rint(GCS 2^24), zq, the words A, B, n_neg, D.  Returns the four words; pool_words gives the
                  record's dev and mdsi from them.

A frame is a list of 2-D integer arrays: [Y, U, V] (U, V of the luma's size or its ceil-half in either direction), [B, G, R] or
[Y].  model: "yuv709" | "bgr" | "gray".  Not pinned against the authors' MATLAB (README, Parity)."""
import math

import numpy as np

MODELS = {"yuv709": 0, "bgr": 1, "gray": 2}
C1, C2, C3 = 140.0, 55.0, 550.0
FIX_G, FIX_Z = float(1 << 24), float(1 << 28)
SQRT_HALF = math.sqrt(0.5)
A_ROWS = ((0.2989, 0.5870, 0.1140), (0.30, 0.04, -0.35), (0.34, -0.60, 0.17))   # L, H, M over R, G, B


def factor(h, w):
    """f = max(1, floor(min(h, w) / 256 + 0.5)): MATLAB's round, half away from zero"""
    return max(1, int(math.floor(min(h, w) / 256.0 + 0.5)))


def grid(h, w):
    f = factor(h, w)
    return f, -(-h // f), -(-w // f)


def box_sum(x, f):
    """[h, w] -> [ceil(h / f), ceil(w / f)]: sample (i, j) is the sum over rows i f + o .. i f + o + f - 1, o = floor(f / 2) -
    (f - 1), and the same columns; positions outside the plane count 0.  Keeps the dtype's arithmetic (integers stay exact)."""
    h, w = x.shape
    hd, wd, p = -(-h // f), -(-w // f), (f - 1) - f // 2
    big = np.zeros((max(hd * f, h + p), max(wd * f, w + p)), x.dtype)
    big[p:p + h, p:p + w] = x
    return big[:hd * f, :wd * f].reshape(hd, f, wd, f).sum(axis=(1, 3))


def replicate(c, h, w):
    """a chroma plane on the luma grid: sample (i >> sv, j >> sh)"""
    sv, sh = int(c.shape[0] != h), int(c.shape[1] != w)
    return c[(np.arange(h) >> sv)[:, None], (np.arange(w) >> sh)[None, :]]


def prewitt(x):
    """Prewitt over 3, divided by 3, zero outside the grid, in the order include/vqa.h states -> gx, gy"""
    p = np.zeros((x.shape[0] + 2, x.shape[1] + 2), np.float64)
    p[1:-1, 1:-1] = x
    s = lambda dy, dx: p[1 + dy:p.shape[0] - 1 + dy, 1 + dx:p.shape[1] - 1 + dx]
    gx = (((s(-1, 1) + s(0, 1)) + s(1, 1)) - ((s(-1, -1) + s(0, -1)) + s(1, -1))) / 3.0
    gy = (((s(1, -1) + s(1, 0)) + s(1, 1)) - ((s(-1, -1) + s(-1, 0)) + s(-1, 1))) / 3.0
    return gx, gy


# ---- the plain float64 form -------------------------------------------------------------------------------------------
def _rgb_float(planes, model, depth):
    s, peak = float(1 << (depth - 8)), float((1 << depth) - 1)
    h, w = planes[0].shape
    if model == "bgr":
        b, g, r = (p.astype(np.float64) for p in planes)
        return 255.0 * r / peak, 255.0 * g / peak, 255.0 * b / peak
    y = (planes[0].astype(np.float64) - 16.0 * s) / (219.0 * s)
    if model == "gray":
        u = v = np.zeros((h, w))
    else:
        u = (replicate(planes[1], h, w).astype(np.float64) - 128.0 * s) / (224.0 * s)
        v = (replicate(planes[2], h, w).astype(np.float64) - 128.0 * s) / (224.0 * s)
    return 255.0 * (y + 1.5748 * v), 255.0 * (y - 0.1873 * u - 0.4681 * v), 255.0 * (y + 1.8556 * u)


def _channels_float(planes, model, depth):
    f = factor(*planes[0].shape)
    r, g, b = (box_sum(c, f) / float(f * f) for c in _rgb_float(planes, model, depth))
    return tuple(a[0] * r + a[1] * g + a[2] * b for a in A_ROWS)


def gcs_float(ref, dist, model, depth=8):
    """-> GCS [hd, wd] float64, unquantised"""
    lr, hr, mr = _channels_float(ref, model, depth)
    ld, hd, md = _channels_float(dist, model, depth)
    mag = lambda x: np.hypot(*prewitt(x))
    a, b, c = mag(lr), mag(ld), mag(0.5 * (lr + ld))
    sim = lambda p, q, k: (2.0 * p * q + k) / (p * p + q * q + k)
    gs = sim(a, b, C1) + sim(b, c, C2) - sim(a, c, C2)
    cs = (2.0 * (hr * hd + mr * md) + C3) / (hr * hr + hd * hd + mr * mr + md * md + C3)
    return 0.6 * gs + 0.4 * cs


def pool_float(gcs):
    """-> dev, mdsi of a GCS map: the principal complex quarter root, the mean absolute deviation, its quarter power"""
    z = np.abs(gcs) ** 0.25 * np.where(gcs < 0, complex(SQRT_HALF, SQRT_HALF), 1.0 + 0.0j)
    dev = float(np.mean(np.abs(z - np.mean(z))))
    return dev, dev ** 0.25


def mdsi_float(ref, dist, model, depth=8):
    return pool_float(gcs_float(ref, dist, model, depth))


# ---- the device's form, op for op -------------------------------------------------------------------------------------
def matrix(model, depth, f):
    """the twelve doubles of include/vqa.h: mat[L, H, M][plane 0, 1, 2, count]"""
    s, peak = float(1 << (depth - 8)), float((1 << depth) - 1)
    rgb = [[0.0] * 4 for _ in range(3)]
    o0 = o1 = 0.0
    if model == "bgr":
        k = 255.0 / peak
        rgb[0][2] = k; rgb[1][1] = k; rgb[2][0] = k
    else:
        ky, kc = 255.0 / (219.0 * s), (0.0 if model == "gray" else 255.0 / (224.0 * s))
        rgb[0][0] = ky; rgb[0][2] = 1.5748 * kc
        rgb[1][0] = ky; rgb[1][1] = -0.1873 * kc; rgb[1][2] = -0.4681 * kc
        rgb[2][0] = ky; rgb[2][1] = 1.8556 * kc
        o0, o1 = 16.0 * s, 128.0 * s
    for c in range(3):
        rgb[c][3] = -((o0 * rgb[c][0] + o1 * rgb[c][1]) + o1 * rgb[c][2])
    ff = float(f) * float(f)
    return [[((a[0] * rgb[0][j] + a[1] * rgb[1][j]) + a[2] * rgb[2][j]) / ff for j in range(4)] for a in A_ROWS]


def _channels_quantised(planes, model, depth):
    h, w = planes[0].shape
    f = factor(h, w)
    full = [planes[0].astype(np.int64)] + [replicate(p, h, w).astype(np.int64) for p in planes[1:]]
    while len(full) < 3:
        full.append(np.zeros((h, w), np.int64))
    s0, s1, s2 = (box_sum(p, f).astype(np.float64) for p in full)
    cnt = box_sum(np.ones((h, w), np.int64), f).astype(np.float64)
    return tuple(((m[0] * s0 + m[1] * s1) + m[2] * s2) + m[3] * cnt for m in matrix(model, depth, f))


def g_quantised(ref, dist, model, depth=8):
    """-> g [hd, wd] int64 = rint(GCS 2^24), GCS in the device's order of operations"""
    lr, hr, mr = _channels_quantised(ref, model, depth)
    ld, hd, md = _channels_quantised(dist, model, depth)
    rx, ry = prewitt(lr)
    dx, dy = prewitt(ld)
    fx, fy = 0.5 * (rx + dx), 0.5 * (ry + dy)
    qr, qd, qf = rx * rx + ry * ry, dx * dx + dy * dy, fx * fx + fy * fy
    sim = lambda p, q, k: (2.0 * np.sqrt(p * q) + k) / ((p + q) + k)
    gs = (sim(qr, qd, C1) + sim(qd, qf, C2)) - sim(qr, qf, C2)
    cs = (2.0 * (hr * hd + mr * md) + C3) / (((hr * hr + hd * hd) + (mr * mr + md * md)) + C3)
    return np.rint((0.6 * gs + 0.4 * cs) * FIX_G).astype(np.int64)


def quarter_root(g):
    """zq = rint(sqrt(sqrt(|g| 2^-24)) 2^28) as int64"""
    return np.rint(np.sqrt(np.sqrt(np.abs(g).astype(np.float64) * (1.0 / FIX_G))) * FIX_Z).astype(np.int64)


def words_of(g):
    """the four words A, B, n_neg, D of a map of g"""
    g = np.asarray(g, np.int64).reshape(-1)
    zq, neg, n = quarter_root(g), g < 0, float(g.size)
    a, b = int(zq[~neg].sum()), int(zq[neg].sum())
    bi = float(b) * SQRT_HALF
    m_re, m_im = (float(a) + bi) / n, bi / n
    z = zq.astype(np.float64)
    re, im = np.where(neg, z * SQRT_HALF, z), np.where(neg, z * SQRT_HALF, 0.0)
    dr, di = re - m_re, im - m_im
    d = int(np.rint(np.sqrt(dr * dr + di * di)).astype(np.int64).sum())
    return a, b, int(neg.sum()), d


def pool_words(words, n):
    """the record's dev and mdsi from its four words (vqa_mdsi_wait's host formulas)"""
    dev = float(words[3]) / (float(n) * FIX_Z)
    return dev, math.sqrt(math.sqrt(dev))


def mdsi_quantised(ref, dist, model, depth=8):
    """-> (A, B, n_neg, D)"""
    return words_of(g_quantised(ref, dist, model, depth))


def derived_bar(gcs):
    """What may separate the integer pooling from the float pooling on THIS map: g = rint(GCS 2^24) moves a sample's GCS by at
    most 2^-25, hence its |GCS|^(1/4) by at most the change below (the quarter root is steep at 0, so this is no constant; at
    |GCS| < 2^-25 the whole value |GCS|^(1/4) + (2^-25)^(1/4) bounds it).  |z - mean z| is 1-Lipschitz in z and in the mean, and
    the mean moves by at most the mean of the changes: twice the mean per-sample change.  zq, the mean's use of it and the
    rounded deviation add at most 3 * 2^-29 per sample."""
    a, e = np.abs(np.asarray(gcs, np.float64)).reshape(-1), 2.0 ** -25
    change = np.maximum((a + e) ** 0.25 - a ** 0.25, a ** 0.25 - np.maximum(a - e, 0.0) ** 0.25)
    return 2.0 * float(change.mean()) + 3.0 * 2.0 ** -29
