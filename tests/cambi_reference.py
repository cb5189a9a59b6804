"""CAMBI restated in NumPy from the text of include/vqa.h (vqa_cambi_submit), integers only: not from the kernels.  Box counts
come from integral images of one indicator plane per level, which is a different route from the kernels' window walk."""
import numpy as np

SCALES = 5
WINDOW = 65
WEIGHTS = (16, 8, 4, 2, 1)


def to10(x, depth):
    """step 1: raw samples -> 10 bits"""
    x = np.asarray(x).astype(np.int64)
    if depth < 10:
        return np.minimum(1023, x << (10 - depth))
    r = (1 << (depth - 11)) if depth > 10 else 0
    return np.minimum(1023, (x + r) >> (depth - 10))


def anti_dither(t):
    """step 2: the rounded 2x2 mean, indices clamped"""
    p = np.pad(t, ((0, 1), (0, 1)), mode="edge")
    return (p[:-1, :-1] + p[:-1, 1:] + p[1:, :-1] + p[1:, 1:] + 2) >> 2


def box_sum(a, radius):
    """the sum of `a` over the (2 radius + 1)^2 window centred on every sample, zeros outside the plane"""
    h, w = a.shape
    ii = np.zeros((h + 1, w + 1), np.int64)
    ii[1:, 1:] = a.astype(np.int64).cumsum(0).cumsum(1)
    y0 = np.maximum(np.arange(h) - radius, 0)
    y1 = np.minimum(np.arange(h) + radius, h - 1) + 1
    x0 = np.maximum(np.arange(w) - radius, 0)
    x1 = np.minimum(np.arange(w) + radius, w - 1) + 1
    return ii[y1][:, x1] - ii[y0][:, x1] - ii[y1][:, x0] + ii[y0][:, x0]


def mask0(y0):
    """step 3: Z, S and m0"""
    p = np.pad(y0, ((0, 1), (0, 1)), mode="edge")
    z = (p[:-1, :-1] == p[:-1, 1:]) & (p[:-1, :-1] == p[1:, :-1])
    return box_sum(z, 3) > 24


def round_u(num, den):
    """u = (num 2^17 + den) / (2 den) in integer division"""
    return (num * (1 << 17) + den) // (2 * den)


def contrast(y, m, detail=False):
    """step 5 for one scale: u [h, w] int64 (0 where m = 0); detail=True: also the k whose contrast is the largest (0 where u = 0;
    the smallest such k on a tie)"""
    r = WINDOW // 2
    area = box_sum(np.ones(y.shape, np.int64), r)
    levels = np.unique(y[m])
    need = np.unique((levels[:, None] + np.arange(-4, 5)[None, :]).ravel())
    counts = {int(v): box_sum(m & (y == v), r) for v in need if ((y == v) & m).any()}
    zero = np.zeros(y.shape, np.int64)
    u = np.zeros(y.shape, np.int64)
    best = np.zeros(y.shape, np.int64)
    for c in levels:
        here = m & (y == c)
        n0 = counts[int(c)]
        for k in (1, 2, 3, 4):
            for sign in (-1, 1):
                nk = counts.get(int(c) + sign * k, zero)
                v = round_u(k * n0 * nk, np.maximum((n0 + nk) * area, 1))
                better = here & (v > u)
                u[better] = v[better]
                best[better] = k
    return (u, best) if detail else u


def scales(plane, depth):
    """steps 1-4: [(y_s, m_s)] for s = 0..4"""
    y = anti_dither(to10(plane, depth))
    m = mask0(y)
    out = []
    for _ in range(SCALES):
        out.append((y, m))
        y, m = y[::2, ::2], m[::2, ::2]
    return out


def top_count(n):
    return max(1, (3 * n) // 10)


def cambi_words(plane, depth, detail=False):
    """-> {"top": [5], "k": [5], "masked": [5]} Python ints; detail=True: also "best" = per scale the set of winning k"""
    top, ks, masked, best = [], [], [], []
    for y, m in scales(plane, depth):
        u, b = contrast(y, m, detail=True)
        k = top_count(y.size)
        flat = np.sort(u.ravel())[::-1]
        top.append(int(flat[:k].sum()))
        ks.append(k)
        masked.append(int(m.sum()))
        best.append(set(int(v) for v in np.unique(b[u > 0])))
    out = {"top": top, "k": ks, "masked": masked}
    if detail:
        out["best"] = best
    return out


def pool_and_score(top, k):
    """steps 6-7 from the integer words, in double, in the order the header states"""
    pool = [float(t) / (float(kk) * 65536.0) for t, kk in zip(top, k)]
    s = 0.0
    for wgt, p in zip(WEIGHTS, pool):
        s = s + float(wgt) * p
    return pool, s / 31.0


def counts_at(y, m, i, j):
    """step 5 at one sample, by walking its window: (A, {d: n_d for d = -4..4})"""
    r = WINDOW // 2
    h, w = y.shape
    a, n = 0, {d: 0 for d in range(-4, 5)}
    for yy in range(max(i - r, 0), min(i + r, h - 1) + 1):
        for xx in range(max(j - r, 0), min(j + r, w - 1) + 1):
            a += 1
            d = int(y[yy, xx]) - int(y[i, j])
            if m[yy, xx] and -4 <= d <= 4:
                n[d] += 1
    return a, n
