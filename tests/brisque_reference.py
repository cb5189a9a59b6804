"""A NumPy restatement of BRISQUE's features as include/vqa.h defines them (vqa_brisque_submit), written from that text alone:
once in float64 (the definition: no rounding of the field) and once in integers (u = rint(m 2^16), pairs classed by the sign of
the exact product) as the library forms its 60 words.  tests/test_brisque_host.py pins the float64 one against SciPy, torch and
closed forms; tests/test_gpu_brisque.py holds the library against both.

The bars (derived in the header's "Accuracy"; D = 2^-17 is what the one rounding can move m by, E_M what the device's double
moments may differ from this file's by, B = D + E_M, M = 2.742 the bound of |m|).  Per sample m moves by at most B, m^2 by
2 |m| B + B^2; per pair p moves by (|m_a| + |m_b|) B + B^2 and the rounding of |p| adds D, p^2 moves by 2 |p| dp + dp^2.
Summed over a field, with E = mean |m| and A = mean |p| of the float64 restatement (never of the library):
    mean |m|                 B                                  = BAR_ABS_M
    mean m^2                 2 E B + B^2                        <= 2 M B + B^2          = BAR_M2
    mean |p| (all pairs)     2 E B + B^2 + D                    <= (2 M + 1) B + B^2    = BAR_ABS_P
    sum p^2 / N per class    2 A BAR_ABS_P + BAR_ABS_P^2        <= 2 M^2 BAR_ABS_P + ..  = BAR_P2;  a pair changes class only
                             if one of its two m is within B of zero, and then |p| < M B: its square is below BAR_ABS_P^2
    n_neg, n_pos             the number of pairs with min(|m_a|, |m_b|) <= B, counted on the float64 field
The first three never exceed 1e-4."""
import math

import numpy as np

Q = 16
D = 2.0 ** -(Q + 1)
E_M = 2e-9            # 2.742 * 64 ulp(65535^2) / (2 * 257^2) = 1.2e-9 at 16 bits, less below: the moments' own error on m
M_MAX = 2.742
BAR_ABS_M = D + E_M
BAR_M2 = 2 * M_MAX * BAR_ABS_M + BAR_ABS_M ** 2
BAR_ABS_P = (2 * M_MAX + 1) * BAR_ABS_M + BAR_ABS_M ** 2
BAR_P2 = 2 * M_MAX * M_MAX * BAR_ABS_P + BAR_ABS_P ** 2
assert max(BAR_ABS_M, BAR_M2, BAR_ABS_P) <= 1e-4



def bar_m2(abs_m):
    return min(BAR_M2, 2 * abs_m * BAR_ABS_M + BAR_ABS_M ** 2)


def bar_abs_p(abs_m):
    return min(BAR_ABS_P, 2 * abs_m * BAR_ABS_M + BAR_ABS_M ** 2 + D)


def bar_p2(abs_p):
    return min(BAR_P2, 2 * abs_p * BAR_ABS_P + BAR_ABS_P ** 2)


GRID_N = 9801
GAM = (200 + np.arange(GRID_N)) / 1000.0
ORIENTATIONS = ("H", "V", "D1", "D2")
WORD_KEYS = ("n_neg", "n_pos", "sum_abs_p", "sq_neg_lo", "sq_neg_hi", "sq_pos_lo", "sq_pos_hi")
TAPS = np.array([-3, -9, 29, 111, 111, 29, -9, -3], np.int64)


def gamma_ratio(g):
    """G(1/g) G(3/g) / G(2/g)^2"""
    return math.exp(math.lgamma(1.0 / g) + math.lgamma(3.0 / g) - 2.0 * math.lgamma(2.0 / g))


_TAB = {}


def tables():
    if not _TAB:
        _TAB["r"] = np.array([gamma_ratio(g) for g in GAM])
        _TAB["inv"] = np.array([math.exp(2.0 * math.lgamma(2.0 / g) - math.lgamma(1.0 / g) - math.lgamma(3.0 / g)) for g in GAM])
    return _TAB["r"], _TAB["inv"]


def window():
    k = np.arange(-3, 4, dtype=np.float64)
    g = np.exp(-k * k / (2.0 * (7.0 / 6.0) ** 2))
    w = np.outer(g, g)
    return w / w.sum()


def moments(x):
    """sum w x and sum w x^2 with zero outside the plane -> (mu, sxx)"""
    x = np.asarray(x, np.float64)
    h, w = x.shape
    win = window()
    p1 = np.zeros((h + 6, w + 6))
    p1[3:-3, 3:-3] = x
    p2 = p1 * p1
    mu, sxx = np.zeros((h, w)), np.zeros((h, w))
    for a in range(7):
        for b in range(7):
            mu += win[a, b] * p1[a:a + h, b:b + w]
            sxx += win[a, b] * p2[a:a + h, b:b + w]
    return mu, sxx


def mscn(x, depth):
    c = ((1 << depth) - 1) / 255.0
    x = np.asarray(x, np.float64)
    mu, sxx = moments(x)
    return (x - mu) / (np.sqrt(np.abs(sxx - mu * mu)) + c)


def _mirror(i, n):
    m = np.mod(i, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def half_int(x):
    """65536 half(x), exact, int64"""
    x = np.asarray(x).astype(np.int64)
    for axis in (0, 1):
        n = x.shape[axis]
        o = np.arange((n + 1) // 2)
        acc = 0
        for k in range(8):
            acc = acc + TAPS[k] * np.take(x, _mirror(2 * o - 3 + k, n), axis=axis)
        x = acc
    return x


def half(x):
    return half_int(x) / 65536.0


def shifted(m):
    """the four partners of every sample, with wrap-around: H, V, D1, D2"""
    up, dn = np.roll(m, 1, axis=0), np.roll(m, -1, axis=0)
    return [np.roll(m, 1, axis=1), up, np.roll(up, 1, axis=1), np.roll(dn, 1, axis=1)]


def scales(x, depth):
    """the two sample fields in float64"""
    return [np.asarray(x, np.float64), half(x)]


# ---- float64: the definition --------------------------------------------------------------------------------------------
def float_moments(x, depth):
    """per scale: dict(n, abs_m, m2, and per orientation n_neg, n_pos, abs_p, sq_neg, sq_pos (sums over N), near (the pairs one
    of whose m is within D + E_M of zero)), m itself"""
    out = []
    for xs in scales(x, depth):
        m = mscn(xs, depth)
        n = m.size
        d = dict(n=n, m=m, abs_m=np.abs(m).mean(), m2=(m * m).mean(), o=[])
        for b in shifted(m):
            p = m * b
            d["o"].append(dict(n_neg=int((p < 0).sum()), n_pos=int((p > 0).sum()), abs_p=np.abs(p).sum() / n,
                               sq_neg=(p[p < 0] ** 2).sum() / n, sq_pos=(p[p > 0] ** 2).sum() / n,
                               near=int((np.minimum(np.abs(m), np.abs(b)) <= BAR_ABS_M).sum())))
        out.append(d)
    return out


def fit_ggd(sigma2, e):
    """-> (alpha, grid index)"""
    r, _ = tables()
    rho = sigma2 / (e * e)
    k = int(np.argmin(np.abs(rho - r)))
    return (200 + k) / 1000.0, k


def aggd_rn(n, n_neg, n_pos, abs_p, sq_neg, sq_pos):
    """sums over N -> (l, r, rn)"""
    l, r = math.sqrt(sq_neg * n / n_neg), math.sqrt(sq_pos * n / n_pos)
    gh = l / r
    rhat = abs_p * abs_p / (sq_neg + sq_pos)
    return l, r, rhat * (gh ** 3 + 1.0) * (gh + 1.0) / (gh * gh + 1.0) ** 2


def fit_rn(rn):
    _, inv = tables()
    k = int(np.argmin((inv - rn) ** 2))
    return (200 + k) / 1000.0, k


def aggd_mean(l, r, al):
    l1, l2, l3 = math.lgamma(1.0 / al), math.lgamma(2.0 / al), math.lgamma(3.0 / al)
    return (r - l) * math.exp(l2 - l1) * math.exp(0.5 * (l1 - l3))


def float_features(x, depth):
    """-> (features [36], flags, grid indices [10] (-1 where degenerate))"""
    ft, flags, ks = np.zeros(36), 0, []
    for s, d in enumerate(float_moments(x, depth)):
        if d["abs_m"] == 0:
            flags |= 1 << (5 * s)
            ks.append(-1)
        else:
            ft[18 * s], k = fit_ggd(d["m2"], d["abs_m"])
            ft[18 * s + 1] = d["m2"]
            ks.append(k)
        for o, q in enumerate(d["o"]):
            if q["n_neg"] == 0 or q["n_pos"] == 0 or q["sq_pos"] == 0:
                flags |= 1 << (5 * s + 1 + o)
                ks.append(-1)
                continue
            l, r, rn = aggd_rn(d["n"], q["n_neg"], q["n_pos"], q["abs_p"], q["sq_neg"], q["sq_pos"])
            al, k = fit_rn(rn)
            ft[18 * s + 2 + 4 * o: 18 * s + 6 + 4 * o] = (al, aggd_mean(l, r, al), l * l, r * r)
            ks.append(k)
    return ft, flags, ks


# ---- integers: what the library's words are -------------------------------------------------------------------------------
def quantise(m):
    return np.rint(m * float(1 << Q)).astype(np.int64)


def words_of_u(u):
    """the 30 words of one scale from its integer field"""
    w = dict(sum_abs_u=int(np.abs(u).sum()), sum_u2=int((u * u).sum()))
    for k in WORD_KEYS:
        w[k] = []
    for b in shifted(u):
        e = u * b
        mag = (np.abs(e) + (1 << (Q - 1))) >> Q
        sq = mag * mag
        neg, pos = e < 0, e > 0
        w["n_neg"].append(int(neg.sum()))
        w["n_pos"].append(int(pos.sum()))
        w["sum_abs_p"].append(int(mag[neg | pos].sum()))
        w["sq_neg_lo"].append(int((sq[neg] & 0xffffffff).sum()))
        w["sq_neg_hi"].append(int((sq[neg] >> 32).sum()))
        w["sq_pos_lo"].append(int((sq[pos] & 0xffffffff).sum()))
        w["sq_pos_hi"].append(int((sq[pos] >> 32).sum()))
    return w


def words(x, depth):
    """[scale] -> the words, from this file's float64 m"""
    return [words_of_u(quantise(mscn(xs, depth))) for xs in scales(x, depth)]


def record_words(rec):
    """a BRISQUE_DTYPE record -> [scale] -> the words as Python integers"""
    out = []
    for s in range(2):
        w = dict(sum_abs_u=int(rec["sum_abs_u"][s]), sum_u2=int(rec["sum_u2"][s]))
        for k in WORD_KEYS:
            w[k] = [int(v) for v in rec[k][s]]
        out.append(w)
    return out


def scale_sizes(h, w):
    return [h * w, ((h + 1) // 2) * ((w + 1) // 2)]


def word_moments(ws, h, w):
    """the words -> the moments in the float restatement's units: [scale] dict(abs_m, m2, o=[dict(n_neg, n_pos, abs_p, sq_neg,
    sq_pos)])"""
    out = []
    q1 = float(1 << Q)
    q2 = q1 * q1
    for s, n in enumerate(scale_sizes(h, w)):
        x = ws[s]
        d = dict(n=n, abs_m=x["sum_abs_u"] / q1 / n, m2=x["sum_u2"] / q2 / n, o=[])
        for o in range(4):
            sn = float((x["sq_neg_hi"][o] << 32) + x["sq_neg_lo"][o])
            sp = float((x["sq_pos_hi"][o] << 32) + x["sq_pos_lo"][o])
            d["o"].append(dict(n_neg=x["n_neg"][o], n_pos=x["n_pos"][o], abs_p=x["sum_abs_p"][o] / q1 / n,
                               sq_neg=sn / q2 / n, sq_pos=sp / q2 / n))
        out.append(d)
    return out


def word_features(ws, h, w):
    """the host's part of include/vqa.h, in its order of operations: the words -> (features [36], flags, grid indices [10])"""
    ft, flags, ks = np.zeros(36), 0, []
    q1 = float(1 << Q)
    q2 = q1 * q1
    r_tab, inv_tab = tables()
    for s, n in enumerate(scale_sizes(h, w)):
        x = ws[s]
        cnt = float(n)
        if x["sum_abs_u"] == 0:
            flags |= 1 << (5 * s)
            ks.append(-1)
        else:
            sigma2, e = float(x["sum_u2"]) / q2 / cnt, float(x["sum_abs_u"]) / q1 / cnt
            k = int(np.argmin(np.abs(sigma2 / (e * e) - r_tab)))
            ft[18 * s], ft[18 * s + 1] = (200 + k) / 1000.0, sigma2
            ks.append(k)
        for o in range(4):
            sn = float((x["sq_neg_hi"][o] << 32) + x["sq_neg_lo"][o])
            sp = float((x["sq_pos_hi"][o] << 32) + x["sq_pos_lo"][o])
            if x["n_neg"][o] == 0 or x["n_pos"][o] == 0 or sp == 0.0:
                flags |= 1 << (5 * s + 1 + o)
                ks.append(-1)
                continue
            l, r = math.sqrt(sn / q2 / float(x["n_neg"][o])), math.sqrt(sp / q2 / float(x["n_pos"][o]))
            gh = l / r
            ea = float(x["sum_abs_p"][o]) / q1 / cnt
            e2 = float(((x["sq_neg_hi"][o] + x["sq_pos_hi"][o]) << 32) + x["sq_neg_lo"][o] + x["sq_pos_lo"][o]) / q2 / cnt
            rhat = ea * ea / e2
            g2 = gh * gh
            rn = rhat * (g2 * gh + 1.0) * (gh + 1.0) / ((g2 + 1.0) * (g2 + 1.0))
            k = int(np.argmin((inv_tab - rn) * (inv_tab - rn)))
            al = (200 + k) / 1000.0
            ft[18 * s + 2 + 4 * o: 18 * s + 6 + 4 * o] = (al, aggd_mean(l, r, al), l * l, r * r)
            ks.append(k)
    return ft, flags, ks


# ---- the admission rule ---------------------------------------------------------------------------------------------------
def alpha_spans(x, depth):
    """per fit (10): how many grid steps alpha moves at most when every moment of the float64 restatement moves by its bar
    (every corner of the box is tried; the ratios are monotone in each moment between corners).  None for a degenerate fit."""
    spans = []
    for d in float_moments(x, depth):
        if d["abs_m"] == 0:
            spans.append(None)
        else:
            k0 = fit_ggd(d["m2"], d["abs_m"])[1]
            ks = [fit_ggd(max(d["m2"] + a * bar_m2(d["abs_m"]), 1e-300), max(d["abs_m"] + b * BAR_ABS_M, 1e-300))[1]
                  for a in (-1, 1) for b in (-1, 1)]
            spans.append(max(abs(k - k0) for k in ks))
        for q in d["o"]:
            if q["n_neg"] == 0 or q["n_pos"] == 0 or q["sq_pos"] == 0:
                spans.append(None)
                continue
            k0 = fit_rn(aggd_rn(d["n"], q["n_neg"], q["n_pos"], q["abs_p"], q["sq_neg"], q["sq_pos"])[2])[1]
            worst = 0
            for a in (-1, 1):
                for b in (-1, 1):
                    for c in (-1, 1):
                        for e in (-1, 1):
                            for f in (-1, 1):
                                nn, npos = q["n_neg"] + a * q["near"], q["n_pos"] + b * q["near"]
                                sn, sp = q["sq_neg"] + c * bar_p2(q["abs_p"]), q["sq_pos"] + e * bar_p2(q["abs_p"])
                                if nn <= 0 or npos <= 0 or sn <= 0 or sp <= 0:
                                    worst = GRID_N
                                    continue
                                rn = aggd_rn(d["n"], nn, npos, max(q["abs_p"] + f * bar_abs_p(d["abs_m"]), 0.0), sn, sp)[2]
                                worst = max(worst, abs(fit_rn(rn)[1] - k0))
            spans.append(worst)
    return spans


def admitted(x, depth, steps=2):
    return all(s is not None and s <= steps for s in alpha_spans(x, depth))
