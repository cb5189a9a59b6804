"""HaarPSI (Reisenhofer, Bosse, Kutyniok, Wiegand 2018) restated in NumPy from the definition in include/vqa.h, step by step:
the plain float64 form (true alpha, nothing rounded to integers) and the integer form the device uses (u = rint(2^30 sigmoid),
exact sums in Python integers, the host's quotient and logits).  Nothing of the package is imported: this file is the reference
the kernel is compared with."""
import math

import numpy as np

MIN_DIM = 16
FIX = 1 << 30
ALPHA = 4.2
C8 = 30.0
U1 = int(np.rint(FIX / (1.0 + math.exp(-ALPHA))))


def quad_sums(x):
    """S [ceil(h/2), ceil(w/2)] int64: the sum of the input quad at (2i, 2j), a sample outside the plane counting 0 (D = S / 4)"""
    x = np.asarray(x).astype(np.int64)
    h, w = x.shape
    p = np.zeros((h + (h & 1), w + (w & 1)), np.int64)
    p[:h, :w] = x
    return p[0::2, 0::2] + p[1::2, 0::2] + p[0::2, 1::2] + p[1::2, 1::2]


def haar(S):
    """-> H [2][3] int64 arrays of S's shape: H[o][s - 1] = H_s^o at every sample, S = 0 outside.  The window of scale s is rows
    and columns i - K/2 + 1 .. i + K/2, K = 2^s; o = 0 takes its upper rows minus its lower rows, o = 1 its left columns minus its
    right columns."""
    S = np.asarray(S, np.int64)
    h, w = S.shape
    p = np.zeros((h + 7, w + 7), np.int64)   # 3 before, 4 after
    p[3:3 + h, 3:3 + w] = S

    def at(a, b):   # S(i + a, j + b) for every (i, j)
        return p[3 + a:3 + a + h, 3 + b:3 + b + w]

    out = [[None] * 3, [None] * 3]
    for s in (1, 2, 3):
        half = (1 << s) // 2
        lo, hi = range(-half + 1, 1), range(1, half + 1)
        both = list(lo) + list(hi)
        out[0][s - 1] = sum(at(a, b) for a in lo for b in both) - sum(at(a, b) for a in hi for b in both)
        out[1][s - 1] = sum(at(a, b) for b in lo for a in both) - sum(at(a, b) for b in hi for a in both)
    return out


def constant(depth):
    """30 (k k), k = peak / 255: the paper's C on the scale of D"""
    k = ((1 << depth) - 1) / 255.0
    return C8 * (k * k)


def logit(x):
    return math.log(x / (1.0 - x))


def maps(r, d, depth=8):
    """-> (ls [2] float64 arrays, wI [2] int64 arrays) over the downsampled grid: the device's order of operations, which is
    also the plain formula (sim on H with c_s = 4^(s+2) C is the paper's sim on H / 2^(s+2) with C, scaled exactly)"""
    Hr, Hd = haar(quad_sums(r)), haar(quad_sums(d))
    c0 = constant(depth)
    ls, wi = [], []
    for o in (0, 1):
        sims = []
        for s in (1, 2):
            c = float(4 ** (s + 2)) * c0
            a, b = Hr[o][s - 1], Hd[o][s - 1]
            sims.append((2.0 * np.abs(a * b).astype(np.float64) + c) / ((a * a + b * b).astype(np.float64) + c))
        ls.append((sims[0] + sims[1]) * 0.5)
        wi.append(np.maximum(np.abs(Hr[o][2]), np.abs(Hd[o][2])))
    return ls, wi


def haarpsi(r, d, depth=8):
    """-> (haarpsi, similarity) of one plane pair in plain float64: true alpha, no rounding to integers.  All-zero planes (no
    weight anywhere) give (1.0, sigmoid(alpha))."""
    ls, wi = maps(r, d, depth)
    den = float(sum(int(w.sum()) for w in wi))
    if den == 0.0:
        return 1.0, 1.0 / (1.0 + math.exp(-ALPHA))
    num = sum(float(np.sum(w.astype(np.float64) / (1.0 + np.exp(-ALPHA * l)))) for l, w in zip(ls, wi))
    x = num / den   # (the paper's weight is wI / 32: the scale cancels)
    return (logit(x) / ALPHA) ** 2, x


def words(r, d, depth=8):
    """the three integer words of a pair: (den, num low, num high) - as ONE split of the total (the device splits per thread;
    hi 2^32 + lo is the same integer)"""
    ls, wi = maps(r, d, depth)
    den = num = 0
    for l, w in zip(ls, wi):
        u = np.rint(FIX / (1.0 + np.exp(-ALPHA * l))).astype(np.int64)
        u[l == 1.0] = U1
        den += int(w.sum())
        num += sum(int(a) * int(b) for a, b in zip(u.reshape(-1), w.reshape(-1)))
    return den, num & 0xffffffff, num >> 32


def pool_words(den, lo, hi):
    """the host's formulas of include/vqa.h on the three words: -> (haarpsi, similarity)"""
    x1 = U1 / FIX
    if den == 0:
        return 1.0, x1
    q, rem = divmod((hi << 32) + lo, den)
    x = (float(q) + float(rem) / float(den)) / FIX
    t = logit(x) / logit(x1)
    return t * t, x


def haarpsi_fixed(r, d, depth=8):
    """-> (haarpsi, similarity, (den, num)) through the integer form"""
    den, lo, hi = words(r, d, depth)
    a, b = pool_words(den, lo, hi)
    return a, b, (den, (hi << 32) + lo)
