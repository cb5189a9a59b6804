#!/usr/bin/env python3
"""Third-party pins for HaarPSI: SciPy's convolve2d on seeded 8-bit planes -> tests/golden/haarpsi_pins.json.

TEST INFRASTRUCTURE.  Needs SciPy (1.15.3 wrote the committed fixture).  Per pair, in plain float64 with the true alpha = 4.2 and
nothing rounded to integers:

    D      = convolve2d(x, ones(2, 2) / 4, mode="full") sliced at ceil((K - 1) / 2) = 1, then [0::2, 0::2]
    coeffs = convolve2d(D, haar_s, mode="full") sliced at ceil((K - 1) / 2), K = 2^s, for s = 1, 2, 3, where haar_s is
             2^-s ones(K, K) with its upper half negated, and its transpose
    sim    = (2 |c_r c_d| + 30) / (c_r^2 + c_d^2 + 30) at s = 1, 2;  ls = their mean;  w = max(|c_r|, |c_d|) at s = 3
    x      = sum sigmoid(4.2 ls) w / sum w over both orientations;  haarpsi = (log(x / (1 - x)) / 4.2)^2

The slice start ceil((K - 1) / 2) of the FULL convolution is MATLAB's conv2(.., 'same') for an even kernel: output i reads
inputs i - K/2 + 1 .. i + K/2.  (SciPy's own mode="same" starts one sample earlier, which is why it is not used.)  The fixture
pins the restatement of tests/haarpsi_reference.py - windows, zero border, constants, pooling - against an independent
convolution; it does not pin anything against the authors' files, which were not at hand.

    python scripts/gen_haarpsi_pins.py
"""
import json
import math
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(REPO, "tests", "golden", "haarpsi_pins.json")
SEED = 2018
SHAPES = ((24, 40), (24, 40), (16, 16), (25, 39), (32, 18), (24, 40))   # one of them odd both ways
ALPHA, C = 4.2, 30.0


def make_pairs():
    """-> list of (r, d) int64 8-bit planes: noisy copies, unrelated noise, a blurred and a posterised copy.  Importable by the
    tests."""
    rng = np.random.default_rng(SEED)
    out = []
    for k, (h, w) in enumerate(SHAPES):
        y, x = np.mgrid[0:h, 0:w]
        r = np.clip(np.rint(110 + 90 * np.sin(x / 5.0 + k) * np.cos(y / 4.0) + rng.integers(-20, 21, (h, w))), 0, 255).astype(np.int64)
        if k == 1:
            d = rng.integers(0, 256, (h, w)).astype(np.int64)
        elif k == 4:
            d = (r // 32) * 32 + 16
        else:
            d = np.clip(r + rng.integers(-6 * (k + 1), 6 * (k + 1) + 1, (h, w)), 0, 255).astype(np.int64)
        out.append((r, d))
    return out


def same(x, kern):
    """MATLAB's conv2(x, kern, 'same') for a square kernel of even size K, from SciPy's full convolution"""
    from scipy.signal import convolve2d
    k = kern.shape[0]
    s = math.ceil((k - 1) / 2)
    full = convolve2d(x, kern, mode="full")
    return full[s:s + x.shape[0], s:s + x.shape[1]]


def haarpsi(r, d):
    def coeffs(x):
        D = same(x.astype(np.float64), np.ones((2, 2)) / 4.0)[0::2, 0::2]
        out = []
        for s in (1, 2, 3):
            k = 1 << s
            f = np.ones((k, k)) / k
            f[:k // 2, :] = -f[:k // 2, :]
            out.append((same(D, f), same(D, f.T)))
        return out
    cr, cd = coeffs(r), coeffs(d)
    num = den = 0.0
    for o in (0, 1):
        sims = [(2.0 * np.abs(cr[s][o] * cd[s][o]) + C) / (cr[s][o] ** 2 + cd[s][o] ** 2 + C) for s in (0, 1)]
        ls = (sims[0] + sims[1]) / 2.0
        w = np.maximum(np.abs(cr[2][o]), np.abs(cd[2][o]))
        num += float(np.sum(w / (1.0 + np.exp(-ALPHA * ls))))
        den += float(np.sum(w))
    x = num / den
    return (math.log(x / (1.0 - x)) / ALPHA) ** 2, x


def main():
    import scipy
    pins = []
    for r, d in make_pairs():
        v, x = haarpsi(r, d)
        pins.append({"h": int(r.shape[0]), "w": int(r.shape[1]), "ref": r.reshape(-1).tolist(), "dist": d.reshape(-1).tolist(),
                     "haarpsi": v, "similarity": x})
    with open(FIXTURE, "w") as f:
        json.dump({"scipy": scipy.__version__, "seed": SEED, "alpha": ALPHA, "C": C, "pins": pins}, f, separators=(",", ":"))
    print("wrote", FIXTURE, [round(p["haarpsi"], 6) for p in pins])


if __name__ == "__main__":
    main()
