#!/usr/bin/env python3
"""Third-party pins for the artefact measures: SciPy's convolve2d and uniform_filter1d on seeded planes ->
tests/golden/artifacts_pins.json.

TEST INFRASTRUCTURE.  Needs SciPy (1.15.3 wrote the committed fixture).  Per plane, in plain float64:

    lap     = sum |convolve2d(x, [[1, -2, 1], [-2, 4, -2], [1, -2, 1]], mode="valid")|        (integers: exact)
    B       = uniform_filter1d(x, size=9, axis, mode="nearest"): the 9-tap mean, used only where the window lies inside
    dF, dB  = |x(i) - x(i - 1)|, |B(i) - B(i - 1)| on i = 5 .. n - 5 along the axis;  V = max(0, dF - dB)
    blur    = (sum dF - sum V) / sum dF                                                        per direction
    mean9   = B on its inside positions, as a list (the restatement's window sums / 9 are held against it)

The fixture pins the restatement of tests/artifacts_reference.py - the Laplacian's taps and domain, the 9-tap window, the blur
domain and the telescoped difference - against an independent convolution and an independent mean filter that really blurs.

    python scripts/gen_artifacts_pins.py
"""
import json
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(REPO, "tests", "golden", "artifacts_pins.json")
SEED = 1996
CASES = ((16, 16, 8), (17, 25, 8), (23, 37, 10), (24, 20, 16))   # h, w, depth


def make_planes():
    """-> list of (plane int64 [h, w], depth): a sinusoid texture with noise on it, the last one plain noise.  Importable by the
    tests."""
    rng = np.random.default_rng(SEED)
    out = []
    for k, (h, w, depth) in enumerate(CASES):
        peak = (1 << depth) - 1
        y, x = np.mgrid[0:h, 0:w]
        if k == len(CASES) - 1:
            p = rng.integers(0, peak + 1, (h, w))
        else:
            p = np.clip(np.rint(peak * (0.45 + 0.35 * np.sin(x / 3.0 + k) * np.cos(y / 4.0)) + rng.integers(-peak // 16, peak // 16 + 1, (h, w))), 0, peak)
        out.append((p.astype(np.int64), depth))
    return out


def blur_along(x, axis):
    from scipy.ndimage import uniform_filter1d
    x = np.moveaxis(x.astype(np.float64), axis, 0)
    b = uniform_filter1d(x, size=9, axis=0, mode="nearest")
    n = x.shape[0]
    i = np.arange(5, n - 4)
    df = np.abs(x[i] - x[i - 1])
    db = np.abs(b[i] - b[i - 1])
    v = np.maximum(0.0, df - db)
    return float((df.sum() - v.sum()) / df.sum()), np.moveaxis(b[4:n - 4], 0, axis)


def main():
    import scipy
    from scipy.signal import convolve2d
    kern = np.array([[1, -2, 1], [-2, 4, -2], [1, -2, 1]], np.float64)
    pins = []
    for p, depth in make_planes():
        blur_v, mean_v = blur_along(p, 0)
        blur_h, mean_h = blur_along(p, 1)
        pins.append({"h": int(p.shape[0]), "w": int(p.shape[1]), "depth": depth, "plane": p.reshape(-1).tolist(),
                     "lap": float(np.abs(convolve2d(p.astype(np.float64), kern, mode="valid")).sum()),
                     "blur_h": blur_h, "blur_v": blur_v, "mean9_h": mean_h.reshape(-1).tolist(), "mean9_v": mean_v.reshape(-1).tolist()})
    with open(FIXTURE, "w") as f:
        json.dump({"scipy": scipy.__version__, "seed": SEED, "pins": pins}, f, separators=(",", ":"))
    print("wrote", FIXTURE, [(round(q["blur_h"], 6), round(q["blur_v"], 6), q["lap"]) for q in pins])


if __name__ == "__main__":
    main()
