#!/usr/bin/env python3
"""Third-party pins for MDSI's two linear stages: SciPy on seeded planes -> tests/golden/mdsi_pins.json.

TEST INFRASTRUCTURE: needs SciPy (the fixture was made with 1.15.3); nothing of this repository is imported.  Per factor f = 1..5

    box = scipy.signal.convolve2d(x, ones((f, f)), mode="full")[c:c + h, c:c + w][::f, ::f],  c = ceil((f - 1) / 2)

which is MATLAB's conv2(x, ones(f), 'same') kept at 1:f:end - 'same' takes the central part of the full result starting at
ceil((f - 1) / 2), which for an even kernel is NOT where SciPy's own mode="same" starts - as integer sums (the division by f^2 is
left to the reader), and on the f = 2 result

    gx = convolve2d(D, [[1, 0, -1]] * 3 / 3, mode="same"),  gy = convolve2d(D, [[1, 1, 1], [0, 0, 0], [-1, -1, -1]] / 3, mode="same")

(convolution flips the kernel: gx is right minus left, gy is bottom minus top; 'same' pads with zeros).  MDSI as a whole is not
pinned: no implementation of it was available.

    python scripts/gen_mdsi_pins.py
"""
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(REPO, "tests", "golden", "mdsi_pins.json")
SEED = 2016
SHAPE = (23, 31)      # odd both ways, not a multiple of 2, 3, 4 or 5; 24 and 32 would hide the cut last window
FACTORS = (1, 2, 3, 4, 5)


def make_plane():
    """-> the seeded int64 8-bit plane.  Importable by the tests."""
    return np.random.default_rng(SEED).integers(0, 256, SHAPE).astype(np.int64)


def main():
    import scipy
    from scipy.signal import convolve2d
    x = make_plane()
    h, w = x.shape
    out = {"versions": {"scipy": scipy.__version__, "numpy": np.__version__, "python": sys.version.split()[0]},
           "shape": list(SHAPE), "sum": int(x.sum()), "box": {}}
    for f in FACTORS:
        c = (f - 1 + 1) // 2
        full = convolve2d(x, np.ones((f, f), np.int64), mode="full")
        out["box"][str(f)] = full[c:c + h, c:c + w][::f, ::f].astype(np.int64).tolist()
    d = np.array(out["box"]["2"], np.float64) / 4.0
    kx = np.array([[1.0, 0.0, -1.0]] * 3) / 3.0
    out["gx"] = convolve2d(d, kx, mode="same").tolist()
    out["gy"] = convolve2d(d, kx.T, mode="same").tolist()
    with open(FIXTURE, "w") as fp:
        json.dump(out, fp, separators=(",", ":"))
        fp.write("\n")
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes")


if __name__ == "__main__":
    main()
