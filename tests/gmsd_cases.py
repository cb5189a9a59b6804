"""The shapes and contents of the GMSD parity matrix, shared by tests/test_gmsd_host.py (what does the float64 restatement and
its integer form give on them?) and tests/test_gpu_gmsd.py (the GPU against the restatement), so that both see the same samples.
Integer-only and seeded.

Shapes (h, w), the smallest at which the kernel can still go wrong: the minimum 16 x 16; 33 x 67, both odd, so that the last row
and column of the 2x2 stage are half-weight sums; 67 x 130, whose downsampled grid of 34 x 65 lies two rows past the horizontal
and one column past the vertical seam of the kernel's 64 x 32 tile (four workgroups, three of them nearly empty)."""
import numpy as np

SHAPES = ((16, 16), (33, 67), (67, 130))
DEPTHS = (8, 10, 16)
CONTENTS = ("natural", "noise", "identical", "ends", "flat_peak")
YUV_SHAPE = (135, 241)            # 4:2:0 with odd chroma (68 x 121): three planes, two geometry groups
BAR = 2.0 ** -24                  # gmsd and gms_mean against the unquantised float64 restatement (derived in test_gpu_gmsd.py)


def pair(name, h, w, depth, seed=0):
    """-> (r, d) int64 [h, w] planes of `depth` bits"""
    rng = np.random.default_rng(1000 * h + w + 7 * depth + seed)
    peak = (1 << depth) - 1
    if name == "natural":        # a smooth gradient with a few edges, and +-12 levels (8-bit scale) of noise on the copy
        y, x = np.mgrid[0:h, 0:w]
        base = 40.0 + 150.0 * (0.5 + 0.5 * np.sin(x / 9.0) * np.cos(y / 7.0)) + 30.0 * ((x // 11 + y // 13) % 2)
        r = np.rint(base * peak / 255.0).astype(np.int64)
        d = r + np.rint(rng.integers(-12, 13, (h, w)) * (peak / 255.0)).astype(np.int64)
        return np.clip(r, 0, peak), np.clip(d, 0, peak)
    if name == "noise":          # unrelated uniform noise over the full range
        return rng.integers(0, peak + 1, (h, w)).astype(np.int64), rng.integers(0, peak + 1, (h, w)).astype(np.int64)
    if name == "identical":
        r = rng.integers(0, peak + 1, (h, w)).astype(np.int64)
        return r, r.copy()
    if name == "ends":           # flat 0 against the flat maximum: only the border ring departs from 1
        return np.zeros((h, w), np.int64), np.full((h, w), peak, np.int64)
    if name == "flat_peak":
        return np.full((h, w), peak, np.int64), np.full((h, w), peak, np.int64)
    raise KeyError(name)


def matrix():
    """(content, shape, depth): every content on every shape at 8 bits, and every content at every depth on 33 x 67"""
    out = [(c, s, 8) for c in CONTENTS for s in SHAPES]
    out += [(c, (33, 67), dp) for c in CONTENTS for dp in DEPTHS if dp != 8]
    return out


def dtype_of(depth):
    return np.uint16 if depth > 8 else np.uint8
