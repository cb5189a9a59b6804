"""The shapes and contents of the HaarPSI parity matrix, shared by tests/test_haarpsi_host.py (what do the float64 restatement
and its integer form give on them?) and the GPU tests (the GPU against the restatement), so that both see the same samples.
Integer-only and seeded.

Shapes (h, w), the smallest at which the kernel can still go wrong: the minimum 16 x 16, whose 8 x 8 grid holds one whole
8-window and whose every apron sample is zero; 33 x 47, odd both ways (half-weight last row and column, one partial tile);
135 x 241, whose grid of 68 x 121 is 3 x 2 tiles of 64 x 32 with partial last tiles, so that windows cross tile seams both ways."""
import numpy as np

SHAPES = ((16, 16), (33, 47), (135, 241))
DEPTHS = (8, 10, 16)
CONTENTS = ("natural", "noise", "identical", "posterised")
HOSTILE = ("flat_zero", "flat_peak", "ends", "anti", "anti_noise", "step")
YUV_SHAPE = (135, 241)            # 4:2:0 with odd chroma (68 x 121): three planes, two geometry groups
BAR = 4e-8                        # haarpsi and similarity against the unquantised float64 restatement (derived in include/vqa.h)


def pair(name, h, w, depth, seed=0):
    """-> (r, d) int64 [h, w] planes of `depth` bits"""
    rng = np.random.default_rng(1000 * h + w + 7 * depth + seed)
    peak = (1 << depth) - 1
    y, x = np.mgrid[0:h, 0:w]
    smooth = 40.0 + 150.0 * (0.5 + 0.5 * np.sin(x / 9.0) * np.cos(y / 7.0))
    if name == "natural":        # a smooth field with a few edges, and +-12 levels (8-bit scale) of noise on the copy
        base = smooth + 30.0 * ((x // 11 + y // 13) % 2)
        r = np.rint(base * peak / 255.0).astype(np.int64)
        d = r + np.rint(rng.integers(-12, 13, (h, w)) * (peak / 255.0)).astype(np.int64)
        return np.clip(r, 0, peak), np.clip(d, 0, peak)
    if name == "noise":          # unrelated uniform noise over the full range
        return rng.integers(0, peak + 1, (h, w)).astype(np.int64), rng.integers(0, peak + 1, (h, w)).astype(np.int64)
    if name == "identical":
        r = rng.integers(0, peak + 1, (h, w)).astype(np.int64)
        return r, r.copy()
    if name == "posterised":     # a smooth field against its copy cut to 8 levels
        r = np.rint(smooth * peak / 255.0).astype(np.int64)
        q = (peak + 1) // 8
        return r, np.clip((r // q) * q + q // 2, 0, peak)
    if name == "flat_zero":
        return np.zeros((h, w), np.int64), np.zeros((h, w), np.int64)
    if name == "flat_peak":
        return np.full((h, w), peak, np.int64), np.full((h, w), peak, np.int64)
    if name == "ends":           # flat 0 against the flat maximum: weight on the border ring only
        return np.zeros((h, w), np.int64), np.full((h, w), peak, np.int64)
    if name == "anti":           # a checkerboard of 4 x 4 blocks at the range ends against its inverse
        r = ((x // 4 + y // 4) % 2).astype(np.int64) * peak
        return r, peak - r
    if name == "anti_noise":     # full-range noise against its inverse
        r = rng.integers(0, peak + 1, (h, w)).astype(np.int64)
        return r, peak - r
    if name == "step":           # one level: a flat field against a copy whose right half is one level higher
        r = np.full((h, w), peak // 2, np.int64)
        d = r.copy()
        d[:, w // 2:] += 1
        return r, d
    raise KeyError(name)


def matrix():
    """(content, shape, depth): every content on every shape at 8 bits, and every content at 10 and 16 bits on 33 x 47"""
    out = [(c, s, 8) for c in CONTENTS for s in SHAPES]
    out += [(c, (33, 47), dp) for c in CONTENTS for dp in DEPTHS if dp != 8]
    return out


def hostile_matrix():
    """(content, shape, depth): every hostile content on 33 x 47 at every depth, and on 135 x 241 at 8 bits"""
    return [(c, (33, 47), dp) for c in HOSTILE for dp in DEPTHS] + [(c, (135, 241), 8) for c in HOSTILE]


def dtype_of(depth):
    return np.uint16 if depth > 8 else np.uint8
