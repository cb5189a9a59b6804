"""The shapes and contents of the CAMBI parity matrix, shared by tests/test_cambi_host.py (what does the restatement give on
them, and is the matrix not vacuous?) and tests/test_gpu_cambi.py (the GPU against the restatement), so that both see the same
samples.  Integer-only and seeded.

Shapes (h, w), the smallest at which the kernels can still go wrong: the minimum 16 x 16, where every window is clipped on all
sides and scale 4 is 1 x 1; 41 x 71, both odd, so that decimation rounds up, the 65-wide window is clipped in height everywhere
and covers the full width only at columns 32 to 38; 67 x 131, which crosses the seam of k_cambi_contrast's 32 x 32 tile
(CAMBI_TILE) by 3 samples in both directions at scale 0 (67 = 64 + 3, 131 = 128 + 3) and still has a seam at scale 1 (34 x 66:
2 past either way).  The mask kernel's 64 x 16 tile is crossed by the same shape (131 = 128 + 3, 67 = 64 + 3)."""
import numpy as np

SHAPES = ((16, 16), (41, 71), (67, 131))
DEPTHS = (8, 10, 12, 16)
BANDED = ("staircase", "dither", "halves", "top_ramp")       # contents that must score: the host test says how much
ZERO = ("flat", "noise", "flat_zero", "flat_peak")          # contents whose every word but k is 0
CONTENTS = BANDED + ZERO
YUV_SHAPE = (135, 241)            # 4:2:0 with odd chroma (68 x 121): three planes, two geometry groups
BGR_SHAPE = (33, 67)              # packed bgr24: pixel step 3


def band_width(w):
    """the staircase's band: at least 6 columns, so that more than 24 of a 7 x 7 window's samples have equal neighbours"""
    return max(6, w // 11)


def ramp10(h, w, base, dither=None):
    """a staircase in 10-bit levels: vertical bands whose steps cycle through 1, 2, 3, 4, 5 (1, 4 on a plane too narrow for
    six bands); the lower half is shifted by
    five columns, so that band ends meet tile seams at different places"""
    bw = band_width(w)
    steps = np.array([1, 2, 3, 4, 5] if w // bw >= 6 else [1, 4])   # (a 16-wide plane holds three bands: v, v + 1, v + 5)
    level = np.concatenate([[0], np.cumsum(steps[np.arange(w // bw + 2) % len(steps)])])
    x = np.arange(w)
    rows = np.where(np.arange(h)[:, None] < h // 2, x[None, :], x[None, :] + 5)
    t = base + level[rows // bw]
    if dither is not None:
        t = t + dither
    return t


def ramp8(h, w, base):
    """the staircase at 8 bits, in 8-bit levels: one level is four 10-bit levels, so a 1-level step is a contrast of k = 4 and
    anything larger is out of reach.  The steps cycle through 1, 3, 3: every third band has no band within reach, and what a
    sample of it scores comes from the single samples laid over it (dots, dither)."""
    bw = band_width(w)
    steps = np.array([1, 3, 3])
    level = np.concatenate([[0], np.cumsum(steps[np.arange(w // bw + 2) % 3])])
    x = np.arange(w)
    rows = np.where(np.arange(h)[:, None] < h // 2, x[None, :], x[None, :] + 5)
    return base + level[rows // bw]


def dots(h, w, py, px):
    """single samples one level up on a lattice: the 2x2 mean turns each 8-bit dot into four samples one 10-bit level up,
    the only way flat 8-bit content comes by a neighbour level at k = 1"""
    d = np.zeros((h, w), np.int64)
    d[3::py, 2::px] = 1
    return d


def plane8(name, h, w, rng):
    """the banded contents at 8 bits, made in 8-bit levels"""
    if name == "staircase":
        return ramp8(h, w, 75) + dots(h, w, 7, 5)
    if name == "dither":         # +-1 on a 24th of the samples: a four-level dither sample empties the mask around it
        return ramp8(h, w, 75) + rng.integers(-1, 2, (h, w)) * (rng.integers(0, 24, (h, w)) == 0)
    if name == "halves":         # v | v + 1: k = 4
        t = np.full((h, w), 128, np.int64)
        t[:, w // 2:] += 1
        return t + dots(h, w, 7, 11)
    t = ramp8(h, w, 0)           # top_ramp: the last band is 255, where the dots are clipped away
    return np.minimum(t + (255 - int(t.max())) + dots(h, w, 7, 5), 255)


def plane(name, h, w, depth, seed=0):
    """-> int64 [h, w] plane of `depth` bits.  From 10 bits up the banded contents are made on the 10-bit scale and brought
    to the depth exactly (t << (depth - 10); at 9 bits t >> 1); at 8 bits they are made in 8-bit levels (plane8)."""
    rng = np.random.default_rng(1000 * h + w + 7 * depth + seed)
    peak = (1 << depth) - 1
    if depth == 8 and name in BANDED:
        return plane8(name, h, w, rng)

    def to_depth(t):
        t = np.clip(t, 0, 1023).astype(np.int64)
        return t << (depth - 10) if depth >= 10 else t >> (10 - depth)     # (9 bits: two 10-bit levels a code)

    if name == "staircase":
        return to_depth(ramp10(h, w, 300))
    if name == "dither":         # the same ramp with +-1 dither on a quarter of the samples: the 2x2 stage undoes part of it
        d = rng.integers(-1, 2, (h, w)) * (rng.integers(0, 4, (h, w)) == 0)
        return to_depth(ramp10(h, w, 300, d))
    if name == "halves":         # v | v + 2
        t = np.full((h, w), 512, np.int64)
        t[:, w // 2:] += 2
        return to_depth(t)
    if name == "top_ramp":       # the ramp ends at 1023: v + k would pass the top of the range
        t = ramp10(h, w, 0)
        return to_depth(t + (1023 - int(t.max())))
    if name == "flat":
        return np.full((h, w), peak // 3, np.int64)
    if name == "noise":          # uniform over the full range: no two neighbours agree, the mask is empty
        return rng.integers(0, peak + 1, (h, w)).astype(np.int64)
    if name == "flat_zero":
        return np.zeros((h, w), np.int64)
    if name == "flat_peak":
        return np.full((h, w), peak, np.int64)
    raise KeyError(name)


def matrix():
    """(content, shape, depth): every content on every shape at 10 bits, and every content at the other depths on 41 x 71"""
    out = [(c, s, 10) for c in CONTENTS for s in SHAPES]
    out += [(c, (41, 71), dp) for c in CONTENTS for dp in DEPTHS if dp != 10]
    return out


def full_contrast(depth):
    """a 16 x 138 plane on which u reaches 65536, the last bin of the histogram, at scale 1: rows 0..7 are v and rows 8..15
    four 10-bit levels above.  The transition row of the 2x2 mean is row 7, odd, so scale 1 (rows 0, 2, .., 14; 8 x 69) does
    not have it: four rows of v and four of v + 4.  Every sample of scale 1 is masked but the corner samples (columns 0, 1 and
    68 of the outer rows), so the windows of columns 34 and 35 - columns 2..66 and 3..67, all eight rows, A = 520 - hold
    n_0 = n_4 = 260: c = 4 * 260 * 260 / (520 * 520) = 1 exactly, at sixteen samples."""
    t = np.full((16, 138), 500, np.int64)
    t[8:, :] += 4
    return t >> 2 if depth == 8 else t << (depth - 10)


def dtype_of(depth):
    return np.uint16 if depth > 8 else np.uint8
