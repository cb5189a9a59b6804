"""Cases of the spatial-registration tests (tests/test_shift_host.py, tests/test_gpu_shift.py, tests/test_gpu_shift_pass.py).

Content: the two streams of a parity case are UNRELATED random frames (their own seeds), no symmetry between the streams or the
axes - a transposed tile, swapped operands, a grid read backwards or dy taken for dx changes words.  A translated case is the
reference moved by a known shift with other noise where the move leaves the plane.  tests/test_shift_host.py shows on the CPU
that every noise case has ONE smallest word in each grid and every translated case ONE zero, so the GPU assertions on where
the minimum lies cannot be met by accident."""
import numpy as np

ROWS = 8      # k_shift: SHIFT_ROWS, the reference rows M - R .. h - M + R - 1 of a workgroup's visit (N.SHIFT_ROWS)
FLUSH = 512   # k_shift: SHIFT_FLUSH, the matrix steps of 64 core columns between two flushes (N.SHIFT_FLUSH)

# (w, h, R, M, depth).  A core of ONE sample at one tile, at the edge of one tile, at nine tiles and under M > R (16-bit content
# where the grid is large: 1089 squares of 8-bit differences cannot all differ);
ONE_SAMPLE = [(3, 3, 1, 1, 8), (15, 15, 7, 7, 16), (33, 33, 16, 16, 16), (5, 5, 1, 2, 8)]
# widths 17, 63, 64, 65, 130 of the plane, and 68 and 69, whose core of 64 and 65 columns is one matrix step and one more;
WIDTHS = [(w, 9, 2, 2, 8) for w in (17, 63, 64, 65, 130, 68, 69)]
# heights: with R = M = 1 the kernel walks h reference rows, so h is one below, at, one above ROWS, and twice it plus one;
HEIGHTS = [(21, h, 1, 1, 8) for h in (ROWS - 1, ROWS, ROWS + 1, 2 * ROWS + 1)]
# radii: one tile, the edge of one tile, four tiles, the edge of four, nine tiles - a core of 21 x 11;
RADII = [(2 * r + 21, 2 * r + 11, r, r, 8) for r in (1, 7, 8, 15, 16)]
# and a margin above the radius
MARGINS = [(37, 19, 2, 5, 8), (40, 30, 8, 9, 8)]
GEOMETRY = ONE_SAMPLE + WIDTHS + HEIGHTS + RADII + MARGINS
DEPTHS = [(45, 19, 3, 3, d) for d in (8, 10, 16)] + [(45, 19, 8, 8, 10)]
# (w, h, R, M, (dy, dx)): the reference translated by (3, -2), and by the corner (-R, R) of one tile and of four
TRANSLATED = [(40, 30, 4, 4, (3, -2)), (40, 30, 4, 4, (-4, 4)), (48, 40, 8, 8, (-8, 8))]

# The accumulator range.  k_shift (csrc/k_shift.hip): a wave visits ROWS reference rows of all the core's columns, one matrix
# step per 64 columns and row (the steps start at the multiple of 4 at or below M, so a row takes at least (w - 2M) / 64 of
# them), and adds its 32-bit accumulators into the 64-bit words every FLUSH steps.  With R = M = 1 and h = ROWS + 2 the first
# visit is ROWS rows of at least (w - 2) / 64 = 130 steps: 1040 steps or more, flushed at 512, at 1024 and at the end - every
# accumulator twice before the last.  Between two flushes the shared HL / LH accumulator of 16-bit samples gathers
# 2 * 64 * 512 products of up to 128 * 128: 2^30, which a missing flush would double past 2^31.
RANGE_PLANE = (64 * 130 + 2, ROWS + 2, 1, 1)
RANGE_LEVELS = [(0, 65535), (65535, 65535), (65535, 0)]   # (distorted, reference) at 16 bits


def dtype_of(depth):
    return np.uint16 if depth > 8 else np.uint8


def mono(w, h, depth=8):
    return [(w, h, 0, w * (2 if depth > 8 else 1), 2 if depth > 8 else 1) + ((depth,) if depth > 8 else ())]


def clip(n, h, w, depth, seed, full_range=False):
    """n unrelated random frames [n, h, w]; full_range: over the whole sample type (above-peak values at depths below 16)"""
    top = (1 << (16 if depth > 8 else 8)) if full_range else (1 << depth)
    return np.random.default_rng(seed).integers(0, top, (n, h, w)).astype(dtype_of(depth))


def pair(case, n=2):
    """(w, h, R, M, depth) -> (ref, dist): unrelated noise, seeded by the case"""
    w, h, R, M, depth = case
    seed = 1000 * w + 10 * h + R + M
    return clip(n, h, w, depth, 2 * seed + 1), clip(n, h, w, depth, 2 * seed + 2)


def translated(ref, dy, dx, seed):
    """dist with dist(y, x) = ref(y + dy, x + dx) wherever that lies inside the plane, and other noise elsewhere"""
    n, h, w = ref.shape
    dist = np.random.default_rng(seed).integers(0, 256, ref.shape).astype(ref.dtype)
    ys, xs = slice(max(0, -dy), min(h, h - dy)), slice(max(0, -dx), min(w, w - dx))
    dist[:, ys, xs] = ref[:, ys.start + dy:ys.stop + dy, xs.start + dx:xs.stop + dx]
    return dist


def translated_pair(case, n=2):
    w, h, R, M, (dy, dx) = case
    ref = clip(n, h, w, 8, 31 * w + h + R)
    return ref, translated(ref, dy, dx, 77 * w + R)


def moved_clip(n=6, h=48, w=64, shift=(2, -2), seed=11):
    """the clip of the pass tests: the distorted stream is the reference moved by two samples on both axes, +-2 of noise on it"""
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 256, (n, h, w)).astype(np.uint8)
    moved = translated(ref, shift[0], shift[1], seed + 1).astype(np.int64)
    return ref, np.clip(moved + rng.integers(-2, 3, moved.shape), 0, 255).astype(np.uint8)


def smallest(grid):
    """-> ((dy, dx) of the smallest word, how many words are that small)"""
    g = np.asarray(grid)
    R = g.shape[0] // 2
    a, b = np.unravel_index(int(np.argmin(g)), g.shape)
    return (int(a) - R, int(b) - R), int((g == g.min()).sum())
