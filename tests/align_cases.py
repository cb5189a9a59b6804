"""Cases of the temporal-alignment tests (tests/test_align_host.py, tests/test_gpu_align.py, tests/test_gpu_align_pass.py).

Content: the two streams of a parity case are UNRELATED random frames (their own seeds), every frame different and no symmetry
between the streams - a transposed tile, a swapped operand or a band read backwards changes words.  The alignment scenarios are
the three of the issue: a clip with a reference frame dropped and an encoded frame repeated, a static clip, a late start."""
import numpy as np

# (n_dist, n_ref, offset, radius): one frame; tiles that are not full; a negative offset; the widest band over few frames, far
# into the reference; more distorted than reference frames; three full tiles at the radius where a band meets four tiles
COUNTS = [(1, 1, 0, 0), (17, 23, 0, 8), (16, 16, -3, 4), (5, 40, 20, 32), (33, 7, 0, 2), (48, 48, 0, 16)]
OUT_OF_RANGE = (4, 4, 100, 3)   # every pair names a reference frame that does not exist
# (w, h) of the 8-bit geometry cases: one sample; a row shorter than a 16-sample group; a row that is no multiple of 16 over more
# rows than a workgroup takes (ALIGN_ROWS = 8); a row of exactly four groups
GEOMETRY = [(1, 1), (15, 3), (37, 19), (64, 2)]
DEPTHS = (9, 10, 12, 15, 16)
# The accumulator range.  k_align_cross (csrc/k_align.hip): a workgroup takes ALIGN_ROWS = 8 rows of the plane, and a wave adds
# its 32-bit accumulators into the 64-bit words every ALIGN_FLUSH = 512 matrix steps of 64 samples.  512 x 300 (the issue's) is
# 38 workgroups' ranges, but 8 rows of it are 4096 samples - below the 131072 at which a missing flush overflows.  16400 x 9 is
# two ranges (rows 0 .. 7, row 8), and the first is 131200 samples of every frame in ONE wave: 4 flushes, and past 131071.
RANGE_PLANES = [(512, 300), (16400, 9)]
RANGE_LEVELS = {8: [(0, 0), (255, 255), (0, 255)], 16: [(0, 0), (65535, 65535), (0, 65535)]}


def dtype_of(depth):
    return np.uint16 if depth > 8 else np.uint8


def clip(n, h, w, depth, seed, full_range=False):
    """n unrelated random frames [n, h, w]; full_range: over the whole sample type (above-peak values at depths below 16)"""
    top = (1 << (16 if depth > 8 else 8)) if full_range else (1 << depth)
    return np.random.default_rng(seed).integers(0, top, (n, h, w)).astype(dtype_of(depth))


def mono(w, h, depth=8):
    return [(w, h, 0, w * (2 if depth > 8 else 1), 2 if depth > 8 else 1) + ((depth,) if depth > 8 else ())]


def dropped_and_repeated(n=40, h=12, w=16, seed=7):
    """-> (ref [n], enc [n], the reference index of every encoded frame): reference frame 10 is dropped, so encoded frames 10 .. 24
    show reference frames 11 .. 25; encoded frame 25 repeats reference frame 25, after which the streams are in step again;
    +-3 of noise on every encoded frame"""
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 256, (n, h, w)).astype(np.int64)
    index = list(range(10)) + list(range(11, 26)) + [25] + list(range(26, 40))
    index = index[:n]
    enc = np.clip(ref[index] + rng.integers(-3, 4, (len(index), h, w)), 0, 255)
    return ref.astype(np.uint8), enc.astype(np.uint8), index


def static_clip(n=12, h=12, w=16, seed=3):
    rng = np.random.default_rng(seed)
    one = rng.integers(0, 256, (1, h, w))
    ref = np.repeat(one, n, axis=0).astype(np.uint8)
    return ref, ref.copy()


def late_start(n=30, h=12, w=16, seed=5, late=3):
    """the encoded stream starts `late` frames into the reference: enc[j] = ref[j + late]"""
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 256, (n + late, h, w)).astype(np.uint8)
    return ref, ref[late:].copy()
