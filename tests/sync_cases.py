"""Cases of the clip-wide sync tests (tests/test_sync_host.py, tests/test_gpu_sync.py, tests/test_gpu_sync_pass.py).

Content: the clips of a parity case are UNRELATED random frames (their own seeds), every frame different and no symmetry between
the two streams - a transposed tile, a swapped operand or a diagonal read backwards changes words."""
import numpy as np

# (h, w) of the 8-bit signature cases: one-sample cells; one cell row of two rows; cells of unequal sizes on both axes; cells of
# 3 x 4 (a chunk of 16 samples meets five cells); a row of 1030 samples - the wide path, chunks that meet two cells and a last,
# partial chunk
GEOMETRY = [(16, 16), (17, 16), (37, 19), (64, 48), (20, 1030)]
PADDED = (21, 130, 131, 1)   # h, w, row_stride, lead: every row starts at another alignment (the narrow path, w < 256)
DEPTHS = (9, 10, 12, 15, 16)
# (n_dist, n_ref) of the cross: one pair; one row, one column (tiles of one frame against two tiles); one full tile; tiles that
# are not full on either side; several tiles with more reference frames; more distorted frames; many tile diagonals and long walks
COUNTS = [(1, 1), (1, 17), (17, 1), (16, 16), (15, 33), (48, 100), (130, 70), (1000, 3000)]
BIG = 1000   # from here on the reference takes the vectorised route (sync_reference.cross_fast)


def dtype_of(depth):
    return np.uint16 if depth > 8 else np.uint8


def clip(n, h, w, depth, seed, full_range=False):
    """n unrelated random frames [n, h, w]; full_range: over the whole sample type (above-peak values at depths below 16)"""
    top = (1 << (16 if depth > 8 else 8)) if full_range else (1 << depth)
    return np.random.default_rng(seed).integers(0, top, (n, h, w)).astype(dtype_of(depth))


def mono(w, h, depth=8):
    return [(w, h, 0, w * (2 if depth > 8 else 1), 2 if depth > 8 else 1) + ((depth,) if depth > 8 else ())]


def random_sigs(n, seed):
    """n unrelated signatures over the whole byte range"""
    return np.random.default_rng(seed).integers(0, 256, (n, 256)).astype(np.uint8)


def panning_clip(n=300, h=270, w=480, step=3, seed=21):
    """n frames of a texture of 8 x 8 blocks that pans `step` samples per frame"""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, 256, ((h + 7) // 8, (w + step * n + 7) // 8)).astype(np.uint8)
    tex = np.kron(coarse, np.ones((8, 8), np.uint8))
    return np.stack([tex[:h, step * t:step * t + w] for t in range(n)])


def noisy(frames, amp, seed):
    """+-amp of noise on every sample, clipped to the byte range"""
    rng = np.random.default_rng(seed)
    return np.clip(frames.astype(np.int64) + rng.integers(-amp, amp + 1, frames.shape), 0, 255).astype(np.uint8)


def late_start(late=37, n=300, length=200):
    """-> (ref [n], dist [length]): dist[j] = ref[j + late] with +-3 of noise"""
    ref = panning_clip(n)
    return ref, noisy(ref[late:late + length], 3, 22)


def excerpt(n=24, h=19, w=37, at=5, length=12, seed=23):
    """-> (ref: n unrelated frames, dist: ref[at : at + length], identical)"""
    ref = clip(n, h, w, 8, seed)
    return ref, ref[at:at + length].copy()


def pass_clip(n=20, h=48, w=64, at=3, length=12, seed=31):
    """the clip of the pass tests, yuv420p [n, h w 3 / 2]: n unrelated reference frames and `length` distorted frames made from
    ref[at : at + length] with +-2 of noise"""
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 256, (n, h * w * 3 // 2)).astype(np.uint8)
    return ref, noisy(ref[at:at + length], 2, seed + 1)


def half_size(yuv, h, w):
    """the 2 x 2 mean (rounded) of every plane of yuv420p frames [n, h w 3 / 2] -> [n, (h / 2) (w / 2) 3 / 2]"""
    n = yuv.shape[0]
    out = []
    at = 0
    for ph, pw in ((h, w), (h // 2, w // 2), (h // 2, w // 2)):
        p = yuv[:, at:at + ph * pw].reshape(n, ph // 2, 2, pw // 2, 2).astype(np.int64)
        out.append(((p.sum(axis=(2, 4)) + 2) // 4).astype(np.uint8).reshape(n, -1))
        at += ph * pw
    return np.ascontiguousarray(np.concatenate(out, axis=1))
