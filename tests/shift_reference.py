"""The restatement of vqa_shift_submit's definition (include/vqa.h) in NumPy:
sse[j][dy + R][dx + R] = sum over M <= y < h - M, M <= x < w - M of (d_j(y, x) - r_j(y + dy, x + dx))^2, formed DIRECTLY in
int64, shift by shift - no correlation, no sample offset, no energies, so it shares no algebra with the kernel.  `loops` says
the same with a double loop over Python integers, for the hand-computed grids."""
import numpy as np

from align_reference import plane_series  # noqa: F401  (the samples of one plane tuple of every frame -> int64 [n, h, w])


def grid(ref, dist, radius, margin=None):
    """ref, dist: int64 [h, w] -> uint64 [2 radius + 1, 2 radius + 1]; every value stays below 2^28 * 2^32 = 2^60"""
    R = int(radius)
    M = R if margin is None else int(margin)
    h, w = dist.shape
    assert ref.shape == dist.shape and M >= R >= 1 and h >= 2 * M + 1 and w >= 2 * M + 1
    core = dist[M:h - M, M:w - M].astype(np.int64)
    out = np.zeros((2 * R + 1, 2 * R + 1), np.uint64)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            e = core - ref[M + dy:h - M + dy, M + dx:w - M + dx].astype(np.int64)
            out[dy + R, dx + R] = int((e * e).sum(dtype=np.int64))
    return out


def grids(ref, dist, radius, margin=None):
    """ref, dist: int64 [n, h, w] -> uint64 [n, 2 radius + 1, 2 radius + 1]"""
    return np.stack([grid(r, d, radius, margin) for r, d in zip(ref, dist)])


def loops(ref, dist, radius, margin=None):
    """the same grid from nested lists, sample by sample, in Python integers"""
    R = int(radius)
    M = R if margin is None else int(margin)
    h, w = len(dist), len(dist[0])
    return [[sum((int(dist[y][x]) - int(ref[y + dy][x + dx])) ** 2 for y in range(M, h - M) for x in range(M, w - M))
             for dx in range(-R, R + 1)] for dy in range(-R, R + 1)]
