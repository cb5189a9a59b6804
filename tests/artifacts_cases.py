"""The shared cases of the artefact-measure tests (tests/test_artifacts_host.py, tests/test_gpu_artifacts.py): the geometry,
depth and layout grid - the smallest set at which a 64 x 32 tile with a 5 / 4 apron and groups of four samples can go wrong -
and the planes with closed-form answers.  Integer-only and seeded."""
import numpy as np

import motion_cases as K

# (h, w), depth, layout, frames per content kind.  16 x 16: the minimum (a blur domain of 7 rows); 17 x 25: one sample past a
# multiple of 8 either way, rows that are not aligned to the load; 33 x 65 and 47 x 35: one sample past the tile's edge either
# way, and more columns than rows; 66 x 98 4:2:0: chroma planes of 33 x 49; 64 x 96: exact tiles; 12 and 16 bits; packed bgr24.
# The tile is 64 x 32, so no further sizes are needed to cross it by one.
GRID = [((16, 16), 8, "gray", 4), ((17, 25), 8, "gray", 4), ((33, 65), 8, "gray", 3), ((47, 35), 8, "gray", 3),
        ((66, 98), 8, "yuv420p", 3), ((64, 96), 10, "yuv420p10le", 3), ((40, 56), 12, "yuv444p12le", 3),
        ((50, 70), 16, "gray16le", 3), ((40, 56), 8, "bgr24", 3)]
IDS = ["%dx%d-%s" % (g[0][0], g[0][1], g[2]) for g in GRID]


def blocks(h, w, depth, shift=(0, 0), seed=1):
    """constant 8 x 8 blocks of random levels whose grid is shifted by shift = (columns, rows): every horizontal step lies on a
    boundary c with c mod 8 == shift[0], every vertical one on r mod 8 == shift[1]; neighbouring blocks differ"""
    sx, sy = shift
    rng = np.random.default_rng(seed)
    by, bx = (h + 15) // 8 + 1, (w + 15) // 8 + 1
    lev = rng.integers(0, (1 << depth) // 2, (by, bx)).astype(np.int64) * 2
    lev += (np.add.outer(np.arange(by), np.arange(bx)) & 1)          # a checker of parities: neighbours never tie
    i, j = np.arange(h)[:, None], np.arange(w)[None, :]
    return lev[(i + 8 - sy) // 8, (j + 8 - sx) // 8]


def ramp(h, w):
    """x(i, j) = j"""
    return np.broadcast_to(np.arange(w, dtype=np.int64), (h, w)).copy()


def checker(h, w, peak):
    i, j = np.arange(h)[:, None], np.arange(w)[None, :]
    return ((i + j) & 1).astype(np.int64) * peak


def impulse(h, w, y, x, v):
    a = np.zeros((h, w), np.int64)
    a[y, x] = v
    return a


def checker_words(h, w, peak, counts):
    """the closed form of the 0 / peak checkerboard: every step is `peak`, dB9 spans 9 samples and is `peak` too, so
    9 dF - dB9 = 8 peak; |L| = |4 a + 4 a - 8 b| = 8 peak"""
    return dict(edge_h=[peak * h * c for c in counts(w)], edge_v=[peak * w * c for c in counts(h)],
                blur_f_h=peak * h * (w - 9), blur_v_h=8 * peak * h * (w - 9), blur_f_v=peak * w * (h - 9),
                blur_v_v=8 * peak * w * (h - 9), lap=8 * peak * (h - 2) * (w - 2))


def gray_frames(planes, depth):
    """a list of [h, w] integer planes -> (frames [n, h * w] uint8 / uint16, gray plane tuples)"""
    from rtvqa_amd.engine import yuv_planes
    h, w = planes[0].shape
    dt = np.uint16 if depth > 8 else np.uint8
    return np.stack([np.asarray(p).astype(dt).reshape(-1) for p in planes]), yuv_planes(h, w, "mono", depth)


def clip(layout, h, w, depth, kind, seed, n):
    return K.clip(layout, h, w, depth, kind, seed, n)
