"""Canny stage 1 on packed 16-bit tile pairs (csrc/k_canny.hip, k_canny_nms4): (edge_strong, edge_weak, edge_count) and the
edge map bit-equal to oracle.c_oracle.canny.

The kernel pairs the four 64-column tiles of a 256-column strip (0&1, 2&3), runs one pair only where a strip has at most
two real tiles, switches to the realigning path where a lane's dword window leaves the image, and captures row r of a
64-row strip in lane r.  The widths sit on both sides of every tile, pair and strip seam (64, 128, 192, 256), of the
4-column minimum and of the interior-path limit x0 + 259 <= w; the heights give strips of one, two and three rows, a full
strip, a strip plus one or two rows and two strips plus one.

Contents.  Uniform noise (dense candidates) and 3-level noise (near ties).  0/255 steps - vertical, horizontal, both
diagonals - and checkerboards: the largest magnitudes there are.  Sobel's gx + gy is twice a sum of six pixels, so
|gx| + |gy| tops out at 6 * 255 = 1530, not at 1020 + 1020: the diagonal steps reach 1530, and the threshold pairs
around 2040 select nothing while (1529, 1530) selects exactly those pixels.  Ramps are plateaus of one non-zero
magnitude that tie in every direction, one per direction class.  Sector patches put single pixels next to the two
boundaries of OpenCV's fixed-point sector test, horizontal iff |gy| < a1 = (13573 |gx| + 32767) >> 15 and vertical iff
|gy| > a2 = (79109 |gx|) >> 15.  gx and gy always have the same parity, so for a given |gx| only one of a1 - 1, a1 and one
of a2, a2 + 1 can occur: each patch pair takes that one and the nearest value across the boundary (2 away), every pair in
all four sign combinations of (gx, gy), which covers both diagonals.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import c_oracle as co

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = [4, 5, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 259, 260, 320, 513]
HEIGHTS = [1, 2, 3, 63, 64, 66, 129]
GEOMETRIES = [(65, w) for w in WIDTHS] + [(h, 257) for h in HEIGHTS]
THRESHOLDS = [(100, 200), (0, 0), (-5, 10), (2039, 2040), (2040, 2041), (200, 100), (150, 150), (1529, 1530)]
SECTOR_GX = [6, 7, 10, 11, 37, 64, 100, 101, 150, 201]
CELL = 8  # sector patches sit on a grid of 8 x 8 cells of a black frame


def a1(gx):
    return (13573 * gx + 32767) >> 15


def a2(gx):
    return (79109 * gx) >> 15


def sector_cases():
    """(|gx|, |gy|, class) on both sides of both boundaries, at the nearest values the parity of gx + gy allows"""
    out = []
    for g in SECTOR_GX:
        lo = a1(g) - 1 if (a1(g) - 1 - g) % 2 == 0 else a1(g) - 2     # horizontal side: |gy| <= a1 - 1
        out += [(g, lo, "h"), (g, lo + 2, "d")]
        lo = a2(g) if (a2(g) - g) % 2 == 0 else a2(g) - 1             # diagonal side: |gy| <= a2
        out += [(g, lo, "d"), (g, lo + 2, "v")]
    return out


def sector_patches(h, w):
    """a black frame with one patch per grid cell that fits: the pixel right of the centre is u, the one below it v, the
    one below right t, so gx = 2u + t and gy = 2v + t at the centre; mirrored in x and / or y for the other signs.
    Returns the frame and [(y, x, gx, gy, class)] of the centres."""
    g = np.zeros((h, w), np.uint8)
    centres = []
    cases = [(c, sx, sy) for c in sector_cases() for sx in (1, -1) for sy in (1, -1)]
    k = 0
    for cy in range(3, h - 3, CELL):
        for cx in range(3, w - 3, CELL):
            (agx, agy, cls), sx, sy = cases[k % len(cases)]
            k += 1
            t = agx & 1
            g[cy, cx + sx] = (agx - t) // 2
            g[cy + sy, cx] = (agy - t) // 2
            g[cy + sy, cx + sx] = t
            centres.append((cy, cx, sx * agx, sy * agy, cls))
    return g, centres


def contents(h, w):
    """three batches of three gray frames"""
    r = np.random.default_rng(7000 * h + w)
    yy, xx = np.mgrid[0:h, 0:w]
    noise = [r.integers(0, 256, (h, w), dtype=np.uint8), r.integers(0, 256, (h, w), dtype=np.uint8),
             (r.integers(0, 3, (h, w)) * 7).astype(np.uint8)]
    steps = np.zeros((h, w), np.uint8)   # quadrants: vertical and horizontal 0/255 steps; two diagonal steps across them
    steps[(xx >= w // 2) ^ (yy >= h // 2)] = 255
    steps[(xx + yy) % 48 < 6] = 255
    steps[(xx - yy) % 56 < 5] = 0
    hard = [steps, (((xx + yy) & 1) * 255).astype(np.uint8), ((((xx >> 1) + (yy >> 1)) & 1) * 255).astype(np.uint8)]
    ramps = np.zeros((h, w), np.int64)   # four bands of rows: gradients (24, 0), (0, 24), (8, 8), (8, 24) away from the seams
    band = yy * 4 // max(h, 1)
    for b, (kx, ky) in enumerate(((3, 0), (0, 3), (1, 1), (1, 3))):
        ramps = np.where(band == b, (kx * xx + ky * yy) % 256, ramps)
    sect = [sector_patches(h, w)[0], ramps.astype(np.uint8), np.ascontiguousarray(sector_patches(h, w)[0][::-1, ::-1])]
    return [np.stack(noise), np.stack(hard), np.stack(sect)]


def as_bgr(g):
    return np.ascontiguousarray(np.repeat(g[..., None], 3, axis=-1))  # BGR2GRAY of (v, v, v) is v


_WANT = {}


def want(h, w):
    """the oracle's (count, strong, weak, map) of every frame of every batch at every threshold pair, computed once"""
    if (h, w) not in _WANT:
        _WANT[(h, w)] = [[[co.canny(g, lo, hi, want_map=True) for g in batch] for batch in contents(h, w)]
                         for lo, hi in THRESHOLDS]
    return _WANT[(h, w)]


def run(eng, h, w):
    """the engine's records and edge maps, in the order of want()"""
    from rtvqa_amd import _native as N
    out = []
    for lo, hi in THRESHOLDS:
        per_batch = []
        for batch in contents(h, w):
            rec = eng.complexity(as_bgr(batch), mask=N.M_EDGE, canny=(lo, hi))
            per_batch.append([(int(rec[i]["edge_count"]), int(rec[i]["edge_strong"]), int(rec[i]["edge_weak"]),
                               eng.debug_plane(2, i, h, w)) for i in range(len(batch))])
        out.append(per_batch)
    return out


def check(eng, h, w):
    got, ref = run(eng, h, w), want(h, w)
    for t, (lo, hi) in enumerate(THRESHOLDS):
        for b in range(len(ref[t])):
            for i in range(len(ref[t][b])):
                cnt, strong, weak, emap = ref[t][b][i]
                assert got[t][b][i][1:3] == (strong, weak), (h, w, lo, hi, b, i, got[t][b][i][1:3], (strong, weak))
                bad = got[t][b][i][3] != emap
                assert not bad.any(), (h, w, lo, hi, b, i, "edge map differs at", np.argwhere(bad)[:8].tolist())
                assert got[t][b][i][0] == cnt, (h, w, lo, hi, b, i)


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", GEOMETRIES)
def test_pair_packed_nms_matches_the_oracle(engine, h, w):
    check(engine, h, w)


def classify(gx, gy):
    """OpenCV's sector test as the oracle forms it"""
    ax, ay = abs(int(gx)), abs(int(gy)) << 15
    t22 = ax * 13573
    return "h" if ay < t22 else ("v" if ay > t22 + (ax << 16) else "d")


def test_the_contents_do_what_they_are_for():
    """Oracle only.  The sector patches land where they were aimed and change class across each pair, in all four sign
    combinations; the per-|gx| thresholds the kernel uses say the same as the sector test for every possible gradient;
    the ramps are plateaus of one magnitude on which nothing survives; the diagonal steps reach the largest magnitude."""
    h, w = 65, 257
    g, centres = sector_patches(h, w)
    dx, dy, mag = co.sobel_l1(g)
    seen = set()
    for (cy, cx, gx, gy, cls) in centres:
        assert (int(dx[cy, cx]), int(dy[cy, cx])) == (gx, gy), (cy, cx)
        assert classify(gx, gy) == cls, (gx, gy, cls)
        seen.add((abs(gx), abs(gy), cls, gx < 0, gy < 0))
    cases = sector_cases()
    assert len(seen) == 4 * len(cases)          # every case in every sign combination fits into 65 x 257
    for k in range(0, len(cases), 2):           # each pair: same |gx|, |gy| two apart, classes differ
        (ga, ya, ca), (gb, yb, cb) = cases[k], cases[k + 1]
        assert ga == gb and yb == ya + 2 and ca != cb
        assert (ya < a1(ga) <= yb) or (ya <= a2(ga) < yb)
    ax, ay = np.meshgrid(np.arange(1021, dtype=np.int64), np.arange(1021, dtype=np.int64), indexing="ij")
    m = ax + ay
    th1, th2 = (92682 * ax + 65534) >> 16, (223754 * ax) >> 16
    assert (th1 == ax + ((13573 * ax + 32767) >> 15)).all() and (th2 == ax + ((79109 * ax) >> 15)).all()
    assert ((m < th1) == ((ay << 15) < 13573 * ax)).all() and ((m > th2) == ((ay << 15) > 13573 * ax + (ax << 16))).all()
    assert int(th2.max()) == 3482 and (th1 <= th2).all()
    batches = contents(h, w)
    ramps = batches[2][1]
    _, _, rmag = co.sobel_l1(ramps)
    quarter = h // 4
    for b, mval in enumerate((24, 24, 16, 32)):
        inner = rmag[b * quarter + 2:(b + 1) * quarter - 2, 2:60]   # away from the band seams and the wrap of % 256
        assert (inner == mval).all(), (b, np.unique(inner))
    emap = co.canny(ramps, 0, 0, want_map=True)[3]
    assert not emap[2:quarter - 2, 2:60].any() and not emap[2 * quarter + 2:3 * quarter - 2, 2:60].any()
    assert co.canny(batches[0][0], 0, 0)[0] > h * w // 8            # while noise keeps plenty
    _, _, smag = co.sobel_l1(batches[1][0])
    assert int(smag.max()) == 1530
    cnt_top = co.canny(batches[1][0], 1529, 1530)
    assert cnt_top[1] == 0 and cnt_top[2] > 0                        # weak candidates only: m == 1530 is not above 1530
    assert co.canny(batches[1][0], 2039, 2040)[1:] == (0, 0)


_CHILD = (
    "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
    "import numpy as np\n"
    "import rtvqa_amd\n"
    "import test_gpu_canny_nms_pairs as T\n"
    "eng = rtvqa_amd.Engine(0)\n"
    "assert eng.lib.vqa_build_flavour() != 0\n"
    "out = {}\n"
    "for h, w in T.LAB_GEOMETRIES:\n"
    "    got = T.run(eng, h, w)\n"
    "    out['rec_%%d_%%d' %% (h, w)] = np.array([[[f[:3] for f in b] for b in t] for t in got], np.int64)\n"
    "    out['map_%%d_%%d' %% (h, w)] = np.stack([f[3] for t in got for b in t for f in b])\n"
    "np.savez(sys.argv[1], **out)\n"
    "print('NMS-PAIRS-OK')\n"
)
LAB_GEOMETRIES = [(65, 5), (65, 129), (65, 257), (65, 320), (65, 513), (1, 257), (66, 257), (129, 257)]


@pytest.mark.gpu
def test_previous_kernel_gives_the_same_planes_and_records(tmp_path):
    """Lab build: VQA_NMS_VARIANT=3 (the lane-per-column kernel with its mask logic on the scalar unit, kept for the A/B)
    and the shipped pair-packed kernel on the same inputs: identical records and edge maps (selectors are read once per
    process: one subprocess per setting)."""
    from rtvqa_amd import _native as N
    assert os.path.exists(N.LAB_LIB_PATH), "the lab library is a build product of the same make (csrc/Makefile, target lab)"
    code = _CHILD % (REPO_ROOT, os.path.join(REPO_ROOT, "tests"))
    res = {}
    for variant in ("3", "4"):
        env = dict(os.environ, VQA_LIB_PATH=N.LAB_LIB_PATH, VQA_NMS_VARIANT=variant)
        path = str(tmp_path / ("v%s.npz" % variant))
        r = subprocess.run([sys.executable, "-c", code, path], env=env, capture_output=True, text=True, timeout=600, cwd=REPO_ROOT)
        assert r.returncode == 0 and "NMS-PAIRS-OK" in r.stdout, (variant, r.stdout[-400:], r.stderr[-1200:])
        res[variant] = np.load(path)
    assert sorted(res["3"].files) == sorted(res["4"].files) and len(res["3"].files) == 2 * len(LAB_GEOMETRIES)
    for k in res["3"].files:
        assert (res["3"][k] == res["4"][k]).all(), k
    h, w = LAB_GEOMETRIES[2]
    ref = want(h, w)
    rec = res["4"]["rec_%d_%d" % (h, w)]
    assert rec.shape[:3] == (len(THRESHOLDS), 3, 3) and rec[0, 0, 0].tolist() == list(ref[0][0][0][:3])
