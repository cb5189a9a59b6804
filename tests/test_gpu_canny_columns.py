"""Canny stage 1 captures per COLUMN (csrc/k_canny.hip): the bit-planes hold the transposed frame, one word per frame
column and 64 rows, and hysteresis and the count run on them with height and width swapped.  Checked here:
(edge_count, edge_strong, edge_weak) exact against oracle.c_oracle.canny, the edge map read back through
vqa_debug_read_plane equal to the oracle's map pixel for pixel, and a frame and its transpose giving equal counts.

Shapes (h x w), chosen for the seams of the layout: 5 x 3 takes the narrow-frame fallback; 1 x 70 and 70 x 1 are
degenerate strips; 64 x 64, 65 x 63, 63 x 65 are a whole tile and a partial one in either direction (bits >= h must be
0, words >= w unread); 67 x 100 is a one-pair strip; 130 x 257 has a strip whose second tile group holds one column,
and crosses two 16-row group boundaries; 33 x 778 has an interior, a realigning and a last strip in one row, and a
height that is no multiple of 16; 200 x 135 is taller than wide, so a swap of h and w in the wrong place shows.

Contents.  Uniform noise; 0/255 diagonal steps (their magnitude 1530 is the largest there is: the thresholds
(1529, 1530) select exactly them); a flat field; and three drawings of one-pixel lines of value 30 on black - vertical
lines, horizontal lines, a serpentine - whose flanks have the magnitude 120, weak under (100, 200), with ONE pixel of
value 80 per line: its flanks are the only strong pixels, so every other edge pixel of the line is there because
hysteresis carried it along the line, across tile seams along either axis.
"""
import numpy as np
import pytest

from oracle import c_oracle as co

SHAPES = [(5, 3), (1, 70), (70, 1), (64, 64), (65, 63), (63, 65), (67, 100), (130, 257), (33, 778), (200, 135)]
THRESHOLDS = [(100, 200), (-1, -1), (2041, 2041), (200, 100), (1529, 1530)]
WEAK_V, STRONG_V = 30, 80   # line values: flank magnitudes 4 * 30 = 120 (weak), 2 * 80 + 2 * 30 = 220 (strong)


def vertical_lines(h, w):
    g = np.zeros((h, w), np.uint8)
    for k, x in enumerate(range(2, w, 23)):
        g[:, x] = WEAK_V
        g[(7 + 29 * k) % h, x] = STRONG_V
    return g


def serpentine(h, w):
    """one line that winds inward, 12 pixels between its turns, its bright pixel near the start.  It always turns the same
    way: at a right-angle turn the chain of flank pixels on the outer side is broken by the suppression, the one on the
    inner side is not, so a line that turned both ways would lose its connection at the second turn"""
    g = np.zeros((h, w), np.uint8)
    top, left, bottom, right = min(2, h - 1), min(2, w - 1), h - 3, w - 3
    y0 = top
    while top <= bottom and left <= right:
        g[top, left:right + 1] = WEAK_V
        g[top:bottom + 1, right] = WEAK_V
        g[bottom, left:right + 1] = WEAK_V
        top += 12
        g[top:bottom + 1, left] = WEAK_V      # up the left side, to the row where the next turn of the winding starts
        left, bottom, right = left + 12, bottom - 12, right - 12
        if top <= bottom:
            g[top, left - 12:left + 1] = WEAK_V
    g[y0, min(5, w - 1)] = STRONG_V
    return g


def contents(h, w):
    """two batches of three gray frames"""
    r = np.random.default_rng(9000 * h + w)
    yy, xx = np.mgrid[0:h, 0:w]
    steps = np.zeros((h, w), np.uint8)
    steps[(xx + yy) % 48 < 6] = 255
    steps[(xx - yy) % 56 < 5] = 255
    flat = np.full((h, w), 128, np.uint8)
    a = np.stack([r.integers(0, 256, (h, w), dtype=np.uint8), steps, flat])
    b = np.stack([vertical_lines(h, w), np.ascontiguousarray(vertical_lines(w, h).T), serpentine(h, w)])
    return [a, b]


def as_bgr(g):
    return np.ascontiguousarray(np.repeat(g[..., None], 3, axis=-1))  # BGR2GRAY of (v, v, v) is v


_WANT = {}


def want(h, w):
    """the oracle's (count, strong, weak, map) of every frame of every batch at every threshold pair, computed once"""
    if (h, w) not in _WANT:
        _WANT[(h, w)] = [[[co.canny(g, lo, hi, want_map=True) for g in batch] for batch in contents(h, w)]
                         for lo, hi in THRESHOLDS]
    return _WANT[(h, w)]


def run(eng, batch, lo, hi, maps=True):
    from rtvqa_amd import _native as N
    n, h, w = batch.shape
    rec = eng.complexity(as_bgr(batch), mask=N.M_EDGE, canny=(lo, hi))
    return [(int(rec[i]["edge_count"]), int(rec[i]["edge_strong"]), int(rec[i]["edge_weak"]),
             eng.debug_plane(2, i, h, w) if maps else None) for i in range(n)]


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", SHAPES)
def test_column_planes_match_the_oracle(engine, h, w):
    ref = want(h, w)
    for t, (lo, hi) in enumerate(THRESHOLDS):
        for b, batch in enumerate(contents(h, w)):
            got = run(engine, batch, lo, hi)
            for i in range(len(batch)):
                cnt, strong, weak, emap = ref[t][b][i]
                print(h, w, lo, hi, b, i, "got", got[i][:3], "want", (cnt, strong, weak))
                assert got[i][1:3] == (strong, weak), (h, w, lo, hi, b, i, got[i][1:3], (strong, weak))
                bad = got[i][3] != emap
                assert not bad.any(), (h, w, lo, hi, b, i, "edge map differs at", np.argwhere(bad)[:8].tolist())
                assert got[i][0] == cnt, (h, w, lo, hi, b, i, got[i][0], cnt)


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", SHAPES)
def test_a_frame_and_its_transpose_give_equal_counts(engine, h, w):
    ref = want(h, w)
    for t, (lo, hi) in enumerate(THRESHOLDS):
        for b, batch in enumerate(contents(h, w)):
            tr = np.ascontiguousarray(batch.transpose(0, 2, 1))
            got = run(engine, tr, lo, hi, maps=False)
            for i in range(len(batch)):
                print(h, w, lo, hi, b, i, "transposed", got[i][:3], "want", ref[t][b][i][:3])
                assert got[i][:3] == ref[t][b][i][:3], (h, w, lo, hi, b, i, got[i][:3], ref[t][b][i][:3])


def test_the_contents_do_what_they_are_for():
    """Oracle only.  Canny commutes with transposition on every case; the lines are weak but for the flanks of their one
    bright pixel and reach the count only through hysteresis, over more than one tile along either axis; the diagonal
    steps are what (1529, 1530) selects; the flat field and (2041, 2041) select nothing at any threshold."""
    for h, w in SHAPES:
        ref = want(h, w)
        for t, (lo, hi) in enumerate(THRESHOLDS):
            for b, batch in enumerate(contents(h, w)):
                for i, g in enumerate(batch):
                    cnt, strong, weak, emap = co.canny(np.ascontiguousarray(g.T), lo, hi, want_map=True)
                    assert (cnt, strong, weak) == ref[t][b][i][:3], (h, w, lo, hi, b, i)
                    assert (emap.T == ref[t][b][i][3]).all(), (h, w, lo, hi, b, i)
        assert all(f[0] == 0 for b in ref[2] for f in b)                  # (2041, 2041)
        assert ref[0][0][2][:3] == (0, 0, 0)                              # flat field, (100, 200)
        assert ref[1][0][2][:3] == (0, 0, 0)                              # ... and (-1, -1): a candidate that beats no neighbour
        assert h * w < 64 or ref[1][0][0][1] > h * w // 16                # while noise under (-1, -1) is all strong
        assert ref[3][0][0][:3] == ref[0][0][0][:3]                       # low > high is (high, low)
    h, w = 200, 135
    ref = want(h, w)
    for i, axis in ((0, 0), (1, 1)):      # vertical lines cross tile seams along y, horizontal ones along x
        cnt, strong, weak, emap = ref[0][1][i]
        assert 0 < strong <= 6 * len(range(2, (w, h)[axis], 23)) and cnt == strong + weak and weak > 20 * strong
        tiles = {(p[axis] >> 6) for p in np.argwhere(emap)}
        assert len(tiles) == (((h, w)[axis] + 63) >> 6), tiles
    cnt, strong, weak, emap = ref[0][1][2]  # the serpentine: one seed, and the edge reaches the last tile row and column
    assert 0 < strong <= 6 and cnt > 50 * strong
    assert emap[128:, :].any() and emap[:, 128:].any() and emap[:64, :64].any()
    _, _, smag = co.sobel_l1(contents(h, w)[0][1])
    assert int(smag.max()) == 1530
    top = want(h, w)[4][0][1]
    assert top[1] == 0 and top[2] > 0 and top[0] == 0                     # m == 1530 is above 1529, not above 1530
