"""Block-SAD with one lane per dx group (csrc/k_sad.hip): sad_sum, mv_d2_hist[129] and sad_blocks bit-equal to
oracle.c_oracle.block_sad.

A wave owns 16 blocks as 16x1, 8x2 or 4x4, whichever leaves the fewest block slots empty, so the shapes are the ones
at which that geometry changes: one block; 2x3 blocks; 17 blocks wide (a partial group in every arrangement); 5x5 blocks
(partial groups in both directions); ragged edges (33x47: whole blocks only); one block row 32 blocks wide (the 16x1
choice); 4x4 blocks (the 4x4 choice); 144x272 and 48x528, the smallest planes with an INTERIOR tile - every candidate
of its 16 blocks valid, loads and validity on their lane-constant fast paths - for 8x2 and 4x4, and for 16x1.  Every
width but 64 gets a pitch wider than itself (gray planes are padded to 64 bytes).  The contents make ties: flat against
flat (every candidate ties; d^2, then raster order decide), flat against a brighter flat, one-bit noise, and stripes
whose period puts equal SADs at several displacements; uniform noise makes the never-valid dx = -8, which shares a
QSAD with dx = -7..-5, win now and then if it is not excluded.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import c_oracle as co

pytestmark = pytest.mark.gpu

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(16, 16), (32, 48), (48, 272), (80, 80), (33, 47), (16, 512), (64, 64), (144, 272), (48, 528)]
RANGES = [0, 1, 3, 7]


def gray_sequence(h, w):
    """eight gray frames -> seven (prev, curr) pairs, and the pair (prev0 = frame 0, frame 1) or none for the first"""
    r = np.random.default_rng(1000 * h + w)
    big = r.integers(0, 256, (h + 16, w + 16), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([
        big[8:8 + h, 8:8 + w],                                   # noise
        big[8 - 2:8 - 2 + h, 8 + 3:8 + 3 + w],                   # the same noise, panned by (dy, dx) = (2, -3)
        np.full((h, w), 128, np.uint8),                          # flat
        np.full((h, w), 128, np.uint8),                          # flat again: every candidate ties at 0
        np.full((h, w), 130, np.uint8),                          # a brighter flat: every candidate ties at 512
        r.integers(0, 2, (h, w), dtype=np.uint8),                # one-bit noise: many near ties
        ((xx % 4 < 2) * 200 + (yy % 8 < 4) * 40).astype(np.uint8),       # stripes: equal SADs 4 apart in x, 8 in y
        (((xx + 1) % 4 < 2) * 200 + ((yy + 3) % 8 < 4) * 40).astype(np.uint8),  # the stripes, moved by (3, 1)
    ])


def as_bgr(g):
    return np.repeat(g[..., None], 3, axis=-1)  # BGR2GRAY of (v, v, v) is v


_WANT = {}


def want(h, w, rng):
    """the oracle's records of the seven pairs, computed once per (shape, range)"""
    key = (h, w, rng)
    if key not in _WANT:
        g = gray_sequence(h, w)
        _WANT[key] = [co.block_sad(g[i], g[i + 1], rng) for i in range(len(g) - 1)]
    return _WANT[key]


def check(eng, h, w, rng):
    from rtvqa_amd import _native as N
    g = gray_sequence(h, w)
    ref = want(h, w, rng)
    nb = (h // 16) * (w // 16)
    # first_has_prev = 1: frame 0 is prev0, all seven records carry a pair
    rec = eng.complexity(as_bgr(g[1:]), prev0=as_bgr(g[0]), mask=N.M_MOTION, sad_range=rng)
    for i, (n_, sad, hist) in enumerate(ref):
        got = (int(rec[i]["sad_blocks"]), int(rec[i]["sad_sum"]))
        assert got == (n_, sad) and n_ == nb, (h, w, rng, i, got, (n_, sad))
        assert (rec[i]["mv_d2_hist"] == hist).all(), (h, w, rng, i, np.nonzero(rec[i]["mv_d2_hist"])[0], np.nonzero(hist)[0])
    # first_has_prev = 0: the first frame has no pair and scores nothing
    rec = eng.complexity(as_bgr(g), mask=N.M_MOTION, sad_range=rng)
    assert int(rec[0]["sad_sum"]) == 0 and not rec[0]["mv_d2_hist"].any(), (h, w, rng)
    for i, (n_, sad, hist) in enumerate(ref):
        assert int(rec[i + 1]["sad_sum"]) == sad and (rec[i + 1]["mv_d2_hist"] == hist).all(), (h, w, rng, i)
        assert int(rec[i + 1]["sad_blocks"]) == n_, (h, w, rng, i)


@pytest.mark.parametrize("rng", RANGES)
@pytest.mark.parametrize("h,w", SHAPES)
def test_lane_group_kernel_matches_the_oracle(engine, h, w, rng):
    check(engine, h, w, rng)


def test_the_contents_do_tie():
    """what the contents are for: flat pairs put every block on (0, 0), the pan is found, the stripes tie away from (0, 0)"""
    ref = want(80, 80, 7)
    assert ref[2][2][0] == 25 and ref[2][1] == 0            # flat against flat
    assert ref[3][2][0] == 25 and ref[3][1] == 25 * 512     # flat against the brighter flat
    assert ref[0][2][13] >= 9                               # interior blocks find (2, -3): d^2 = 13
    assert ref[6][2][0] == 0 and ref[6][1] == 0             # the moved stripes match exactly, never at (0, 0)


@pytest.mark.parametrize("knob", ["VQA_SAD_TILE=1", "VQA_SAD_TILE=2", "VQA_SAD_TILE=3", "VQA_SAD_VARIANT=1"])
def test_every_arrangement_and_the_previous_kernel(knob):
    """Lab build: each arrangement forced on every shape (the shipped launcher picks one per shape), and the lane-per-dy
    kernel this one replaced, kept for the A/B (selectors are read once per process: one subprocess per setting)."""
    from rtvqa_amd import _native as N
    assert os.path.exists(N.LAB_LIB_PATH), "the lab library is a build product of the same make (csrc/Makefile, target lab)"
    code = (
        "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import rtvqa_amd\n"
        "import test_gpu_sad_lane_groups as T\n"
        "eng = rtvqa_amd.Engine(0)\n"
        "assert eng.lib.vqa_build_flavour() != 0\n"
        "for h, w in T.SHAPES:\n"
        "    for rng in (7, 3):\n"
        "        T.check(eng, h, w, rng)\n"
        "print('LANE-GROUPS-OK')\n" % (REPO_ROOT, os.path.join(REPO_ROOT, "tests"))
    )
    name, value = knob.split("=")
    env = dict(os.environ, VQA_LIB_PATH=N.LAB_LIB_PATH)
    env[name] = value
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600, cwd=REPO_ROOT)
    assert r.returncode == 0 and "LANE-GROUPS-OK" in r.stdout, (r.stdout[-400:], r.stderr[-1200:])
