"""Hostile content on the host side (no GPU): is every entry of tests/test_gpu_hostile.py's matrix a fair test of the kernels and
not of fp32 itself?  A content enters a metric's matrix only if the reference alone is stable on it: its float32 run within half
the GPU bar of its float64 run.  What fails that is left out by name in hostile_cases.EXCLUDED (at most two of the seven pair
contents per metric and depth) and its deviation is printed here.  Also: the SSIM of every pair is far from 0 (the bar is
relative), the SAD contents do tie between candidates of different d^2 and the oracle takes the smaller, the two Canny oracles
agree on the threshold content, and the Farneback oracle is finite on static degenerate pairs."""
import numpy as np
import pytest

import adm_reference as A
import hbd_reference as H
import hostile_cases as K
import vif_reference as V
from oracle import c_oracle as co
from oracle import np_oracle as no

HALF = 5e-5


def _dev_ssim(r, d, depth):
    L = (1 << depth) - 1
    a, b = H.ssim_gauss(r, d, L), H.ssim_gauss(r, d, L, dtype=np.float32)
    return abs(a - b) / abs(a), a


def _dev_vif(r, d, depth):
    a, b = V.vif(r, d, depth), V.vif(r, d, depth, dtype=np.float32)
    return max(np.abs(a[2] - b[2]).max(), abs(a[3] - b[3])), a


def _dev_adm(r, d, depth):
    a, b = A.adm(r, d, depth), A.adm(r, d, depth, dtype=np.float32)
    return max(np.abs(a[2] - b[2]).max(), abs(a[3] - b[3])), a


DEV = {"ssim": _dev_ssim, "vif": _dev_vif, "adm": _dev_adm}


@pytest.mark.parametrize("metric", ["ssim", "vif", "adm"])
def test_float32_stays_within_half_the_bar_on_every_entry_of_the_matrix(metric):
    worst = ("", 0.0)
    for tag, r, d, depth in K.case_planes(metric):
        e, ref = DEV[metric](r, d, depth)
        print(metric, tag, "float32 deviation %.2e" % e)
        worst = max(worst, (tag, e), key=lambda x: x[1])
        assert e <= HALF, (metric, tag, e)
        if metric == "ssim":
            assert abs(ref) >= 0.1, (tag, ref)           # the relative bar is well defined
    print(metric, "worst float32 deviation of the matrix: %.2e (%s)" % (worst[1], worst[0]))


def test_the_exclusions_are_few_and_their_deviations():
    """what is left out, per metric: the deviation that keeps it out (the largest over the metric's shapes), and the cap"""
    for metric, excl in K.EXCLUDED.items():
        for depth in K.DEPTHS:
            out = {c for c, d in excl if d == depth}
            assert len(out) <= K.MAX_EXCLUDED, (metric, depth, out)
            assert out <= {K.content_of(n) for n in K.PAIRS_OF[metric]}
        for content, depth in excl:
            for name in [n for n in K.PAIRS_OF[metric] if K.content_of(n) == content]:
                e = max(DEV[metric](*K.pair(name, h, w, depth), depth)[0] for h, w in K.SHAPES[metric])
                print("excluded from", metric, ":", name, depth, "bits, float32 deviation %.2e" % e)
    # the 2-px noisy checkerboard ADM does not take (hostile_cases.PAIRS_OF)
    for depth in K.DEPTHS:
        print("adm, checker2_noisy", depth, "bits, float32 deviation %.2e" % _dev_adm(*K.pair("checker2_noisy", 163, 201, depth), depth)[0])


def test_the_vif_contents_sit_where_they_are_meant_to():
    """checker_inv: s12 < 0 on every sample, scale0 exactly 0; the flat fields: the s1 < 2 branch on every sample (den = the
    sample count); faint2.83: samples on both sides of s1 = 2"""
    for depth in K.DEPTHS:
        h, w = 47, 35
        num, den, scale, _v = V.vif(*K.pair("checker_inv", h, w, depth), depth)
        assert scale[0] == 0.0 and num[0] == 0.0
        for name in ("bright_flat", "dark_flat"):
            num, den, scale, _v = V.vif(*K.pair(name, h, w, depth), depth)
            assert den[0] == h * w and 0.999 < scale[0] < 1.0, (name, depth, den, scale)
        r, _d = K.pair("faint2.83", h, w, depth)
        x = r.astype(np.float64) / (1 << (depth - 8)) - 128.0
        t = V.taps(0)
        s1 = V.filt(x * x, t) - V.filt(x, t) ** 2
        assert 0.1 < (s1 < V.NSQ).mean() < 0.9, (depth, (s1 < V.NSQ).mean())


def test_the_ssim_of_the_anti_correlated_pair_is_negative():
    for depth in K.DEPTHS:
        r, d = K.pair("checker_inv", 67, 259, depth)
        assert H.ssim_gauss(r, d, (1 << depth) - 1) < -0.99


def _brute_sad(prev, curr, rng):
    """-> per interior block (every candidate inside the frame): (set of d2 among the candidates at the minimal SAD, block index)"""
    h, w = curr.shape
    nby, nbx = h // 16, w // 16
    P, Cu = prev.astype(np.int64), curr.astype(np.int64)
    out = []
    for by in range(nby):
        for bx in range(nbx):
            y0, x0 = by * 16, bx * 16
            if y0 - rng < 0 or y0 + 16 + rng > h or x0 - rng < 0 or x0 + 16 + rng > w:
                continue
            sads = {}
            for dy in range(-rng, rng + 1):
                for dx in range(-rng, rng + 1):
                    s = int(np.abs(Cu[y0:y0 + 16, x0:x0 + 16] - P[y0 + dy:y0 + dy + 16, x0 + dx:x0 + dx + 16]).sum())
                    sads.setdefault(s, set()).add(dy * dy + dx * dx)
            out.append((sads[min(sads)], min(sads), by * nbx + bx))
    return out


@pytest.mark.parametrize("name", K.SAD_TIES)
def test_the_sad_contents_tie_and_the_oracle_takes_the_smaller_d2(name):
    seen = 0
    for (h, w), rng in zip(K.BGR_SHAPES, (7, 3)):
        prev, curr = K.gray_pair(name, h, w)
        nb, sad, hist, mv = co.block_sad(prev, curr, rng, want_mv=True)
        blocks = _brute_sad(prev, curr, rng)
        assert blocks, (h, w, rng)
        tied = [b for b in blocks if len(b[0]) >= 2]
        assert 2 * len(tied) >= len(blocks), (name, h, w, len(tied), len(blocks))
        for d2s, _s, k in tied:
            got = int(mv[k][0]) ** 2 + int(mv[k][1]) ** 2
            assert got == min(d2s), (name, k, got, d2s)
            assert got == {"flat_step": 0}.get(name, 1)
        seen += len(tied)
        assert (no.block_sad(prev, curr, rng)[2] == hist).all()
    assert seen >= 3


def test_zero_against_full_is_65280_a_block():
    prev, curr = K.gray_pair("zero_full", 48, 80)
    nb, sad, hist = co.block_sad(prev, curr, 7)
    assert (nb, sad, int(hist[0])) == (15, 15 * 65280, 15)


def test_the_gray_plane_of_a_gray_frame_is_the_plane():
    for name in K.COMPLEXITY:
        for g in K.gray_pair(name, 37, 53):
            assert (co.bgr2gray(K.bgr(g)) == g).all(), name


@pytest.mark.parametrize("h,w", K.BGR_SHAPES)
def test_the_two_canny_oracles_agree_and_the_steps_sit_on_the_thresholds(h, w):
    import scipy.ndimage as ndi
    for name in K.CANNY + K.DEGENERATE:
        g = K.gray_pair(name, h, w)[1]
        for lo, hi in ((100, 200), (20, 60)):
            cnt, strong, weak, emap = co.canny(g, lo, hi, want_map=True)
            ncnt, nstrong, nweak, nmap = no.canny(g, lo, hi)
            assert (cnt, strong, weak) == (ncnt, nstrong, nweak), (name, lo, hi)
            assert ((emap != 0) == (nmap != 0)).all(), (name, lo, hi)
    g = K.gray_pair("canny_steps", h, w)[1].astype(np.int32)
    mag = np.abs(ndi.sobel(g, axis=1, mode="nearest")) + np.abs(ndi.sobel(g, axis=0, mode="nearest"))
    counts = {m: int((mag == m).sum()) for m in (96, 100, 104, 196, 200, 204)}
    print(h, w, "pixels per Sobel L1 magnitude", counts)
    assert all(c > 0 for c in counts.values()), counts
    assert (co.sobel_l1(g.astype(np.uint8))[2] == mag).all()
    # the decisions at equality: a magnitude of exactly `low` is no edge, one of exactly `high` is weak, not strong
    cnt, strong, weak, emap = co.canny(g.astype(np.uint8), 100, 200, want_map=True)
    assert not emap[mag == 100].any() and strong <= int((mag > 200).sum())
    diag = K.gray_pair("diag45", h, w)[1]
    dx, dy, _m = co.sobel_l1(diag)
    assert ((np.abs(dx) == np.abs(dy)) & (dx != 0)).sum() >= min(h, w) // 2      # |gx| = |gy|: the sector boundary


def test_farneback_is_finite_on_static_degenerate_pairs():
    for h, w in K.BGR_SHAPES:
        for name in K.DEGENERATE + ("flat_step",):
            prev, curr = K.gray_pair(name, h, w)
            v, nv = co.farneback(prev, curr), no.farneback_mean_mag(prev, curr)
            print("farneback", name, h, w, "C oracle %.3e NumPy %.3e" % (v, nv))
            assert np.isfinite(v) and np.isfinite(nv) and v >= 0.0, (name, v, nv)


def test_the_generators_are_seeded_and_in_range():
    for depth in K.DEPTHS:
        L = (1 << depth) - 1
        for name in K.PAIRS + ("checker3_noisy", K.ENDS):
            a, b = K.pair(name, 47, 35, depth), K.pair(name, 47, 35, depth)
            for u, v in zip(a, b):
                assert (np.asarray(u) == np.asarray(v)).all() and 0 <= np.min(u) and np.max(u) <= L, (name, depth)
            if name != K.ENDS:
                assert (a[0] != a[1]).any()
    r, d, planes = K.frames(["natural", "checker_inv"], 47, 35, 10, "420")
    assert r.shape == (2, 47 * 35 + 2 * 24 * 18) and r.dtype == np.uint16 and len(planes) == 3
    assert K.bgr_sequence(37, 53).shape == (2 * len(K.COMPLEXITY), 37, 53, 3)
