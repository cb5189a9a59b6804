"""CPU: the full-frame DCT's parity matrix (tests/dct_full_cases.py) is sound before it is run on a GPU - every class of the three
launchers has a case, the planner's list of lengths is what the cases were placed against, the float64 reference is stable on
every frame it judges, and each probe moves the judged L1 by ten bars or more when the defect it was built for is applied to the
reference's own arrays.  tests/test_gpu_dct_full.py is the GPU side.

What an impulse cannot see: its spectrum is 40 c_u(y) c_v(x), so its L1 is 40 S_h(y) S_w(x) with S_n(i) = sum_k |c_k(i)|, and for
n a power of two S_n is the same for every i (to 1e-14 at n = 128 and 3e-13 at 2048; it varies by 2e-4 at n = 4000, 5 % at 150
and 21 % at 135).  An impulse tests how a sample is WEIGHTED - a sample skipped, read twice or scaled - not WHERE it is: two
samples exchanged give the same L1 on such a side.  Place is the natural content's job (a row dropped moves its L1 by 3.2e-3 ..
5e-2) and the cosines' (a frequency's twiddles: 2.6e-3 .. 1e-2).

The reference alone: SciPy's float32 dctn against its float64 one, below a tenth of the bar on every frame and pair - at most
6.5e-7 on energy and 4.0e-6 on L1 (135 x 241, cosine (134, 0)).  The float32 run takes the row pass first, as the kernels do
(DC.dct2).  The order matters in float32 and on one item decides the check: the cosine (0, 384) of 257 x 385 is constant along
y, its spectrum one row of 385 coefficients with L1 = 7624, while the samples themselves have sum |x| sqrt(257) = 117000.  The
second pass leaves rounding noise relative to what the first pass hands it.  Rows first, the column pass meets the sparse row
spectrum and its noise on the 256 x 385 coefficients that are exactly 0 is 2.1e-6 of L1; columns first (SciPy's default order),
the 257-point pass - a prime length, where SciPy's float32 transform leaves 1.8e-6 per unit of DC against 2.4e-7 at 255 - meets
the dense samples, and |.| adds its noise up to 1.14e-5 of L1.  test_the_order_of_the_passes prints both and holds the two
passes written out as scipy.fft.dct calls to the same bound."""
import numpy as np
import pytest

import dct_full_cases as DC

TEETH = 10 * DC.RTOL        # a defect must move the judged L1 by ten bars
ANGLE = 1e-2                # radians, the rotation of a cosine's main coefficient


def test_path_of_gives_every_case_the_class_it_was_placed_for():
    for c in DC.CASES:
        assert DC.path_of(c.h, c.w) == c.path, (DC.case_id(c), c.why, DC.path_of(c.h, c.w))
        if c.radices is not None:
            assert tuple(DC.fft_radices(c.w)) == c.radices, (DC.case_id(c), DC.fft_radices(c.w))
    for (h, w) in DC.PROBED:
        assert any((c.h, c.w) == (h, w) for c in DC.CASES), (h, w)
    assert len({DC.case_id(c) for c in DC.CASES}) == len(DC.CASES)


def test_every_class_of_the_three_launchers_has_a_case_and_a_probed_plane():
    paths = {c.path for c in DC.CASES}
    assert {"valu", "mfma"} <= paths
    fft = [p for p in paths if p[0] == "fft"]
    assert {p[1] for p in fft} == {"rows<2048,256>", "rows<4096,512>"}
    assert {p[2] for p in fft} == {"cols8<1152>", "cols8<2048>", "cols<false>"}     # cols<true>: test_the_planners_list
    probed = {DC.path_of(h, w) for (h, w) in DC.PROBED}
    assert {"valu", "mfma"} <= probed
    assert {p[1] for p in probed if p[0] == "fft"} == {"rows<2048,256>", "rows<4096,512>"}
    assert {p[2] for p in probed if p[0] == "fft"} == {"cols8<1152>", "cols8<2048>", "cols<false>"}
    # every radix occurs in a row transform and in a column transform, and a plan without a radix-8 or radix-4 pass in both
    for side in (lambda c: c.w, lambda c: c.h):
        plans = [DC.fft_radices(side(c)) for c in DC.CASES if c.path[0] == "fft"]
        assert {r for p in plans for r in p} == {8, 4, 2, 3, 5}
        assert any(not {8, 4} & set(p) for p in plans)
    # the mixed class both ways, the neighbours of h >= 128 && w >= 128, and AUTO's edge
    sizes = {(c.h, c.w): c.path for c in DC.CASES}
    assert sizes[(127, 128)] == sizes[(128, 127)] == "valu" and sizes[(128, 129)] == "mfma"
    assert any(c.path == "valu" and c.h < 128 <= c.w for c in DC.CASES) and any(c.path == "valu" and c.w < 128 <= c.h for c in DC.CASES)
    assert DC.auto_is_full(64, 256) and not DC.auto_is_full(64, 258)
    # an odd lda leaves three rows in four off load8's 16-byte alignment; a last k-step with one valid column, in both products
    assert any(c.path == "mfma" and c.h % 16 == 1 and c.w % 16 == 1 for c in DC.CASES)
    assert all(c.h % 2 or c.w % 2 for c in DC.CASES if c.path == "mfma")


def test_the_planners_list():
    L = DC.fft_lengths()
    assert len(L) == 82 and L[0] == 128 and L[-1] == 4000
    assert max(len(DC.fft_radices(n)) for n in L) == 7 == len(DC.fft_radices(1458))
    # the class bounds: h <= 2040, h <= 1152, w <= 2048 - each tested length is the admitted neighbour of one
    assert max(n for n in L if n <= 2040) == 2000 and min(n for n in L if n > 2040) == 2048
    assert max(n for n in L if n <= 1152) == 1152 and min(n for n in L if n > 1152) == 1200
    assert max(n for n in L if n <= 2048) == 2048 and min(n for n in L if n > 2048) == 2160
    # k_dct_fft_cols<true> needs 2040 < h <= (65536 - 64) / 32 = 2046: 2042 = 2 * 1021, 2044 = 4 * 7 * 73, 2046 = 2 * 3 * 11 * 31,
    # so no admitted height takes it - unreachable through the C ABI
    assert not [n for n in L if 2041 <= n <= 2046]
    assert all(DC.cols_class(n) != "cols<true>" for n in L)
    assert (2042, 2044, 2046) == (2 * 1021, 4 * 7 * 73, 2 * 3 * 11 * 31)
    # every admitted length fits the default 64 KiB of LDS in both kernels; 2000 and 4000 are the two tightest
    for n in L:
        rows, cols = DC.lds_bytes(n, n)
        assert rows <= 32000 and cols <= 64032, (n, rows, cols)
    assert DC.lds_bytes(2000, 128)[1] == DC.lds_bytes(4000, 128)[1] == 64032 and DC.lds_bytes(128, 4000)[0] == 32000


# ---- the reference alone ---------------------------------------------------------------------------------------------------------
def _ratios(planes):
    """planes [k, h, w] in batch order -> the largest float32-to-float64 ratio on energy and on L1.  L1 is taken as the kernels
    take it, on the difference plane (an exact integer): two float32 transforms of whole planes leak the rounding noise of the
    large plane into the small difference (csrc/k_dct_fft.hip, "Packing history")"""
    e = l = 0.0
    p = planes.astype(np.int64)
    for i in range(1, len(p)):
        e = max(e, DC.rel(DC.energy(p[i], np.float32), DC.energy(p[i])))
        d = p[i - 1] - p[i]
        if d.any():
            l = max(l, DC.rel(float(np.abs(DC.dct2(d, np.float32)).astype(np.float64).sum()), float(np.abs(DC.dct2(d)).sum())))
    return e, l


@pytest.mark.parametrize("case", DC.CASES, ids=DC.case_id)
def test_the_reference_alone_is_stable_on_the_natural_content(case):
    e, l = _ratios(DC.planes_of(case))
    print("reference, float32 against float64, %s: energy %.2e, L1 %.2e" % (DC.case_id(case), e, l))
    assert e < DC.RTOL / 10 and l < DC.RTOL / 10


@pytest.mark.parametrize("h,w", DC.PROBED, ids=lambda v: str(v))
def test_the_reference_alone_is_stable(h, w):
    """on the probe frames"""
    pr = DC.probes(h, w)
    g = DC.probe_batch(h, w)[..., 0]
    worst = (0.0, None)
    e = 0.0
    for k, probe in enumerate(pr):
        ek, lk = _ratios(g[2 * k:2 * k + 2])
        e = max(e, ek)
        worst = max(worst, (lk, probe))
    print("reference, float32 against float64, probes of %d x %d: energy %.2e, L1 %.2e at %s" % (h, w, e, worst[0], worst[1]))
    assert e < DC.RTOL / 10 and worst[0] < DC.RTOL / 10, worst


@pytest.mark.parametrize("h,w", DC.PROBED, ids=lambda v: str(v))
def test_the_order_of_the_passes(h, w):
    """DC.dct2 takes the row pass first, as the kernels do.  The judged float64 value does not depend on the order; the float32
    one does, and the same bound holds for the two passes written out as two scipy.fft.dct calls, rows first.  The figure of the
    other order is printed: what a float32 pipeline that ran the columns first would be held against"""
    import scipy.fft
    cols_first = (0, 1)
    worst64, two_pass, other = 0.0, (0.0, None), (0.0, None)
    for probe in DC.probes(h, w):
        d = DC.probe_plane(h, w, probe) - DC.base_plane(h, w)
        want = _l1(d)
        worst64 = max(worst64, DC.rel(float(np.abs(DC.dct2(d, axes=cols_first)).sum()), want))
        x = d.astype(np.float32)
        y = scipy.fft.dct(scipy.fft.dct(x, axis=1, norm="ortho"), axis=0, norm="ortho")
        two_pass = max(two_pass, (DC.rel(float(np.abs(y).astype(np.float64).sum()), want), probe))
        other = max(other, (DC.rel(float(np.abs(DC.dct2(d, np.float32, axes=cols_first)).astype(np.float64).sum()), want), probe))
    print("order of the passes, probes of %d x %d: float64 either way %.1e; float32 as two scipy.fft.dct passes, rows first, %.2e at %s; "
          "float32 dctn, columns first, %.2e at %s" % (h, w, worst64, two_pass[0], two_pass[1], other[0], other[1]))
    assert worst64 < 1e-12
    assert two_pass[0] < DC.RTOL / 10, two_pass


# ---- teeth -----------------------------------------------------------------------------------------------------------------------
def _l1(d):
    return float(np.abs(DC.dct2(d)).sum())


@pytest.mark.parametrize("h,w", DC.PROBED, ids=lambda v: str(v))
def test_an_impulse_sees_its_samples_weight(h, w):
    """the pixel weighted 0 or 2 in the pair's difference, and the closed form 40 S_h(y) S_w(x)"""
    least = 1.0
    for (y, x) in DC.impulses(h, w):
        d = (DC.probe_plane(h, w, ("impulse", (y, x))) - DC.base_plane(h, w)).astype(np.float64)
        assert d[y, x] == DC.IMPULSE and np.count_nonzero(d) == 1
        want = _l1(d)
        assert DC.rel(DC.IMPULSE * DC.basis_l1(h)[y] * DC.basis_l1(w)[x], want) < 1e-12
        for weight in (0.0, 2.0):
            bad = d.copy()
            bad[y, x] *= weight
            least = min(least, DC.rel(_l1(bad), want))
    print("teeth, impulses of %d x %d: a weight of 0 or 2 moves L1 by at least %.3f" % (h, w, least))
    assert least >= TEETH


@pytest.mark.parametrize("h,w", DC.PROBED, ids=lambda v: str(v))
def test_a_cosine_sees_its_frequencys_twiddle(h, w):
    """the main coefficient rotated by 1e-2 rad against a neighbour: energy stays, as under a wrong twiddle, and L1 moves by
    about share * (cos t + sin t - 1)"""
    least, least_share = 1.0, 1.0
    for (u, v) in DC.cosines(h, w):
        D = DC.dct2(DC.cosine_plane(h, w, u, v))
        want = float(np.abs(D).sum())
        share = abs(D[u, v]) / want
        assert abs(D[u, v]) == np.abs(D).max()
        nv = v - 1 if v else v + 1
        a, b = D[u, v], D[u, nv]
        bad = D.copy()
        bad[u, v], bad[u, nv] = a * np.cos(ANGLE) - b * np.sin(ANGLE), a * np.sin(ANGLE) + b * np.cos(ANGLE)
        assert DC.rel(float((bad ** 2).sum()), float((D ** 2).sum())) < 1e-12
        move = DC.rel(float(np.abs(bad).sum()), want)
        print("teeth, cosine (%d, %d) of %d x %d: share %.3f, a rotation by %.0e rad moves L1 by %.2e (share * (cos + sin - 1) = %.2e)" % (
            u, v, h, w, share, ANGLE, move, share * (np.cos(ANGLE) + np.sin(ANGLE) - 1)))
        least, least_share = min(least, move), min(least_share, share)
    assert least_share > 0.25 and least >= TEETH, (least_share, least)


@pytest.mark.parametrize("case", DC.CASES, ids=DC.case_id)
def test_the_natural_content_sees_a_dropped_row(case):
    """one input row of the pair's difference read as 0.  The row's own share of L1 goes and the notch's broadband spectrum comes,
    and on one pair the two can cancel (128 x 2160, row 64 of the second pair: 4.7e-4); the GPU test judges every pair of a case,
    so a row counts as seen when one of the case's three pairs moves by ten bars"""
    p = DC.planes_of(case).astype(np.float64)
    d = [p[i - 1] - p[i] for i in range(1, len(p))]
    want = [_l1(x) for x in d]
    least = 1.0
    for r in (0, 1, case.h // 2, case.h - 2, case.h - 1):
        seen = 0.0
        for x, l in zip(d, want):
            bad = x.copy()
            bad[r] = 0.0
            seen = max(seen, DC.rel(_l1(bad), l))
        least = min(least, seen)
    print("teeth, natural content of %s: a dropped row moves L1 by at least %.2e" % (DC.case_id(case), least))
    assert least >= TEETH


def test_what_an_impulse_cannot_see():
    """S_n(i) does not depend on i when n is a power of two: an impulse tests a sample's weight, not its place"""
    for n, flat in ((128, True), (2048, True), (150, False), (135, False), (4000, False)):
        s = DC.basis_l1(n)
        spread = float(np.ptp(s) / s.mean())
        print("S_%d: %.6f .. %.6f, spread %.1e" % (n, s.min(), s.max(), spread))
        assert (spread < 1e-12) == flat
    assert float(np.ptp(DC.basis_l1(128)) / DC.basis_l1(128).mean()) < 1e-13
