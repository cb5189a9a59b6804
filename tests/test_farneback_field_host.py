"""CPU side of the per-pixel Farneback check (tests/farneback_field_cases.py, tests/test_gpu_farneback_field.py):
(a) how far the reference is from itself - the C restatement (float32 where OpenCV is) against the float64 restatement - on every
    case: the figure the flow bars are made of;
(b) the seam table is the launchers': their constants are read out of csrc/k_farneback.hip and every seam the cases were chosen
    for is in the table of its shape;
(c) the two checks have teeth where flow_mag_mean has none."""
import numpy as np
import pytest

import farneback_field_cases as fc
from oracle import c_oracle as co

NP_CASES = [c for c in fc.cases() if min(c[0]) >= 10]


# ---- (a) the reference's own distance --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", NP_CASES, ids=fc.case_id)
def test_reference_distance(case, record_property):
    """e = max over pairs, pixels and components of |flow_C - flow_64|.  Measured here on the CPU (flow components: 1 to 3.6 on the
    panned textures, up to 20 on noise):
        panned textures, every shape      6e-7 .. 4.6e-6, no pixel excluded
        noise, 33 x 40 .. 70 x 500        1.9e-6 .. 2.8e-5
        noise, 264 x 520 and 263 x 519    2.6e-4 and 9.4e-4: over the cap, judged on the expansions only"""
    e, (pair, y, x, comp) = fc.measured_e(case)
    print("\n%s: e = %.3g at pair %d, %s, component %d; bar %.3g" % (fc.case_id(case), e, pair, fc.describe(case[0], 0, y, x), comp,
                                                                   fc.bar_of(case)))
    record_property("e", e)
    assert e > 0   # two restatements, two precisions: never the same field
    if case[1] != "noise":
        assert fc.MARGIN * e < fc.CAP, "a panned texture the reference itself is unstable on: choose another"
        assert fc.judged_on_flow(case)
    assert (e > fc.CAP) == (case in fc.EXPANSIONS_ONLY), e
    if case in fc.EXPANSIONS_ONLY:
        assert 0.5 * fc.EXPANSIONS_ONLY[case] < e < 2 * fc.EXPANSIONS_ONLY[case]   # the figure the module states
    bar = fc.bar_of(case)
    assert float(np.spacing(np.float32(np.abs(fc.flow_c(case)[0]).max()))) <= bar <= fc.CAP
    assert bar == fc.CAP or bar == max(fc.MARGIN * e, float(np.spacing(np.float32(np.abs(fc.flow_c(case)[0]).max()))))


def test_the_small_case_borrows_its_distance():
    """9 x 9 has no float64 run (np_oracle is valid from 10 x 10): it is judged against the C oracle with the e of 33 x 40"""
    for content in fc.CONTENTS:
        assert fc.e_of(((9, 9), content)) == fc.measured_e(((33, 40), content))[0]
        assert fc.judged_on_flow(((9, 9), content)) and fc.bar_of(((9, 9), content)) <= fc.CAP
        assert fc.levels_of(9, 9) == fc.levels_of(33, 40) == 0


def test_case_frames():
    for case in fc.cases():
        g, f = fc.gray_frames(case), fc.bgr_frames(case)
        assert g.shape == (fc.PLANES,) + case[0] and f.shape == g.shape + (3,)
        assert all((co.bgr2gray(f[i]) == g[i]).all() for i in range(fc.PLANES))   # the device's gray planes are these
        assert g.std() > 10 and not (g[0] == g[1]).all()
    # the pans are what they say: frame k + 1 is frame k moved by (px, py)
    for name, (_, px, py, _) in fc.PAN.items():
        g = fc.gray_frames(((97, 131), name))
        a = g[1][max(-py, 0):97 - max(py, 0), max(-px, 0):131 - max(px, 0)]
        b = g[0][max(py, 0):97 - max(-py, 0), max(px, 0):131 - max(-px, 0)]
        assert (a == b).all(), name


# ---- the oracle's export ---------------------------------------------------------------------------------------------------------
def test_oracle_expansion_export():
    """co.farneback_expansion runs the lines vqo_farneback_mean_mag runs (one function holds them); its geometry is the cases
    module's, and it is the float32 neighbour of the float64 restatement's expansion"""
    for shape in fc.SHAPES:
        g = fc.gray_frames((shape, "pan"))[0]
        for k in range(fc.levels_of(*shape) + 1):
            r, levels = co.farneback_expansion(g, k)
            assert levels == fc.levels_of(*shape) and r.shape == fc.level_size(shape[0], shape[1], k) + (5,) and r.dtype == np.float32
            assert np.isfinite(r).all() and np.abs(r).max() > 0
        with pytest.raises(ValueError):
            co.farneback_expansion(g, fc.levels_of(*shape) + 1)
    # finest level of a frame: blur with (1/4, 1/2, 1/4) and expand; a plane that is linear in x has b2 = its slope
    h, w = 40, 48
    ramp = np.tile((np.arange(w) * 3).astype(np.uint8), (h, 1))
    r = co.farneback_expansion(ramp, 0)[0]
    assert np.allclose(r[8:-8, 8:-8, 1], 3.0, atol=1e-4) and np.allclose(r[8:-8, 8:-8, 0], 0.0, atol=1e-4)
    assert np.allclose(r[8:-8, 8:-8, 2:], 0.0, atol=1e-4)


def test_read_back_rejects_a_null_context():
    from rtvqa_amd import _native as N
    buf = np.zeros(8, np.float32)
    assert N.load().vqa_debug_read_farneback(None, 0, 0, 0, buf.ctypes.data, 1, 1) == N.VQA_ERR_INVALID


# ---- (b) the seam table ----------------------------------------------------------------------------------------------------------
def test_geometry_constants_are_the_kernels():
    """a change of FI_OUT, PM_OUT or their kin in csrc/k_farneback.hip fails here, not silently"""
    src = fc.source_constants()
    for k, v in src.items():
        assert getattr(fc, k) == v, (k, v)
    assert (fc.FI_OUT, fc.PM_OUT) == (242, 246)


def _has(shape, level, kernel, kind, pos):
    return (level, kernel, kind, pos) in fc.seam_table(shape)


def test_seam_table_has_the_seams_the_shapes_were_chosen_for():
    big, odd, wide = (264, 520), (263, 519), (70, 500)
    assert [fc.level_size(*big, k) for k in range(4)] == [(264, 520), (132, 260), (66, 130), (33, 65)] and fc.levels_of(*big) == 3
    assert [fc.level_size(*odd, k) for k in range(4)] == [(263, 519), (132, 260), (66, 130), (33, 65)] and fc.levels_of(*odd) == 3
    assert [fc.blur_taps(k) for k in range(4)] == [3, 3, 9, 19]
    for shape in (big, odd):
        # the finest level: two interior column seams of each marching kernel
        for kernel, cuts in (("k_fb_iter", (242, 484)), ("k_fb_polyexp_march", (246, 492)), ("k_fb_level3<1>", (256, 512)),
                             ("k_fb_upflow", (256, 512))):
            for x in cuts:
                assert _has(shape, 0, kernel, "col", x), (shape, kernel, x)
        # level 1 (132 x 260): one of each
        for kernel, x in (("k_fb_iter", 242), ("k_fb_polyexp_march", 246), ("k_fb_upflow", 256)):
            assert _has(shape, 1, kernel, "col", x), (shape, kernel, x)
        # levels 2 and 3: the tiled kernel with 9 and 19 taps, 32 x 8 level pixels per tile
        for k, (lh, lw) in ((2, (66, 130)), (3, (33, 65))):
            assert fc.level_kernel(3, *shape, k) == ("k_fb_level<2,16>", 32, 8)
            assert _has(shape, k, "k_fb_level<2,16>", "col", 32) and _has(shape, k, "k_fb_level<2,16>", "col", lw - lw % 32)
            assert _has(shape, k, "k_fb_level<2,16>", "row", 8) and _has(shape, k, "k_fb_level<2,16>", "row", 32)
        # row strips: k_fb_iter's are multiples of 16 (and restarts lie between them), k_fb_polyexp_march's at least 32 rows,
        # k_fb_level3's multiples of 4, k_fb_upflow's tiles 8 rows
        rows = [(k, n, p) for k, n, kind, p in fc.seam_table(shape) if kind == "row"]
        assert any(k == 0 and n == "k_fb_iter" for k, n, p in rows) and all(p % 16 == 0 for k, n, p in rows if n == "k_fb_iter")
        assert any(k == 0 and n == "k_fb_polyexp_march" and p >= 32 for k, n, p in rows)
        assert any(k == 0 and n == "k_fb_level3<1>" for k, n, p in rows) and all(p % 4 == 0 for k, n, p in rows if n.startswith("k_fb_level3"))
        assert _has(shape, 0, "k_fb_upflow", "row", 8) and _has(shape, 0, "k_fb_iter", "restart", 16)
    # exact halving against the bilinear tile kernel at level 1
    assert fc.level_kernel(3, *big, 0)[0] == fc.level_kernel(3, *odd, 0)[0] == "k_fb_level3<1>"
    assert fc.level_kernel(3, *big, 1)[0] == "k_fb_level3<2>" and _has(big, 1, "k_fb_level3<2>", "col", 256)
    assert fc.level_kernel(3, *odd, 1) == ("k_fb_level<2,64>", 31, 31)
    assert _has(odd, 1, "k_fb_level<2,64>", "col", 31) and _has(odd, 1, "k_fb_level<2,64>", "col", 248) and _has(odd, 1, "k_fb_level<2,64>", "row", 124)
    # 70 x 500: one coarser level, wide and short
    assert fc.levels_of(*wide) == 1 and fc.level_size(*wide, 1) == (35, 250) and fc.level_kernel(3, *wide, 1)[0] == "k_fb_level3<2>"
    for kernel, cuts in (("k_fb_iter", (242, 484)), ("k_fb_polyexp_march", (246, 492)), ("k_fb_level3<1>", (256,)), ("k_fb_upflow", (256,))):
        for x in cuts:
            assert _has(wide, 0, kernel, "col", x)
    assert _has(wide, 1, "k_fb_iter", "col", 242) and _has(wide, 1, "k_fb_polyexp_march", "col", 246)
    assert fc.iter_geometry(fc.PAIRS, 35, 250)[1] == 1 and fc.polyexp_geometry(fc.PLANES, 35, 250)[1] == 1   # one strip at level 1
    # the small ones: one column block, the replicated / reflected edges are all there is
    assert fc.levels_of(97, 131) == 1 and fc.level_kernel(3, 97, 131, 1)[0] == "k_fb_level<2,64>"
    assert fc.levels_of(33, 40) == 0 and fc.levels_of(9, 9) == 0
    for shape in ((33, 40), (9, 9)):
        assert not [s for s in fc.seam_table(shape) if s[2] == "col"]
    # batch independence: k_fb_iter picks its strips from the pair count.  At 264 x 520 a pair alone, the 2-pair case and a 9-pair
    # batch all march 6 strips of 48 rows (three column blocks: 18 workgroups per pair, far below the 768 resident at once); the
    # strips change once a batch no longer fits one residency round, from 43 pairs on - MANY_PAIRS marches 5 strips of 64 rows
    assert fc.iter_geometry(1, *big)[1:] == fc.iter_geometry(fc.PAIRS, *big)[1:] == fc.iter_geometry(fc.NINE_PAIRS, *big)[1:] == (6, 48)
    assert fc.iter_geometry(42, *big)[1:] == (6, 48) and fc.iter_geometry(fc.MANY_PAIRS, *big)[1:] == (5, 64)


def test_seams_beside():
    assert "k_fb_iter col 242" in fc.seams_beside((264, 520), 0, 100, 241) and "k_fb_iter col 242" in fc.seams_beside((264, 520), 0, 100, 242)
    assert "k_fb_iter col 242" not in fc.seams_beside((264, 520), 0, 100, 243)
    assert "k_fb_polyexp_march col 246" in fc.describe((264, 520), 0, 3, 250) and "top" in fc.describe((264, 520), 0, 3, 250)


# ---- (c) teeth -------------------------------------------------------------------------------------------------------------------
SEAM_COLUMNS = {(264, 520): (241, 242, 246, 256, 484, 492, 512), (263, 519): (242, 245, 255), (70, 500): (242, 246, 484)}


@pytest.mark.parametrize("shape", list(SEAM_COLUMNS), ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("content", ["pan", "pan2"])
def test_a_wrong_seam_column_is_caught_by_the_field_and_not_by_the_mean(shape, content):
    """One column beside a seam 1 % off: the per-pixel bar rejects it; the mean magnitude moves by less than the 1e-4 relative that
    test_farneback_motion_parity allows, which is why that test cannot see it."""
    case = (shape, content)
    want = fc.flow_c(case)[0][0]
    bar = fc.bar_of(case)
    assert fc.flow_gap(want, want)[0] == 0.0 <= bar
    for x in SEAM_COLUMNS[shape]:
        assert fc.seams_beside(shape, 0, 0, x), x
        bad = want.copy()
        bad[:, x, :] *= np.float32(1.01)
        gap, (y, xx, comp) = fc.flow_gap(bad, want)
        assert gap > bar and xx == x, (x, gap, bar)                    # the field check sees it, and says where
        assert gap > 100 * bar                                         # by a wide margin: 1 % of a 2-pixel flow against a bar of ~1e-5
        m0, m1 = fc.fixed_point_mean(want)[0], fc.fixed_point_mean(bad)[0]
        assert 0 < abs(m1 - m0) < 1e-4 * m0, (x, m0, m1)               # the mean does not


def test_the_fixed_point_mean_is_the_oracles_mean():
    for case in (((264, 520), "pan"), ((33, 40), "noise")):
        f, means = fc.flow_c(case)
        for p in range(fc.PAIRS):
            m, t = fc.fixed_point_mean(f[p])
            assert abs(m - means[p]) <= 2.0 ** -29 + 1e-15 * means[p]   # half a quantum per pixel at the most, on average


def test_one_wrong_value_in_an_expansion_is_caught_and_located():
    case = ((263, 519), "pan")
    for level, (y, x, c) in ((0, (17, 246, 3)), (1, (130, 31, 0)), (3, (32, 64, 4))):
        want = fc.expansion_c(case, 1, level)
        assert fc.first_difference(want, want.copy()) is None
        bad = want.copy()
        bad[y, x, c] = np.nextafter(bad[y, x, c], np.float32(np.inf))   # one unit in the last place
        assert fc.first_difference(bad, want) == (y, x, c)
        assert abs(float(bad[y, x, c]) - float(want[y, x, c])) <= 1e-6 * max(abs(float(want[y, x, c])), 1e-30) + 1e-44
    # -0.0 against 0.0 and NaN payloads are differences too: the comparison is of bits
    a = np.zeros((2, 2, 5), np.float32)
    b = a.copy()
    b[1, 0, 2] = -0.0
    assert fc.first_difference(b, a) == (1, 0, 2)
