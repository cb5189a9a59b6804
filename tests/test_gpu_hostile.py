"""GPU: every kernel on hostile content (tests/hostile_cases.py) against the references the suite already uses, at the suite's
own bars.  Flat fields at the ends of the range, anti-correlated pairs, faint texture around VIF's s1 = 2, equal SADs, Sobel
magnitudes on Canny's thresholds, 0 against the maximum.  tests/test_hostile_host.py shows on the CPU that every (content,
depth, metric) compared here is a fair test of a kernel: the reference's own float32 run stays within half the bar.  The shapes
are the suite's small ones: they cross a tile seam and leave a ragged edge.  Every comparison prints its error; the last test
prints the worst gap per metric (DESIGN.md section 3 quotes them)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import adm_reference as A
import hbd_reference as H
import hostile_cases as K
import motion_cases as MC
import motion_reference as MO
import msssim_reference as MS
import vif_reference as V
from oracle import c_oracle as co
from oracle import pipeline as pl

pytestmark = pytest.mark.gpu

RTOL = 1e-4               # SSIM and DCT floats (tests/test_gpu_parity.py, tests/test_gpu_quality_hbd.py)
BAR = 1e-4                # absolute: VIF and ADM scales, MS-SSIM's per-level means
MOTION_BAR = 26 * 2.0 ** -17          # tests/test_gpu_motion.py
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORST = {}


def _note(metric, gap, tag):
    if gap >= WORST.get(metric, (-1.0, ""))[0]:
        WORST[metric] = (float(gap), tag)


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-30)


def _ids(cases):
    return ["%s-%d-%dx%d-%s" % c for c in cases]


def _check_quality(res, r, d, planes, mode, depth, tag):
    """SSE exact, SSIM within RTOL of tests/hbd_reference.py and, at 8 bits, of the C oracle.  vf_ssim at 8 bits is measured
    against the C oracle alone: FFmpeg's 8-bit path takes its constants as integers (ssim_c1 = 416, ssim_c2 = 235963), the
    high-depth path hbd_reference restates takes them as floats (416.16..).  Texture does not notice; all L against all 0, whose
    SSIM is c1 / (s1^2 + c1), is 3.8e-4 apart between the two, and the device follows the 8-bit path at 8 bits (the gap to the
    high-depth form is printed)."""
    metric = "ssim_gauss" if mode == "gauss" else "vf_ssim"
    for i in range(r.shape[0]):
        sse, ssim = H.frame_quality(r[i], d[i], planes, mode, depth)
        refs = [ssim]
        if depth == 8:
            sse8, ssim8 = pl.frame_quality(r[i], d[i], planes, mode)
            assert sse8 == sse
            refs = [ssim, ssim8] if mode == "gauss" else [ssim8]
        for p in range(len(planes)):
            got = float(res[i, p]["ssim"])
            gaps = [_rel(got, w[p]) for w in refs]
            print(tag, mode, "plane", p, "sse", int(res[i, p]["sse"]), "ssim %.9f ref %.9f" % (got, ssim[p]), "rel", " ".join("%.2e" % g for g in gaps),
                  "to hbd_reference %.2e" % _rel(got, ssim[p]))
            _note(metric, max(gaps), tag)
            assert int(res[i, p]["sse"]) == sse[p], (tag, p, int(res[i, p]["sse"]), sse[p])
            assert max(gaps) <= RTOL, (tag, p, got, [w[p] for w in refs])


# ---- Gaussian SSIM, vf_ssim, SSE ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,depth,h,w,chroma", K.cases("ssim"), ids=_ids(K.cases("ssim")))
def test_gaussian_ssim_and_sse(engine, name, depth, h, w, chroma):
    from rtvqa_amd import _native as N
    r, d, planes = K.frames(name, h, w, depth, chroma)
    _check_quality(engine.quality(r, d, planes, N.SSIM_GAUSS), r, d, planes, "gauss", depth, "%s %d bits" % (name, depth))


@pytest.mark.parametrize("name,depth,h,w,chroma", K.cases("ssim"), ids=_ids(K.cases("ssim")))
def test_vf_ssim_and_sse(engine, name, depth, h, w, chroma):
    from rtvqa_amd import _native as N
    r, d, planes = K.frames(name, h, w, depth, chroma)
    _check_quality(engine.quality(r, d, planes, N.SSIM_FFMPEG), r, d, planes, "ffmpeg", depth, "%s %d bits" % (name, depth))


@pytest.mark.parametrize("depth", K.DEPTHS)
def test_the_ends_of_the_range(engine, depth):
    """all L against all 0 (SSE = L^2 h w: the largest a plane can have), all L against all L, all 0 against all 0: vf_ssim at the
    bar, SSE exact, identical planes exactly 1.0 in vf_ssim and 1 within 1e-6 in the Gaussian window (the suite's known answer)"""
    from rtvqa_amd import _native as N
    h, w = 67, 259
    L = (1 << depth) - 1
    r, d, planes = K.frames(K.ENDS, h, w, depth)
    res = engine.quality(r, d, planes, N.SSIM_FFMPEG)
    assert int(res[0, 0]["sse"]) == L * L * h * w
    _check_quality(res, r, d, planes, "ffmpeg", depth, "%s %d bits" % (K.ENDS, depth))
    assert int(engine.quality(r, d, planes, N.SSIM_GAUSS)[0, 0]["sse"]) == L * L * h * w
    for x in (r, d):
        same = engine.quality(x, x, planes, N.SSIM_FFMPEG)
        assert int(same[0, 0]["sse"]) == 0 and float(same[0, 0]["ssim"]) == 1.0
        same = engine.quality(x, x, planes, N.SSIM_GAUSS)
        assert int(same[0, 0]["sse"]) == 0 and abs(float(same[0, 0]["ssim"]) - 1.0) <= 1e-6
    for name in K.PAIRS:        # identical hostile planes
        x = K.frames(name, h, w, depth)[0]
        same = engine.quality(x, x, planes, N.SSIM_FFMPEG)
        assert int(same[0, 0]["sse"]) == 0 and float(same[0, 0]["ssim"]) == 1.0, name


# ---- MS-SSIM --------------------------------------------------------------------------------------------------------------------
MS_CASES = [(n, d, 170, 161, "mono") for d in K.DEPTHS for n in K.PAIRS] + [("checker2_noisy", 8, 322, 324, "420")]


@pytest.mark.parametrize("name,depth,h,w,chroma", MS_CASES, ids=_ids(MS_CASES))
def test_msssim(engine, name, depth, h, w, chroma):
    from rtvqa_amd import _native as N
    r, d, planes = K.frames(name, h, w, depth, chroma)
    res, cs, ssim = engine.quality(r, d, planes, N.SSIM_MS, scales=True)
    sse_w, cs_w, ssim_w, ms_w = MS.frame_msssim(r[0], d[0], planes, depth)
    for p in range(len(planes)):
        ec, es = np.abs(cs[0, p] - cs_w[p]).max(), np.abs(ssim[0, p] - ssim_w[p]).max()
        got = float(res[0, p]["ssim"])
        print(name, depth, "plane", p, "cs err %.2e ssim err %.2e" % (ec, es), "ms %.9f ref %.9f" % (got, ms_w[p]))
        _note("msssim per-level mean", max(ec, es), "%s %d bits" % (name, depth))
        assert int(res[0, p]["sse"]) == sse_w[p]
        assert ec <= BAR and es <= BAR, (p, cs[0, p], cs_w[p], ssim[0, p], ssim_w[p])
        own = MS.combine(cs[0, p], ssim[0, p])
        assert abs(got - own) <= 1e-12 * own, (p, got, own)
        bound = MS.value_bound(cs_w[p], ssim_w[p], BAR)
        if bound is not None:
            _note("msssim value", abs(got - ms_w[p]), "%s %d bits" % (name, depth))
            assert abs(got - ms_w[p]) <= bound, (p, got, ms_w[p], bound)
        if min(list(cs_w[p][:4]) + [ssim_w[p][4]]) < -1e-3:
            assert got == 0.0, (p, got)
    if name == "checker_inv":
        assert cs_w[0][0] < -0.99 and float(res[0, 0]["ssim"]) == 0.0      # a negative level-0 mean: exactly 0, not NaN


# ---- VIF ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,depth,h,w,chroma", K.cases("vif"), ids=_ids(K.cases("vif")))
def test_vif(engine, name, depth, h, w, chroma):
    r, d, planes = K.frames(name, h, w, depth, chroma)
    got = engine.vif(r, d, planes)
    tag = "%s %d bits %dx%d" % (name, depth, h, w)
    for p, pln in enumerate(planes):
        num, den, scale, vif = V.vif(K.plane_of(r[0], pln), K.plane_of(d[0], pln), depth)
        g = got[0, p]
        es, ev = np.abs(g["scale"] - scale).max(), abs(float(g["vif"]) - vif)
        print(tag, "plane", p, "scale", np.round(scale, 6), "vif %.6f" % vif, "err scale %.2e vif %.2e" % (es, ev))
        _note("vif", max(es, ev), tag)
        assert np.isfinite(g["num"]).all() and np.isfinite(g["den"]).all() and np.isfinite(g["scale"]).all() and np.isfinite(g["vif"])
        assert es <= BAR, (tag, p, g["scale"], scale)
        assert ev <= BAR, (tag, p, float(g["vif"]), vif)
        assert np.abs(g["num"] - num).max() <= BAR * den.max() and np.abs(g["den"] - den).max() <= BAR * den.max()
        if name == "checker_inv":
            assert scale[0] == 0.0 and abs(g["scale"][0]) <= BAR      # s12 < 0 on every sample of the plane


# ---- ADM ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,depth,h,w,chroma", K.cases("adm"), ids=_ids(K.cases("adm")))
def test_adm(engine, name, depth, h, w, chroma):
    import test_gpu_adm as TA
    r, d, planes = K.frames(name, h, w, depth, chroma)
    got = engine.adm(r, d, planes)
    tag = "%s %d bits %dx%d" % (name, depth, h, w)
    for p, pln in enumerate(planes):
        _num, _den, scale, adm2 = A.adm(K.plane_of(r[0], pln), K.plane_of(d[0], pln), depth)
        _note("adm", max(np.abs(got[0, p]["scale"] - scale).max(), abs(float(got[0, p]["adm2"]) - adm2)), tag)
    TA._check(got, r, d, planes, depth, tag, count=False)        # the plain bar: admissible content needs no widened one


# ---- the motion feature and SI / TI ---------------------------------------------------------------------------------------------
CLIPS = [(n, d, 75, 93, "mono") for d in K.DEPTHS for n in K.PAIRS] + [(K.ENDS, 16, 75, 93, "mono"), (K.ENDS, 8, 75, 93, "mono"),
                                                                        ("checker_inv", 10, 75, 93, "420")]


@pytest.mark.parametrize("name,depth,h,w,chroma", CLIPS, ids=_ids(CLIPS))
def test_motion_feature(engine, name, depth, h, w, chroma):
    f, planes = K.clip(name, h, w, depth, chroma)
    got = engine.motion(f, planes)
    want = np.stack([MO.motion(MC.plane_series(f, p), depth) for p in planes], axis=1)
    gap = np.abs(got["motion"] - want)
    print(name, depth, "motion", np.round(want[1], 6).tolist(), "gap %.3e" % gap.max(), "bar %.3e" % MOTION_BAR)
    _note("motion", gap.max(), "%s %d bits" % (name, depth))
    assert (got[0]["motion"] == 0.0).all()
    assert gap.max() <= MOTION_BAR, (name, depth, gap)
    area = np.array([p[0] * p[1] for p in planes], np.float64)
    assert np.array_equal(got["motion"], got["sad"] / area)
    assert (got["sad"] * 65536.0 == np.rint(got["sad"] * 65536.0)).all()
    if name == K.ENDS:           # every blurred sample moves by 255.99.. (tap sum)^2
        assert abs(float(got[1, 0]["motion"]) - ((1 << depth) - 1) / float(1 << (depth - 8)) * sum(MO.TAPS) ** 2) <= MOTION_BAR


@pytest.mark.parametrize("name,depth,h,w,chroma", CLIPS, ids=_ids(CLIPS))
def test_si_ti(engine, name, depth, h, w, chroma):
    import test_gpu_siti as TS
    f, planes = K.clip(name, h, w, depth, chroma)
    got = engine.siti(f, planes)
    keep = dict(TS.WORST)
    TS.WORST.update(si=0.0, ti=0.0, quanta=0, tag="")
    try:
        TS._check(got, f, planes, depth, "%s %d bits" % (name, depth))     # the integer words exact, si / ti at that file's bars
        _note("si", TS.WORST["si"], "%s %d bits" % (name, depth))
        _note("ti", TS.WORST["ti"], "%s %d bits" % (name, depth))
        _note("si quanta off", TS.WORST["quanta"], "%s %d bits" % (name, depth))
    finally:
        TS.WORST.clear()
        TS.WORST.update(keep)
    if name == K.ENDS:
        L = (1 << depth) - 1
        assert int(got[1, 0]["diff_sum"]) == -L * h * w and int(got[1, 0]["diff_sq"]) == L * L * h * w and float(got[1, 0]["ti"]) == 0.0


# ---- the complexity suite -----------------------------------------------------------------------------------------------------
def _complexity(engine, *a, **kw):
    rec = engine.complexity(*a, **kw)
    assert not rec["hyst_overflow"].any()
    return rec


def _check_sad(rec, seq, rng, tag):
    for i in range(rec.shape[0]):
        nb, sad, hist = co.block_sad(co.bgr2gray(seq[i]), co.bgr2gray(seq[i + 1]), rng)
        got = (int(rec[i]["sad_blocks"]), int(rec[i]["sad_sum"]))
        print(tag, "range", rng, "frame", i, "blocks, sad", got, "d2 bins", np.nonzero(rec[i]["mv_d2_hist"])[0].tolist())
        assert got == (nb, sad), (tag, rng, i, got, (nb, sad))
        assert (rec[i]["mv_d2_hist"] == hist).all(), (tag, rng, i, np.nonzero(rec[i]["mv_d2_hist"])[0], np.nonzero(hist)[0])


@pytest.mark.parametrize("rng", [7, 3])
@pytest.mark.parametrize("h,w", K.BGR_SHAPES)
def test_block_sad_ties_and_ends(engine, h, w, rng):
    """every content's (prev, curr) and the seams between contents: equal SADs go to the smaller d^2, 0 against 255 is 65280 a block"""
    from rtvqa_amd import _native as N
    seq = K.bgr_sequence(h, w)
    rec = _complexity(engine, seq[1:], prev0=seq[0], mask=N.M_MOTION, sad_range=rng)
    _check_sad(rec, seq, rng, "%dx%d" % (h, w))
    k = 2 * K.COMPLEXITY.index("zero_full")
    assert int(rec[k]["sad_sum"]) == 65280 * (h // 16) * (w // 16)
    k = 2 * K.COMPLEXITY.index("flat_step")
    assert int(rec[k]["mv_d2_hist"][0]) == (h // 16) * (w // 16)


def test_block_sad_ties_through_the_pruned_lab_variant():
    """the successive-elimination search of the lab build (VQA_SAD_VARIANT=2) must break the same ties the same way"""
    from rtvqa_amd import _native as N
    assert os.path.exists(N.LAB_LIB_PATH), "the lab library is a build product of the same make (csrc/Makefile, target lab)"
    code = (
        "import sys, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import rtvqa_amd, hostile_cases as K\n"
        "from rtvqa_amd import _native as N\n"
        "from oracle import c_oracle as co\n"
        "eng = rtvqa_amd.Engine(0)\n"
        "assert eng.lib.vqa_build_flavour() != 0\n"
        "for h, w in K.BGR_SHAPES:\n"
        "    seq = K.bgr_sequence(h, w)\n"
        "    for R in (7, 3):\n"
        "        rec = eng.complexity(seq[1:], prev0=seq[0], mask=N.M_MOTION, sad_range=R)\n"
        "        for i in range(rec.shape[0]):\n"
        "            nb, sad, hist = co.block_sad(co.bgr2gray(seq[i]), co.bgr2gray(seq[i + 1]), R)\n"
        "            assert int(rec[i]['sad_blocks']) == nb and int(rec[i]['sad_sum']) == sad and (rec[i]['mv_d2_hist'] == hist).all(), (h, w, R, i)\n"
        "print('PRUNED-OK')\n" % (REPO, os.path.join(REPO, "tests"))
    )
    env = dict(os.environ, VQA_SAD_VARIANT="2", VQA_LIB_PATH=N.LAB_LIB_PATH)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300, cwd=REPO)
    assert r.returncode == 0 and "PRUNED-OK" in r.stdout, (r.stdout[-400:], r.stderr[-1200:])


@pytest.mark.parametrize("low,high", [(100, 200), (20, 60)])
@pytest.mark.parametrize("h,w", K.BGR_SHAPES)
def test_canny_on_the_thresholds(engine, h, w, low, high):
    """Sobel magnitudes of exactly low and exactly high, the 45 degree sector boundary, plateaus of equal magnitude (NMS's > on one
    side and >= on the other): strong, weak, the count and the edge map are exact"""
    from rtvqa_amd import _native as N
    seq = K.bgr_sequence(h, w)
    rec = _complexity(engine, seq, mask=N.M_EDGE, canny=(low, high))
    for i in range(seq.shape[0]):
        name = K.COMPLEXITY[i // 2] + ("" if i & 1 else " (prev)")
        cnt, strong, weak, edges = co.canny(co.bgr2gray(seq[i]), low, high, want_map=True)
        got = (int(rec[i]["edge_strong"]), int(rec[i]["edge_weak"]), int(rec[i]["edge_count"]))
        print("%dx%d" % (h, w), (low, high), name, "strong, weak, count", got)
        assert got == (strong, weak, cnt), (name, got, (strong, weak, cnt))
        emap = engine.debug_plane(2, i, h, w)
        assert (emap == edges).all(), "%s: the edge map differs at %d pixels" % (name, int((emap != edges).sum()))


def _orb(frame):
    return co.orb64_count(co.bgr2gray(co.resize_linear(frame, 64, 64)))


@pytest.mark.parametrize("h,w", K.BGR_SHAPES)
def test_the_integer_outputs_in_one_submit(engine, h, w):
    """gray plane, histograms, sum_gray2, edge count, block SAD, ORB count and response of every content in one M_ALL submit; the
    resize planes at (33, 17) and at the exact-halving size"""
    from rtvqa_amd import _native as N
    seq = K.bgr_sequence(h, w)
    rec = _complexity(engine, seq[1:], prev0=seq[0], mask=N.M_ALL, dct_mode=N.DCT_BLOCK8)
    for i in range(rec.shape[0]):
        f = seq[i + 1]
        g = co.bgr2gray(f)
        assert (engine.debug_plane(3, i, h, w) == g).all(), i
        assert (rec[i]["hist_gray"] == co.hist_u8(g)).all(), i
        for c in range(3):
            assert (rec[i]["hist_bgr"][c] == co.hist_u8(f, offset=c, step=3)).all(), (i, c)
        assert int(rec[i]["sum_gray2"]) == int((g.astype(np.int64) ** 2).sum()), i
        cnt, strong, weak = co.canny(g, 100, 200)
        assert (int(rec[i]["edge_strong"]), int(rec[i]["edge_weak"]), int(rec[i]["edge_count"])) == (strong, weak, cnt), i
        assert (int(rec[i]["orb_keypoints"]), int(rec[i]["orb_response"])) == _orb(f), i
    _check_sad(rec, seq, 7, "M_ALL %dx%d" % (h, w))
    sizes = [(33, 17)] + ([(w // 2, h // 2)] if h % 2 == 0 and w % 2 == 0 else [])
    for rw, rh in sizes:
        rec = _complexity(engine, seq, mask=N.M_GRAY_HIST | N.M_COLOR_HIST | N.M_DCT | N.M_EDGE, resize=(rw, rh))
        for i in range(seq.shape[0]):
            a = co.resize_linear(co.bgr2gray(seq[i]), rw, rh)
            rb = co.resize_linear(seq[i], rw, rh)
            b = co.bgr2gray(rb)
            assert (engine.debug_plane(0, i, rh, rw) == a).all(), (rw, rh, i)
            assert (engine.debug_plane(1, i, rh, rw) == b).all(), (rw, rh, i)
            assert (rec[i]["hist_gray"] == co.hist_u8(b)).all(), (rw, rh, i)
            for c in range(3):
                assert (rec[i]["hist_bgr"][c] == co.hist_u8(rb, offset=c, step=3)).all(), (rw, rh, i, c)
            assert int(rec[i]["sum_gray2"]) == int((a.astype(np.int64) ** 2).sum()), (rw, rh, i)
            assert int(rec[i]["edge_count"]) == co.canny(b, 100, 200)[0], (rw, rh, i)


def _check_dct(rec, seq, want, tag, metric):
    """want[i] = (energy, L1 against frame i - 1) in float64 for seq[i]; rec[i] belongs to seq[i + 1]"""
    for i in range(rec.shape[0]):
        name = K.COMPLEXITY[(i + 1) // 2]
        e, l1 = want[i + 1]
        ge, gl = float(rec[i]["dct_energy"]), float(rec[i]["temporal_dct_l1"])
        s2 = float(rec[i]["sum_gray2"])
        static = np.array_equal(seq[i], seq[i + 1])
        ee = 0.0 if s2 == 0 else _rel(ge, e)
        el = 0.0 if static else _rel(gl, l1)
        print(tag, "frame", i + 1, name, "energy %.6e rel %.2e parseval %.2e" % (ge, ee, 0.0 if s2 == 0 else _rel(ge, s2)),
              "L1 %.6e ref %.6e rel %.2e" % (gl, l1, el))
        _note(metric, max(ee, el), "%s %s" % (tag, name))
        if s2 == 0:
            assert ge == 0.0, (tag, i, ge)                      # an all-0 plane has energy exactly 0
        else:
            assert ee <= RTOL, (tag, i, name, ge, e)
            assert _rel(ge, s2) <= RTOL, (tag, i, name, ge, s2)      # Parseval
        if static:
            assert gl == 0.0, (tag, i, name, gl)               # a frame against itself
        else:
            assert l1 > 0 and el <= RTOL, (tag, i, name, gl, l1)


@pytest.mark.parametrize("h,w", K.BGR_SHAPES)
def test_dct8_energy_and_temporal_l1(engine, h, w):
    from rtvqa_amd import _native as N
    seq = K.bgr_sequence(h, w)
    rec = _complexity(engine, seq[1:], prev0=seq[0], mask=N.M_DCT | N.M_TEMPORAL_DCT, dct_mode=N.DCT_BLOCK8)
    gray = [co.bgr2gray(f) for f in seq]
    want = [None] + [co.dct8x8(gray[i - 1], gray[i])[:2] for i in range(1, len(gray))]
    _check_dct(rec, seq, want, "dct8 %dx%d" % (h, w), "dct8")


@pytest.mark.parametrize("h,w", K.BGR_SHAPES + [(128, 160), (134, 262)])
def test_full_frame_dct_energy_and_temporal_l1(engine, h, w):
    """below 128 on a side the vector-ALU products, 128 x 160 the shortest FFT lengths, 134 x 262 the MFMA products; the largest AC
    energy and L1 a frame pair can have (the 2-px checkerboard against its inverse, all-255 against all-0)"""
    import scipy.fft
    from rtvqa_amd import _native as N
    seq = K.bgr_sequence(h, w)
    rec = _complexity(engine, seq[1:], prev0=seq[0], mask=N.M_DCT | N.M_TEMPORAL_DCT, dct_mode=N.DCT_FULL)
    coef = [scipy.fft.dctn(co.bgr2gray(f).astype(np.float64), norm="ortho") for f in seq]
    want = [None] + [(float((coef[i] ** 2).sum()), float(np.abs(coef[i - 1] - coef[i]).sum())) for i in range(1, len(coef))]
    _check_dct(rec, seq, want, "full dct %dx%d" % (h, w), "dct full")


@pytest.mark.parametrize("h,w", K.BGR_SHAPES)
def test_farneback_on_static_degenerate_pairs(engine, h, w):
    """where the oracle's mean magnitude is 0 the device's is 0; elsewhere the bar of tests/test_gpu_parity.py's Farneback tests
    (1e-4 relative plus 1e-7: on vstep and ramp the flow is rounding noise of 1e-12, the two oracles differ by a factor of 40)"""
    from rtvqa_amd import _native as N
    for name in K.DEGENERATE + ("flat_step",):
        prev, curr = K.gray_pair(name, h, w)
        rec = _complexity(engine, K.bgr(curr)[None], prev0=K.bgr(prev), mask=N.M_MOTION, motion_mode=N.MOTION_FARNEBACK)
        want, got = co.farneback(prev, curr), float(rec[0]["flow_mag_mean"])
        print("farneback", name, "%dx%d" % (h, w), "device %.6e oracle %.6e" % (got, want))
        assert np.isfinite(got)
        if want == 0.0:
            assert got == 0.0, (name, got)
        else:
            _note("farneback", abs(got - want), "%s %dx%d" % (name, h, w))
            assert abs(got - want) <= RTOL * want + 1e-7, (name, got, want)


# ---- neighbours in one batch ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [8, 10])
def test_records_do_not_depend_on_the_neighbours_in_the_batch(engine, depth):
    """[natural, checker_inv, bright_flat, natural] in one batch: every record is byte for byte that of the pair submitted alone -
    the negative totals of the anti-correlated pair (two's complement through unsigned atomics) do not reach a neighbour"""
    from rtvqa_amd import _native as N
    h, w = 67, 99
    r, d, planes = K.frames(["natural", "checker_inv", "bright_flat", "natural"], h, w, depth)
    runs = {"gauss": lambda a, b: engine.quality(a, b, planes, N.SSIM_GAUSS), "vif": lambda a, b: engine.vif(a, b, planes),
            "adm": lambda a, b: engine.adm(a, b, planes)}
    for kind, run in runs.items():
        whole = run(r, d)
        for i in range(4):
            alone = run(r[i:i + 1], d[i:i + 1])
            assert alone.tobytes() == whole[i:i + 1].tobytes(), (kind, i, alone, whole[i])
        assert whole[0:1].tobytes() == whole[3:4].tobytes(), kind
    assert float(runs["gauss"](r, d)[1, 0]["ssim"]) < -0.99


def test_the_worst_gap_per_metric():
    """runs after the tests above (pytest keeps the file's order): the figures DESIGN.md section 3 quotes"""
    for metric in sorted(WORST):
        print("hostile matrix, worst gap: %-22s %.3e  (%s)" % (metric, WORST[metric][0], WORST[metric][1]))
