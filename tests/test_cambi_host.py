"""CAMBI on the host side (no GPU): the integer NumPy restatement of tests/cambi_reference.py against answers worked out by hand
from the text of include/vqa.h, the 10-bit conversions, the rounding of u against Python's fractions, a condition that keeps
the GPU matrix from being vacuous, the additive ABI (vqa_cambi_submit, vqa_cambi_wait, vqa_cambi_metrics, the new kernel ids),
the JSON log and the row, the config key and the stream request."""
import ctypes as C
import json
from fractions import Fraction

import numpy as np
import pytest

import cambi_cases as CC
import cambi_reference as R
from rtvqa_amd import _native as N
from rtvqa_amd import stream
from rtvqa_amd import video_processing as vp

GOOD = {"crf": 23, "vmaf_model_path": None, "resize_width": 64, "resize_height": 64, "frame_interval": 10}
FIELDS = ("top", "k", "masked", "pool", "cambi")


def _u(k, n0, nk, a):
    """round-to-nearest of k n0 nk / ((n0 + nk) A) at a step of 2^-16, halves up, in exact rational arithmetic"""
    c = Fraction(k * n0 * nk, (n0 + nk) * a)
    assert 0 <= c <= 1
    return int(c * 65536 + Fraction(1, 2))      # int() floors a non-negative Fraction


# ---- by hand ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_two_flat_halves_at_a_sample_whose_window_is_whole(k):
    """An 80 x 100 plane at 10 bits, t = v in columns 0..59 and v + k from column 60 on; the sample (40, 50): its window is rows
    8..72, columns 18..82, A = 65 * 65 = 4225, and every sample in it is at least 8 from the border, so m0 = 1 throughout (a
    7 x 7 window holds at most two columns with Z = 0: S >= 35).
    Step 2 makes a transition column: y0(., 59) = (2 v + 2 (v + k) + 2) >> 2 = v + ((k + 1) >> 1): v + 1, v + 1, v + 2, v + 2,
    v + 3 for k = 1..5.  For k = 1 that IS v + 1: the edge moves one column to the left and there is no third level.
    Columns of the window: v in 18..58 (41 columns), the transition column 59, v + k in 60..82 (23 columns).
      n_0 = 41 * 65 = 2665; k = 1: n_1 = 24 * 65 = 1560; k >= 2: n_T = 65 at d = (k + 1) >> 1, and n_k = 23 * 65 = 1495
      (k = 5: v + 5 is out of reach, only the transition column at d = 3 is counted).
    So a 5-level step does NOT score nothing under this definition: the transition column, one level in between, is masked
    and within reach of both halves.  Its contrast is small: 3 * 2665 * 65 / (2730 * 4225)."""
    v = 400
    t = np.full((80, 100), v, np.int64)
    t[:, 60:] += k
    y = R.anti_dither(R.to10(t, 10))
    m = R.mask0(y)
    assert (y[:, :59] == v).all() and (y[:, 59] == v + ((k + 1) >> 1)).all() and (y[:, 60:] == v + k).all()
    assert m[8:73, 18:83].all()
    a, n = R.counts_at(y, m, 40, 50)
    want = {d: 0 for d in range(-4, 5)}
    want[0] = 2665
    if k == 1:
        want[1] = 1560
        cands = [_u(1, 2665, 1560, 4225)]
    else:
        want[(k + 1) >> 1] = 65
        cands = [_u((k + 1) >> 1, 2665, 65, 4225)]
        if k <= 4:
            want[k] = 1495
            cands.append(_u(k, 2665, 1495, 4225))
    assert a == 4225 and n == want
    u = R.contrast(y, m)
    assert int(u[40, 50]) == max(cands) > 0
    pinned = {1: 15263, 2: 29712, 3: 44568, 4: 59424, 5: 2953}      # floor(65536 c + 1/2) of the fractions above, worked out once
    assert int(u[40, 50]) == pinned[k]


def test_the_16_x_16_plane_down_to_its_1_x_1_scale():
    """t = v in columns 0..7, v + 1 in columns 8..15.  y0 = v in columns 0..6 and v + 1 from column 7 (the k = 1 edge moves
    left).  Z = 0 in column 6 only.  S(i, j) = R(i) C(j) with R = rows of the 7-window in the plane: 4 5 6 7..7 6 5 4, and
    C = its columns less column 6 where it is in reach (j = 3..9): 4 5 6 | 6 x 7 | 7 7 7 | 6 5 4.  m0 = R C > 24:
      rows 0, 15 (R = 4): C = 7 only, j = 10..12; rows 1, 14 (R = 5) and 2, 13 (R = 6): C >= 5, j = 1..14; rows 3..12: all.
      masked_0 = 2 * 3 + 4 * 14 + 10 * 16 = 222.  Every window is the whole plane: A = 256 and the counts are the same for
      every sample of a level: n(v) = 4 * 6 + 10 * 7 = 94 (columns <= 6), n(v + 1) = 222 - 94 = 128.  K_0 = 76.
    Scale 1 (rows and columns 0, 2, .., 14): row 0 keeps j = 10, 12; rows 2 and 14 keep 2..14 (7); rows 4..12 keep all 8:
      masked_1 = 2 + 7 + 5 * 8 + 7 = 56; v in original columns 0, 2, 4, 6: n(v) = 3 + 5 * 4 + 3 = 26, n(v + 1) = 30; A = 64; K_1 = 19.
    Scale 2 (0, 4, 8, 12): row 0 keeps column 12; rows 4, 8, 12 all four: masked_2 = 13; n(v) = 6, n(v + 1) = 7; A = 16; K_2 = 4.
    Scale 3 (0, 8): (8, 0) = v and (8, 8) = v + 1 are masked, row 0 is not: masked_3 = 2, n = 1 and 1, A = 4, K_3 = 1,
      c = 1 / 8: u = 8192 exactly.
    Scale 4: the sample (0, 0), a corner: never masked.  K_4 = 1, top_4 = 0."""
    v = 600
    t = np.full((16, 16), v, np.int64)
    t[:, 8:] += 1
    w = R.cambi_words(t, 10)
    assert w["masked"] == [222, 56, 13, 2, 0] and w["k"] == [76, 19, 4, 1, 1]
    u = [_u(1, 94, 128, 256), _u(1, 26, 30, 64), _u(1, 6, 7, 16), _u(1, 1, 1, 4)]
    assert u == [13875, 14263, 13233, 8192]
    assert w["top"] == [76 * u[0], 19 * u[1], 4 * u[2], u[3], 0]
    pool, score = R.pool_and_score(w["top"], w["k"])
    assert pool == [x / 65536.0 for x in u] + [0.0]
    assert score == (16 * pool[0] + 8 * pool[1] + 4 * pool[2] + 2 * pool[3]) / 31 and 0.0 < score < 1.0
    # the scales themselves
    sc = R.scales(t, 10)
    assert [s[0].shape for s in sc] == [(16, 16), (8, 8), (4, 4), (2, 2), (1, 1)]
    m0 = sc[0][1]
    assert not m0[0, 0] and not m0[0, 9] and m0[0, 10] and m0[0, 12] and not m0[0, 13] and m0[1, 1] and not m0[1, 0] and m0[3, 0]


def test_the_corners_are_never_masked_and_a_flat_field_scores_zero():
    for depth in CC.DEPTHS:
        for shape in CC.SHAPES:
            for name in ("flat", "flat_zero", "flat_peak"):
                p = CC.plane(name, shape[0], shape[1], depth)
                y, m = R.scales(p, depth)[0]
                assert not (m[0, 0] or m[0, -1] or m[-1, 0] or m[-1, -1])
                assert m[3:-3, :].all() and m[:, 3:-3][1:-1].all() and m[0, 3:-3].all()   # edges are masked from 3 in, rows 0 too
                w = R.cambi_words(p, depth)
                assert w["top"] == [0] * 5 and w["masked"][0] == shape[0] * shape[1] - 4 * 5   # each corner loses (0,0) (0,1) (0,2) (1,0) (2,0)
            w = R.cambi_words(CC.plane("noise", shape[0], shape[1], depth), depth)
            assert w["top"] == [0] * 5 and w["masked"] == [0] * 5


def test_to_ten_bits_at_every_depth():
    assert [int(v) for v in R.to10([0, 1, 255], 8)] == [0, 4, 1020]
    assert [int(v) for v in R.to10([0, 1, 1023, 1024, 65535], 10)] == [0, 1, 1023, 1023, 1023]          # the clamp
    assert [int(v) for v in R.to10([0, 1, 2, 5, 6, 4093, 4094, 4095, 5000, 65535], 12)] == [0, 0, 1, 1, 2, 1023, 1023, 1023, 1023, 1023]
    assert [int(v) for v in R.to10([0, 31, 32, 95, 96, 65471, 65472, 65535], 16)] == [0, 0, 1, 1, 2, 1023, 1023, 1023]
    # exact upscaling is undone exactly: a 10-bit plane reads the same at 12 and 16 bits
    t = np.arange(1024)
    for depth in (12, 16):
        assert (R.to10(t << (depth - 10), depth) == t).all()
    assert (R.to10(t[::4] >> 2, 8) == t[::4]).all()


def test_the_rounding_of_u_against_fractions():
    rng = np.random.default_rng(3)
    cases = [(1, 1, 1, 4), (4, 2, 2, 4), (4, 2112, 2113, 4225), (1, 1, 4224, 4225), (3, 4225 // 2, 1, 4225), (2, 3, 5, 64)]
    cases += [(int(k), int(a), int(b), int(a + b + c)) for k, a, b, c in
              zip(rng.integers(1, 5, 300), rng.integers(1, 2100, 300), rng.integers(1, 2100, 300), rng.integers(0, 30, 300))]
    for k, n0, nk, a in cases:
        num, den = k * n0 * nk, (n0 + nk) * a
        assert int(R.round_u(num, den)) == _u(k, n0, nk, a), (k, n0, nk, a)
    assert _u(4, 2, 2, 4) == 65536                       # the largest value: k = 4, both levels half the window
    assert int(R.round_u(np.int64(1), np.int64(8))) == 8192 and int(R.round_u(np.int64(3), np.int64(8))) == 24576
    assert int(R.round_u(np.int64(1), np.int64(1 << 17))) == 1 and int(R.round_u(np.int64(1), np.int64((1 << 17) + 1))) == 0   # a half rounds up


def test_the_box_counts_against_a_walk():
    p = CC.plane("dither", 41, 71, 10)
    y, m = R.scales(p, 10)[0]
    u, best = R.contrast(y, m, detail=True)
    rng = np.random.default_rng(1)
    seen = 0
    for i, j in zip(rng.integers(0, 41, 40), rng.integers(0, 71, 40)):
        if not m[i, j]:
            assert u[i, j] == 0
            continue
        a, n = R.counts_at(y, m, int(i), int(j))
        cand = [(_u(k, n[0], n[s * k], a), -k) for k in (1, 2, 3, 4) for s in (-1, 1) if n[s * k]]
        assert int(u[i, j]) == (max(cand)[0] if cand else 0)
        seen += 1
    assert seen >= 10


@pytest.mark.parametrize("name,shape,depth", [c for c in CC.matrix() if c[0] in CC.BANDED],
                         ids=["%s-%dx%d-%d" % (c, s[0], s[1], dp) for c, s, dp in CC.matrix() if c in CC.BANDED])
def test_the_gpu_matrix_is_not_vacuous(name, shape, depth):
    """on at least one scale: a tenth of the samples masked, a top-K sum above 0, a sample whose best k is 1 and one whose best
    k is larger.  (At 8 bits one level is four 10-bit levels and flat bands alone have no neighbour at k = 1: the 8-bit
    contents carry single samples one level up, which the 2x2 mean turns into a level at k = 1.)"""
    w = R.cambi_words(CC.plane(name, shape[0], shape[1], depth), depth, detail=True)
    n = [(-(-shape[0] // (1 << s))) * (-(-shape[1] // (1 << s))) for s in range(5)]
    assert w["k"] == [max(1, 3 * v // 10) for v in n]

    def spread(b):
        return 1 in b and any(k > 1 for k in b)

    assert any(10 * w["masked"][s] >= n[s] and w["top"][s] > 0 and spread(w["best"][s]) for s in range(5)), w
    pool, score = R.pool_and_score(w["top"], w["k"])
    assert 0.0 < score <= 1.0 and all(0.0 <= v <= 1.0 for v in pool)


def test_the_dither_is_partly_undone_and_the_top_of_the_range_is_reached():
    for shape in CC.SHAPES[1:]:
        a = R.cambi_words(CC.plane("staircase", shape[0], shape[1], 10), 10)
        b = R.cambi_words(CC.plane("dither", shape[0], shape[1], 10), 10)
        assert 0 < b["masked"][0] < a["masked"][0] and 2 * b["masked"][0] > a["masked"][0]    # a quarter of the samples dithered
        p = CC.plane("top_ramp", shape[0], shape[1], 10)
        assert p.max() == 1023
        assert R.cambi_words(p, 10)["top"] == a["top"]                                         # the same ramp, moved up


@pytest.mark.parametrize("depth", [8, 10])
def test_the_largest_u_is_reached_at_scale_1(depth):
    """cambi_cases.full_contrast: worked out there by hand"""
    p = CC.full_contrast(depth)
    y, m = R.scales(p, depth)[1]
    assert y.shape == (8, 69) and (y[:4] == 500).all() and (y[4:] == 504).all()
    assert m[:, 2:68].all() and not m[0, 0] and not m[0, 1] and not m[1, 0] and not m[0, 68]
    a, n = R.counts_at(y, m, 3, 34)
    assert a == 520 and n[0] == 260 and n[4] == 260
    u = R.contrast(y, m)
    assert (u[:, 34:36] == 65536).all() and u.max() == 65536 and (u[:, 33] < 65536).all() and (u[:, 36] < 65536).all()
    w = R.cambi_words(p, depth)
    assert w["k"][1] == 165 and w["top"][1] > 16 * 65536


# ---- the ABI ---------------------------------------------------------------------------------------------------------------
def test_the_additive_abi():
    from rtvqa_amd.engine import CAMBI_DTYPE
    assert N.VQA_ABI_VERSION == 8
    assert (N.K_LIMIT, N.K_CAMBI_MASK, N.K_CAMBI_DECIMATE, N.K_CAMBI_CONTRAST, N.K_CAMBI_TOPK, N.K_TERMINUS) == (28, 29, 30, 31, 32, 33)
    assert N.K_IDS_TOLD == N.K_IDS_LISTED + N.K_IDS_CAMBI and N.K_LIMIT not in N.K_IDS_TOLD
    assert C.sizeof(N.VqaCambiMetrics) == 168 == CAMBI_DTYPE.itemsize and CAMBI_DTYPE.names == FIELDS
    assert [CAMBI_DTYPE.fields[k][1] for k in FIELDS] == [0, 40, 80, 120, 160]
    assert [getattr(N.VqaCambiMetrics, k).offset for k in FIELDS] == [0, 40, 80, 120, 160]
    for sym in ("vqa_cambi_submit", "vqa_cambi_wait"):
        assert sym in N.SIGNATURES
    lib = N.load()
    lib.vqa_kernel_name.restype = C.c_char_p
    names = [lib.vqa_kernel_name(k) for k in N.K_IDS_CAMBI]
    assert names == [b"k_cambi_mask", b"k_cambi_decimate", b"k_cambi_contrast", b"k_cambi_topk"]
    assert lib.vqa_kernel_name(28) == b"?" and lib.vqa_kernel_name(33) == b"?" and lib.vqa_kernel_name(27) == b"k_gmsd"
    header = open(N.HEADER_PATH).read() if hasattr(N, "HEADER_PATH") else None
    if header is not None:
        assert "vqa_cambi_submit" in header


# ---- the log and the row ---------------------------------------------------------------------------------------------------
def _records(n):
    from rtvqa_amd.engine import CAMBI_DTYPE
    rec = np.zeros(n, CAMBI_DTYPE)
    rec["cambi"] = [0.125, 0.0, 0.25][:n]
    return rec


def _gmsd(n):
    from rtvqa_amd.engine import GMSD_DTYPE
    rec = np.zeros(n, GMSD_DTYPE)
    rec["gmsd"] = [0.5, 0.0, 0.75][:n]
    return rec


def test_the_json_log_and_what_the_row_takes_from_it(tmp_path):
    from rtvqa_amd.engine import ADM_DTYPE, VIF_DTYPE
    vif = np.array([[0.5, 0.9, 0.95, 0.99], [0.7, 0.8, 0.97, 1.01], [0.6, 0.85, 0.96, 1.0]])
    adm = np.zeros(3, ADM_DTYPE)
    adm["adm2"], adm["scale"] = [0.9, 0.95, 0.85], 0.9
    rec, gm = _records(3), _gmsd(3)
    old, log, only = str(tmp_path / "old.json"), str(tmp_path / "vmaf.json"), str(tmp_path / "cambi.json")
    vp.write_vif_log(old, vif, adm, gmsd=gm)
    vp.write_vif_log(log, vif, adm, gmsd=gm, cambi=rec)
    doc0, doc = json.load(open(old)), json.load(open(log))
    assert "cambi" not in json.dumps(doc0)
    names0 = list(doc0["frames"][0]["metrics"])
    assert names0[-1] == "gmsd"
    assert list(doc["frames"][1]["metrics"]) == names0 + ["cambi"] == list(doc["pooled_metrics"])     # exactly the named key
    for i in range(3):
        m = doc["frames"][i]["metrics"]
        assert {k: m[k] for k in names0} == doc0["frames"][i]["metrics"] and m["cambi"] == float(rec["cambi"][i])
    assert {k: doc["pooled_metrics"][k] for k in names0} == doc0["pooled_metrics"]
    p = doc["pooled_metrics"]["cambi"]
    assert sorted(p) == ["harmonic_mean", "max", "mean", "min"]
    assert p["min"] == 0.0 and p["max"] == 0.25 and p["mean"] == 0.125
    vp.write_vif_log(only, cambi=rec)
    assert list(json.load(open(only))["frames"][0]["metrics"]) == ["cambi"]
    pl, sl = tmp_path / "psnr.log", tmp_path / "ssim.log"
    pl.write_text("n:1 mse_avg:1.00 psnr_avg:48.13 \n")
    sl.write_text("n:1 Y:0.990000 All:0.990000 (20.000000)\n")
    m0 = vp.extract_metrics_from_logs(str(pl), str(sl), old, "x", 23, 1000, "64x64", 30.0)
    m = vp.extract_metrics_from_logs(str(pl), str(sl), log, "x", 23, 1000, "64x64", 30.0)
    assert list(m0)[-1] == "GMSD" and list(m) == list(m0) + ["CAMBI"]                                 # exactly the named column
    assert {k: m[k] for k in m0} == m0 and m["CAMBI"] == 0.125
    base = ["Bitrate (kbps)", "Resolution (px)", "Frame Rate (fps)", "CRF", "PSNR", "SSIM"]
    assert list(vp.extract_metrics_from_logs(str(pl), str(sl), only, "x", 23, 1000, "64x64", 30.0)) == base + ["CAMBI"]
    # logs without the key are what they were, byte for byte
    again = str(tmp_path / "again.json")
    vp.write_vif_log(again, vif, adm, gmsd=gm, cambi=None)
    assert open(again, "rb").read() == open(old, "rb").read()
    # the pass's tuple -> the log: the last element is CAMBI's [n, p], GMSD's the one before it
    v = np.zeros((3, 1), VIF_DTYPE)
    v["scale"][:, 0, :] = vif
    q = (None, None, v, adm[:, None], gm[:, None], rec[:, None])
    vp._write_feature_log(again, q, dict(vif=True, adm=True, motion=False, siti=False, psnr_hvs=False, ciede=False, gmsd=True, cambi=True))
    assert open(again, "rb").read() == open(log, "rb").read()
    vp._write_feature_log(again, q[:-1], dict(vif=True, adm=True, motion=False, siti=False, psnr_hvs=False, ciede=False, gmsd=True))
    assert open(again, "rb").read() == open(old, "rb").read()
    vp._write_feature_log(again, (None, None, rec[:, None]), dict(vif=False, adm=False, motion=False, siti=False, psnr_hvs=False, ciede=False, gmsd=False, cambi=True))
    assert open(again, "rb").read() == open(only, "rb").read()


def test_a_model_does_not_read_the_new_key():
    from rtvqa_amd import vmaf_model

    class Model:
        features = ["vif_scale0", "adm2", "motion2"]

    x = vmaf_model.feature_matrix(Model, {"vif_scale0": [0.5, 0.7], "adm2": [0.9, 0.95], "motion2": [0.0, 1.0], "cambi": [0.1, 0.2]})
    assert x.shape == (2, 3)


def test_config_key():
    vp.validate_config(dict(GOOD))
    vp.validate_config(dict(GOOD, cambi=True))
    vp.validate_config(dict(GOOD, cambi=False, gmsd=True, ciede=True, vif=True))
    for bad in (1, 0, "true", None, "only"):
        with pytest.raises(ValueError) as e:
            vp.validate_config(dict(GOOD, cambi=bad))
        assert str(e.value) == "cambi must be true or false."


def test_the_stream_request():
    p = [(16, 16, 0, 16, 1), (8, 8, 256, 8, 1), (8, 8, 320, 8, 1)]
    assert stream.Quality(p).cambi is False and stream.Quality(p, vif=True, adm=True, motion=True, siti=True, psnr_hvs=True, ciede=True, gmsd=True).cambi is False
    assert stream.Quality(p, cambi=True).cambi is True and stream.Quality(p, cambi="only").cambi == "only"
    assert stream.Quality(p, cambi=True).ssim is True and stream.Quality(p, cambi="only").ssim is False
    assert stream.Quality(p, cambi=True).gmsd is False
    for bad in (1, "yes", None):
        with pytest.raises(ValueError):
            stream.Quality(p, cambi=bad)
    with pytest.raises(ValueError):
        stream.Quality(p, N.SSIM_MS, scales=True, cambi="only")
    z = np.zeros((0, 384), np.uint8)
    # an empty clip: without the request the tuples are what they were; with it ONE further last element, after GMSD's
    for kw, length in ((dict(), 2), (dict(vif=True), 3), (dict(gmsd=True), 3), (dict(ciede=True, gmsd=True), 4),
                       (dict(vif=True, adm=True, motion=True, siti=True, psnr_hvs=True, ciede=True, gmsd=True), 9)):
        q0, _ = stream.run(z, z, quality=stream.Quality(p, **kw))
        q1, _ = stream.run(z, z, quality=stream.Quality(p, cambi=True, **kw))
        assert len(q0) == length and len(q1) == length + 1, kw
        assert q1[-1].shape == (0, 3) and q1[-1].dtype.names == FIELDS
        for a, b in zip(q0, q1):
            assert (a is None and b is None) or (a.dtype == b.dtype and a.shape == b.shape)
    q, _ = stream.run(z, z, quality=stream.Quality(p, cambi="only"))
    assert len(q) == 3 and q[0] is None and q[1] is None and q[2].shape == (0, 3)
