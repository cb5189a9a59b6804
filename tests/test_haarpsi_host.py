"""Host: the NumPy restatement of HaarPSI (tests/haarpsi_reference.py) pinned against SciPy's convolution
(tests/golden/haarpsi_pins.json, scripts/gen_haarpsi_pins.py) and by hand-computed answers, the quantised integer form against
the plain float64 form on every shared case, the bounds of the device's words, and the Python layers around the kernel - ABI,
config key, log and row - through their stub paths.  No GPU."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import haarpsi_cases as HC
import haarpsi_reference as R
from rtvqa_amd import _native as N
from rtvqa_amd import stream
from rtvqa_amd import video_processing as vp

FIELDS = ("den", "num_lo", "num_hi", "similarity", "haarpsi")
GOOD = {"crf": 23, "resize_width": 64, "resize_height": 64, "frame_interval": 10}
PINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "haarpsi_pins.json")


# ---- (a) third-party pins -------------------------------------------------------------------------------------------------------
def test_the_restatement_against_scipy_pins():
    doc = json.load(open(PINS))
    assert doc["alpha"] == R.ALPHA and doc["C"] == R.C8 and len(doc["pins"]) == 6
    assert any(p["h"] % 2 and p["w"] % 2 for p in doc["pins"])
    for p in doc["pins"]:
        r = np.array(p["ref"], np.int64).reshape(p["h"], p["w"])
        d = np.array(p["dist"], np.int64).reshape(p["h"], p["w"])
        v, x = R.haarpsi(r, d)
        assert abs(v - p["haarpsi"]) <= 1e-12 and abs(x - p["similarity"]) <= 1e-12, (p["h"], p["w"], v, p["haarpsi"])
        assert 0.0 < v < 1.0


# ---- (b) hand-computed answers ---------------------------------------------------------------------------------------------------
def test_h1_of_a_row_ramp_by_hand():
    """x(y, .) = 10 y on 16 x 16: S(i, .) = 2 (20 i + 20 i + 10) = 80 i + 20 on 8 x 8.  Inside, H_1^0 = two columns of
    S(i) - S(i+1) = -160 and H_1^1 = 0; the last column has one column inside (-80, and H_1^1 = S(i) + S(i+1) = 160 i + 120);
    the last row has nothing below it (H_1^0 = 2 S(7) = 1160, H_1^1 = 0); the corner is S(7, 7) = 580 both ways."""
    x = np.repeat(10 * np.arange(16)[:, None], 16, axis=1)
    S = R.quad_sums(x)
    assert S.shape == (8, 8) and (S == (80 * np.arange(8) + 20)[:, None]).all()
    H = R.haar(S)
    h0, h1 = H[0][0], H[1][0]
    assert (h0[:7, :7] == -160).all() and (h1[:7, :7] == 0).all()
    assert (h0[:7, 7] == -80).all() and (h1[:7, 7] == 160 * np.arange(7) + 120).all()
    assert (h0[7, :7] == 1160).all() and (h1[7, :7] == 0).all()
    assert h0[7, 7] == 580 and h1[7, 7] == 580


def test_a_flat_field_has_coefficients_on_the_border_ring_only():
    """a flat v on 32 x 32 (S = 4 v on 16 x 16): H_s^0 vanishes wherever the window's rows i - K/2 + 1 .. i + K/2 lie inside,
    whatever the column (a short row of the window is short above and below alike), and nowhere else; H_s^1 likewise by columns"""
    v = 37
    S = R.quad_sums(np.full((32, 32), v))
    assert (S == 4 * v).all()
    H = R.haar(S)
    for s, half in ((1, 1), (2, 2), (3, 4)):
        inside = np.zeros(16, bool)
        inside[half - 1:16 - half] = True
        h0, h1 = H[0][s - 1], H[1][s - 1]
        assert (h0[inside, :] == 0).all() and (h0[~inside, :] != 0).all(), s
        assert (h1[:, inside] == 0).all() and (h1[:, ~inside] != 0).all(), s
    # by hand at scale 3: row 0 has 1 row above the seam and 4 below it, all 8 columns inside at column 5
    assert H[0][2][0, 5] == (1 - 4) * 8 * 4 * v and H[0][2][15, 5] == 4 * 8 * 4 * v
    # the weight of flat against flat is there, the similarity is 1 everywhere: exactly 1
    assert R.haarpsi_fixed(np.full((32, 32), v), np.full((32, 32), v))[:2] == (1.0, R.U1 / R.FIX)


def test_the_last_row_and_column_of_an_odd_plane_are_half_weight():
    S = R.quad_sums(np.full((17, 19), 9))
    assert S.shape == (9, 10)
    assert (S[:8, :9] == 36).all() and (S[8, :9] == 18).all() and (S[:8, 9] == 18).all() and S[8, 9] == 9


def test_the_even_windows_sit_where_matlab_puts_them():
    """one S = 1 at (9, 11): scale s sees it in rows i = 9 - K/2 .. 9 + K/2 - 1 and columns j = 11 - K/2 .. 11 + K/2 - 1; H^0
    is +1 where it lies in the upper half (i >= 9) and -1 below, H^1 +1 where it lies in the left half (j >= 11).  A window
    shifted by one sample either way moves every one of these."""
    S = np.zeros((20, 24), np.int64)
    S[9, 11] = 1
    H = R.haar(S)
    for s, half in ((1, 1), (2, 2), (3, 4)):
        want0, want1 = np.zeros_like(S), np.zeros_like(S)
        want0[9:9 + half, 11 - half:11 + half] = 1
        want0[9 - half:9, 11 - half:11 + half] = -1
        want1[9 - half:9 + half, 11:11 + half] = 1
        want1[9 - half:9 + half, 11 - half:11] = -1
        assert (H[0][s - 1] == want0).all() and (H[1][s - 1] == want1).all(), s


def test_constants():
    assert R.U1 == 1057878328 and R.FIX == N.HAARPSI_FIX and R.ALPHA == N.HAARPSI_ALPHA
    assert abs(R.logit(R.U1 / R.FIX) / R.ALPHA - 1.0) < 8e-9          # alpha' against alpha
    assert R.constant(8) == 30.0 and R.constant(16) == 30.0 * 257.0 * 257.0
    # the derivative bound of the header: 2 / (alpha X (1 - X)) at X = sigmoid(alpha)
    X = 1.0 / (1.0 + math.exp(-R.ALPHA))
    assert 2.0 / (R.ALPHA * X * (1.0 - X)) < 32.8 and 2.0 ** -31 * 32.8 + 1.6e-8 < HC.BAR


# ---- (c) exact answers, and the integer form against the float form ---------------------------------------------------------------
def test_identical_and_all_zero_planes_give_exactly_one():
    for depth in HC.DEPTHS:
        for shape in HC.SHAPES:
            r, _ = HC.pair("noise", shape[0], shape[1], depth)
            v, x, (den, num) = R.haarpsi_fixed(r, r, depth)
            assert v == 1.0 and x == R.U1 / R.FIX and den > 0 and num == R.U1 * den
            z = np.zeros(shape, np.int64)
            assert R.haarpsi_fixed(z, z, depth) == (1.0, R.U1 / R.FIX, (0, 0))
            assert R.haarpsi(z, z, depth)[0] == 1.0


ALL = HC.matrix() + HC.hostile_matrix()


@pytest.mark.parametrize("name,shape,depth", ALL, ids=["%s-%dx%d-%d" % (c, s[0], s[1], dp) for c, s, dp in ALL])
def test_the_integer_form_stays_within_the_bar_of_the_float_form(name, shape, depth):
    r, d = HC.pair(name, shape[0], shape[1], depth)
    v, x = R.haarpsi(r, d, depth)
    fv, fx, (den, num) = R.haarpsi_fixed(r, d, depth)
    assert abs(fv - v) <= HC.BAR and abs(fx - x) <= HC.BAR, (fv - v, fx - x)
    assert 0.5 < x <= 1.0 / (1.0 + math.exp(-R.ALPHA)) + 1e-14 and 0.0 < v <= 1.0 + 1e-12   # (the float form's own sums round)
    assert fv <= 1.0
    # symmetric in its arguments, word for word
    assert R.words(d, r, depth) == R.words(r, d, depth)
    if name in ("ends", "anti", "anti_noise", "noise", "posterised"):
        assert v < 0.9                                         # non-vacuous: these are far from 1
    if name == "step":
        assert 0.999 < v < 1.0


def test_depth_scaling_is_exact_in_the_float_form():
    """the same clip times 257 at 16 bits: H scales by 257 and c_s by 257^2, so the similarities agree to roundings"""
    r, d = HC.pair("natural", 33, 47, 8)
    a, b = R.haarpsi(r, d, 8), R.haarpsi(r * 257, d * 257, 16)
    assert abs(a[0] - b[0]) <= 1e-12 and abs(a[1] - b[1]) <= 1e-13


# ---- (d) the bounds of the device's words -------------------------------------------------------------------------------------------
def test_word_bounds_at_16_bit_full_range():
    peak = 65535
    # bands of 8 rows at the peak and at 0: S alternates in bands of 4 rows, and at a seam the 8 x 8 window is full above, empty below
    x = np.zeros((64, 64), np.int64)
    x[(np.arange(64) // 8) % 2 == 0] = peak
    H = R.haar(R.quad_sums(x))
    assert np.abs(H[0][2]).max() == 128 * peak < 1 << 23
    assert np.abs(H[0][1]).max() == 32 * peak and np.abs(H[0][0]).max() == 8 * peak
    assert (32 * peak) ** 2 * 2 < 1 << 45                       # H_r^2 + H_d^2, and 2 |H_r H_d|
    term = (1 << 30) * (128 * peak)
    assert term < 1 << 53 and 16 * term < 1 << 57               # a term; a thread's 16 terms, split there
    # the size limit: hd wd <= 2^26 + 2^22 + 5 samples, two terms each
    terms = 2 * ((1 << 26) + (1 << 22) + 5)
    assert terms * (128 * peak) < 1 << 51                       # den
    assert terms * ((1 << 32) - 1) < 1 << 60                    # num_lo, however the terms are grouped
    assert terms * (term >> 32) < 1 << 53                       # num_hi
    assert 2 * (1 << 26) * (128 * peak) < 1 << 50               # den, even sides
    # full-range noise at 16 bits on the largest shared shape: the words of the restatement are far inside
    r, d = HC.pair("noise", 135, 241, 16)
    den, lo, hi = R.words(r, d, 16)
    assert den < 1 << 40 and lo < 1 << 32 and 0 < hi < 1 << 40


# ---- (e) the ABI --------------------------------------------------------------------------------------------------------------------
def test_the_additive_abi():
    from rtvqa_amd.engine import HAARPSI_DTYPE
    assert N.VQA_ABI_VERSION == 8
    assert (N.K_BOUND, N.K_HAARPSI, N.K_FINIS) == (36, 37, 38)
    assert N.K_IDS_SHOWN == N.K_IDS_GIVEN + (37,) and N.K_BOUND not in N.K_IDS_SHOWN
    assert C.sizeof(N.VqaHaarpsiMetrics) == 40 == HAARPSI_DTYPE.itemsize and HAARPSI_DTYPE.names == FIELDS
    assert [HAARPSI_DTYPE.fields[k][1] for k in FIELDS] == [0, 8, 16, 24, 32]
    assert [getattr(N.VqaHaarpsiMetrics, k).offset for k in FIELDS] == [0, 8, 16, 24, 32]
    for sym in ("vqa_haarpsi_submit", "vqa_haarpsi_wait"):
        assert sym in N.SIGNATURES
    lib = N.load()
    lib.vqa_kernel_name.restype = C.c_char_p
    assert lib.vqa_kernel_name(37) == b"k_haarpsi"
    assert lib.vqa_kernel_name(36) == b"?" and lib.vqa_kernel_name(38) == b"?" and lib.vqa_kernel_name(35) == b"k_xpsnr_sse"


# ---- (f) config, log and row --------------------------------------------------------------------------------------------------------
def test_config_key():
    vp.validate_config(dict(GOOD))
    vp.validate_config(dict(GOOD, haarpsi=True))
    vp.validate_config(dict(GOOD, haarpsi=False, xpsnr=True, gmsd=True, vif=True))
    for bad in (1, 0, "true", None, "only"):
        with pytest.raises(ValueError) as e:
            vp.validate_config(dict(GOOD, haarpsi=bad))
        assert str(e.value) == "haarpsi must be true or false."


def _records(n):
    from rtvqa_amd.engine import HAARPSI_DTYPE
    rec = np.zeros(n, HAARPSI_DTYPE)
    rec["haarpsi"] = [0.875, 1.0, 0.25][:n]
    return rec


def _xpsnr(n):
    from rtvqa_amd.engine import XPSNR_DTYPE
    rec = np.zeros(n, XPSNR_DTYPE)
    rec["xpsnr"] = [41.5, 43.0, 39.25][:n]
    return rec


def test_the_json_log_and_what_the_row_takes_from_it(tmp_path):
    from rtvqa_amd.engine import ADM_DTYPE, VIF_DTYPE
    vif = np.array([[0.5, 0.9, 0.95, 0.99], [0.7, 0.8, 0.97, 1.01], [0.6, 0.85, 0.96, 1.0]])
    adm = np.zeros(3, ADM_DTYPE)
    adm["adm2"], adm["scale"] = [0.9, 0.95, 0.85], 0.9
    rec, xps = _records(3), _xpsnr(3)
    old, log, only = str(tmp_path / "old.json"), str(tmp_path / "vmaf.json"), str(tmp_path / "haarpsi.json")
    vp.write_vif_log(old, vif, adm, xpsnr=xps)
    vp.write_vif_log(log, vif, adm, xpsnr=xps, haarpsi=rec)
    doc0, doc = json.load(open(old)), json.load(open(log))
    assert "haarpsi" not in json.dumps(doc0)
    names0 = list(doc0["frames"][0]["metrics"])
    assert names0[-1] == "xpsnr"
    assert list(doc["frames"][1]["metrics"]) == names0 + ["haarpsi"] == list(doc["pooled_metrics"])   # after xpsnr
    vals = [0.875, 1.0, 0.25]
    for i in range(3):
        m = doc["frames"][i]["metrics"]
        assert {k: m[k] for k in names0} == doc0["frames"][i]["metrics"] and m["haarpsi"] == vals[i]
    assert {k: doc["pooled_metrics"][k] for k in names0} == doc0["pooled_metrics"]
    p = doc["pooled_metrics"]["haarpsi"]
    assert sorted(p) == ["harmonic_mean", "max", "mean", "min"]
    assert p["min"] == 0.25 and p["max"] == 1.0 and abs(p["mean"] - np.mean(vals)) <= 1e-15
    vp.write_vif_log(only, haarpsi=rec)
    assert list(json.load(open(only))["frames"][0]["metrics"]) == ["haarpsi"]
    pl, sl = tmp_path / "psnr.log", tmp_path / "ssim.log"
    pl.write_text("n:1 mse_avg:1.00 psnr_avg:48.13 \n")
    sl.write_text("n:1 Y:0.990000 All:0.990000 (20.000000)\n")
    m0 = vp.extract_metrics_from_logs(str(pl), str(sl), old, "x", 23, 1000, "64x64", 30.0)
    m = vp.extract_metrics_from_logs(str(pl), str(sl), log, "x", 23, 1000, "64x64", 30.0)
    assert list(m0)[-1] == "XPSNR" and list(m) == list(m0) + ["HAARPSI"]                              # after XPSNR
    assert {k: m[k] for k in m0} == m0 and abs(m["HAARPSI"] - np.mean(vals)) <= 1e-15
    base = ["Bitrate (kbps)", "Resolution (px)", "Frame Rate (fps)", "CRF", "PSNR", "SSIM"]
    assert list(vp.extract_metrics_from_logs(str(pl), str(sl), only, "x", 23, 1000, "64x64", 30.0)) == base + ["HAARPSI"]
    # logs without the key are what they were, byte for byte
    again = str(tmp_path / "again.json")
    vp.write_vif_log(again, vif, adm, xpsnr=xps, haarpsi=None)
    assert open(again, "rb").read() == open(old, "rb").read()
    # the pass's tuple -> the log: the last element is HaarPSI's [n, p], XPSNR's the one before it
    v = np.zeros((3, 1), VIF_DTYPE)
    v["scale"][:, 0, :] = vif
    q = (None, None, v, adm[:, None], xps[:, None], rec[:, None])
    vp._write_feature_log(again, q, dict(vif=True, adm=True, motion=False, siti=False, psnr_hvs=False, ciede=False, gmsd=False, cambi=False, xpsnr=True, haarpsi=True))
    assert open(again, "rb").read() == open(log, "rb").read()
    vp._write_feature_log(again, q[:-1], dict(vif=True, adm=True, motion=False, siti=False, psnr_hvs=False, ciede=False, gmsd=False, cambi=False, xpsnr=True))
    assert open(again, "rb").read() == open(old, "rb").read()
    vp._write_feature_log(again, (None, None, rec[:, None]), dict(vif=False, adm=False, motion=False, siti=False, psnr_hvs=False, ciede=False, gmsd=False, cambi=False, xpsnr=False, haarpsi=True))
    assert open(again, "rb").read() == open(only, "rb").read()


def test_a_model_does_not_read_the_new_key():
    from rtvqa_amd import vmaf_model

    class Model:
        features = ["vif_scale0", "adm2", "motion2"]

    x = vmaf_model.feature_matrix(Model, {"vif_scale0": [0.5, 0.7], "adm2": [0.9, 0.95], "motion2": [0.0, 1.0], "haarpsi": [0.9, 0.8]})
    assert x.shape == (2, 3)


def test_the_stream_request():
    p = [(16, 16, 0, 16, 1), (16, 16, 256, 16, 1), (16, 16, 512, 16, 1)]
    every = dict(vif=True, adm=True, motion=True, siti=True, psnr_hvs=True, ciede=True, gmsd=True, cambi=True, xpsnr=True)
    assert stream.Quality(p).haarpsi is False and stream.Quality(p, **every).haarpsi is False
    assert stream.Quality(p, haarpsi=True).haarpsi is True and stream.Quality(p, haarpsi="only").haarpsi == "only"
    assert stream.Quality(p, haarpsi=True).ssim is True and stream.Quality(p, haarpsi="only").ssim is False
    assert stream.Quality(p, haarpsi=True).xpsnr is False
    for bad in (1, "yes", None):
        with pytest.raises(ValueError):
            stream.Quality(p, haarpsi=bad)
    with pytest.raises(ValueError):
        stream.Quality(p, N.SSIM_MS, scales=True, haarpsi="only")
    z = np.zeros((0, 768), np.uint8)
    # an empty clip: without the request the tuples are what they were; with it ONE further last element, after XPSNR's
    for kw, length in ((dict(), 2), (dict(vif=True), 3), (dict(xpsnr=True), 3), (dict(gmsd=True, xpsnr=True), 4), (every, 11)):
        q0, _ = stream.run(z, z, quality=stream.Quality(p, **kw))
        q1, _ = stream.run(z, z, quality=stream.Quality(p, haarpsi=True, **kw))
        assert len(q0) == length and len(q1) == length + 1, kw
        assert q1[-1].shape == (0, 3) and q1[-1].dtype.names == FIELDS
        for a, b in zip(q0, q1):
            assert (a is None and b is None) or (a.dtype == b.dtype and a.shape == b.shape)
    q, _ = stream.run(z, z, quality=stream.Quality(p, haarpsi="only"))
    assert len(q) == 3 and q[0] is None and q[1] is None and q[2].shape == (0, 3)
