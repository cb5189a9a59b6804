"""Host: the NumPy restatement of the no-reference artefact measures (tests/artifacts_reference.py) held to hand-computed
answers for every closed form include/vqa.h names, the telescoped blur against the untelescoped one word for word, the phase
counts by enumeration, the Laplacian sum and the 9-tap mean against SciPy through a committed fixture, and the Python layers
around the kernel - ABI, config key, log and row - through their stub paths.  No GPU."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import artifacts_cases as AC
import artifacts_reference as R
from rtvqa_amd import _native as N
from rtvqa_amd import stream
from rtvqa_amd import video_processing as vp

FIELDS = ("edge_h", "edge_v", "blur_f_h", "blur_v_h", "blur_f_v", "blur_v_v", "lap", "phase_h", "phase_v", "blockiness",
          "blockiness_max", "blur_h", "blur_v", "blur", "noise")
GOOD = {"crf": 23, "resize_width": 64, "resize_height": 64, "frame_interval": 10}
PINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "artifacts_pins.json")


# ---- (a) hand answers ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", (8, 10, 16))
def test_blocks_and_shifted_blocks(depth):
    h, w = 40, 72
    m = R.measure(AC.blocks(h, w, depth), depth)
    assert m["edge_h"][0] > 0 and m["edge_v"][0] > 0 and m["edge_h"][1:] == [0] * 7 and m["edge_v"][1:] == [0] * 7
    assert m["blockiness"] == 1.0 and m["blockiness_max"] == 1.0 and (m["phase_h"], m["phase_v"]) == (0, 0)
    assert m["r_h"] == [1.0] + [-1.0] * 7
    m = R.measure(AC.blocks(h, w, depth, (3, 5)), depth)
    assert (m["phase_h"], m["phase_v"]) == (3, 5) and m["blockiness_max"] == 1.0 and m["blockiness"] == -1.0
    assert [p for p in range(8) if m["edge_h"][p]] == [3] and [p for p in range(8) if m["edge_v"][p]] == [5]
    # two levels side by side, by hand: one boundary at column 8 of 16 columns, a step of 7 in each of 16 rows
    x = np.zeros((16, 16), np.int64)
    x[:, 8:] = 7
    m = R.measure(x, 8)
    assert m["edge_h"] == [7 * 16] + [0] * 7 and m["edge_v"] == [0] * 8 and m["r_h"][0] == 1.0 and m["r_v"] == [0.0] * 8
    assert m["blockiness"] == 0.5 and m["phase_v"] == 0                          # the lowest phase on a tie


@pytest.mark.parametrize("depth", (8, 12, 16))
def test_the_checkerboard_reads_one_ninth(depth):
    peak = (1 << depth) - 1
    for h, w in ((16, 16), (33, 65), (64, 96)):
        x = AC.checker(h, w, peak)
        assert R.words(x) == AC.checker_words(h, w, peak, R.counts)
        m = R.measure(x, depth)
        assert m["blur_h"] == m["blur_v"] == m["blur"] and abs(m["blur"] - 1.0 / 9.0) <= 2.0 ** -55
        # every boundary carries the same step: no phase stands out
        assert max(abs(r) for r in m["r_h"] + m["r_v"]) <= 1e-15


def test_the_ramp_and_the_flat_plane():
    m = R.measure(AC.ramp(20, 50), 8)
    assert m["blur_h"] == 1.0 and m["blur_v"] == 0.0 and m["blur"] == 1.0 and m["lap"] == 0 and m["noise"] == 0.0
    assert m["blur_f_h"] == 20 * 41 and m["blur_v_h"] == 0 and m["blur_f_v"] == 0
    assert m["edge_h"] == [20 * c for c in R.counts(50)] and max(abs(r) for r in m["r_h"]) <= 1e-15
    for depth in (8, 16):
        for v in (0, (1 << depth) - 1):
            m = R.measure(np.full((16, 24), v, np.int64), depth)
            for k in R.WORDS[2:]:
                assert m[k] == 0
            assert m["edge_h"] == [0] * 8 == m["edge_v"] and (m["phase_h"], m["phase_v"]) == (0, 0)
            for k in R.DOUBLES:
                assert m[k] == 0.0 and not np.isnan(m[k]), k


def test_one_impulse():
    """v at (32, 64): the centre adds |4 v|, its four neighbours |-2 v| and the four corners |v|: lap = 16 v.  The steps lie on
    the boundaries 64 and 65 (phases 0 and 1) in both directions; dB9 is non-zero only 4 before and 5 after, where dF is 0"""
    v = 200
    wd = R.words(AC.impulse(70, 130, 32, 64, v))
    e = [v, v, 0, 0, 0, 0, 0, 0]
    assert wd == dict(edge_h=e, edge_v=e, blur_f_h=2 * v, blur_v_h=18 * v, blur_f_v=2 * v, blur_v_v=18 * v, lap=16 * v)
    # beside the border the windows that leave the plane drop out: (0, 0) has no Laplacian window centred in the interior but
    # the one at (1, 1), and no boundary to its left or above
    wd = R.words(AC.impulse(16, 16, 0, 0, v))
    assert wd["lap"] == v and wd["edge_h"] == [0, v] + [0] * 6 and wd["edge_v"] == [0, v] + [0] * 6
    assert wd["blur_f_h"] == 0 and wd["blur_v_h"] == 0


def test_noise_and_smooth_texture_have_no_blockiness_and_noise_reads_its_sigma():
    rng = np.random.default_rng(7)
    h = w = 256
    noise = rng.integers(0, 256, (h, w)).astype(np.int64)
    y, x = np.mgrid[0:h, 0:w]
    smooth = np.rint(128 + 60 * np.sin(x / 9.0) * np.cos(y / 7.0) + 40 * np.sin((x + 2 * y) / 23.0)).astype(np.int64)
    for name, p in (("noise", noise), ("smooth", smooth)):
        m = R.measure(p, 8)
        print(name, m["blockiness"], m["blockiness_max"], m["blur"], m["noise"])
        assert abs(m["blockiness"]) <= 0.03 and -0.03 <= m["blockiness_max"] <= 0.06, name
    # Gaussian noise of sigma 5 on a flat field, rounded to integers (which adds 1/12 to the variance): the estimator's mean
    # is sigma, and its standard error over 254^2 windows that overlap ninefold is far below the 2 % asked here
    g = np.rint(128 + 5.0 * rng.standard_normal((h, w))).astype(np.int64)
    m = R.measure(g, 8)
    print("sigma 5:", m["noise"])
    assert abs(m["noise"] - np.sqrt(25.0 + 1.0 / 12.0)) <= 0.1
    m10 = R.measure(g * 4, 10)                                                   # the 8-bit scale at every depth
    assert m10["noise"] == m["noise"] and m10["blur"] == m["blur"] and m10["blockiness"] == m["blockiness"]


def _gauss_blur(x, sigma):
    r = int(4 * sigma)
    k = np.exp(-0.5 * (np.arange(-r, r + 1) / sigma) ** 2)
    k /= k.sum()
    p = np.pad(x.astype(np.float64), r, mode="reflect")
    p = np.apply_along_axis(lambda v: np.convolve(v, k, mode="valid"), 0, p)
    return np.apply_along_axis(lambda v: np.convolve(v, k, mode="valid"), 1, p)


def test_a_gaussian_blur_raises_the_blur_figure():
    rng = np.random.default_rng(11)
    x = np.clip(np.rint(_gauss_blur(rng.integers(0, 256, (200, 200)), 1.0) * 1.0), 0, 255).astype(np.int64)
    x = np.clip((x - 128) * 4 + 128, 0, 255)                                     # a texture with detail at every scale
    sharp = R.measure(x, 8)["blur"]
    soft = R.measure(np.rint(_gauss_blur(x, 3.0)).astype(np.int64), 8)["blur"]
    print("blur: texture %.3f, after a Gaussian of sigma 3 %.3f" % (sharp, soft))
    assert 0.0 < sharp < 0.5 < soft < 1.0 and soft - sharp > 0.2


# ---- (b) the telescoping, proved --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,depth", [((16, 16), 8), ((17, 25), 8), ((33, 20), 10), ((24, 41), 16)])
def test_the_telescoped_blur_is_the_untelescoped_blur(shape, depth):
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    for _ in range(4):
        x = rng.integers(0, 1 << depth, shape).astype(np.int64)
        assert R.words(x) == R.words(x, untelescoped=True)
    x = AC.checker(shape[0], shape[1], (1 << depth) - 1)
    assert R.words(x) == R.words(x, untelescoped=True)


# ---- (c) the counts ---------------------------------------------------------------------------------------------------------------
def test_the_phase_counts_by_enumeration():
    want = {16: [1, 2, 2, 2, 2, 2, 2, 2], 17: [2] * 8, 23: [2, 3, 3, 3, 3, 3, 3, 2], 24: [2, 3, 3, 3, 3, 3, 3, 3], 25: [3] * 8}
    for n, cnt in want.items():
        assert R.counts(n) == cnt and sum(cnt) == n - 1
        # the closed form the library uses
        assert cnt == [(n - 1) // 8 if p == 0 else ((n - 1 - p) // 8 + 1 if n - 1 >= p else 0) for p in range(8)]
        # the words of a plane of ones-steps count the boundaries: x(i, j) = j has a step of 1 on every boundary
        assert R.words(AC.ramp(16, n))["edge_h"] == [16 * c for c in cnt]


# ---- (d) against SciPy, through the fixture ---------------------------------------------------------------------------------------
def test_the_laplacian_and_the_mean_filter_against_scipy_pins():
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
    import gen_artifacts_pins as G
    doc = json.load(open(PINS))
    assert doc["scipy"] == "1.15.3" and len(doc["pins"]) == len(G.CASES)
    for pin, (plane, depth) in zip(doc["pins"], G.make_planes()):
        h, w = pin["h"], pin["w"]
        x = np.array(pin["plane"], np.int64).reshape(h, w)
        assert np.array_equal(x, plane) and depth == pin["depth"]               # the generator's planes are the fixture's
        m = R.measure(x, depth)
        assert float(m["lap"]) == pin["lap"]
        assert abs(m["blur_h"] - pin["blur_h"]) <= 1e-12 and abs(m["blur_v"] - pin["blur_v"]) <= 1e-12
        # the 9-tap window sums of the untelescoped form, as ninths, are SciPy's mean where the window lies inside
        b_h = sum(x[:, 4 + k:w - 4 + k] for k in range(-4, 5)) / 9.0
        b_v = sum(x[4 + k:h - 4 + k, :] for k in range(-4, 5)) / 9.0
        peak = float((1 << depth) - 1)
        assert np.abs(b_h.reshape(-1) - np.array(pin["mean9_h"])).max() <= 1e-12 * peak
        assert np.abs(b_v.reshape(-1) - np.array(pin["mean9_v"])).max() <= 1e-12 * peak


# ---- (e) the ABI --------------------------------------------------------------------------------------------------------------------
def test_the_abi():
    from rtvqa_amd.engine import ARTIFACTS_DTYPE
    assert ARTIFACTS_DTYPE.names == FIELDS and ARTIFACTS_DTYPE.itemsize == C.sizeof(N.VqaArtifactsMetrics) == 21 * 8 + 8 + 6 * 8
    assert [f[0] for f in N.VqaArtifactsMetrics._fields_] == list(FIELDS)
    assert N.ARTIFACTS_MIN_DIM == 16 and (N.K_ARTIFACTS, N.K_STOP, N.K_CLOSE) == (42, 43, 41)
    for sym in ("vqa_artifacts_submit", "vqa_artifacts_wait"):
        assert sym in N.SIGNATURES
    lib = N.load()
    assert lib.vqa_abi_version() == 8
    lib.vqa_kernel_name.restype = C.c_char_p
    assert lib.vqa_kernel_name(42) == b"k_artifacts" and lib.vqa_kernel_name(40) == b"k_vca_sum"
    assert lib.vqa_kernel_name(41) == b"?" and lib.vqa_kernel_name(43) == b"?"


# ---- (f) config, log and row --------------------------------------------------------------------------------------------------------
def test_config_key():
    vp.validate_config(dict(GOOD))
    vp.validate_config(dict(GOOD, artifacts=True))
    vp.validate_config(dict(GOOD, artifacts=False, vca=True, cambi=True))
    for bad in (1, 0, "true", None, "only"):
        with pytest.raises(ValueError) as e:
            vp.validate_config(dict(GOOD, artifacts=bad))
        assert str(e.value) == "artifacts must be true or false."


def _records(n):
    from rtvqa_amd.engine import ARTIFACTS_DTYPE
    rec = np.zeros(n, ARTIFACTS_DTYPE)
    rec["blockiness"], rec["blur"], rec["noise"] = [0.25, -0.5, 1.0][:n], [0.125, 0.5, 0.75][:n], [4.0, 2.5, 0.0][:n]
    rec["blockiness_max"], rec["blur_h"] = 9.0, 9.0                              # (never logged)
    return rec


def test_the_json_log_and_what_the_row_takes_from_it(tmp_path):
    from rtvqa_amd.engine import VCA_DTYPE
    vca = np.zeros(3, VCA_DTYPE)
    vca["e"], vca["h"], vca["l"] = [52.5, 60.25, 40.0], [0.0, 7.75, 20.25], [64.0, 63.5, 65.5]
    vif = np.array([[0.5, 0.9, 0.95, 0.99], [0.7, 0.8, 0.97, 1.01], [0.6, 0.85, 0.96, 1.0]])
    rec = _records(3)
    mine = ["blockiness", "blur", "noise"]
    old, log, only = str(tmp_path / "old.json"), str(tmp_path / "vmaf.json"), str(tmp_path / "art.json")
    vp.write_vif_log(old, vif, vca=vca)
    vp.write_vif_log(log, vif, vca=vca, artifacts=rec)
    doc0, doc = json.load(open(old)), json.load(open(log))
    assert "blockiness" not in json.dumps(doc0) and "noise" not in json.dumps(doc0)
    names0 = list(doc0["frames"][0]["metrics"])
    assert names0[-1] == "vca_l"
    assert list(doc["frames"][1]["metrics"]) == names0 + mine == list(doc["pooled_metrics"])
    for i in range(3):
        m = doc["frames"][i]["metrics"]
        assert {k: m[k] for k in names0} == doc0["frames"][i]["metrics"]
        assert (m["blockiness"], m["blur"], m["noise"]) == (rec["blockiness"][i], rec["blur"][i], rec["noise"][i])
    assert {k: doc["pooled_metrics"][k] for k in names0} == doc0["pooled_metrics"]
    p = doc["pooled_metrics"]["blockiness"]
    assert sorted(p) == ["harmonic_mean", "max", "mean", "min"]
    assert p["min"] == -0.5 and p["max"] == 1.0 and p["mean"] == 0.25
    vp.write_vif_log(only, artifacts=rec)
    assert list(json.load(open(only))["frames"][0]["metrics"]) == mine
    pl, sl = tmp_path / "psnr.log", tmp_path / "ssim.log"
    pl.write_text("n:1 mse_avg:1.00 psnr_avg:48.13 \n")
    sl.write_text("n:1 Y:0.990000 All:0.990000 (20.000000)\n")
    m0 = vp.extract_metrics_from_logs(str(pl), str(sl), old, "x", 23, 1000, "64x64", 30.0)
    m = vp.extract_metrics_from_logs(str(pl), str(sl), log, "x", 23, 1000, "64x64", 30.0)
    assert list(m0)[-1] == "VCA_L" and list(m) == list(m0) + ["BLOCKINESS", "BLUR", "NOISE"]          # after VCA_L
    assert {k: m[k] for k in m0} == m0
    assert m["BLOCKINESS"] == 0.25 and abs(m["BLUR"] - 1.375 / 3.0) <= 1e-15 and abs(m["NOISE"] - 6.5 / 3.0) <= 1e-15
    base = ["Bitrate (kbps)", "Resolution (px)", "Frame Rate (fps)", "CRF", "PSNR", "SSIM"]
    assert list(vp.extract_metrics_from_logs(str(pl), str(sl), only, "x", 23, 1000, "64x64", 30.0)) == base + ["BLOCKINESS", "BLUR", "NOISE"]
    # logs without the key are what they were, byte for byte
    again = str(tmp_path / "again.json")
    vp.write_vif_log(again, vif, vca=vca, artifacts=None)
    assert open(again, "rb").read() == open(old, "rb").read()
    # the pass's tuple -> the log: the last element is the artefact records [n, p], VCA's the one before it
    from rtvqa_amd.engine import VIF_DTYPE
    v = np.zeros((3, 1), VIF_DTYPE)
    v["scale"][:, 0, :] = vif
    q = (None, None, v, vca[:, None], rec[:, None])
    vp._write_feature_log(again, q, dict(vif=True, adm=False, vca=True, artifacts=True))
    assert open(again, "rb").read() == open(log, "rb").read()
    vp._write_feature_log(again, q[:-1], dict(vif=True, adm=False, vca=True))
    assert open(again, "rb").read() == open(old, "rb").read()
    vp._write_feature_log(again, (None, None, rec[:, None]), dict(vif=False, adm=False, artifacts=True))
    assert open(again, "rb").read() == open(only, "rb").read()


def test_a_model_does_not_read_the_new_keys():
    from rtvqa_amd import vmaf_model

    class Model:
        features = ["vif_scale0", "adm2", "motion2"]

    x = vmaf_model.feature_matrix(Model, {"vif_scale0": [0.5, 0.7], "adm2": [0.9, 0.95], "motion2": [0.0, 1.0], "blur": [0.3, 0.4]})
    assert x.shape == (2, 3)


def test_the_stream_request():
    p = [(32, 32, 0, 32, 1), (32, 32, 1024, 32, 1), (32, 32, 2048, 32, 1)]
    every = dict(vif=True, adm=True, motion=True, siti=True, psnr_hvs=True, ciede=True, gmsd=True, cambi=True, xpsnr=True,
                 haarpsi=True, vca=True)
    assert stream.Quality(p).artifacts is False and stream.Quality(p, **every).artifacts is False
    assert stream.Quality(p, artifacts=True).artifacts is True and stream.Quality(p, artifacts="only").artifacts == "only"
    assert stream.Quality(p, artifacts=True).ssim is True and stream.Quality(p, artifacts="only").ssim is False
    assert stream.Quality(p, artifacts=True).cambi is False
    for bad in (1, "yes", None):
        with pytest.raises(ValueError):
            stream.Quality(p, artifacts=bad)
    with pytest.raises(ValueError):
        stream.Quality(p, N.SSIM_MS, scales=True, artifacts="only")
    z = np.zeros((0, 3072), np.uint8)
    # an empty clip: without the request the tuples are what they were; with it ONE further last element, after VCA's
    for kw, length in ((dict(), 2), (dict(vif=True), 3), (dict(vca=True), 3), (dict(cambi=True, vca=True), 4), (every, 13)):
        q0, _ = stream.run(z, z, quality=stream.Quality(p, **kw))
        q1, _ = stream.run(z, z, quality=stream.Quality(p, artifacts=True, **kw))
        assert len(q0) == length and len(q1) == length + 1, kw
        assert q1[-1].shape == (0, 3) and q1[-1].dtype.names == FIELDS
        for a, b in zip(q0, q1):
            assert (a is None and b is None) or (a.dtype == b.dtype and a.shape == b.shape)
    q, _ = stream.run(z, z, quality=stream.Quality(p, artifacts="only"))
    assert len(q) == 3 and q[0] is None and q[1] is None and q[2].shape == (0, 3)
