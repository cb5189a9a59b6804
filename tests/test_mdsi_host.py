"""MDSI on the host side (no GPU): the two NumPy restatements of tests/mdsi_reference.py against SciPy (tests/golden/
mdsi_pins.json: the box stage for f = 1..5, the even-kernel centring included, and the Prewitt stage), the rounding ties of the
factor in C, in the engine and in the restatement, hand-made known answers, the sign convention, the admission of every case the
GPU tests compare, the additive ABI (vqa_mdsi_submit, vqa_mdsi_wait, vqa_mdsi_factor, vqa_mdsi_metrics, VQA_K_MDSI_MAP / _DEV),
the JSON log and the row, the config key and the stream request."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import mdsi_cases as MC
import mdsi_reference as R
from rtvqa_amd import _native as N
from rtvqa_amd import stream
from rtvqa_amd import video_processing as vp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOOD = {"crf": 23, "vmaf_model_path": None, "resize_width": 64, "resize_height": 64, "frame_interval": 10}
FIELDS = ("sum_pos", "sum_neg", "n_neg", "sum_dev", "count", "factor", "reserved", "dev", "mdsi")
MATRIX = MC.matrix()


def _planes(v, h, w, n=3):
    return [np.full((h, w), v, np.int64)] * n


# ---- the third-party pin ---------------------------------------------------------------------------------------------------
def test_the_box_stage_and_prewitt_against_scipy():
    """convolve2d of SciPy 1.15.3: the box sums are equal as integers for f = 1..5; gx and gy to 1e-12"""
    sys.path.insert(0, os.path.join(REPO, "scripts"))
    try:
        import gen_mdsi_pins as G
    finally:
        sys.path.pop(0)
    fx = json.load(open(os.path.join(REPO, "tests", "golden", "mdsi_pins.json")))
    x = G.make_plane()
    assert fx["versions"]["scipy"] == "1.15.3" and int(x.sum()) == fx["sum"] and list(x.shape) == fx["shape"]
    assert sorted(fx["box"]) == ["1", "2", "3", "4", "5"]
    for f in (1, 2, 3, 4, 5):
        want = np.array(fx["box"][str(f)], np.int64)
        assert want.shape == (-(-x.shape[0] // f), -(-x.shape[1] // f))
        assert (R.box_sum(x, f) == want).all(), f
    # the even kernel's centring: window 0 of f = 2 is rows 0..1 (GMSD's 2x2 stage), of f = 4 rows -1..2, of f = 3 rows -1..1
    assert fx["box"]["2"][0][0] == int(x[0:2, 0:2].sum())
    assert fx["box"]["4"][0][0] == int(x[0:3, 0:3].sum()) and fx["box"]["3"][0][0] == int(x[0:2, 0:2].sum())
    assert fx["box"]["4"][1][1] == int(x[3:7, 3:7].sum())
    gx, gy = R.prewitt(R.box_sum(x, 2) / 4.0)
    assert np.abs(gx - np.array(fx["gx"])).max() <= 1e-12 and np.abs(gy - np.array(fx["gy"])).max() <= 1e-12


# ---- the factor ------------------------------------------------------------------------------------------------------------
def test_the_factor_at_the_rounding_ties():
    """MATLAB's round, half away from zero: 640 gives 3 where Python's round gives 2"""
    from rtvqa_amd.engine import mdsi_factor
    lib = N.load()
    for m, f in ((16, 1), (383, 1), (384, 2), (639, 2), (640, 3), (895, 3), (896, 4), (1080, 4), (16384, 64)):
        for h, w in ((m, m), (m, 2 * m + 1), (m + 7, m)):
            assert lib.vqa_mdsi_factor(h, w) == mdsi_factor(h, w) == R.factor(h, w) == f, (h, w)
    assert round(640 / 256) == 2
    for shape, f in MC.FACTORS.items():
        assert R.factor(*shape) == f
        assert R.grid(*shape)[1:] == (-(-shape[0] // f), -(-shape[1] // f))
    assert lib.vqa_mdsi_factor(0, 16) == 0 and lib.vqa_mdsi_factor(16, -1) == 0


# ---- known answers ---------------------------------------------------------------------------------------------------------
def test_identical_inputs_give_the_exact_words_and_zero():
    for layout, shape, depth in (("bgr24", (33, 67), 8), ("yuv420p", (33, 67), 10), ("gray", (16, 16), 8), ("yuv420p", (385, 391), 8)):
        r, _ = MC.pair("noise", layout, shape[0], shape[1], depth)
        n = np.prod(R.grid(*shape)[1:])
        words = R.mdsi_quantised(r, r, MC.MODEL[layout], depth)
        assert words == (int(n) << 28, 0, 0, 0), (layout, shape)
        assert R.pool_words(words, n) == (0.0, 0.0)
        assert (R.g_quantised(r, r, MC.MODEL[layout], depth) == 1 << 24).all()


def test_flat_zero_against_flat_peak_in_bgr():
    """L = 254.9745, H = -2.55, M = -22.95 against zeros: every gradient vanishes in the interior, so GS = 1 and
    CS = 550 / (2.55^2 + 22.95^2 + 550) = 550 / 1083.205"""
    z, p = _planes(0, 20, 24), _planes(255, 20, 24)
    want = 0.6 + 0.4 * 550.0 / 1083.205
    assert abs(want - 0.803101) < 1e-6
    gcs = R.gcs_float(z, p, "bgr")
    assert np.abs(gcs[1:-1, 1:-1] - want).max() <= 1e-12
    g = R.g_quantised(z, p, "bgr")
    assert (g[1:-1, 1:-1] == int(np.rint(want * (1 << 24)))).all()
    assert (np.abs(gcs[0, :] - want) > 1e-3).all()            # the border ring sees the zero fill


def test_a_gray_yuv_clip_gives_the_same_bits_at_444_and_420():
    h, w = 33, 67
    (y, _, _), (yd, _, _) = MC.pair("natural", "yuv444p", h, w)
    words = []
    for layout in ("yuv444p", "yuv422p", "yuv420p"):
        sizes = MC.plane_sizes(layout, h, w)
        r = [y] + [np.full(s, 128, np.int64) for s in sizes[1:]]
        d = [yd] + [np.full(s, 128, np.int64) for s in sizes[1:]]
        words.append(R.mdsi_quantised(r, d, "yuv709"))
    assert words[0] == words[1] == words[2] and words[0][3] > 0


def test_a_clip_scores_the_same_at_8_bits_and_after_exact_upscaling_to_16():
    """samples times 256: Y - 16 s, U - 128 s and s all scale by 256 exactly, so only the roundings of the twelve doubles differ"""
    r, d = MC.pair("natural", "yuv420p", 33, 67)
    a = R.mdsi_float(r, d, "yuv709", 8)
    b = R.mdsi_float([p * 256 for p in r], [p * 256 for p in d], "yuv709", 16)
    assert abs(a[0] - b[0]) <= 1e-12 and abs(a[1] - b[1]) <= 1e-12
    wa = R.pool_words(R.mdsi_quantised(r, d, "yuv709", 8), 33 * 67)
    wb = R.pool_words(R.mdsi_quantised([p * 256 for p in r], [p * 256 for p in d], "yuv709", 16), 33 * 67)
    assert abs(wa[0] - wb[0]) <= R.derived_bar(R.gcs_float(r, d, "yuv709", 8))


@pytest.mark.parametrize("shape", [(67, 130), (16, 16)], ids=["67x130", "16x16"])
def test_removed_edges_score_higher_than_added_edges(shape):
    """the sign convention of the fused-image term: a textured reference against a flat distorted image (edges removed) is
    worse than the swap (edges added); with the two C2 terms exchanged the order flips"""
    r, d = MC.pair("texture_flat", "bgr24", *shape)
    removed, added = R.mdsi_float(r, d, "bgr")[1], R.mdsi_float(d, r, "bgr")[1]
    print("removed %.4f added %.4f" % (removed, added))
    assert removed > added + 0.05
    wr, wa = R.mdsi_quantised(r, d, "bgr"), R.mdsi_quantised(d, r, "bgr")
    n = shape[0] * shape[1]
    assert R.pool_words(wr, n)[1] > R.pool_words(wa, n)[1] + 0.05


# ---- admission -------------------------------------------------------------------------------------------------------------
def _admit(r, d, model, depth, tag):
    gcs = R.gcs_float(r, d, model, depth)
    dev, _ = R.pool_float(gcs)
    bar = R.derived_bar(gcs)
    words = R.mdsi_quantised(r, d, model, depth)
    got, _ = R.pool_words(words, gcs.size)
    print("%s dev %.9f integer %.9f gap %.2e bar %.2e n_neg %d of %d" % (tag, dev, got, abs(got - dev), bar, words[2], gcs.size))
    assert bar <= MC.BAR_LIMIT, (tag, bar)
    assert abs(got - dev) <= bar, (tag, got, dev, bar)
    return words


def test_the_matrix_has_every_case():
    assert len(MATRIX) == MC.MATRIX_CASES == 151 and len(set(MATRIX)) == 151
    for shape in MC.SMALL:
        for layout in MC.LAYOUTS:
            assert {c for c, l, s, dp in MATRIX if l == layout and s == shape and dp == 8} == set(MC.CONTENTS)
    for shape in MC.LARGE:
        assert {l for c, l, s, dp in MATRIX if s == shape} == {"yuv420p", "bgr24"}
    assert {dp for c, l, s, dp in MATRIX if s == (33, 67)} == {8, 10, 16}


@pytest.mark.parametrize("case", MATRIX, ids=[MC.case_id(c) for c in MATRIX])
def test_every_case_of_the_matrix_is_admitted(case):
    """the integer pooling within the bar mdsi_reference.derived_bar derives from THIS case's |GCS| values, and that bar at most
    1e-6; unrelated noise must reach the complex branch"""
    name, layout, (h, w), depth = case
    r, d = MC.pair(name, layout, h, w, depth)
    words = _admit(r, d, MC.MODEL[layout], depth, MC.case_id(case))
    if name == "noise":
        assert words[2] > 0
    if name in ("identical", "flat_zero", "flat_peak"):
        assert words == (R.grid(h, w)[1] * R.grid(h, w)[2] << 28, 0, 0, 0)


def test_the_frames_of_the_slice_test_are_admitted():
    for layout, h, w, depth in MC.SLICE_LAYOUTS:
        rs, ds = MC.slice_pool(layout, h, w, depth)
        assert len(rs) == MC.SLICE_FRAMES
        seen = {_admit(r, d, MC.MODEL[layout], depth, "%s frame %d" % (layout, i)) for i, (r, d) in enumerate(zip(rs, ds))}
        assert len(seen) == MC.SLICE_FRAMES                                       # seven frames, seven different records


# ---- ABI -------------------------------------------------------------------------------------------------------------------
def test_the_additive_abi():
    assert N.VQA_ABI_VERSION == 8
    assert C.sizeof(N.VqaMdsiMetrics) == 64
    assert [getattr(N.VqaMdsiMetrics, f).offset for f in FIELDS] == [0, 8, 16, 24, 32, 40, 44, 48, 56]
    from rtvqa_amd.engine import MDSI_DTYPE
    assert MDSI_DTYPE.itemsize == 64 and MDSI_DTYPE.names == FIELDS
    assert (N.K_MDSI_MAP, N.K_MDSI_DEV, N.K_BRINK) == (48, 49, 50) and N.K_EDGE == 47
    assert N.K_IDS_TOTAL == N.K_IDS_WHOLE + (48, 49) and 47 not in N.K_IDS_TOTAL
    assert (N.MDSI_YUV709, N.MDSI_BGR, N.MDSI_GRAY) == (0, 1, 2) == tuple(R.MODELS[k] for k in ("yuv709", "bgr", "gray"))
    assert N.MDSI_FIX_G == R.FIX_G == 1 << 24 and N.MDSI_FIX_Z == R.FIX_Z == 1 << 28 and N.MDSI_MIN_DIM == 16
    txt = open(os.path.join(REPO, "include", "vqa.h")).read()
    for name, val in (("VQA_K_MDSI_MAP", 48), ("VQA_K_MDSI_DEV", 49), ("VQA_K_BRINK", 50), ("VQA_K_EDGE", 47)):
        assert re.search(r"%s\s*=\s*%d\b" % (name, val), txt), name
    assert re.search(r"#define VQA_ABI_VERSION\s+8", txt)
    part = txt[txt.index("---- MDSI (Nafchi"):]
    part = part[:part.index("vqa_mdsi_factor(int height")]
    assert "this text is what is\n * built" in part or "this text is what is built" in part
    for word in ("NOT pinned", "floor(min(h, w) / 256 + 0.5)", "Prewitt", "C1 = 140, C2 = 55, C3 = 550", "rint(GCS 2^24)",
                 "principal complex root", "NOT symmetric", "0.5 (g_r + g_d)", "at least 16 x 16", "h w <= 2^28"):
        assert word in part, word
    lib = N.load()
    for sym in ("vqa_mdsi_submit", "vqa_mdsi_wait", "vqa_mdsi_factor"):
        assert hasattr(lib, sym)
    lib.vqa_kernel_name.restype = C.c_char_p
    assert lib.vqa_kernel_name(48) == b"k_mdsi_map" and lib.vqa_kernel_name(49) == b"k_mdsi_dev"
    assert lib.vqa_kernel_name(47) == b"?" and lib.vqa_kernel_name(50) == b"?"
    assert lib.vqa_kernel_name(N.K_BRISQUE_SEAM) == b"k_brisque_seam"
    # argument checks that need no device
    assert lib.vqa_mdsi_submit(None, None, None, 0, 0, 0, 0, None, 0, 0) == N.VQA_ERR_INVALID
    assert lib.vqa_mdsi_wait(None, None, 0) == N.VQA_ERR_INVALID
    for k in (47, 48, 49, 50):
        assert lib.vqa_profile_read(None, k, None, None, 0) == N.VQA_ERR_INVALID


def test_the_header_to_the_c_compiler(tmp_path):
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "vqa.h"\n'
           'int (*submit)(vqa_ctx *, const uint8_t *, const uint8_t *, int, int, int64_t, int64_t, const vqa_plane_desc *, int, int) '
           '= vqa_mdsi_submit;\n'
           'int (*wait_)(vqa_ctx *, vqa_mdsi_metrics *, int) = vqa_mdsi_wait;\n'
           'int main(void){printf("%zu %zu %zu %zu %zu %d %d %d %d %d %d %d %d %d\\n", sizeof(vqa_mdsi_metrics), '
           'offsetof(vqa_mdsi_metrics, sum_dev), offsetof(vqa_mdsi_metrics, factor), offsetof(vqa_mdsi_metrics, dev), '
           'offsetof(vqa_mdsi_metrics, mdsi), VQA_K_MDSI_MAP, VQA_K_MDSI_DEV, VQA_K_BRINK, VQA_K_EDGE, VQA_ABI_VERSION, '
           'VQA_MDSI_YUV709, VQA_MDSI_BGR, VQA_MDSI_GRAY, vqa_mdsi_factor(640, 644));'
           'return submit == 0 || wait_ == 0;}\n')
    (tmp_path / "s.c").write_text(src)
    lib_dir = os.path.dirname(N.LIB_PATH)
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), "-o", str(tmp_path / "s"), str(tmp_path / "s.c"),
                           "-L", lib_dir, "-l:" + os.path.basename(N.LIB_PATH), "-Wl,-rpath," + lib_dir,
                           "-Wl,--allow-shlib-undefined"])
    assert subprocess.check_output([str(tmp_path / "s")]).decode().split() == ["64", "24", "40", "48", "56", "48", "49", "50", "47",
                                                                              "8", "0", "1", "2", "3"]


# ---- the log and the row ---------------------------------------------------------------------------------------------------
def _records(n):
    from rtvqa_amd.engine import MDSI_DTYPE
    rec = np.zeros(n, MDSI_DTYPE)
    rec["mdsi"], rec["dev"] = [0.5, 0.0, 0.25][:n], [0.0625, 0.0, 0.00390625][:n]
    return rec


def _brisque(n):
    from rtvqa_amd.engine import BRISQUE_DTYPE
    rec = np.zeros(n, BRISQUE_DTYPE)
    rec["features"] = np.arange(n * 36, dtype=np.float64).reshape(n, 36) / 8.0
    return rec


def _gmsd(n):
    from rtvqa_amd.engine import GMSD_DTYPE
    rec = np.zeros(n, GMSD_DTYPE)
    rec["gmsd"] = [0.125, 0.0, 0.25][:n]
    return rec


def test_the_json_log_and_what_the_row_takes_from_it(tmp_path):
    rec, bq, gm = _records(3), _brisque(3), _gmsd(3)
    old, log, only = str(tmp_path / "old.json"), str(tmp_path / "vmaf.json"), str(tmp_path / "mdsi.json")
    vp.write_vif_log(old, gmsd=gm, brisque=bq)
    vp.write_vif_log(log, gmsd=gm, brisque=bq, mdsi=rec)
    doc0, doc = json.load(open(old)), json.load(open(log))
    assert "mdsi" not in json.dumps(doc0)
    names0 = list(doc0["frames"][0]["metrics"])
    assert names0[-1] == "brisque_35"
    assert list(doc["frames"][1]["metrics"]) == names0 + ["mdsi"] == list(doc["pooled_metrics"])      # exactly the named key
    for i in range(3):
        m = doc["frames"][i]["metrics"]
        assert {k: m[k] for k in names0} == doc0["frames"][i]["metrics"] and m["mdsi"] == float(rec["mdsi"][i])
    assert {k: doc["pooled_metrics"][k] for k in names0} == doc0["pooled_metrics"]
    p = doc["pooled_metrics"]["mdsi"]
    assert sorted(p) == ["harmonic_mean", "max", "mean", "min"]
    assert p["min"] == 0.0 and p["max"] == 0.5 and p["mean"] == 0.25
    vp.write_vif_log(only, mdsi=rec)
    assert list(json.load(open(only))["frames"][0]["metrics"]) == ["mdsi"]
    pl, sl = tmp_path / "psnr.log", tmp_path / "ssim.log"
    pl.write_text("n:1 mse_avg:1.00 psnr_avg:48.13 \n")
    sl.write_text("n:1 Y:0.990000 All:0.990000 (20.000000)\n")
    m0 = vp.extract_metrics_from_logs(str(pl), str(sl), old, "x", 23, 1000, "64x64", 30.0)
    m = vp.extract_metrics_from_logs(str(pl), str(sl), log, "x", 23, 1000, "64x64", 30.0)
    assert list(m0)[-1] == "BRISQUE_SIGMA2" and list(m) == list(m0) + ["MDSI"]                        # exactly the named column
    assert {k: m[k] for k in m0} == m0 and m["MDSI"] == 0.25
    base = ["Bitrate (kbps)", "Resolution (px)", "Frame Rate (fps)", "CRF", "PSNR", "SSIM"]
    assert list(vp.extract_metrics_from_logs(str(pl), str(sl), only, "x", 23, 1000, "64x64", 30.0)) == base + ["MDSI"]
    # logs without the key are what they were, byte for byte
    again = str(tmp_path / "again.json")
    vp.write_vif_log(again, gmsd=gm, brisque=bq, mdsi=None)
    assert open(again, "rb").read() == open(old, "rb").read()
    # the pass's tuple -> the log: the last element is MDSI's [n], BRISQUE's [n, p] the one before it
    q = (None, None, gm[:, None], bq[:, None], rec)
    vp._write_feature_log(again, q, dict(vif=False, adm=False, gmsd=True, brisque=True, mdsi=True))
    assert open(again, "rb").read() == open(log, "rb").read()
    vp._write_feature_log(again, q[:-1], dict(vif=False, adm=False, gmsd=True, brisque=True))
    assert open(again, "rb").read() == open(old, "rb").read()
    vp._write_feature_log(again, (None, None, rec), dict(vif=False, adm=False, mdsi=True))
    assert open(again, "rb").read() == open(only, "rb").read()


def test_a_model_does_not_read_the_new_key():
    from rtvqa_amd import vmaf_model

    class Model:
        features = ["vif_scale0", "adm2", "motion2"]

    x = vmaf_model.feature_matrix(Model, {"vif_scale0": [0.5, 0.7], "adm2": [0.9, 0.95], "motion2": [0.0, 1.0], "mdsi": [0.1, 0.2]})
    assert x.shape == (2, 3)


def test_config_key():
    vp.validate_config(dict(GOOD))
    vp.validate_config(dict(GOOD, mdsi=True))
    vp.validate_config(dict(GOOD, mdsi=False, ciede=True, gmsd=True, brisque=True))
    for bad in (1, 0, "true", None, "only"):
        with pytest.raises(ValueError) as e:
            vp.validate_config(dict(GOOD, mdsi=bad))
        assert str(e.value) == "mdsi must be true or false."


def test_the_stream_request():
    p = [(16, 16, 0, 16, 1), (8, 8, 256, 8, 1), (8, 8, 320, 8, 1)]
    assert stream.Quality(p).mdsi is False and stream.Quality(p, vif=True, ciede=True, gmsd=True, brisque=True).mdsi is False
    assert stream.Quality(p, mdsi=True).mdsi is True and stream.Quality(p, mdsi="only").mdsi == "only"
    assert stream.Quality(p, mdsi=True).ssim is True and stream.Quality(p, mdsi="only").ssim is False
    assert stream.Quality(p, mdsi=True).ciede is False and stream.Quality([(32, 32, 0, 32, 1)], mdsi=True).mdsi is True   # one plane will do
    for bad in (1, "yes", None):
        with pytest.raises(ValueError):
            stream.Quality(p, mdsi=bad)
    with pytest.raises(ValueError):
        stream.Quality(p, N.SSIM_MS, scales=True, mdsi="only")
    with pytest.raises(ValueError):
        stream.Quality(p[:2], mdsi=True)                                          # two planes
    z = np.zeros((0, 384), np.uint8)
    # an empty clip: without the request the tuples are what they were; with it ONE further last element, after BRISQUE's
    for kw, length in ((dict(), 2), (dict(vif=True), 3), (dict(brisque=True), 3), (dict(gmsd=True, brisque=True), 4),
                       (dict(vif=True, adm=True, motion=True, siti=True, psnr_hvs=True, ciede=True, artifacts=True, brisque=True), 10)):
        q0, _ = stream.run(z, z, quality=stream.Quality(p, **kw))
        q1, _ = stream.run(z, z, quality=stream.Quality(p, mdsi=True, **kw))
        assert len(q0) == length and len(q1) == length + 1, kw
        assert q1[-1].shape == (0,) and q1[-1].dtype.names == FIELDS
        for a, b in zip(q0, q1):
            assert (a is None and b is None) or (a.dtype == b.dtype and a.shape == b.shape)
    q, _ = stream.run(z, z, quality=stream.Quality(p, mdsi="only"))
    assert len(q) == 3 and q[0] is None and q[1] is None and q[2].shape == (0,)
