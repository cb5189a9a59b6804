"""GMSD on the host side (no GPU): the NumPy restatement of tests/gmsd_reference.py against SciPy (tests/golden/gmsd_pins.json:
the Prewitt stage, its zero border and the pooling) and against hand-made known answers (the 2x2 stage, which the fixture does
not pin), the integer form of the pooling, the additive ABI (vqa_gmsd_submit, vqa_gmsd_wait, vqa_gmsd_metrics, VQA_K_GMSD), the
JSON log and the row, the config key and the stream request."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import gmsd_cases as GC
import gmsd_reference as R
from rtvqa_amd import _native as N
from rtvqa_amd import stream
from rtvqa_amd import video_processing as vp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOOD = {"crf": 23, "vmaf_model_path": None, "resize_width": 64, "resize_height": 64, "frame_interval": 10}
FIELDS = ("sum_u", "sum_u2_lo", "sum_u2_hi", "count", "gms_mean", "gmsd")


# ---- the third-party pin ---------------------------------------------------------------------------------------------------
def test_the_restatement_against_scipy():
    """convolve2d(.., 'same') of SciPy 1.7.1 and numpy.std(ddof=1): 1e-9 on m^2 = q / 144 and on gmsd (and the mean)"""
    sys.path.insert(0, os.path.join(REPO, "scripts"))
    try:
        import gen_gmsd_pins as G
    finally:
        sys.path.pop(0)
    fx = json.load(open(os.path.join(REPO, "tests", "golden", "gmsd_pins.json")))
    pairs = G.make_pairs()
    assert len(pairs) == len(fx["pairs"]) == 6 and fx["versions"]["scipy"] == "1.7.1"
    assert [[int(r.sum()), int(d.sum())] for r, d in pairs] == fx["sums"]              # the same planes as when it was made
    for (r, d), p in zip(pairs, fx["pairs"]):
        assert np.abs(R.grad_sq(R.downsample(r)) - np.array(p["m2_r"])).max() <= 1e-9
        assert np.abs(R.grad_sq(R.downsample(d)) - np.array(p["m2_d"])).max() <= 1e-9
        g, m = R.gmsd(r, d)
        assert abs(g - p["gmsd"]) <= 1e-9 and abs(m - p["gms_mean"]) <= 1e-9


# ---- known answers --------------------------------------------------------------------------------------------------------
def test_the_2x2_stage_on_a_quad_pattern():
    """every quad holds (a, b; c, d) = (10, 20; 30, 60) plus 4 k for quad number k: D = 30 + 4 k"""
    h, w = 6, 8
    x = np.zeros((h, w), np.int64)
    want = np.zeros((3, 4))
    for i in range(3):
        for j in range(4):
            k = 4 * i + j
            x[2 * i:2 * i + 2, 2 * j:2 * j + 2] = np.array([[10, 20], [30, 60]]) + 4 * k
            want[i, j] = 30.0 + 4 * k
    assert (R.downsample(x) == want).all()


def test_an_odd_plane_keeps_its_last_row_and_column_at_half_weight():
    h, w = 17, 19
    x = np.arange(h * w, dtype=np.int64).reshape(h, w) % 251
    D = R.downsample(x)
    assert D.shape == (9, 10)
    assert (D[:8, :9] == x[:16, :18].reshape(8, 2, 9, 2).sum(axis=(1, 3)) / 4.0).all()
    assert (D[8, :9] == (x[16, 0:18:2] + x[16, 1:18:2]) / 4.0).all()               # last row: two samples over 4
    assert (D[:8, 9] == (x[0:16:2, 18] + x[1:16:2, 18]) / 4.0).all()               # last column likewise
    assert D[8, 9] == x[16, 18] / 4.0                                              # the corner: one sample over 4
    assert ((4 * D) == np.rint(4 * D)).all()                                       # S = 4 D is an integer


def test_a_flat_field_has_gradient_on_its_border_ring_only():
    """D = 255 everywhere, 0 outside: q = (12 gx)^2 + (12 gy)^2 is 0 inside, (3 * 1020)^2 = 9363600 on the edges (three samples
    against the zero fill in one direction, nothing in the other) and 2 (2 * 1020)^2 = 8323200 at the corners (two samples in
    both directions).  By hand, the corners are therefore NOT the largest: an edge sample is, by the factor 9 / 8."""
    q = np.rint(144.0 * R.grad_sq(R.downsample(np.full((20, 24), 255, np.int64)))).astype(np.int64)
    assert q.shape == (10, 12) and (q[1:-1, 1:-1] == 0).all()
    edge = (3 * 1020) ** 2
    assert (q[0, 1:-1] == edge).all() and (q[-1, 1:-1] == edge).all() and (q[1:-1, 0] == edge).all() and (q[1:-1, -1] == edge).all()
    corner = 2 * (2 * 1020) ** 2
    assert all(q[c] == corner for c in ((0, 0), (0, -1), (-1, 0), (-1, -1)))
    assert corner < edge < 2 ** 25
    # a clamp instead of the zero fill would leave the whole field without gradient
    g, m = R.gmsd(np.full((20, 24), 255, np.int64), np.zeros((20, 24), np.int64))
    assert g > 0.3 and m < 1.0
    assert q.max() == edge                     # (the corners see two sides but only two samples of each)


def test_a_vertical_step_edge():
    """D = 0 left of column 6 and 100 from there on: gx = 100 on the two columns beside the step, in the interior rows"""
    x = np.zeros((24, 24), np.int64)
    x[:, 12:] = 100
    gx, gy = R.prewitt(R.downsample(x))
    assert (np.abs(gx[1:-1, 5]) == 100.0).all() and (np.abs(gx[1:-1, 6]) == 100.0).all()
    assert (gx[1:-1, :5] == 0).all() and (gx[1:-1, 7:-1] == 0).all() and (gy[1:-1, :] == 0).all()
    assert (np.abs(gx[1:-1, -1]) == 100.0).all()                                  # the right border: 100 against the zero fill
    m2 = R.grad_sq(R.downsample(x))
    assert m2[4, 5] == 10000.0 and m2[4, 3] == 0.0
    # against a flat plane the similarity at the step is T / (m^2 + T)
    g = R.gms_map(x, np.zeros_like(x))
    assert abs(g[4, 5] - 170.0 / (10000.0 + 170.0)) <= 1e-15 and g[4, 3] == 1.0


# ---- pooling, symmetry, depth ----------------------------------------------------------------------------------------------
def test_the_integer_pooling_equals_the_float_pooling():
    """u = rint(gms 2^24): both results move by less than 2^-24 on every case of the GPU matrix (largest seen: 9.3e-9)"""
    worst = 0.0
    for name, (h, w), depth in GC.matrix():
        r, d = GC.pair(name, h, w, depth)
        g, m = R.gmsd(r, d, depth)
        gf, mf, (su, su2) = R.gmsd_fixed(r, d, depth)
        n = ((h + 1) // 2) * ((w + 1) // 2)
        assert su <= n << 24 and su2 <= n << 48
        worst = max(worst, abs(g - gf), abs(m - mf))
        assert abs(g - gf) <= GC.BAR and abs(m - mf) <= GC.BAR, (name, h, w, depth)
    print("integer form against float form: %.2e" % worst)
    assert worst <= 1e-8


def test_identical_planes_give_exact_zero_in_the_integer_form():
    for name in ("identical", "flat_peak"):
        for depth in GC.DEPTHS:
            r, d = GC.pair(name, 33, 67, depth)
            gf, mf, (su, su2) = R.gmsd_fixed(r, d, depth)
            n = 17 * 34
            assert gf == 0.0 and mf == 1.0 and su == n << 24 and su2 == n << 48


def test_the_pair_is_symmetric():
    for name in ("natural", "noise", "ends"):
        r, d = GC.pair(name, 33, 67, 8)
        assert R.gmsd(r, d) == R.gmsd(d, r) and R.gmsd_fixed(r, d) == R.gmsd_fixed(d, r)


def test_unrelated_noise_scores_near_0p2():
    r, d = GC.pair("noise", 67, 130, 8)
    g, m = R.gmsd(r, d)
    assert 0.15 <= g <= 0.25 and 0.75 <= m <= 0.9


def test_a_clip_scores_the_same_at_any_depth_after_exact_upscaling():
    """65535 = 257 * 255: the pair times 257 at 16 bits has q times 257^2 and T times 257^2"""
    for name in ("natural", "noise", "ends"):
        r, d = GC.pair(name, 33, 67, 8)
        a, b = R.gmsd(r, d, 8), R.gmsd(r * 257, d * 257, 16)
        assert abs(a[0] - b[0]) <= 1e-12 and abs(a[1] - b[1]) <= 1e-12


# ---- ABI -------------------------------------------------------------------------------------------------------------------
def test_the_additive_abi():
    assert N.VQA_ABI_VERSION == 8
    assert C.sizeof(N.VqaGmsdMetrics) == 48
    assert [getattr(N.VqaGmsdMetrics, f).offset for f in FIELDS] == [0, 8, 16, 24, 32, 40]
    from rtvqa_amd.engine import GMSD_DTYPE
    assert GMSD_DTYPE.itemsize == 48 and GMSD_DTYPE.names == FIELDS
    assert (N.K_GMSD, N.K_LIMIT) == (27, 28) and (N.K_CIEDE, N.K_BEYOND) == (25, 26)
    assert N.K_IDS_LISTED == N.K_IDS_NAMED + (27,) and 26 not in N.K_IDS_LISTED
    assert N.GMSD_MIN_DIM == R.MIN_DIM == 16 and N.GMSD_FIX == R.FIX == 1 << 24
    txt = open(os.path.join(REPO, "include", "vqa.h")).read()
    assert re.search(r"VQA_K_GMSD\s*=\s*27", txt) and re.search(r"VQA_K_LIMIT\s*=\s*28", txt) and re.search(r"VQA_K_BEYOND\s*=\s*26", txt)
    assert re.search(r"#define VQA_ABI_VERSION\s+8", txt)
    part = txt[txt.index("---- GMSD: gradient magnitude similarity deviation"):]
    assert "this text is\n * what is built" in part or "this text is what is built" in part
    for word in ("2x2 mean", "Prewitt", "T = 170 (peak / 255)^2", "divisor N - 1", "rint(gms 2^24)", "128-bit", "at least 16 x 16"):
        assert word in part, word
    lib = N.load()
    assert hasattr(lib, "vqa_gmsd_submit") and hasattr(lib, "vqa_gmsd_wait")       # both symbols are exported
    lib.vqa_kernel_name.restype = C.c_char_p
    assert lib.vqa_kernel_name(N.K_GMSD) == b"k_gmsd"
    assert lib.vqa_kernel_name(26) == b"?" and lib.vqa_kernel_name(N.K_LIMIT) == b"?"
    assert lib.vqa_kernel_name(N.K_CIEDE) == b"k_ciede"
    # argument checks that need no device
    assert lib.vqa_gmsd_submit(None, None, None, 0, 0, 0, 0, None, 0) == N.VQA_ERR_INVALID
    assert lib.vqa_gmsd_wait(None, None, 0) == N.VQA_ERR_INVALID
    assert lib.vqa_profile_read(None, N.K_GMSD, None, None, 0) == N.VQA_ERR_INVALID


def test_the_header_struct_is_48_bytes_to_the_c_compiler(tmp_path):
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "vqa.h"\n'
           'int (*submit)(vqa_ctx *, const uint8_t *, const uint8_t *, int, int, int64_t, int64_t, const vqa_plane_desc *, int) '
           '= vqa_gmsd_submit;\n'
           'int (*wait_)(vqa_ctx *, vqa_gmsd_metrics *, int) = vqa_gmsd_wait;\n'
           'int main(void){printf("%zu %zu %zu %zu %zu %zu %zu %d %d %d %d\\n", sizeof(vqa_gmsd_metrics), '
           'offsetof(vqa_gmsd_metrics, sum_u), offsetof(vqa_gmsd_metrics, sum_u2_lo), offsetof(vqa_gmsd_metrics, sum_u2_hi), '
           'offsetof(vqa_gmsd_metrics, count), offsetof(vqa_gmsd_metrics, gms_mean), offsetof(vqa_gmsd_metrics, gmsd), '
           'VQA_K_GMSD, VQA_K_LIMIT, VQA_K_BEYOND, VQA_ABI_VERSION);'
           'return submit == 0 || wait_ == 0;}\n')
    (tmp_path / "s.c").write_text(src)
    lib_dir = os.path.dirname(N.LIB_PATH)
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), "-o", str(tmp_path / "s"), str(tmp_path / "s.c"),
                           "-L", lib_dir, "-l:" + os.path.basename(N.LIB_PATH), "-Wl,-rpath," + lib_dir,
                           "-Wl,--allow-shlib-undefined"])
    assert subprocess.check_output([str(tmp_path / "s")]).decode().split() == ["48", "0", "8", "16", "24", "32", "40", "27", "28",
                                                                              "26", "8"]


# ---- the log and the row ---------------------------------------------------------------------------------------------------
def _records(n):
    from rtvqa_amd.engine import GMSD_DTYPE
    rec = np.zeros(n, GMSD_DTYPE)
    rec["gmsd"], rec["gms_mean"] = [0.125, 0.0, 0.25][:n], [0.9, 1.0, 0.8][:n]
    return rec


def _ciede(n):
    from rtvqa_amd.engine import CIEDE_DTYPE
    rec = np.zeros(n, CIEDE_DTYPE)
    rec["ciede2000"] = [38.75, np.inf, 120.0][:n]
    return rec


def _hvs(n):
    from rtvqa_amd.engine import PSNR_HVS_DTYPE
    rec = np.zeros(n, PSNR_HVS_DTYPE)
    rec["psnr_hvs"], rec["psnr_hvsm"] = [41.25, np.inf, 38.5][:n], [47.0, np.inf, 120.0][:n]
    return rec


def test_the_json_log_and_what_the_row_takes_from_it(tmp_path):
    from rtvqa_amd.engine import ADM_DTYPE, VIF_DTYPE
    vif = np.array([[0.5, 0.9, 0.95, 0.99], [0.7, 0.8, 0.97, 1.01], [0.6, 0.85, 0.96, 1.0]])
    adm = np.zeros(3, ADM_DTYPE)
    adm["adm2"], adm["scale"] = [0.9, 0.95, 0.85], 0.9
    rec, hv, ce = _records(3), _hvs(3), _ciede(3)
    old, log, only = str(tmp_path / "old.json"), str(tmp_path / "vmaf.json"), str(tmp_path / "gmsd.json")
    vp.write_vif_log(old, vif, adm, psnr_hvs=hv, ciede=ce)
    vp.write_vif_log(log, vif, adm, psnr_hvs=hv, ciede=ce, gmsd=rec)
    doc0, doc = json.load(open(old)), json.load(open(log))
    assert "gmsd" not in json.dumps(doc0)
    names0 = list(doc0["frames"][0]["metrics"])
    assert names0[-1] == "ciede2000"
    assert list(doc["frames"][1]["metrics"]) == names0 + ["gmsd"] == list(doc["pooled_metrics"])      # exactly the named key
    for i in range(3):
        m = doc["frames"][i]["metrics"]
        assert {k: m[k] for k in names0} == doc0["frames"][i]["metrics"] and m["gmsd"] == float(rec["gmsd"][i])
    assert {k: doc["pooled_metrics"][k] for k in names0} == doc0["pooled_metrics"]
    p = doc["pooled_metrics"]["gmsd"]
    assert sorted(p) == ["harmonic_mean", "max", "mean", "min"]
    assert p["min"] == 0.0 and p["max"] == 0.25 and p["mean"] == 0.125
    vp.write_vif_log(only, gmsd=rec)
    assert list(json.load(open(only))["frames"][0]["metrics"]) == ["gmsd"]
    pl, sl = tmp_path / "psnr.log", tmp_path / "ssim.log"
    pl.write_text("n:1 mse_avg:1.00 psnr_avg:48.13 \n")
    sl.write_text("n:1 Y:0.990000 All:0.990000 (20.000000)\n")
    m0 = vp.extract_metrics_from_logs(str(pl), str(sl), old, "x", 23, 1000, "64x64", 30.0)
    m = vp.extract_metrics_from_logs(str(pl), str(sl), log, "x", 23, 1000, "64x64", 30.0)
    assert list(m0)[-1] == "CIEDE2000" and list(m) == list(m0) + ["GMSD"]                             # exactly the named column
    assert {k: m[k] for k in m0} == m0 and m["GMSD"] == 0.125
    base = ["Bitrate (kbps)", "Resolution (px)", "Frame Rate (fps)", "CRF", "PSNR", "SSIM"]
    assert list(vp.extract_metrics_from_logs(str(pl), str(sl), only, "x", 23, 1000, "64x64", 30.0)) == base + ["GMSD"]
    # logs without the key are what they were, byte for byte
    again = str(tmp_path / "again.json")
    vp.write_vif_log(again, vif, adm, psnr_hvs=hv, ciede=ce, gmsd=None)
    assert open(again, "rb").read() == open(old, "rb").read()
    # the pass's tuple -> the log: the last element is GMSD's [n, p], CIEDE2000's [n] the one before it
    v = np.zeros((3, 1), VIF_DTYPE)
    v["scale"][:, 0, :] = vif
    q = (None, None, v, adm[:, None], hv[:, None], ce, rec[:, None])
    vp._write_feature_log(again, q, dict(vif=True, adm=True, motion=False, siti=False, psnr_hvs=True, ciede=True, gmsd=True))
    assert open(again, "rb").read() == open(log, "rb").read()
    vp._write_feature_log(again, q[:-1], dict(vif=True, adm=True, motion=False, siti=False, psnr_hvs=True, ciede=True))
    assert open(again, "rb").read() == open(old, "rb").read()
    vp._write_feature_log(again, (None, None, rec[:, None]), dict(vif=False, adm=False, motion=False, siti=False, psnr_hvs=False, ciede=False, gmsd=True))
    assert open(again, "rb").read() == open(only, "rb").read()


def test_a_model_does_not_read_the_new_key():
    from rtvqa_amd import vmaf_model

    class Model:
        features = ["vif_scale0", "adm2", "motion2"]

    x = vmaf_model.feature_matrix(Model, {"vif_scale0": [0.5, 0.7], "adm2": [0.9, 0.95], "motion2": [0.0, 1.0], "gmsd": [0.1, 0.2]})
    assert x.shape == (2, 3)


def test_config_key():
    vp.validate_config(dict(GOOD))
    vp.validate_config(dict(GOOD, gmsd=True))
    vp.validate_config(dict(GOOD, gmsd=False, ciede=True, psnr_hvs=True, vif=True))
    for bad in (1, 0, "true", None, "only"):
        with pytest.raises(ValueError) as e:
            vp.validate_config(dict(GOOD, gmsd=bad))
        assert str(e.value) == "gmsd must be true or false."


def test_the_stream_request():
    p = [(16, 16, 0, 16, 1), (8, 8, 256, 8, 1), (8, 8, 320, 8, 1)]
    assert stream.Quality(p).gmsd is False and stream.Quality(p, vif=True, adm=True, motion=True, siti=True, psnr_hvs=True, ciede=True).gmsd is False
    assert stream.Quality(p, gmsd=True).gmsd is True and stream.Quality(p, gmsd="only").gmsd == "only"
    assert stream.Quality(p, gmsd=True).ssim is True and stream.Quality(p, gmsd="only").ssim is False
    assert stream.Quality(p, gmsd=True).ciede is False and stream.Quality([(32, 32, 0, 32, 1)], gmsd=True).gmsd is True   # one plane will do
    for bad in (1, "yes", None):
        with pytest.raises(ValueError):
            stream.Quality(p, gmsd=bad)
    with pytest.raises(ValueError):
        stream.Quality(p, N.SSIM_MS, scales=True, gmsd="only")
    z = np.zeros((0, 384), np.uint8)
    # an empty clip: without the request the tuples are what they were; with it ONE further last element, after CIEDE2000's
    for kw, length in ((dict(), 2), (dict(vif=True), 3), (dict(ciede=True), 3), (dict(psnr_hvs=True, ciede=True), 4),
                       (dict(vif=True, adm=True, motion=True, siti=True, psnr_hvs=True, ciede=True), 8)):
        q0, _ = stream.run(z, z, quality=stream.Quality(p, **kw))
        q1, _ = stream.run(z, z, quality=stream.Quality(p, gmsd=True, **kw))
        assert len(q0) == length and len(q1) == length + 1, kw
        assert q1[-1].shape == (0, 3) and q1[-1].dtype.names == FIELDS
        for a, b in zip(q0, q1):
            assert (a is None and b is None) or (a.dtype == b.dtype and a.shape == b.shape)
    q, _ = stream.run(z, z, quality=stream.Quality(p, gmsd="only"))
    assert len(q) == 3 and q[0] is None and q[1] is None and q[2].shape == (0, 3)
