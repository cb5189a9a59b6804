"""PU21-PSNR / PU21-SSIM on the host side (no GPU): vqa_pu21_encode through ctypes against the values include/vqa.h states, its
monotony and its clamp; the header's constants as text; the additive ABI (ids 53, 54, 55; 52 stays unknown; ABI 8); the Gaussian
stage of the restatement of tests/pu21_reference.py against SciPy; its SSIM on hand cases; the quantised restatement against the
unquantised one within the bars (mse: derived; pu_ssim: measured here and recorded in DESIGN.md 4s); the two-word join at the
worst case; the JSON log, the row, the cap, the config keys, the stream request and the argument errors of every Python layer."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import pu21_cases as PC
import pu21_reference as R
from rtvqa_amd import _native as N
from rtvqa_amd import stream
from rtvqa_amd import video_processing as vp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOOD = {"crf": 23, "vmaf_model_path": None, "resize_width": 64, "resize_height": 64, "frame_interval": 10}
FIELDS = ("sse_y_lo", "sse_y_hi", "sse_rgb_lo", "sse_rgb_hi", "ssim_q", "windows", "mse_y", "mse_rgb", "pu_psnr", "pu_psnr_rgb",
          "pu_ssim")
KNOWN = ((0.005, 5.47e-10), (100.0, 256.3838973127), (10000.0, 595.3939200201))


# ---- the encoding ----------------------------------------------------------------------------------------------------------
def test_the_host_encoding_through_ctypes():
    lib = N.load()
    v = [lib.vqa_pu21_encode(l) for l, _ in KNOWN]
    assert abs(v[0] - KNOWN[0][1]) <= 1e-12 and v[0] > 0.0                      # (three figures are stated: 5.47e-10)
    for got, (l, want) in zip(v[1:], KNOWN[1:]):
        assert abs(got - want) <= 1e-9 * want, (l, got, want)
    grid = np.geomspace(R.L_MIN, R.L_MAX, 100000)
    enc = np.array([lib.vqa_pu21_encode(float(l)) for l in grid])
    assert (np.diff(enc) > 0).all()                                              # strictly increasing over the whole range
    assert np.abs(enc - R.encode(grid)).max() <= 1e-9                            # and the restatement's V
    for below in (0.0, 1e-9, 0.004999, -3.0):
        assert lib.vqa_pu21_encode(below) == v[0]
    for above in (10000.0001, 1e6, float("inf")):
        assert lib.vqa_pu21_encode(above) == v[2]
    assert int(np.rint(v[2] * R.FIX)) < 2 ** 26


def test_the_header_states_every_constant():
    txt = open(os.path.join(REPO, "include", "vqa.h")).read()
    part = txt[txt.index("---- PU21 HDR quality"):]
    part = part[:part.index("VQA_API int vqa_pu21_wait")]
    for word in ("0.353487901", "0.3734658629", "8.277049286e-05", "0.9062562627", "0.09150303166", "0.9099517204", "596.3148142",
                 "(0.01 * 256)^2", "(0.03 * 256)^2", "[0.005, 10000]", "256.3838973127", "595.3939200201", "5.47e-10",
                 "NOT pinned", "banding_glare", "rint(V 2^16)", "rint(ssim 2^24)", "at least 16 x 16", "256 MiB", "EXACTLY"):
        assert word in part, word
    assert tuple(float(x) for x in ("0.353487901", "0.3734658629", "8.277049286e-05", "0.9062562627", "0.09150303166",
                                    "0.9099517204", "596.3148142")) == R.P


# ---- ABI -------------------------------------------------------------------------------------------------------------------
def test_the_additive_abi():
    assert N.VQA_ABI_VERSION == 8
    assert C.sizeof(N.VqaPu21Metrics) == 88
    assert [getattr(N.VqaPu21Metrics, f).offset for f in FIELDS] == list(range(0, 88, 8))
    from rtvqa_amd.engine import PU21_DTYPE
    assert PU21_DTYPE.itemsize == 88 and PU21_DTYPE.names == FIELDS
    assert (N.K_PU21_ENCODE, N.K_PU21_SSIM, N.K_RIM) == (53, 54, 55) and N.K_VERGE == 52
    assert N.K_IDS_GRAND == N.K_IDS_SUM + (53, 54) and 52 not in N.K_IDS_GRAND and N.K_IDS_SUM == N.K_IDS_TOTAL + (51,)
    assert N.PU21_FIX == R.FIX == 1 << 16 and N.PU21_MIN_DIM == R.MIN_DIM == 16 and N.PU21_SSIM_TILE == R.TILE
    txt = open(os.path.join(REPO, "include", "vqa.h")).read()
    for name, val in (("VQA_K_PU21_ENCODE", 53), ("VQA_K_PU21_SSIM", 54), ("VQA_K_RIM", 55), ("VQA_K_VERGE", 52)):
        assert re.search(r"%s\s*=\s*%d\b" % (name, val), txt), name
    assert re.search(r"#define VQA_ABI_VERSION\s+8", txt)
    lib = N.load()
    for sym in ("vqa_pu21_submit", "vqa_pu21_wait", "vqa_pu21_encode"):
        assert hasattr(lib, sym)
    lib.vqa_kernel_name.restype = C.c_char_p
    assert lib.vqa_kernel_name(53) == b"k_pu21_encode" and lib.vqa_kernel_name(54) == b"k_pu21_ssim"
    assert lib.vqa_kernel_name(52) == b"?" and lib.vqa_kernel_name(55) == b"?" and lib.vqa_kernel_name(51) == b"k_itp"
    assert lib.vqa_pu21_submit(None, None, None, 0, 0, 0, 0, None, 0, 0, 0, 0) == N.VQA_ERR_INVALID
    assert lib.vqa_pu21_wait(None, None, 0) == N.VQA_ERR_INVALID
    # the read-back of the maps is the lab build's alone
    shipped = C.CDLL(os.path.join(REPO, "real-time-video-quality-analysis_amd", "csrc", "libvqa_hip.so"))
    assert not hasattr(shipped, "vqa_pu21_lab_read_maps")
    assert hasattr(C.CDLL(N.LAB_LIB_PATH), "vqa_pu21_lab_read_maps")
    assert b"VQA_PU21_SUBSLICE" in open(N.LAB_LIB_PATH, "rb").read()


def test_the_header_to_the_c_compiler(tmp_path):
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "vqa.h"\n'
           'int (*submit)(vqa_ctx *, const uint8_t *, const uint8_t *, int, int, int64_t, int64_t, const vqa_plane_desc *, int, int, '
           'int, int) = vqa_pu21_submit;\n'
           'int (*wait_)(vqa_ctx *, vqa_pu21_metrics *, int) = vqa_pu21_wait;\n'
           'double (*enc)(double) = vqa_pu21_encode;\n'
           'int main(void){printf("%zu %zu %zu %zu %d %d %d %d %d %.10f\\n", sizeof(vqa_pu21_metrics), '
           'offsetof(vqa_pu21_metrics, ssim_q), offsetof(vqa_pu21_metrics, mse_y), offsetof(vqa_pu21_metrics, pu_ssim), '
           'VQA_K_PU21_ENCODE, VQA_K_PU21_SSIM, VQA_K_RIM, VQA_K_VERGE, VQA_ABI_VERSION, enc(100.0));'
           'return submit == 0 || wait_ == 0;}\n')
    (tmp_path / "s.c").write_text(src)
    lib_dir = os.path.dirname(N.LIB_PATH)
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), "-o", str(tmp_path / "s"), str(tmp_path / "s.c"),
                           "-L", lib_dir, "-l:" + os.path.basename(N.LIB_PATH), "-Wl,-rpath," + lib_dir,
                           "-Wl,--allow-shlib-undefined"])
    assert subprocess.check_output([str(tmp_path / "s")]).decode().split() == ["88", "32", "48", "80", "53", "54", "55", "52", "8",
                                                                              "256.3838973127"]


# ---- the restatement -------------------------------------------------------------------------------------------------------
def test_the_gaussian_stage_against_scipy():
    from scipy import ndimage, signal
    g = np.array(R.window())
    assert abs(g.sum() - 1.0) <= 1e-15 and (g == g[::-1]).all() and abs(g[5] / g[4] - np.exp(1 / 4.5)) <= 1e-15
    rng = np.random.default_rng(7)
    v = rng.uniform(0.0, 596.0, (23, 29))
    got = R.filt(v)
    sep = ndimage.correlate1d(ndimage.correlate1d(v, g, axis=1, mode="constant"), g, axis=0, mode="constant")[5:-5, 5:-5]
    full = signal.convolve2d(v, np.outer(g, g), mode="valid")
    assert got.shape == (13, 19) == sep.shape == full.shape
    assert np.abs(got - sep).max() <= 1e-12 * 596.0 and np.abs(got - full).max() <= 1e-12 * 596.0


def test_the_ssim_on_hand_cases():
    rng = np.random.default_rng(8)
    x = rng.integers(0, 1 << 26, (20, 18)).astype(np.float64) / R.FIX
    assert (R.ssim_map(x, x) == 1.0).all()                                      # identical frames: exactly 1
    a, b = 37.25, 412.5
    s = R.ssim_map(np.full((16, 16), a), np.full((16, 16), b))
    assert np.abs(s - (2 * a * b + R.C1) / (a * a + b * b + R.C1)).max() <= 1e-9   # two constants: the luminance term alone
    mean = 300.0
    d = rng.uniform(-200.0, 200.0, (16, 16))
    assert (R.ssim_map(mean + d, mean - d) < 0).all()                           # a frame against its negative about a mean
    assert R.C1 == 2.56 * 2.56 and R.C2 == 7.68 * 7.68


def test_quantised_against_unquantised():
    worst = {"ssim": (0.0, ""), "mse": (0.0, "")}
    for case in PC.matrix():
        for i, (f, q, qa, qb) in enumerate(PC.reference(case)):
            tag = "%s frame %d" % (PC.case_id(case), i)
            for k in ("mse_y", "mse_rgb"):
                bar = 2.0 ** -15 * np.sqrt(f[k]) + 2.0 ** -32                    # each difference moves by at most 2^-16
                gap = abs(q[k] - f[k])
                if gap / bar > worst["mse"][0]:
                    worst["mse"] = (gap / bar, tag + " " + k)
                assert gap <= bar, (tag, k, q[k], f[k])
            gap = abs(q["pu_ssim"] - f["pu_ssim"])
            if gap > worst["ssim"][0]:
                worst["ssim"] = (gap, tag)
            assert gap <= R.SSIM_BAR, (tag, q["pu_ssim"], f["pu_ssim"])
            if case[3] == "equal":
                assert q["sse_y_lo"] == q["sse_y_hi"] == q["sse_rgb_lo"] == q["sse_rgb_hi"] == 0
                assert q["ssim_q"] == q["windows"] << 24 and q["pu_ssim"] == 1.0 and q["pu_psnr"] == float("inf")
            assert qa.max() < 2 ** 26 and qb.max() < 2 ** 26 and qa.min() >= 0
    print("quantised against unquantised over %d cases: pu_ssim gap at most %.3e (%s; bar %.3e), mse gap at most %.3f of its bar (%s)"
          % (len(PC.matrix()), worst["ssim"][0], worst["ssim"][1], R.SSIM_BAR, worst["mse"][0], worst["mse"][1]))
    assert 4.0 * worst["ssim"][0] <= R.SSIM_BAR * 1.01                           # the bar is four times the measured figure


def test_the_two_word_join_at_the_worst_case():
    """black against peak at every sample: every term is the largest there is"""
    top = int(np.rint(float(R.encode(10000.0)) * R.FIX))
    n = 64 * 64
    lo, hi = R.sse_words(np.zeros(n, np.int64), np.full(n, top, np.int64))
    assert R.join(lo, hi) == n * top * top and top * top < 2 ** 52
    assert lo == n * ((top * top) & 0xffffffff) and hi == n * ((top * top) >> 32)
    assert (3 << 28) * 0xffffffff < 2 ** 62 and (3 << 28) * ((top * top) >> 32) < 2 ** 62        # a 2^28-pixel frame: no overflow
    rec = R.finalize((lo, hi, 3 * lo, 3 * hi, n << 24), 74, 74)
    assert rec["mse_y"] == float(n * top * top) / (4294967296.0 * 74 * 74)
    big = R.join(0xfffffffffffffff, 0xfffffffffffffff)                                          # past 2^64: Python integers
    assert big == (0xfffffffffffffff << 32) + 0xfffffffffffffff and big > 2 ** 64


# ---- the log and the row ---------------------------------------------------------------------------------------------------
def _records(n):
    from rtvqa_amd.engine import PU21_DTYPE
    rec = np.zeros(n, PU21_DTYPE)
    rec["pu_psnr"], rec["pu_psnr_rgb"] = [40.0, np.inf, 120.0][:n], [38.0, np.inf, 50.0][:n]
    rec["pu_ssim"] = [0.5, 1.0, 0.75][:n]
    return rec


def _itp(n):
    from rtvqa_amd.engine import ITP_DTYPE
    rec = np.zeros(n, ITP_DTYPE)
    rec["de_mean"], rec["de_max"] = [0.5, 0.0, 0.25][:n], [4.0, 0.0, 8.5][:n]
    return rec


def test_the_json_log_and_what_the_row_takes_from_it(tmp_path):
    rec, it = _records(3), _itp(3)
    old, log, only = str(tmp_path / "old.json"), str(tmp_path / "vmaf.json"), str(tmp_path / "pu.json")
    vp.write_vif_log(old, delta_itp=it)
    vp.write_vif_log(log, delta_itp=it, pu21=rec)
    doc0, doc = json.load(open(old)), json.load(open(log))
    assert "pu_" not in json.dumps(doc0)
    names0 = list(doc0["frames"][0]["metrics"])
    assert names0 == ["delta_itp", "delta_itp_max"]
    assert list(doc["frames"][1]["metrics"]) == names0 + ["pu_psnr", "pu_psnr_rgb", "pu_ssim"] == list(doc["pooled_metrics"])
    for i in range(3):
        assert {k: doc["frames"][i]["metrics"][k] for k in names0} == doc0["frames"][i]["metrics"]
    assert [f["metrics"]["pu_psnr"] for f in doc["frames"]] == [40.0, 100.0, 100.0]             # the cap: inf and 120 -> 100.0
    assert [f["metrics"]["pu_psnr_rgb"] for f in doc["frames"]] == [38.0, 100.0, 50.0]
    assert [f["metrics"]["pu_ssim"] for f in doc["frames"]] == [0.5, 1.0, 0.75]
    assert {k: doc["pooled_metrics"][k] for k in names0} == doc0["pooled_metrics"]
    assert doc["pooled_metrics"]["pu_psnr"]["mean"] == 80.0 and doc["pooled_metrics"]["pu_ssim"]["mean"] == 0.75
    vp.write_vif_log(only, pu21=rec)
    assert list(json.load(open(only))["frames"][0]["metrics"]) == ["pu_psnr", "pu_psnr_rgb", "pu_ssim"]
    pl, sl = tmp_path / "psnr.log", tmp_path / "ssim.log"
    pl.write_text("n:1 mse_avg:1.00 psnr_avg:48.13 \n")
    sl.write_text("n:1 Y:0.990000 All:0.990000 (20.000000)\n")
    m0 = vp.extract_metrics_from_logs(str(pl), str(sl), old, "x", 23, 1000, "64x64", 30.0)
    m = vp.extract_metrics_from_logs(str(pl), str(sl), log, "x", 23, 1000, "64x64", 30.0)
    assert list(m0)[-1] == "DELTA_ITP_MAX" and list(m) == list(m0) + ["PU_PSNR", "PU_PSNR_RGB", "PU_SSIM"]
    assert {k: m[k] for k in m0} == m0 and m["PU_PSNR"] == 80.0 and m["PU_PSNR_RGB"] == (38.0 + 100.0 + 50.0) / 3 and m["PU_SSIM"] == 0.75
    assert m["PU_PSNR"] <= 100.0 and vp.PU21_PSNR_CAP == 100.0
    # logs without the key are what they were, byte for byte
    again = str(tmp_path / "again.json")
    vp.write_vif_log(again, delta_itp=it, pu21=None)
    assert open(again, "rb").read() == open(old, "rb").read()
    # the pass's tuple -> the log: the last element is PU21's [n], dE_ITP's [n] the one before it
    q = (None, None, it, rec)
    vp._write_feature_log(again, q, dict(vif=False, adm=False, delta_itp=True, pu21=True))
    assert open(again, "rb").read() == open(log, "rb").read()
    vp._write_feature_log(again, q[:-1], dict(vif=False, adm=False, delta_itp=True))
    assert open(again, "rb").read() == open(old, "rb").read()
    vp._write_feature_log(again, (None, None, rec), dict(vif=False, adm=False, pu21=True))
    assert open(again, "rb").read() == open(only, "rb").read()


def test_config_keys():
    vp.validate_config(dict(GOOD))
    vp.validate_config(dict(GOOD, pu21=True))
    vp.validate_config(dict(GOOD, pu21=True, pu21_transfer="hlg", pu21_range="full"))
    vp.validate_config(dict(GOOD, pu21=False, pu21_transfer="pq", pu21_range="limited", delta_itp=True))
    for bad in (1, 0, "true", None, "only"):
        with pytest.raises(ValueError) as e:
            vp.validate_config(dict(GOOD, pu21=bad))
        assert str(e.value) == "pu21 must be true or false."
    for bad in ("PQ", "sdr", 0, None, True):
        with pytest.raises(ValueError) as e:
            vp.validate_config(dict(GOOD, pu21=True, pu21_transfer=bad))
        assert str(e.value) == 'pu21_transfer must be "pq" or "hlg".'
    for bad in ("tv", "Full", 1, None, False):
        with pytest.raises(ValueError) as e:
            vp.validate_config(dict(GOOD, pu21=True, pu21_range=bad))
        assert str(e.value) == 'pu21_range must be "limited" or "full".'


def test_the_stream_request():
    p = [(16, 16, 0, 16, 1), (8, 8, 256, 8, 1), (8, 8, 320, 8, 1)]
    assert stream.Quality(p).pu21 is False and stream.Quality(p, vif=True, itp=True).pu21 is False
    q = stream.Quality(p, pu21=True)
    assert q.pu21 is True and q.pu21_transfer == "pq" and q.pu21_full_range is False and q.ssim is True and q.itp is False
    q = stream.Quality(p, pu21="only", pu21_transfer="hlg", pu21_full_range=True)
    assert q.pu21 == "only" and q.pu21_transfer == "hlg" and q.pu21_full_range is True and q.ssim is False
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="pu21 must be False, True or 'only'"):
            stream.Quality(p, pu21=bad)
    for bad in ("sdr", "PQ", 0, None):
        with pytest.raises(ValueError, match="pu21_transfer must be 'pq' or 'hlg'"):
            stream.Quality(p, pu21=True, pu21_transfer=bad)
    for bad in (1, "full", None):
        with pytest.raises(ValueError, match="pu21_full_range must be True or False"):
            stream.Quality(p, pu21=True, pu21_full_range=bad)
    with pytest.raises(ValueError):
        stream.Quality(p, N.SSIM_MS, scales=True, pu21="only")
    for k in (1, 2):
        with pytest.raises(ValueError, match="pu21 needs three planes"):
            stream.Quality(p[:k], pu21=True)
    z = np.zeros((0, 384), np.uint8)
    # an empty clip: without the request the tuples are what they were; with it ONE further last element, after dE_ITP's
    for kw, length in ((dict(), 2), (dict(vif=True), 3), (dict(itp=True), 3), (dict(mdsi=True, itp=True), 4)):
        q0, _ = stream.run(z, z, quality=stream.Quality(p, **kw))
        q1, _ = stream.run(z, z, quality=stream.Quality(p, pu21=True, **kw))
        assert len(q0) == length and len(q1) == length + 1, kw
        assert q1[-1].shape == (0,) and q1[-1].dtype.names == FIELDS
        for a, b in zip(q0, q1):
            assert (a is None and b is None) or (a.dtype == b.dtype and a.shape == b.shape)
    q, _ = stream.run(z, z, quality=stream.Quality(p, pu21="only"))
    assert len(q) == 3 and q[0] is None and q[1] is None and q[2].shape == (0,)


def test_the_argument_errors_of_the_entry_points(tmp_path):
    """before anything reaches a device: one-plane layouts, unknown transfers and ranges"""
    g = np.zeros((2, 16, 16), np.uint8)
    y = np.zeros((2, 384), np.uint8)
    with pytest.raises(ValueError, match="pu21 needs three planes"):
        vp.frame_pu21(g, g, "gray", 16, 16)
    for bad in ("sdr", "PQ", 0, None):
        with pytest.raises(ValueError, match="pu21_transfer must be 'pq' or 'hlg'"):
            vp.frame_pu21(y, y, "yuv420p", 16, 16, transfer=bad)
    for bad in ("full", 1, None):
        with pytest.raises(ValueError, match="pu21_full_range must be True or False"):
            vp.frame_pu21(y, y, "yuv420p", 16, 16, full_range=bad)
    logs = [str(tmp_path / n) for n in ("p.log", "s.log", "v.json")]
    with pytest.raises(ValueError, match="pu21 needs three planes"):
        vp.run_ffmpeg_metrics(g, g, *logs, layout="gray", pu21=True)
    with pytest.raises(ValueError, match="pu21_transfer must be 'pq' or 'hlg'"):
        vp.run_ffmpeg_metrics(y, y, *logs, layout="yuv420p", height=16, width=16, pu21=True, pu21_transfer="sdr")
    with pytest.raises(ValueError, match="pu21_full_range must be True or False"):
        vp.run_ffmpeg_metrics(y, y, *logs, layout="yuv420p", height=16, width=16, pu21=True, pu21_full_range="full")
