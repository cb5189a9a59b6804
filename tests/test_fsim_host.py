"""FSIM / FSIMc on the host side (no GPU): vqa_fsim_filter and vqa_fsim_noise_factor through ctypes against the restatement of
tests/fsim_reference.py; the restatement's own properties (FSIM(x, x) = 1, PC within [0, 1], PC unchanged by the centring, the
gray model's fsimc == fsim, its Scharr stage against SciPy); the restatement under an explicit dense float64 DFT against np.fft
on every matrix case; the integer pooling against the float pooling on every case within that case's derived bar; the additive
ABI (ids 56 .. 61, one-past 62; 55 and 52 stay unknown; ABI 8; 56 bytes); the JSON log, the row, the config key and the stream
request."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import fsim_cases as FC
import fsim_reference as R
from rtvqa_amd import _native as N
from rtvqa_amd import stream
from rtvqa_amd import video_processing as vp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOOD = {"crf": 23, "vmaf_model_path": None, "resize_width": 64, "resize_height": 64, "frame_interval": 10}
FIELDS = ("sum_pc", "sum_sim", "sum_simc", "count", "factor", "flags", "fsim", "fsimc")
GRIDS = ((16, 16), (33, 67), (67, 130), (129, 97))
CASES = FC.matrix()


# ---- the host's tables ---------------------------------------------------------------------------------------------------------
def test_the_filter_tables_against_the_restatement():
    """bar: 64 ulp of the table's largest entry.  Measured here: at most 5.6e-16 absolute on tables whose largest entries are
    0.5 .. 1.0 (5 ulp: libm's exp, log, pow and atan2 against NumPy's)."""
    lib = N.load()
    worst = 0.0
    for hd, wd in GRIDS:
        want = R.filters(hd, wd)
        buf = np.empty((hd, wd))
        for o in range(4):
            for s in range(4):
                assert lib.vqa_fsim_filter(hd, wd, s, o, buf.ctypes.data_as(C.POINTER(C.c_double))) == N.VQA_OK
                gap = float(np.abs(buf - want[o, s]).max())
                worst = max(worst, gap)
                assert gap <= 64.0 * np.spacing(float(want[o, s].max())), (hd, wd, s, o, gap)
                assert buf[0, 0] == 0.0
    print("vqa_fsim_filter: largest gap %.3g" % worst)
    buf = np.empty((16, 16))
    p = buf.ctypes.data_as(C.POINTER(C.c_double))
    for bad in ((1, 16, 0, 0), (16, 1025, 0, 0), (16, 16, 4, 0), (16, 16, 0, 4), (16, 16, -1, 0), (16, 16, 0, -1)):
        assert lib.vqa_fsim_filter(*bad, p) == N.VQA_ERR_INVALID, bad
    assert lib.vqa_fsim_filter(16, 16, 0, 0, None) == N.VQA_ERR_INVALID


def test_the_noise_factor_against_the_ifft2_form():
    """the Parseval identity is exact: only rounding differs"""
    lib = N.load()
    for hd, wd in GRIDS:
        for o in range(4):
            got, want = lib.vqa_fsim_noise_factor(hd, wd, o), R.noise_factor(hd, wd, o)
            assert abs(got - want) <= 1e-12 * want, (hd, wd, o, got, want)
    assert np.isnan(lib.vqa_fsim_noise_factor(16, 16, 4)) and np.isnan(lib.vqa_fsim_noise_factor(1, 16, 0))


# ---- the restatement's own properties --------------------------------------------------------------------------------------------
def test_identical_frames_score_one_and_pc_stays_in_range():
    for layout, (h, w) in (("yuv420p", (33, 67)), ("bgr24", (67, 130)), ("gray", (16, 16))):
        r, d = FC.pair("natural", layout, h, w)
        fs, fc, pr, pd, _, _ = R.fsim_float(list(r), list(r), FC.MODEL[layout])
        assert fs == 1.0 and abs(fc - 1.0) <= 1e-15
        for pc in (pr, R.phase_congruency(R.channels(list(d), FC.MODEL[layout])[0])):
            assert pc.min() >= 0.0 and pc.max() <= 1.0 and pc.max() > 0.05


def test_pc_is_unchanged_by_the_centring():
    for name in ("natural", "noise", "half"):
        r, _ = FC.pair(name, "gray", 33, 67)
        y = R.channels(list(r), "gray")[0]
        assert np.abs(R.phase_congruency(y) - R.phase_congruency(y, centre=False)).max() <= 1e-9, name
    flat = np.full((16, 16), 97.0)
    assert (R.phase_congruency(flat) == 0.0).all()


def test_the_gray_model_has_no_chroma_term():
    r, d = FC.pair("natural", "gray", 33, 67)
    fs, fc = R.fsim_float(list(r), list(d), "gray")[:2]
    assert fs == fc and 0.0 < fs < 1.0
    r, d = FC.pair("natural", "bgr24", 33, 67)
    fs, fc = R.fsim_float(list(r), list(d), "bgr")[:2]
    assert fc != fs


def test_the_scharr_stage_against_scipy():
    sig = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(3)
    x = rng.uniform(0.0, 255.0, (33, 67))
    k = np.array([[3.0, 0.0, -3.0], [10.0, 0.0, -10.0], [3.0, 0.0, -3.0]]) / 16.0
    gx, gy = R.scharr(x)
    assert np.abs(gx - sig.convolve2d(x, k, mode="same")).max() <= 1e-12
    assert np.abs(gy - sig.convolve2d(x, k.T, mode="same")).max() <= 1e-12


# ---- the dense DFT against np.fft, on every case ---------------------------------------------------------------------------------
def test_the_dense_dft_against_the_fft_on_every_case():
    """the largest PC gap is printed and must stay below 2^-30, 1/64 of the map's quantum.  Measured here: 1.6e-14."""
    worst, seen = 0.0, set()
    for case in CASES:
        c, l, (h, w), dp = case
        r, d = FC.pair(c, l, h, w, dp)
        for planes in (r, d):
            y = R.channels(list(planes), FC.MODEL[l], dp)[0]
            key = y.tobytes()
            if key in seen:
                continue
            seen.add(key)
            gap = float(np.abs(R.phase_congruency(y, dense=True) - R.phase_congruency(y)).max())
            worst = max(worst, gap)
            assert gap < 2.0 ** -30, (FC.case_id(case), gap)
    print("dense DFT against np.fft: largest PC gap %.3g over %d grids" % (worst, len(seen)))


# ---- the integer pooling against the float pooling, on every case ------------------------------------------------------------------
def test_the_integer_pooling_against_the_float_pooling_on_every_case():
    """every case is admitted: its derived bar 4 N 2^-24 / sum PC_m does not exceed 1e-4 (structureless cases have P = 0 and
    score 1.0 both ways).  Measured here: bars up to 8.3e-6, gaps at most 2.6e-8."""
    assert len(CASES) == FC.MATRIX_CASES
    worst_gap = worst_bar = 0.0
    for case in CASES:
        c, l, (h, w), dp = case
        r, d = FC.pair(c, l, h, w, dp)
        e = FC.expected(case)
        words = R.pool_words(list(r), list(d), FC.MODEL[l], dp, R.quantise(e["pc_r"]), R.quantise(e["pc_d"]))
        fs, fc = R.scores_of(words)
        if c in FC.STRUCTURELESS:
            assert words == (0, 0, 0) and (fs, fc) == (1.0, 1.0) and (e["fsim"], e["fsimc"]) == (1.0, 1.0), FC.case_id(case)
            continue
        assert e["bar"] <= FC.BAR_LIMIT, (FC.case_id(case), e["bar"])
        gap = max(abs(fs - e["fsim"]), abs(fc - e["fsimc"]))
        assert gap <= e["bar"], (FC.case_id(case), gap, e["bar"])
        worst_gap, worst_bar = max(worst_gap, gap), max(worst_bar, e["bar"])
        if c == "identical":
            assert words[0] == words[1] == words[2] and (fs, fc) == (1.0, 1.0)
    print("integer against float pooling: largest gap %.3g, largest bar %.3g" % (worst_gap, worst_bar))


# ---- ABI -------------------------------------------------------------------------------------------------------------------------
def test_the_additive_abi():
    assert N.VQA_ABI_VERSION == 8
    assert C.sizeof(N.VqaFsimMetrics) == 56
    assert [getattr(N.VqaFsimMetrics, f).offset for f in FIELDS] == [0, 8, 16, 24, 32, 36, 40, 48]
    from rtvqa_amd.engine import FSIM_DTYPE
    assert FSIM_DTYPE.itemsize == 56 and FSIM_DTYPE.names == FIELDS
    ids = (N.K_FSIM_LUMA, N.K_FSIM_DFT, N.K_FSIM_ENERGY, N.K_FSIM_MEDIAN, N.K_FSIM_PC, N.K_FSIM_POOL)
    assert ids == (56, 57, 58, 59, 60, 61) and N.K_HEM == 62 and N.K_RIM == 55 and N.K_VERGE == 52
    assert N.K_IDS_ENTIRE == N.K_IDS_GRAND + ids and 55 not in N.K_IDS_ENTIRE and 52 not in N.K_IDS_ENTIRE
    assert (N.FSIM_YUV709, N.FSIM_BGR, N.FSIM_GRAY) == (N.MDSI_YUV709, N.MDSI_BGR, N.MDSI_GRAY) == (0, 1, 2)
    assert N.FSIM_FIX == R.FIX == 1 << 24 and N.FSIM_MIN_DIM == 16 and N.FSIM_MAX_GRID == 1024
    txt = open(os.path.join(REPO, "include", "vqa.h")).read()
    for name, val in (("VQA_K_FSIM_LUMA", 56), ("VQA_K_FSIM_POOL", 61), ("VQA_K_HEM", 62), ("VQA_K_RIM", 55), ("VQA_K_VERGE", 52)):
        assert re.search(r"%s\s*=\s*%d\b" % (name, val), txt), name
    assert re.search(r"#define VQA_ABI_VERSION\s+8", txt)
    part = txt[txt.index("---- FSIM / FSIMc"):]
    part = part[:part.index("VQA_API int vqa_fsim_wait")]
    for word in ("NOT pinned", "phasecong2", "0.596", "0.523", "0.85", "160", "200", "0.03", "0.45", "0.55", "1e-4", "1.7",
                 "rint(PC 2^24)", "256 MiB", "at least 16 x 16", "<= 1024", "first version"):
        assert word in part, word
    lib = N.load()
    for sym in ("vqa_fsim_submit", "vqa_fsim_wait", "vqa_fsim_noise_factor", "vqa_fsim_filter"):
        assert hasattr(lib, sym)
    lib.vqa_kernel_name.restype = C.c_char_p
    names = [lib.vqa_kernel_name(i) for i in range(56, 62)]
    assert names == [b"k_fsim_luma", b"k_fsim_dft", b"k_fsim_energy", b"k_fsim_median", b"k_fsim_pc", b"k_fsim_pool"]
    assert lib.vqa_kernel_name(55) == b"?" and lib.vqa_kernel_name(52) == b"?" and lib.vqa_kernel_name(62) == b"?"
    assert lib.vqa_kernel_name(54) == b"k_pu21_ssim"
    assert lib.vqa_fsim_submit(None, None, None, 0, 0, 0, 0, None, 0, 0) == N.VQA_ERR_INVALID
    assert lib.vqa_fsim_wait(None, None, 0) == N.VQA_ERR_INVALID
    # the read-back of the maps is the lab build's alone
    shipped = C.CDLL(os.path.join(REPO, "real-time-video-quality-analysis_amd", "csrc", "libvqa_hip.so"))
    assert not hasattr(shipped, "vqa_fsim_lab_read_maps")
    assert hasattr(C.CDLL(N.LAB_LIB_PATH), "vqa_fsim_lab_read_maps")
    assert b"VQA_FSIM_SUBSLICE" in open(N.LAB_LIB_PATH, "rb").read()
    assert b"VQA_FSIM_SUBSLICE" not in open(N.LIB_PATH, "rb").read()


def test_the_header_to_the_c_compiler(tmp_path):
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "vqa.h"\n'
           'int (*submit)(vqa_ctx *, const uint8_t *, const uint8_t *, int, int, int64_t, int64_t, const vqa_plane_desc *, int, int) '
           '= vqa_fsim_submit;\n'
           'int (*wait_)(vqa_ctx *, vqa_fsim_metrics *, int) = vqa_fsim_wait;\n'
           'double (*nf)(int, int, int) = vqa_fsim_noise_factor;\n'
           'int (*flt)(int, int, int, int, double *) = vqa_fsim_filter;\n'
           'int main(void){printf("%zu %zu %zu %zu %d %d %d %d %d %d %d\\n", sizeof(vqa_fsim_metrics), '
           'offsetof(vqa_fsim_metrics, factor), offsetof(vqa_fsim_metrics, flags), offsetof(vqa_fsim_metrics, fsimc), '
           'VQA_K_FSIM_LUMA, VQA_K_FSIM_POOL, VQA_K_HEM, VQA_K_RIM, VQA_ABI_VERSION, VQA_FSIM_GRAY, nf(16, 16, 0) > 0.0);'
           'return submit == 0 || wait_ == 0 || flt == 0;}\n')
    (tmp_path / "s.c").write_text(src)
    lib_dir = os.path.dirname(N.LIB_PATH)
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), "-o", str(tmp_path / "s"), str(tmp_path / "s.c"),
                           "-L", lib_dir, "-l:" + os.path.basename(N.LIB_PATH), "-Wl,-rpath," + lib_dir,
                           "-Wl,--allow-shlib-undefined"])
    assert subprocess.check_output([str(tmp_path / "s")]).decode().split() == ["56", "32", "36", "48", "56", "61", "62", "55", "8",
                                                                              "2", "1"]


# ---- the Python layers -------------------------------------------------------------------------------------------------------------
def _records(n):
    from rtvqa_amd.engine import FSIM_DTYPE
    rec = np.zeros(n, FSIM_DTYPE)
    rec["fsim"] = [0.5, 1.0, 0.75][:n]
    rec["fsimc"] = [0.25, 1.0, 0.5][:n]
    return rec


def test_the_json_log_and_what_the_row_takes_from_it(tmp_path):
    from rtvqa_amd.engine import PU21_DTYPE
    rec = _records(3)
    pu = np.zeros(3, PU21_DTYPE)
    pu["pu_psnr"], pu["pu_psnr_rgb"], pu["pu_ssim"] = [40.0, 41.0, 42.0], [38.0, 39.0, 40.0], [0.5, 0.6, 0.7]
    old, log, only = str(tmp_path / "old.json"), str(tmp_path / "vmaf.json"), str(tmp_path / "fsim.json")
    vp.write_vif_log(old, pu21=pu)
    vp.write_vif_log(log, pu21=pu, fsim=rec)
    doc0, doc = json.load(open(old)), json.load(open(log))
    assert "fsim" not in json.dumps(doc0)
    names0 = list(doc0["frames"][0]["metrics"])
    assert names0[-1] == "pu_ssim"
    assert list(doc["frames"][1]["metrics"]) == names0 + ["fsim", "fsimc"] == list(doc["pooled_metrics"])
    assert [f["metrics"]["fsim"] for f in doc["frames"]] == [0.5, 1.0, 0.75]
    assert [f["metrics"]["fsimc"] for f in doc["frames"]] == [0.25, 1.0, 0.5]
    assert {k: doc["pooled_metrics"][k] for k in names0} == doc0["pooled_metrics"]
    vp.write_vif_log(only, fsim=rec)
    assert list(json.load(open(only))["frames"][0]["metrics"]) == ["fsim", "fsimc"]
    pl, sl = tmp_path / "psnr.log", tmp_path / "ssim.log"
    pl.write_text("n:1 mse_avg:1.00 psnr_avg:48.13 \n")
    sl.write_text("n:1 Y:0.990000 All:0.990000 (20.000000)\n")
    m0 = vp.extract_metrics_from_logs(str(pl), str(sl), old, "x", 23, 1000, "64x64", 30.0)
    m = vp.extract_metrics_from_logs(str(pl), str(sl), log, "x", 23, 1000, "64x64", 30.0)
    assert list(m0)[-1] == "PU_SSIM" and list(m) == list(m0) + ["FSIM", "FSIMC"]
    assert {k: m[k] for k in m0} == m0 and m["FSIM"] == 0.75 and m["FSIMC"] == (0.25 + 1.0 + 0.5) / 3
    # logs without the key are what they were, byte for byte
    again = str(tmp_path / "again.json")
    vp.write_vif_log(again, pu21=pu, fsim=None)
    assert open(again, "rb").read() == open(old, "rb").read()
    # the pass's tuple -> the log: the last element is FSIM's [n], PU21's [n] the one before it
    q = (None, None, pu, rec)
    vp._write_feature_log(again, q, dict(vif=False, adm=False, pu21=True, fsim=True))
    assert open(again, "rb").read() == open(log, "rb").read()
    vp._write_feature_log(again, q[:-1], dict(vif=False, adm=False, pu21=True))
    assert open(again, "rb").read() == open(old, "rb").read()
    vp._write_feature_log(again, (None, None, rec), dict(vif=False, adm=False, fsim=True))
    assert open(again, "rb").read() == open(only, "rb").read()


def test_the_config_key():
    vp.validate_config(dict(GOOD))
    vp.validate_config(dict(GOOD, fsim=True))
    vp.validate_config(dict(GOOD, fsim=False, mdsi=True))
    for bad in (1, 0, "true", None, "only"):
        with pytest.raises(ValueError) as e:
            vp.validate_config(dict(GOOD, fsim=bad))
        assert str(e.value) == "fsim must be true or false."


def test_the_stream_request():
    p = [(16, 16, 0, 16, 1), (8, 8, 256, 8, 1), (8, 8, 320, 8, 1)]
    assert stream.Quality(p).fsim is False and stream.Quality(p, vif=True, pu21=True).fsim is False
    q = stream.Quality(p, fsim=True)
    assert q.fsim is True and q.ssim is True and q.mdsi is False
    q = stream.Quality(p[:1], fsim="only")
    assert q.fsim == "only" and q.ssim is False
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="fsim must be False, True or 'only'"):
            stream.Quality(p, fsim=bad)
    with pytest.raises(ValueError):
        stream.Quality(p, N.SSIM_MS, scales=True, fsim="only")
    with pytest.raises(ValueError, match="fsim needs one plane or three"):
        stream.Quality(p[:2], fsim=True)
    z = np.zeros((0, 384), np.uint8)
    # an empty clip: without the request the tuples are what they were; with it ONE further last element, after PU21's
    for kw, length in ((dict(), 2), (dict(vif=True), 3), (dict(pu21=True), 3), (dict(mdsi=True, pu21=True), 4)):
        q0, _ = stream.run(z, z, quality=stream.Quality(p, **kw))
        q1, _ = stream.run(z, z, quality=stream.Quality(p, fsim=True, **kw))
        assert len(q0) == length and len(q1) == length + 1, kw
        assert q1[-1].shape == (0,) and q1[-1].dtype.names == FIELDS
        for a, b in zip(q0, q1):
            assert (a is None and b is None) or (a.dtype == b.dtype and a.shape == b.shape)
    q, _ = stream.run(z, z, quality=stream.Quality(p, fsim="only"))
    assert len(q) == 3 and q[0] is None and q[1] is None and q[2].shape == (0,)
