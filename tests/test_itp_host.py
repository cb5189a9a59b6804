"""dE_ITP (ITU-R BT.2124) on the host side (no GPU): the float64 NumPy restatement of tests/itp_reference.py against known
answers of BT.2100 / BT.2408, its own properties (gray axis, the gray step, equal frames, the clamp, full against limited range),
what float32 would cost (the reason k_itp is double), the additive ABI (vqa_itp_submit, vqa_itp_wait, vqa_itp_metrics,
VQA_K_ITP), the JSON log and the row, the config keys, the stream request and the argument errors of every Python layer.

The HLG table.  Its PQ-signal column and the 0.5 row hold to 1e-8 absolutely.  The cd/m2 figures of the 0.75 and 1.0 rows,
203.15214594 and 1000.0000323, hold to 1e-8 RELATIVE (3e-9 seen): they were recomputed with c = 0.5 - a ln(4a) unrounded, while the
definition built here states c = 0.55991073 (BT.2100's printed value), which gives 203.15214535 and 1000.0000292.  The definition
is what is built; the bar is read as relative for that column, as the PQ EOTF table's is."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import itp_cases as IC
import itp_reference as R
from rtvqa_amd import _native as N
from rtvqa_amd import stream
from rtvqa_amd import video_processing as vp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOOD = {"crf": 23, "vmaf_model_path": None, "resize_width": 64, "resize_height": 64, "frame_interval": 10}
FIELDS = ("sum_q", "max_q", "de_sum", "de_mean", "de_max")


def _flat(v, h=16, w=16):
    return [np.full((h, w), x, np.int64) for x in v]


# ---- known answers ---------------------------------------------------------------------------------------------------------
def test_the_pq_eotf():
    got = R.pq_eotf([0.0, 1.0, 0.5])
    assert got[0] == 0.0
    for g, want in zip(got[1:], (10000.0, 92.24570899)):
        assert abs(g - want) <= 1e-9 * want, (g, want)


def test_the_pq_inverse():
    for x, want in ((100.0, 0.50807842), (203.0, 0.58068888), (1000.0, 0.7518271)):
        assert abs(float(R.pq_inverse(x)) - want) <= 1e-8, (x, want)
    e = np.linspace(0.0, 1.0, 1025)[1:]
    assert np.abs(R.pq_inverse(R.pq_eotf(e)) - e).max() <= 1e-12          # the two are inverses above the EOTF's floor:
    assert float(R.pq_inverse(0.0)) == R.C1 ** R.M2 and 7.3e-7 < R.C1 ** R.M2 < 7.4e-7   # signals below c1^m2 all show as 0 cd/m2


def test_hlg_gray_is_bt2408s():
    """HLG 75 % = 203 cd/m2 = PQ 58 % (see the module's text for the bar of the cd/m2 column)"""
    for e, nits, sig in ((0.5, 50.69702849, 0.44159846), (0.75, 203.15214594, 0.58076719), (1.0, 1000.0000323, 0.7518271)):
        f = R.hlg_display(e, e, e)
        assert f[0] == f[1] == f[2]
        print("HLG %.2f: %.10f cd/m2 (table %.10f, gap %.2e relative), PQ %.10f" % (e, f[0], nits, abs(f[0] - nits) / nits,
                                                                                  R.pq_inverse(f[0])))
        assert abs(float(f[0]) - nits) <= 1e-8 * nits
        assert abs(float(R.pq_inverse(f[0])) - sig) <= 1e-8
    assert abs(float(R.hlg_display(0.5, 0.5, 0.5)[0]) - 50.69702849) <= 1e-8
    assert all(float(x) == 0.0 for x in R.hlg_display(0.0, 0.0, 0.0))      # Ys = 0 gives 0
    assert float(R.hlg_scene(0.5)) == 0.25 / 3.0


def test_the_gray_axis_under_pq():
    e = np.linspace(0.0, 1.0, 257)[1:]          # (E' = 0 shows as 0 cd/m2, whose signal is the floor c1^m2 = 7.3e-7, not 0)
    itp = R.itp_from_rgb(e, e, e, R.PQ)
    assert np.abs(itp[:, 1]).max() < 1e-12 and np.abs(itp[:, 2]).max() < 1e-12
    assert np.abs(itp[:, 0] - e).max() <= 1e-12


def test_the_gray_step_pair():
    """two 10-bit limited-range gray frames, Y = 502 and 503 with neutral chroma 512: 720 / 876 everywhere; three codes: 3 x"""
    a, b = _flat((502, 512, 512)), _flat((503, 512, 512))
    rec = R.record(a, b, 10)
    assert abs(rec["de_mean"] - 720.0 / 876.0) <= 1e-9 and abs(rec["de_max"] - 720.0 / 876.0) <= 1e-9
    assert abs(720.0 / 876.0 - 0.8219178) < 1e-7
    rec3 = R.record(a, _flat((505, 512, 512)), 10)
    assert abs(rec3["de_mean"] - 2160.0 / 876.0) <= 1e-9 and abs(rec3["de_max"] - 2.4657534) < 1e-7
    # the cases the GPU tests use carry the same pair, at every depth and layout
    for (g, d, lay) in IC.GRID:
        for full in (False, True):
            r, x, pl = IC.clip("graystep", lay, g[0], g[1], d, 1, full_range=full)
            rec = IC.reference(r, x, pl, d, IC.model_of(lay), R.PQ, full)[0]
            want = IC.graystep_answer(lay, d, full)
            assert abs(rec["de_mean"] - want) <= 1e-9 and abs(rec["de_max"] - want) <= 1e-9, (lay, full)
    r, x, pl = IC.clip("graystep", "yuv420p10le", 36, 64, 10, 1)
    assert int(r[0, 0]) == 502 and int(x[0, 0]) == 503 and int(r[0, -1]) == 512


def test_equal_frames_give_zero():
    rng = np.random.default_rng(1)
    a = [rng.integers(0, 1024, (16, 16)) for _ in range(3)]
    for t in (R.PQ, R.HLG):
        rec = R.record(a, [p.copy() for p in a], 10, transfer=t)
        assert rec == {"de_mean": 0.0, "de_max": 0.0, "sum_q": 0, "max_q": 0, "q_mean": 0.0, "q_max": 0.0}


def test_the_clamp():
    """code 0 and code P in every plane: finite, and equal to the clamped triple's values"""
    for depth in (8, 10, 16):
        peak = (1 << depth) - 1
        for t in (R.PQ, R.HLG):
            for full in (False, True):
                for v in (0, peak):
                    rgb = R.rgb_from_yuv(v, v, v, depth, full)
                    got = R.itp_from_yuv(v, v, v, depth, t, full)
                    assert np.isfinite(got).all()
                    assert (got == R.itp_from_rgb(*[min(max(float(x), 0.0), 1.0) for x in rgb], transfer=t)).all()
        lo = R.rgb_from_yuv(0, 0, 0, depth)
        hi = R.rgb_from_yuv(peak, peak, peak, depth)
        assert min(float(x) for x in lo) < 0.0 and max(float(x) for x in hi) > 1.0                  # the clamp has work to do
    assert 1.9 < float(R.rgb_from_yuv(1023, 512, 1023, 10)[0]) < 1.95                               # R' near 1.94
    de = R.frame(_flat((0, 0, 0)), _flat((1023, 1023, 1023)), 10)
    assert np.isfinite(de).all() and de.max() < 6800.0


def test_full_and_limited_range_agree_on_one_colour():
    """the same physical colour coded both ways: 16-bit codes chosen so that both decode to the same y, cb, cr up to 1e-5"""
    y, cb, cr = 0.4, 0.05, -0.03
    lim = (round(16 * 256 + y * 219 * 256), round(128 * 256 + cb * 224 * 256), round(128 * 256 + cr * 224 * 256))
    full = (round(y * 65535), round(32768 + cb * 65535), round(32768 + cr * 65535))
    for t in (R.PQ, R.HLG):
        a, b = R.itp_from_yuv(*lim, depth=16, transfer=t), R.itp_from_yuv(*full, depth=16, transfer=t, full_range=True)
        assert float(R.delta(a, b)) < 0.05, (t, float(R.delta(a, b)))       # a few hundredths of a JND: the coding step
    # and the ranges are different readings of the same codes
    assert float(R.delta(R.itp_from_yuv(*lim, depth=16), R.itp_from_yuv(*lim, depth=16, full_range=True))) > 1.0
    # bgr: full_range changes nothing
    assert (R.itp_from_bgr(10, 200, 90, full_range=True) == R.itp_from_bgr(10, 200, 90)).all()


def test_the_quantised_form():
    de = np.array([[0.0, 1.0 + 2.0 ** -21 + 2.0 ** -30], [2.5, 2.0 ** -22]])
    assert R.words(de) == ((1 << 20) + 1 + 5 * (1 << 19), 5 * (1 << 19))
    r, d, pl = IC.clip("noise3", "yuv420p10le", 19, 17, 10, 1)
    rec = IC.reference(r, d, pl, 10, R.YUV2020, R.PQ, False)[0]
    assert abs(rec["q_mean"] - rec["de_mean"]) <= 2.0 ** -21 and abs(rec["q_max"] - rec["de_max"]) <= 2.0 ** -21
    assert R.BAR == 2.0 ** -20 and R.FIX == 2.0 ** 20


def test_float32_is_not_enough():
    """the precision finding: the chain in float32 on the dark case misses the GPU's bar on the mean by an order of magnitude, and
    single pixels by far more - the cancellation E'^(1/m2) - c1 followed by the 6.28th power.  This is why k_itp is double."""
    (h, w), depth, layout = IC.RANGES_ON
    r, d, pl = IC.clip("dark", layout, h, w, depth, 1)
    a, b = R.split_planes(r, pl)[0], R.split_planes(d, pl)[0]
    f64, f32 = R.frame(a, b, depth), R.frame(a, b, depth, dtype=np.float32)
    gap_mean, gap_pixel = abs(float(f64.mean()) - float(f32.mean())), float(np.abs(f64 - f32).max())
    print("float32 against float64 on the dark case: %.3e on the mean, %.3e on a pixel (bar %.3e)" % (gap_mean, gap_pixel, R.BAR))
    assert gap_mean > R.BAR and gap_pixel > 100 * R.BAR


def test_the_bound_of_the_header():
    worst = 720.0 * np.sqrt(1.0 + (13613.0 / 4096.0) ** 2 + (2 * 17933.0 / 4096.0) ** 2)
    assert worst < 6800.0 < 2 ** 13
    assert int(np.rint(6800.0 * R.FIX)) < 2 ** 33 and (2 ** 33) * (2 ** 28) == 2 ** 61


# ---- ABI -------------------------------------------------------------------------------------------------------------------
def test_the_additive_abi():
    assert N.VQA_ABI_VERSION == 8
    assert C.sizeof(N.VqaItpMetrics) == 40
    assert [getattr(N.VqaItpMetrics, f).offset for f in FIELDS] == [0, 8, 16, 24, 32]
    from rtvqa_amd.engine import ITP_DTYPE
    assert ITP_DTYPE.itemsize == 40 and ITP_DTYPE.names == FIELDS
    assert (N.K_ITP, N.K_VERGE) == (51, 52) and N.K_BRINK == 50
    assert N.K_IDS_SUM == N.K_IDS_TOTAL + (51,) and 50 not in N.K_IDS_SUM
    assert (N.ITP_YUV2020, N.ITP_BGR) == (0, 1) == (R.YUV2020, R.BGR)
    assert (N.ITP_PQ, N.ITP_HLG) == (0, 1) == (R.PQ, R.HLG) and N.ITP_TRANSFERS == {"pq": 0, "hlg": 1}
    assert N.ITP_FIX == R.FIX == 1 << 20 and N.ITP_MIN_DIM == R.MIN_DIM == 16
    txt = open(os.path.join(REPO, "include", "vqa.h")).read()
    for name, val in (("VQA_K_ITP", 51), ("VQA_K_VERGE", 52), ("VQA_K_BRINK", 50), ("VQA_ITP_YUV2020", 0), ("VQA_ITP_BGR", 1),
                      ("VQA_ITP_PQ", 0), ("VQA_ITP_HLG", 1)):
        assert re.search(r"%s\s*=\s*%d\b" % (name, val), txt), name
    assert re.search(r"#define VQA_ABI_VERSION\s+8", txt)
    part = txt[txt.index("---- dE_ITP (Recommendation ITU-R BT.2124"):]
    part = part[:part.index("VQA_API int vqa_itp_wait")]
    for word in ("2610 / 16384", "2523 / 4096 * 128", "3424 / 4096", "2413 / 4096 * 32", "2392 / 4096 * 32", "0.17883277",
                 "0.28466892", "0.55991073", "1.4746", "1.8814", "CLAMPED to [0, 1]", "1688", "3688", "13613", "17933",
                 "720 sqrt", "EXACTLY 0", "< 6800 < 2^13", "2^61", "NO SATURATION", "at least 16 x 16", "h w <= 2^28",
                 "16 bytes per frame", "DOUBLE"):
        assert word in part, word
    lib = N.load()
    for sym in ("vqa_itp_submit", "vqa_itp_wait"):
        assert hasattr(lib, sym)
    lib.vqa_kernel_name.restype = C.c_char_p
    assert lib.vqa_kernel_name(51) == b"k_itp" and lib.vqa_kernel_name(50) == b"?" and lib.vqa_kernel_name(52) == b"?"
    assert lib.vqa_kernel_name(N.K_MDSI_DEV) == b"k_mdsi_dev"
    # argument checks that need no device
    assert lib.vqa_itp_submit(None, None, None, 0, 0, 0, 0, None, 0, 0, 0, 0) == N.VQA_ERR_INVALID
    assert lib.vqa_itp_wait(None, None, 0) == N.VQA_ERR_INVALID
    for k in (50, 51, 52):
        assert lib.vqa_profile_read(None, k, None, None, 0) == N.VQA_ERR_INVALID


def test_the_header_to_the_c_compiler(tmp_path):
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "vqa.h"\n'
           'int (*submit)(vqa_ctx *, const uint8_t *, const uint8_t *, int, int, int64_t, int64_t, const vqa_plane_desc *, int, int, '
           'int, int) = vqa_itp_submit;\n'
           'int (*wait_)(vqa_ctx *, vqa_itp_metrics *, int) = vqa_itp_wait;\n'
           'int main(void){printf("%zu %zu %zu %zu %zu %zu %d %d %d %d %d %d %d %d\\n", sizeof(vqa_itp_metrics), '
           'offsetof(vqa_itp_metrics, sum_q), offsetof(vqa_itp_metrics, max_q), offsetof(vqa_itp_metrics, de_sum), '
           'offsetof(vqa_itp_metrics, de_mean), offsetof(vqa_itp_metrics, de_max), VQA_K_ITP, VQA_K_VERGE, VQA_K_BRINK, '
           'VQA_ABI_VERSION, VQA_ITP_YUV2020, VQA_ITP_BGR, VQA_ITP_PQ, VQA_ITP_HLG);'
           'return submit == 0 || wait_ == 0;}\n')
    (tmp_path / "s.c").write_text(src)
    lib_dir = os.path.dirname(N.LIB_PATH)
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), "-o", str(tmp_path / "s"), str(tmp_path / "s.c"),
                           "-L", lib_dir, "-l:" + os.path.basename(N.LIB_PATH), "-Wl,-rpath," + lib_dir,
                           "-Wl,--allow-shlib-undefined"])
    assert subprocess.check_output([str(tmp_path / "s")]).decode().split() == ["40", "0", "8", "16", "24", "32", "51", "52", "50",
                                                                              "8", "0", "1", "0", "1"]


# ---- the log and the row ---------------------------------------------------------------------------------------------------
def _records(n):
    from rtvqa_amd.engine import ITP_DTYPE
    rec = np.zeros(n, ITP_DTYPE)
    rec["de_mean"], rec["de_max"] = [0.5, 0.0, 0.25][:n], [4.0, 0.0, 8.5][:n]
    return rec


def _mdsi(n):
    from rtvqa_amd.engine import MDSI_DTYPE
    rec = np.zeros(n, MDSI_DTYPE)
    rec["mdsi"] = [0.125, 0.0, 0.25][:n]
    return rec


def test_the_json_log_and_what_the_row_takes_from_it(tmp_path):
    rec, md = _records(3), _mdsi(3)
    old, log, only = str(tmp_path / "old.json"), str(tmp_path / "vmaf.json"), str(tmp_path / "itp.json")
    vp.write_vif_log(old, mdsi=md)
    vp.write_vif_log(log, mdsi=md, delta_itp=rec)
    doc0, doc = json.load(open(old)), json.load(open(log))
    assert "delta_itp" not in json.dumps(doc0)
    names0 = list(doc0["frames"][0]["metrics"])
    assert names0 == ["mdsi"]
    assert list(doc["frames"][1]["metrics"]) == names0 + ["delta_itp", "delta_itp_max"] == list(doc["pooled_metrics"])
    for i in range(3):
        m = doc["frames"][i]["metrics"]
        assert {k: m[k] for k in names0} == doc0["frames"][i]["metrics"]
        assert m["delta_itp"] == float(rec["de_mean"][i]) and m["delta_itp_max"] == float(rec["de_max"][i])
    assert {k: doc["pooled_metrics"][k] for k in names0} == doc0["pooled_metrics"]
    p = doc["pooled_metrics"]["delta_itp"]
    assert sorted(p) == ["harmonic_mean", "max", "mean", "min"] and p["min"] == 0.0 and p["max"] == 0.5 and p["mean"] == 0.25
    assert doc["pooled_metrics"]["delta_itp_max"]["max"] == 8.5
    vp.write_vif_log(only, delta_itp=rec)
    assert list(json.load(open(only))["frames"][0]["metrics"]) == ["delta_itp", "delta_itp_max"]
    pl, sl = tmp_path / "psnr.log", tmp_path / "ssim.log"
    pl.write_text("n:1 mse_avg:1.00 psnr_avg:48.13 \n")
    sl.write_text("n:1 Y:0.990000 All:0.990000 (20.000000)\n")
    m0 = vp.extract_metrics_from_logs(str(pl), str(sl), old, "x", 23, 1000, "64x64", 30.0)
    m = vp.extract_metrics_from_logs(str(pl), str(sl), log, "x", 23, 1000, "64x64", 30.0)
    assert list(m0)[-1] == "MDSI" and list(m) == list(m0) + ["DELTA_ITP", "DELTA_ITP_MAX"]             # after MDSI, nothing else
    assert {k: m[k] for k in m0} == m0 and m["DELTA_ITP"] == 0.25 and m["DELTA_ITP_MAX"] == 8.5
    base = ["Bitrate (kbps)", "Resolution (px)", "Frame Rate (fps)", "CRF", "PSNR", "SSIM"]
    assert list(vp.extract_metrics_from_logs(str(pl), str(sl), only, "x", 23, 1000, "64x64", 30.0)) == base + ["DELTA_ITP", "DELTA_ITP_MAX"]
    # logs without the key are what they were, byte for byte
    again = str(tmp_path / "again.json")
    vp.write_vif_log(again, mdsi=md, delta_itp=None)
    assert open(again, "rb").read() == open(old, "rb").read()
    # the pass's tuple -> the log: the last element is dE_ITP's [n], MDSI's [n] the one before it
    q = (None, None, md, rec)
    vp._write_feature_log(again, q, dict(vif=False, adm=False, mdsi=True, delta_itp=True))
    assert open(again, "rb").read() == open(log, "rb").read()
    vp._write_feature_log(again, q[:-1], dict(vif=False, adm=False, mdsi=True))
    assert open(again, "rb").read() == open(old, "rb").read()
    vp._write_feature_log(again, (None, None, rec), dict(vif=False, adm=False, delta_itp=True))
    assert open(again, "rb").read() == open(only, "rb").read()


def test_a_model_does_not_read_the_new_keys():
    from rtvqa_amd import vmaf_model

    class Model:
        features = ["vif_scale0", "adm2", "motion2"]

    x = vmaf_model.feature_matrix(Model, {"vif_scale0": [0.5, 0.7], "adm2": [0.9, 0.95], "motion2": [0.0, 1.0],
                                          "delta_itp": [0.1, 0.2], "delta_itp_max": [1.0, 2.0]})
    assert x.shape == (2, 3)


def test_config_keys():
    vp.validate_config(dict(GOOD))
    vp.validate_config(dict(GOOD, delta_itp=True))
    vp.validate_config(dict(GOOD, delta_itp=True, delta_itp_transfer="hlg", delta_itp_range="full"))
    vp.validate_config(dict(GOOD, delta_itp=False, delta_itp_transfer="pq", delta_itp_range="limited", mdsi=True))
    for bad in (1, 0, "true", None, "only"):
        with pytest.raises(ValueError) as e:
            vp.validate_config(dict(GOOD, delta_itp=bad))
        assert str(e.value) == "delta_itp must be true or false."
    for bad in ("PQ", "sdr", 0, None, True):
        with pytest.raises(ValueError) as e:
            vp.validate_config(dict(GOOD, delta_itp=True, delta_itp_transfer=bad))
        assert str(e.value) == 'delta_itp_transfer must be "pq" or "hlg".'
    for bad in ("tv", "Full", 1, None, False):
        with pytest.raises(ValueError) as e:
            vp.validate_config(dict(GOOD, delta_itp=True, delta_itp_range=bad))
        assert str(e.value) == 'delta_itp_range must be "limited" or "full".'


def test_the_stream_request():
    p = [(16, 16, 0, 16, 1), (8, 8, 256, 8, 1), (8, 8, 320, 8, 1)]
    assert stream.Quality(p).itp is False and stream.Quality(p, vif=True, ciede=True, mdsi=True).itp is False
    q = stream.Quality(p, itp=True)
    assert q.itp is True and q.itp_transfer == "pq" and q.itp_full_range is False and q.ssim is True and q.ciede is False
    q = stream.Quality(p, itp="only", itp_transfer="hlg", itp_full_range=True)
    assert q.itp == "only" and q.itp_transfer == "hlg" and q.itp_full_range is True and q.ssim is False
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="itp must be False, True or 'only'"):
            stream.Quality(p, itp=bad)
    for bad in ("sdr", "PQ", 0, None):
        with pytest.raises(ValueError, match="itp_transfer must be 'pq' or 'hlg'"):
            stream.Quality(p, itp=True, itp_transfer=bad)
    for bad in (1, "full", None):
        with pytest.raises(ValueError, match="itp_full_range must be True or False"):
            stream.Quality(p, itp=True, itp_full_range=bad)
    with pytest.raises(ValueError):
        stream.Quality(p, N.SSIM_MS, scales=True, itp="only")
    with pytest.raises(ValueError, match="itp needs three planes"):
        stream.Quality(p[:1], itp=True)
    with pytest.raises(ValueError, match="itp needs three planes"):
        stream.Quality(p[:2], itp=True)
    z = np.zeros((0, 384), np.uint8)
    # an empty clip: without the request the tuples are what they were; with it ONE further last element, after MDSI's
    for kw, length in ((dict(), 2), (dict(vif=True), 3), (dict(mdsi=True), 3), (dict(ciede=True, mdsi=True), 4),
                       (dict(vif=True, adm=True, motion=True, siti=True, psnr_hvs=True, ciede=True, artifacts=True, brisque=True,
                             mdsi=True), 11)):
        q0, _ = stream.run(z, z, quality=stream.Quality(p, **kw))
        q1, _ = stream.run(z, z, quality=stream.Quality(p, itp=True, **kw))
        assert len(q0) == length and len(q1) == length + 1, kw
        assert q1[-1].shape == (0,) and q1[-1].dtype.names == FIELDS
        for a, b in zip(q0, q1):
            assert (a is None and b is None) or (a.dtype == b.dtype and a.shape == b.shape)
    q, _ = stream.run(z, z, quality=stream.Quality(p, itp="only"))
    assert len(q) == 3 and q[0] is None and q[1] is None and q[2].shape == (0,)


def test_the_argument_errors_of_the_entry_points(tmp_path):
    """before anything reaches a device: one-plane layouts, unknown transfers and ranges"""
    from rtvqa_amd.engine import Engine, bgr_planes, yuv_planes
    g = np.zeros((2, 16, 16), np.uint8)
    y = np.zeros((2, 384), np.uint8)
    with pytest.raises(ValueError, match="delta_itp needs three planes"):
        vp.frame_delta_itp(g, g, "gray", 16, 16)
    for bad in ("sdr", "PQ", 0, None):
        with pytest.raises(ValueError, match="delta_itp_transfer must be 'pq' or 'hlg'"):
            vp.frame_delta_itp(y, y, "yuv420p", 16, 16, transfer=bad)
    for bad in ("full", 1, None):
        with pytest.raises(ValueError, match="delta_itp_full_range must be True or False"):
            vp.frame_delta_itp(y, y, "yuv420p", 16, 16, full_range=bad)
    logs = [str(tmp_path / n) for n in ("p.log", "s.log", "v.json")]
    with pytest.raises(ValueError, match="delta_itp needs three planes"):
        vp.run_ffmpeg_metrics(g, g, *logs, layout="gray", delta_itp=True)
    with pytest.raises(ValueError, match="delta_itp_transfer must be 'pq' or 'hlg'"):
        vp.run_ffmpeg_metrics(y, y, *logs, layout="yuv420p", height=16, width=16, delta_itp=True, delta_itp_transfer="sdr")
    with pytest.raises(ValueError, match="delta_itp_full_range must be True or False"):
        vp.run_ffmpeg_metrics(y, y, *logs, layout="yuv420p", height=16, width=16, delta_itp=True, delta_itp_full_range="full")
    # the engine's helpers need no device either
    assert Engine.itp_model(bgr_planes(16, 16)) == N.ITP_BGR and Engine.itp_model(yuv_planes(16, 16, "420", 10)) == N.ITP_YUV2020
    assert Engine.itp_model(yuv_planes(16, 16, "444", 8)) == N.ITP_YUV2020
    assert Engine.itp_transfer("pq") == 0 and Engine.itp_transfer("hlg") == 1 and Engine.itp_transfer(N.ITP_HLG) == 1
    for bad in ("sdr", 2, None, True):
        with pytest.raises(ValueError, match="transfer must be 'pq' or 'hlg'"):
            Engine.itp_transfer(bad)
