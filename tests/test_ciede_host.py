"""CIEDE2000 on the host side (no GPU): the NumPy restatement of tests/ciede_reference.py against Sharma, Wu and Dalal's published
pairs and against scikit-image (tests/golden/ciede_pins.json), the conversions' known answers, the additive ABI
(vqa_ciede_submit, vqa_ciede_wait, vqa_ciede_metrics, VQA_K_CIEDE), the JSON log and the row, the config keys, the stream request,
and which contents enter the GPU parity matrix."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import ciede_cases as CC
import ciede_reference as R
from rtvqa_amd import _native as N
from rtvqa_amd import stream
from rtvqa_amd import video_processing as vp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOOD = {"crf": 23, "vmaf_model_path": None, "resize_width": 64, "resize_height": 64, "frame_interval": 10}
FIELDS = ("de_sum", "de_mean", "ciede2000")
# Sharma, Wu and Dalal 2005, table 1 (a selection): (L, a, b)1, (L, a, b)2 -> dE00 to four decimals
SHARMA = [((50, 2.6772, -79.7751), (50, 0, -82.7485), 2.0425), ((50, 3.1571, -77.2803), (50, 0, -82.7485), 2.8615),
          ((50, 2.8361, -74.0200), (50, 0, -82.7485), 3.4412), ((50, 0, 0), (50, -1, 2), 2.3669),
          ((50, 2.49, -0.001), (50, -2.49, 0.0009), 7.1792), ((50, 2.49, -0.001), (50, -2.49, 0.0011), 7.2195),
          ((50, -0.001, 2.49), (50, 0.0009, -2.49), 4.8045), ((50, 2.5, 0), (50, 0, -2.5), 4.3065),
          ((50, 2.5, 0), (73, 25, -18), 27.1492), ((50, 2.5, 0), (61, -5, 29), 22.8977), ((50, 2.5, 0), (56, -27, -3), 31.9030),
          ((50, 2.5, 0), (58, 24, 15), 19.4535)]


# ---- known answers --------------------------------------------------------------------------------------------------------
def test_the_published_pairs():
    """rows 5 and 6 differ in b2 by 0.0002 and lie on either side of the hue wrap of equations 10 and 14"""
    for p, q, want in SHARMA:
        got = float(R.de00(np.array(p, float), np.array(q, float)))
        assert abs(got - want) <= 5e-5 + 1e-9, (p, q, got, want)
        assert float(R.de00(np.array(q, float), np.array(p, float))) == got          # symmetric, bit for bit
        assert float(R.de00(np.array(p, float), np.array(p, float))) == 0.0
        g32 = float(R.de00(np.array(p, np.float32), np.array(q, np.float32), dtype=np.float32))
        assert abs(g32 - want) <= 2e-3, (p, q, g32)     # (|a| = 2.49 against b = 0.001: the hue itself is an fp32 matter there)


def _pins():
    sys.path.insert(0, os.path.join(REPO, "scripts"))
    import gen_ciede_pins as G
    pins = json.load(open(os.path.join(REPO, "tests", "golden", "ciede_pins.json")))
    a, b = G.make_pairs()
    assert a.tolist() == pins["rgb_a"] and b.tolist() == pins["rgb_b"] and len(a) >= 200
    assert pins["versions"]["skimage"] == "0.18.3" and [tuple(k) for k in pins["weights"]] == [(1.0, 1.0, 1.0), (0.65, 1.0, 4.0)]
    return pins, a.astype(np.int64), b.astype(np.int64)


def test_the_formula_against_scikit_image():
    """skimage's own Lab values through the restatement's dE00: the same formula, both float64"""
    pins, _, _ = _pins()
    la, lb = np.array(pins["lab_a"]), np.array(pins["lab_b"])
    for k, de, gap in zip(pins["weights"], pins["de"], pins["gaps"]):
        got = R.de00(la, lb, tuple(k))
        print("k = %s: formula gap %.2e (stored %.2e)" % (k, np.abs(got - np.array(de)).max(), gap["formula_max_gap"]))
        assert np.abs(got - np.array(de)).max() <= 1e-9


def test_the_chain_against_scikit_image():
    """from the RGB integers: the two differ by colour constants only; the bar is twice what the generator measured"""
    pins, a, b = _pins()
    ours_a, ours_b = R.lab_from_bgr(a[:, 2], a[:, 1], a[:, 0]), R.lab_from_bgr(b[:, 2], b[:, 1], b[:, 0])
    assert np.abs(ours_a - np.array(pins["lab_a"])).max() < 0.05          # the Lab values themselves: a few hundredths
    # a coarse guard on the stored figures, not the bar: with either colour's Lab triple moved by less than 0.05 per channel, every
    # term of dE00 divided by S >= 1 and k >= 0.65, and a' at most 1.5 a, a pair's dE00 moves by less than
    # 2 sqrt(3) 0.05 1.5 / 0.65 = 0.4
    guard = 2 * np.sqrt(3.0) * 0.05 * 1.5 / 0.65
    for k, de, gap in zip(pins["weights"], pins["de"], pins["gaps"]):
        de, got = np.array(de), R.de00(ours_a, ours_b, tuple(k))
        worst, mean = float(np.abs(got - de).max()), float(abs(got.mean() - de.mean()) / de.mean())
        print("k = %s: per pair %.2e (stored %.2e), on the mean %.2e (stored %.2e)" %
              (k, worst, gap["chain_max_gap"], mean, gap["chain_mean_rel_gap"]))
        assert 0 < gap["chain_max_gap"] < guard and 0 < gap["chain_mean_rel_gap"] * de.mean() < guard
        assert worst <= 2 * gap["chain_max_gap"] and mean <= 2 * gap["chain_mean_rel_gap"]


# The float32 run of the conversions has a bar of its own, from the format alone: every f(t) of a white pixel is a value near 1
# that carries the roundings of the curve, three products and two sums, the division by the white point and the cube root - taken
# as at most F32_ULPS = 8 units of 2^-23 - and L, a and b scale f, or a difference of two f, by 116, 500 and 200.
F32_ULPS = 8
F32_BAR_L, F32_BAR_A, F32_BAR_B = (g * F32_ULPS * 2.0 ** -23 for g in (116.0, 2 * 500.0, 2 * 200.0))


def test_conversion_sanity():
    for depth in (8, 10, 12, 16):
        s = 1 << (depth - 8)
        # float64, the text as it stands: YUV (16 s, 128 s, 128 s) -> L = 0, (235 s, 128 s, 128 s) -> L = 100, |a|, |b| < 1e-9
        black = R.lab_from_yuv(16 * s, 128 * s, 128 * s, depth)
        white = R.lab_from_yuv(235 * s, 128 * s, 128 * s, depth)
        assert abs(black[0]) < 1e-9 and np.abs(black[1:]).max() < 1e-9, (depth, black)
        assert abs(white[0] - 100) < 1e-9 and np.abs(white[1:]).max() < 1e-9, (depth, white)
        # the float32 run of the same text, at the float32 bar
        black = R.lab_from_yuv(16 * s, 128 * s, 128 * s, depth, np.float32)
        white = R.lab_from_yuv(235 * s, 128 * s, 128 * s, depth, np.float32)
        assert black.dtype == white.dtype == np.float32
        assert abs(black[0]) <= F32_BAR_L and abs(black[1]) <= F32_BAR_A and abs(black[2]) <= F32_BAR_B, (depth, black)
        assert abs(white[0] - 100) <= F32_BAR_L and abs(white[1]) <= F32_BAR_A and abs(white[2]) <= F32_BAR_B, (depth, white)
        L = (1 << depth) - 1
        w = R.lab_from_bgr(L, L, L, depth)
        assert abs(w[0] - 100) < 1e-9 and np.abs(w[1:]).max() < 1e-9
        k = R.lab_from_bgr(0, 0, 0, depth)
        assert np.abs(k).max() < 1e-9
        g = R.lab_from_yuv(126 * s, 128 * s, 128 * s, depth)                      # a gray pixel: a = b = 0 up to rounding
        assert 0 < g[0] < 100 and np.abs(g[1:]).max() < 1e-9
    red = R.lab_from_bgr(0, 0, 255)
    assert abs(red[0] - 53.24) < 0.05 and red[1] > 75 and red[2] > 60            # sRGB red: L 53.2, a 80.1, b 67.2
    # out of gamut, unclamped: finite and smooth
    rng = np.random.default_rng(1)
    yuv = rng.integers(0, 256, (3, 4096))
    for dt in (np.float64, np.float32):
        lab = R.lab_from_yuv(*yuv, 8, dt)
        assert np.isfinite(lab).all()
        assert np.isfinite(R.de00(lab[:-1], lab[1:], dtype=dt)).all()


def test_replication_and_the_frame_mean():
    r, d, planes = CC.case((17, 23), 8, "yuv420p", "noise4")
    fr, fd = R.split_planes(r, planes), R.split_planes(d, planes)
    assert [p.shape for p in fr[0]] == [(17, 23), (9, 12), (9, 12)]
    u = R.replicate(fr[0][1], 17, 23)
    assert u.shape == (17, 23) and u[16, 22] == fr[0][1][8, 11] and u[3, 5] == fr[0][1][1, 2]
    with pytest.raises(ValueError):
        R.replicate(fr[0][1][:, :11], 17, 23)
    de = R.frame(fr[0], fd[0])
    assert de.shape == (17, 23) and (R.frame(fr[0], fr[0]) == 0).all() and R.de_mean(fr[0], fr[0]) == 0.0
    assert R.score(0.0) == float("inf") and abs(R.score(1.0) - 45.0) < 1e-15 and abs(R.score(10.0) - 25.0) < 1e-13
    assert R.de_mean(fr[0], fd[0]) == R.de_mean(fd[0], fr[0])
    assert (R.frame(fr[0], fd[0], dtype=np.float32) == R.frame(fd[0], fr[0], dtype=np.float32)).all()
    with pytest.raises(ValueError):
        R.frame([p[:15] for p in fr[0]], [p[:15] for p in fd[0]])
    # the quantum bound: the integer sum of the rounded values against the plain mean
    assert R.quantum_bar() == 2.0 ** -21
    assert abs(R.de_mean_fixed(fr[0], fd[0]) - R.de_mean(fr[0], fd[0])) <= R.quantum_bar() + 1e-15


# ---- admission of the GPU parity matrix ------------------------------------------------------------------------------------
def test_every_content_of_the_gpu_matrix_is_admitted():
    """the restatement in float32 stays within 1e-5 relative of float64 on de_mean, on every content the GPU tests compare,
    at both weight sets: the list is fixed in ciede_cases - the matrix and the further contents (the gray clips with a luma
    offset, the windows of resident frames) - and all of it must pass"""
    assert CC.ADMIT == 1e-5 and CC.GPU_BAR == 1e-4 and len(CC.matrix()) == 2 * len(CC.GRID) == 16
    contents = []
    for (geom, depth, layout, dis) in CC.matrix():
        contents.append(("%dx%d %s %s" % (geom[0], geom[1], layout, dis),) + CC.case(geom, depth, layout, dis) +
                        (depth, CC.model_of(layout)))
    extras = CC.extras()
    assert len(extras) == len(CC.GRAY) + len(CC.ROIS) == 6
    contents += [e + (R.YUV709,) for e in extras]
    worst = 0.0
    for (tag, r, d, planes, depth, model) in contents:
        fr, fd = R.split_planes(r, planes), R.split_planes(d, planes)
        assert len(fr) >= CC.N_FRAMES
        for k in CC.WEIGHTS:
            for i in range(len(fr)):
                a = R.de_mean(fr[i], fd[i], depth, model, k)
                b = R.de_mean(fr[i], fd[i], depth, model, k, np.float32)
                assert np.isfinite(b) and a > 0.5, (tag, k, i, a)
                gap = abs(b - a) / a
                worst = max(worst, gap)
                assert gap <= CC.ADMIT, (tag, k, i, gap)
    print("float32 against float64 on de_mean: at most %.2e" % worst)


# ---- ABI -------------------------------------------------------------------------------------------------------------------
def test_the_additive_abi():
    assert N.VQA_ABI_VERSION == 8
    assert C.sizeof(N.VqaCiedeMetrics) == 24
    assert [getattr(N.VqaCiedeMetrics, f).offset for f in FIELDS] == [0, 8, 16]
    from rtvqa_amd.engine import CIEDE_DTYPE
    assert CIEDE_DTYPE.itemsize == 24 and CIEDE_DTYPE.names == FIELDS
    assert (N.K_CIEDE, N.K_BEYOND, N.K_PAST, N.K_PSNR_HVS) == (25, 26, 24, 23)
    assert N.K_IDS_NAMED == N.K_IDS_EVERY + (25,) and 24 not in N.K_IDS_NAMED
    assert N.CIEDE_MIN_DIM == R.MIN_DIM == 16 and (N.CIEDE_YUV709, N.CIEDE_BGR) == (R.YUV709, R.BGR) == (0, 1)
    assert N.CIEDE_WEIGHTS_CIE == (1.0, 1.0, 1.0) and N.CIEDE_WEIGHTS_LIBVMAF == (0.65, 1.0, 4.0)
    txt = open(os.path.join(REPO, "include", "vqa.h")).read()
    assert re.search(r"VQA_K_CIEDE\s*=\s*25", txt) and re.search(r"VQA_K_BEYOND\s*=\s*26", txt) and re.search(r"VQA_K_PAST\s*=\s*24", txt)
    assert re.search(r"VQA_CIEDE_YUV709\s*=\s*0", txt) and re.search(r"VQA_CIEDE_BGR\s*=\s*1", txt)
    part = txt[txt.index("CIEDE2000 (CIE 142-2001"):]
    assert "this text is\n * what is built" in part or "this text is what is built" in part
    for word in ("S_L =", "S_C =", "S_H =", "R_T =", "R_C =", "dtheta =", "T = 1", "G = 0.5", "SATURATED AT 2^12"):
        assert word in part, word
    lib = N.load()
    assert hasattr(lib, "vqa_ciede_submit") and hasattr(lib, "vqa_ciede_wait")     # both symbols are exported
    lib.vqa_kernel_name.restype = C.c_char_p
    assert lib.vqa_kernel_name(N.K_CIEDE) == b"k_ciede"
    assert lib.vqa_kernel_name(N.K_PAST) == b"?" and lib.vqa_kernel_name(N.K_BEYOND) == b"?"
    assert lib.vqa_kernel_name(N.K_PSNR_HVS) == b"k_psnr_hvs"
    # argument checks that need no device
    assert lib.vqa_ciede_submit(None, None, None, 0, 0, 0, 0, None, 0, 0, None) == N.VQA_ERR_INVALID
    assert lib.vqa_ciede_wait(None, None, 0) == N.VQA_ERR_INVALID
    assert lib.vqa_profile_read(None, N.K_CIEDE, None, None, 0) == N.VQA_ERR_INVALID


def test_the_header_struct_is_24_bytes_to_the_c_compiler(tmp_path):
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "vqa.h"\n'
           'int (*submit)(vqa_ctx *, const uint8_t *, const uint8_t *, int, int, int64_t, int64_t, const vqa_plane_desc *, int, int, '
           'const double *) = vqa_ciede_submit;\n'
           'int (*wait_)(vqa_ctx *, vqa_ciede_metrics *, int) = vqa_ciede_wait;\n'
           'int main(void){printf("%zu %zu %zu %zu %d %d %d %d %d\\n", sizeof(vqa_ciede_metrics), '
           'offsetof(vqa_ciede_metrics, de_sum), offsetof(vqa_ciede_metrics, de_mean), offsetof(vqa_ciede_metrics, ciede2000), '
           'VQA_K_CIEDE, VQA_K_BEYOND, VQA_K_PAST, VQA_CIEDE_BGR, VQA_ABI_VERSION);'
           'return submit == 0 || wait_ == 0;}\n')
    (tmp_path / "s.c").write_text(src)
    lib_dir = os.path.dirname(N.LIB_PATH)
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), "-o", str(tmp_path / "s"), str(tmp_path / "s.c"),
                           "-L", lib_dir, "-l:" + os.path.basename(N.LIB_PATH), "-Wl,-rpath," + lib_dir,
                           "-Wl,--allow-shlib-undefined"])
    assert subprocess.check_output([str(tmp_path / "s")]).decode().split() == ["24", "0", "8", "16", "25", "26", "24", "1", "8"]


# ---- the log and the row ---------------------------------------------------------------------------------------------------
def _records(n):
    from rtvqa_amd.engine import CIEDE_DTYPE
    rec = np.zeros(n, CIEDE_DTYPE)
    rec["ciede2000"] = [38.75, np.inf, 120.0][:n]
    return rec


def _hvs(n):
    from rtvqa_amd.engine import PSNR_HVS_DTYPE
    rec = np.zeros(n, PSNR_HVS_DTYPE)
    rec["psnr_hvs"], rec["psnr_hvsm"] = [41.25, np.inf, 38.5][:n], [47.0, np.inf, 120.0][:n]
    return rec


def _siti(n):
    from rtvqa_amd.engine import SITI_DTYPE
    rec = np.zeros(n, SITI_DTYPE)
    rec["si"], rec["ti"] = [30.0, 40.0, 35.0][:n], [0.0, 4.0, 2.0][:n]
    return rec


def test_the_json_log_and_what_the_row_takes_from_it(tmp_path):
    from rtvqa_amd.engine import ADM_DTYPE
    vif = np.array([[0.5, 0.9, 0.95, 0.99], [0.7, 0.8, 0.97, 1.01], [0.6, 0.85, 0.96, 1.0]])
    adm = np.zeros(3, ADM_DTYPE)
    adm["adm2"], adm["scale"] = [0.9, 0.95, 0.85], 0.9
    mot = np.zeros(3, stream.MOTION_PASS_DTYPE)
    mot["motion"], mot["motion2"] = [0.0, 2.0, 1.0], [0.0, 1.0, 1.0]
    rec, hv, st = _records(3), _hvs(3), _siti(3)
    old, log, only = str(tmp_path / "old.json"), str(tmp_path / "vmaf.json"), str(tmp_path / "cie.json")
    vp.write_vif_log(old, vif, adm, motion=mot, siti=st, psnr_hvs=hv)
    vp.write_vif_log(log, vif, adm, motion=mot, siti=st, psnr_hvs=hv, ciede=rec)
    raw = open(log).read()
    assert "Infinity" not in raw and "NaN" not in raw
    doc0, doc = json.load(open(old)), json.loads(raw)
    assert "ciede2000" not in json.dumps(doc0)
    names0 = list(doc0["frames"][0]["metrics"])
    assert names0[-2:] == ["psnr_hvs", "psnr_hvsm"]
    assert list(doc["frames"][1]["metrics"]) == names0 + ["ciede2000"] == list(doc["pooled_metrics"])
    capped = [38.75, 100.0, 100.0]                                          # min(value, 100.0)
    for i in range(3):
        m = doc["frames"][i]["metrics"]
        assert {k: m[k] for k in names0} == doc0["frames"][i]["metrics"] and m["ciede2000"] == capped[i]
    assert {k: doc["pooled_metrics"][k] for k in names0} == doc0["pooled_metrics"]
    p = doc["pooled_metrics"]["ciede2000"]
    assert sorted(p) == ["harmonic_mean", "max", "mean", "min"]
    assert p["min"] == 38.75 and p["max"] == 100.0 and abs(p["mean"] - np.mean(capped)) <= 1e-13
    vp.write_vif_log(only, ciede=rec)
    assert list(json.load(open(only))["frames"][0]["metrics"]) == ["ciede2000"]
    pl, sl = tmp_path / "psnr.log", tmp_path / "ssim.log"
    pl.write_text("n:1 mse_avg:1.00 psnr_avg:48.13 \n")
    sl.write_text("n:1 Y:0.990000 All:0.990000 (20.000000)\n")
    m0 = vp.extract_metrics_from_logs(str(pl), str(sl), old, "x", 23, 1000, "64x64", 30.0)
    m = vp.extract_metrics_from_logs(str(pl), str(sl), log, "x", 23, 1000, "64x64", 30.0)
    assert list(m0)[-2:] == ["PSNR_HVS", "PSNR_HVSM"] and list(m) == list(m0) + ["CIEDE2000"]
    assert {k: m[k] for k in m0} == m0 and abs(m["CIEDE2000"] - np.mean(capped)) <= 1e-13
    base = ["Bitrate (kbps)", "Resolution (px)", "Frame Rate (fps)", "CRF", "PSNR", "SSIM"]
    assert list(vp.extract_metrics_from_logs(str(pl), str(sl), only, "x", 23, 1000, "64x64", 30.0)) == base + ["CIEDE2000"]
    # logs without the key are what they were, byte for byte
    again = str(tmp_path / "again.json")
    vp.write_vif_log(again, vif, adm, motion=mot, siti=st, psnr_hvs=hv, ciede=None)
    assert open(again, "rb").read() == open(old, "rb").read()
    # the pass's tuple -> the log: the last element is CIEDE2000's [n], PSNR-HVS's the one before it
    from rtvqa_amd.engine import VIF_DTYPE
    v = np.zeros((3, 1), VIF_DTYPE)
    v["scale"][:, 0, :] = vif
    q = (None, None, v, adm[:, None], mot[:, None], st[:, None], hv[:, None], rec)
    vp._write_feature_log(again, q, dict(vif=True, adm=True, motion=True, siti=True, psnr_hvs=True, ciede=True))
    assert open(again, "rb").read() == open(log, "rb").read()
    vp._write_feature_log(again, q[:-1], dict(vif=True, adm=True, motion=True, siti=True, psnr_hvs=True))
    assert open(again, "rb").read() == open(old, "rb").read()
    vp._write_feature_log(again, (None, None, rec), dict(vif=False, adm=False, motion=False, siti=False, psnr_hvs=False, ciede=True))
    assert open(again, "rb").read() == open(only, "rb").read()


def test_a_model_does_not_read_the_new_key():
    from rtvqa_amd import vmaf_model

    class Model:
        features = ["vif_scale0", "adm2", "motion2"]

    x = vmaf_model.feature_matrix(Model, {"vif_scale0": [0.5, 0.7], "adm2": [0.9, 0.95], "motion2": [0.0, 1.0], "ciede2000": [1.0, 2.0]})
    assert x.shape == (2, 3)


def test_config_keys():
    vp.validate_config(dict(GOOD))
    vp.validate_config(dict(GOOD, ciede=True))
    vp.validate_config(dict(GOOD, ciede=False, psnr_hvs=True, vif=True))
    vp.validate_config(dict(GOOD, ciede=True, ciede_weights=[0.65, 1, 4]))
    for bad in (1, 0, "true", None, "only"):
        with pytest.raises(ValueError) as e:
            vp.validate_config(dict(GOOD, ciede=bad))
        assert str(e.value) == "ciede must be true or false."
    for bad in ([1, 1], [1, 1, 0], [1, 1, -2], [1, 1, float("nan")], [1, 1, float("inf")], "111", [True, 1, 1], None):
        with pytest.raises(ValueError) as e:
            vp.validate_config(dict(GOOD, ciede=True, ciede_weights=bad))
        assert str(e.value) == "ciede_weights must be three positive numbers [kL, kC, kH]."


def test_one_plane_layouts_are_refused(tmp_path):
    z = np.zeros((2, 32, 32), np.uint8)
    for layout in ("gray", "gray10le"):
        with pytest.raises(ValueError) as e:
            vp.frame_ciede(z, z, layout, 32, 32)
        assert str(e.value) == "ciede needs three planes"
    with pytest.raises(ValueError) as e:
        vp.run_ffmpeg_metrics(z, z, str(tmp_path / "p"), str(tmp_path / "s"), str(tmp_path / "v"), layout="gray", ciede=True)
    assert str(e.value) == "ciede needs three planes"
    with pytest.raises(ValueError) as e:
        stream.Quality([(32, 32, 0, 32, 1)], ciede=True)
    assert str(e.value) == "ciede needs three planes"


def test_the_engine_counts_the_weights_before_it_converts_them():
    """two or four weights are the documented ValueError, raised before anything is built from them or reaches the library"""
    from rtvqa_amd.engine import Engine
    eng = object.__new__(Engine)                  # no context: the check comes first
    p = [(16, 16, 0, 16, 1), (8, 8, 256, 8, 1), (8, 8, 320, 8, 1)]
    z = np.zeros((1, 384), np.uint8)
    for bad in ((1.0, 1.0), (1.0, 1.0, 1.0, 1.0), ()):
        with pytest.raises(ValueError) as e:
            eng.ciede_submit(z, z, p, weights=bad)
        assert str(e.value) == "weights must be (kL, kC, kH)"
        with pytest.raises(ValueError):
            eng.ciede(z, z, p, weights=bad)


def test_the_stream_request():
    p = [(16, 16, 0, 16, 1), (8, 8, 256, 8, 1), (8, 8, 320, 8, 1)]
    assert stream.Quality(p).ciede is False and stream.Quality(p, vif=True, adm=True, motion=True, siti=True, psnr_hvs=True).ciede is False
    assert stream.Quality(p, ciede=True).ciede is True and stream.Quality(p, ciede="only").ciede == "only"
    assert stream.Quality(p, ciede=True).ssim is True and stream.Quality(p, ciede="only").ssim is False
    assert stream.Quality(p, ciede=True).psnr_hvs is False and stream.Quality(p, ciede=True).ciede_weights == (1.0, 1.0, 1.0)
    assert stream.Quality(p, ciede=True, ciede_weights=[0.65, 1, 4]).ciede_weights == (0.65, 1.0, 4.0)
    for bad in (1, "yes", None):
        with pytest.raises(ValueError):
            stream.Quality(p, ciede=bad)
    for bad in ((1, 1), (0, 1, 1), (1, 1, float("nan"))):
        with pytest.raises(ValueError):
            stream.Quality(p, ciede=True, ciede_weights=bad)
    with pytest.raises(ValueError):
        stream.Quality(p, N.SSIM_MS, scales=True, ciede="only")
    z = np.zeros((0, 384), np.uint8)
    # an empty clip: without the request the tuples are what they were; with it ONE further last element, after PSNR-HVS's
    for kw, length in ((dict(), 2), (dict(vif=True), 3), (dict(psnr_hvs=True), 3), (dict(siti=True, psnr_hvs=True), 4),
                       (dict(vif=True, adm=True, motion=True, siti=True, psnr_hvs=True), 7)):
        q0, _ = stream.run(z, z, quality=stream.Quality(p, **kw))
        q1, _ = stream.run(z, z, quality=stream.Quality(p, ciede=True, **kw))
        assert len(q0) == length and len(q1) == length + 1, kw
        assert q1[-1].shape == (0,) and q1[-1].dtype.names == FIELDS
        for a, b in zip(q0, q1):
            assert (a is None and b is None) or (a.dtype == b.dtype and a.shape == b.shape)
    q, _ = stream.run(z, z, quality=stream.Quality(p, ciede="only"))
    assert len(q) == 3 and q[0] is None and q[1] is None and q[2].shape == (0,)
