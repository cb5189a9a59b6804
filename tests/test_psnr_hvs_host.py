"""PSNR-HVS and PSNR-HVS-M on the host side (no GPU): the NumPy restatement of tests/psnr_hvs_reference.py against known answers,
the additive ABI (vqa_psnr_hvs_submit, vqa_psnr_hvs_wait, vqa_psnr_hvs_metrics, VQA_K_PSNR_HVS), the JSON log and the row, the
config key, the stream request, and which contents enter the GPU parity matrix."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import psnr_hvs_cases as PC
import psnr_hvs_reference as R
from rtvqa_amd import _native as N
from rtvqa_amd import stream
from rtvqa_amd import video_processing as vp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOOD = {"crf": 23, "vmaf_model_path": None, "resize_width": 64, "resize_height": 64, "frame_interval": 10}
FIELDS = ("s_hvs", "s_hvsm", "psnr_hvs", "psnr_hvsm")


# ---- known answers --------------------------------------------------------------------------------------------------------
def test_the_tables_come_from_the_formulas():
    c, csf, msk = R.tables()
    assert np.abs(c @ c.T - np.eye(8)).max() < 1e-15                      # orthonormal
    assert abs(c[0, 0] - np.sqrt(1 / 8)) < 1e-16 and abs(c[1, 0] - 0.5 * np.cos(np.pi / 16)) < 1e-16
    assert [round(float(v), 6) for v in csf[0, :3]] == [1.608443, 2.339553, 2.573509]
    assert [round(float(v), 6) for v in msk[1, :3]] == [0.694444, 0.694444, 0.510204]
    assert R.Q.shape == (8, 8) and R.Q[0, 0] == 16 and R.Q[7, 7] == 99
    assert (csf == 25.735088 / R.Q).all() and (msk == (10.0 / R.Q) ** 2).all()
    c32, csf32, msk32 = R.tables(np.float32)
    assert c32.dtype == np.float32 and (csf32 == csf.astype(np.float32)).all() and (msk32 == msk.astype(np.float32)).all()
    assert abs(float(csf[0, 0]) ** 2 - 2.58709) < 5e-6


def test_identical_planes_give_exactly_zero_and_infinity():
    for depth in (8, 10, 16):
        a, _ = PC.pair("natural", 24, 40, depth)
        for dt in (np.float64, np.float32):
            assert R.psnr_hvs(a, a, depth, dt) == (0.0, 0.0, float("inf"), float("inf"))


def test_a_constant_offset_is_seen_by_the_dc_term_alone():
    """dist = ref + c, no clipping: A - B is 8 c at (0,0) and nothing else; the DC term is never masked"""
    for depth, c in ((8, 3), (8, -7), (10, 5), (16, 3), (16, 100)):
        a, _ = PC.pair("natural", 24, 40, depth)
        a = np.clip(a, 200, (1 << depth) - 201)
        want = c * c * (25.735088 / 16.0) ** 2
        assert abs(want - c * c * 2.58709) <= 2e-6 * want
        for dt, tol in ((np.float64, 1e-12), (np.float32, 1e-6)):
            s, sm, p, pm = R.psnr_hvs(a, a + c, depth, dt)
            assert abs(s - want) <= tol * want and abs(sm - want) <= tol * want, (depth, c, dt)
            assert abs(p - 10 * np.log10(((1 << depth) - 1) ** 2 / want)) < 1e-5


def test_masking_only_ever_takes_away():
    for name, depth in PC.matrix():
        r, d = PC.pair(name, 32, 48, depth)
        for dt in (np.float64, np.float32):
            hvs, hvsm = R.block_sums(r, d, dt)
            assert (hvsm <= hvs).all() and (hvsm >= 0).all(), (name, depth)


def test_rows_and_columns_beyond_the_last_whole_block_are_not_looked_at():
    r, d = PC.pair("natural", 17, 23, 8)
    assert R.psnr_hvs(r, d) == R.psnr_hvs(r[:16, :16], d[:16, :16])
    r2, d2 = r.copy(), d.copy()
    r2[16:, :], r2[:, 16:], d2[16:, :], d2[:, 16:] = 0, 255, 255, 0
    assert R.psnr_hvs(r2, d2) == R.psnr_hvs(r, d)
    with pytest.raises(ValueError):
        R.psnr_hvs(r[:15], d[:15])


def test_the_pair_is_symmetric_and_the_stronger_mask_wins():
    """m = max(m(a), m(b)): a flat block (vari = 0: pop = 0, m = 0) against an impulse is masked by the impulse's own energy"""
    a = np.full((16, 16), 100)
    b = a.copy()
    b[3, 5] += 9
    s, sm, _, _ = R.psnr_hvs(a, b)
    assert 0 < sm < s and R.psnr_hvs(b, a) == (s, sm) + R.psnr_hvs(a, b)[2:]
    r, d = PC.pair("natural", 24, 40, 10)
    for dt in (np.float64, np.float32):
        assert R.psnr_hvs(r, d, 10, dt) == R.psnr_hvs(d, r, 10, dt)


def test_the_quantum_bound():
    assert R.quantum_bar() == 2.0 ** -27
    r, d = PC.pair("natural", 40, 136, 8)
    s, sm, _, _ = R.psnr_hvs(r, d)
    fs, fsm = R.psnr_hvs_fixed(r, d)
    assert abs(fs - s) <= R.quantum_bar() + 1e-15 * s and abs(fsm - sm) <= R.quantum_bar() + 1e-15 * s


# ---- admission of the GPU parity matrix ------------------------------------------------------------------------------------
def test_which_contents_enter_the_gpu_matrix():
    """a (content, depth) enters only if the reference's own float32 run is within 5e-5 relative of float64 on both S - half the
    GPU bar; what fails must be named in psnr_hvs_cases.EXCLUDED, and at most one in ten may be"""
    every = [(n, d) for d in PC.DEPTHS for n in PC.CONTENTS]
    assert len(PC.EXCLUDED) <= PC.MAX_EXCLUDED_SHARE * len(every) and set(PC.EXCLUDED) <= set(every)
    assert PC.ADMIT == 5e-5 == PC.GPU_BAR / 2
    worst = 0.0
    for n, d in every:
        r, dd = PC.pair(n, PC.SHAPE[0], PC.SHAPE[1], d)
        a, b = R.psnr_hvs(r, dd, d), R.psnr_hvs(r, dd, d, np.float32)
        gap = max(abs(b[i] - a[i]) / a[i] for i in (0, 1))
        print("%-15s %2d bits: float32 against float64 %.2e" % (n, d, gap))
        stable = gap <= PC.ADMIT
        assert stable != ((n, d) in PC.EXCLUDED), (n, d, gap)
        worst = max(worst, gap if stable else 0.0)
    assert worst < 1e-5      # (natural texture and uniform noise pass with a wide margin)


# ---- ABI -------------------------------------------------------------------------------------------------------------------
def test_the_additive_abi():
    assert N.VQA_ABI_VERSION == 8
    assert C.sizeof(N.VqaPsnrHvsMetrics) == 32
    assert [getattr(N.VqaPsnrHvsMetrics, f).offset for f in FIELDS] == [0, 8, 16, 24]
    from rtvqa_amd.engine import PSNR_HVS_DTYPE
    assert PSNR_HVS_DTYPE.itemsize == 32 and PSNR_HVS_DTYPE.names == FIELDS
    assert (N.K_PSNR_HVS, N.K_PAST, N.K_LAST, N.K_SITI) == (23, 24, 22, 21)
    assert N.K_IDS_EVERY == tuple(range(14)) + (16, 17, 19, 21, 23) and N.K_IDS_KNOWN == N.K_IDS_EVERY[:-1]
    assert N.PSNR_HVS_MIN_DIM == R.MIN_DIM == 16
    txt = open(os.path.join(REPO, "include", "vqa.h")).read()
    assert re.search(r"VQA_K_PSNR_HVS\s*=\s*23", txt) and re.search(r"VQA_K_PAST\s*=\s*24", txt) and re.search(r"VQA_K_LAST\s*=\s*22", txt)
    assert re.search(r"#define VQA_ABI_VERSION\s+8", txt)
    assert "this text is what is built" in txt[txt.index("PSNR-HVS (Egiazarian"):]
    lib = N.load()
    assert "vqa_psnr_hvs_submit" in N.SIGNATURES and "vqa_psnr_hvs_wait" in N.SIGNATURES
    assert hasattr(lib, "vqa_psnr_hvs_submit") and hasattr(lib, "vqa_psnr_hvs_wait")     # both symbols are exported
    lib.vqa_kernel_name.restype = C.c_char_p
    assert lib.vqa_kernel_name(N.K_PSNR_HVS) == b"k_psnr_hvs"
    assert lib.vqa_kernel_name(N.K_LAST) == b"?" and lib.vqa_kernel_name(N.K_PAST) == b"?"
    assert lib.vqa_kernel_name(N.K_SITI) == b"k_siti"
    assert lib.vqa_abi_version() == 8
    # argument checks that need no device
    assert lib.vqa_psnr_hvs_submit(None, None, None, 0, 0, 0, 0, None, 0) == N.VQA_ERR_INVALID
    assert lib.vqa_psnr_hvs_wait(None, None, 0) == N.VQA_ERR_INVALID
    assert lib.vqa_profile_read(None, N.K_PSNR_HVS, None, None, 0) == N.VQA_ERR_INVALID


def test_the_header_struct_is_32_bytes_to_the_c_compiler(tmp_path):
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "vqa.h"\n'
           'int (*submit)(vqa_ctx *, const uint8_t *, const uint8_t *, int, int, int64_t, int64_t, const vqa_plane_desc *, int) = '
           'vqa_psnr_hvs_submit;\n'
           'int (*wait_)(vqa_ctx *, vqa_psnr_hvs_metrics *, int) = vqa_psnr_hvs_wait;\n'
           'int main(void){printf("%zu %zu %zu %zu %zu %d %d %d %d\\n", sizeof(vqa_psnr_hvs_metrics), '
           'offsetof(vqa_psnr_hvs_metrics, s_hvs), offsetof(vqa_psnr_hvs_metrics, s_hvsm), offsetof(vqa_psnr_hvs_metrics, psnr_hvs), '
           'offsetof(vqa_psnr_hvs_metrics, psnr_hvsm), VQA_K_PSNR_HVS, VQA_K_PAST, VQA_K_LAST, VQA_ABI_VERSION);'
           'return submit == 0 || wait_ == 0;}\n')
    (tmp_path / "s.c").write_text(src)
    lib_dir = os.path.dirname(N.LIB_PATH)
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), "-o", str(tmp_path / "s"), str(tmp_path / "s.c"),
                           "-L", lib_dir, "-l:" + os.path.basename(N.LIB_PATH), "-Wl,-rpath," + lib_dir,
                           "-Wl,--allow-shlib-undefined"])
    assert subprocess.check_output([str(tmp_path / "s")]).decode().split() == ["32", "0", "8", "16", "24", "23", "24", "22", "8"]


# ---- the log and the row ---------------------------------------------------------------------------------------------------
def _records(n):
    from rtvqa_amd.engine import PSNR_HVS_DTYPE
    rec = np.zeros(n, PSNR_HVS_DTYPE)
    rec["psnr_hvs"] = [41.25, np.inf, 38.5][:n]
    rec["psnr_hvsm"] = [47.0, np.inf, 120.0][:n]
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
    rec, st = _records(3), _siti(3)
    old, log, only = str(tmp_path / "old.json"), str(tmp_path / "vmaf.json"), str(tmp_path / "hvs.json")
    vp.write_vif_log(old, vif, adm, motion=mot, siti=st)
    vp.write_vif_log(log, vif, adm, motion=mot, siti=st, psnr_hvs=rec)
    raw = open(log).read()
    assert "Infinity" not in raw and "NaN" not in raw
    doc0, doc = json.load(open(old)), json.loads(raw)
    assert "psnr_hvs" not in json.dumps(doc0)
    names0 = list(doc0["frames"][0]["metrics"])
    assert names0[-2:] == ["si", "ti"]
    assert list(doc["frames"][1]["metrics"]) == names0 + ["psnr_hvs", "psnr_hvsm"] == list(doc["pooled_metrics"])
    capped = {"psnr_hvs": [41.25, 100.0, 38.5], "psnr_hvsm": [47.0, 100.0, 100.0]}          # min(value, 100.0) dB
    assert vp.PSNR_HVS_DB_CAP == 100.0
    for i in range(3):
        m = doc["frames"][i]["metrics"]
        assert {k: m[k] for k in names0} == doc0["frames"][i]["metrics"]
        assert m["psnr_hvs"] == capped["psnr_hvs"][i] and m["psnr_hvsm"] == capped["psnr_hvsm"][i]
    assert {k: doc["pooled_metrics"][k] for k in names0} == doc0["pooled_metrics"]
    for k in ("psnr_hvs", "psnr_hvsm"):
        p, x = doc["pooled_metrics"][k], np.array(capped[k])
        assert sorted(p) == ["harmonic_mean", "max", "mean", "min"]
        assert p["min"] == x.min() and p["max"] == x.max() and abs(p["mean"] - x.mean()) <= 1e-13
    vp.write_vif_log(only, psnr_hvs=rec)
    assert list(json.load(open(only))["frames"][0]["metrics"]) == ["psnr_hvs", "psnr_hvsm"]
    pl, sl = tmp_path / "psnr.log", tmp_path / "ssim.log"
    pl.write_text("n:1 mse_avg:1.00 psnr_avg:48.13 \n")
    sl.write_text("n:1 Y:0.990000 All:0.990000 (20.000000)\n")
    base = ["Bitrate (kbps)", "Resolution (px)", "Frame Rate (fps)", "CRF", "PSNR", "SSIM"]
    feats = ["VIF_scale0", "VIF_scale1", "VIF_scale2", "VIF_scale3", "ADM2", "ADM_scale0", "ADM_scale1", "ADM_scale2", "ADM_scale3",
             "MOTION2", "MOTION", "SI", "TI"]
    m = vp.extract_metrics_from_logs(str(pl), str(sl), log, "x", 23, 1000, "64x64", 30.0)
    assert list(m) == base + feats + ["PSNR_HVS", "PSNR_HVSM"]
    assert abs(m["PSNR_HVS"] - np.mean(capped["psnr_hvs"])) <= 1e-13 and abs(m["PSNR_HVSM"] - np.mean(capped["psnr_hvsm"])) <= 1e-13
    assert list(vp.extract_metrics_from_logs(str(pl), str(sl), only, "x", 23, 1000, "64x64", 30.0)) == base + ["PSNR_HVS", "PSNR_HVSM"]
    # rows and logs without the key are what they were, byte for byte
    m0 = vp.extract_metrics_from_logs(str(pl), str(sl), old, "x", 23, 1000, "64x64", 30.0)
    assert list(m0) == base + feats and {k: m[k] for k in m0} == m0
    again = str(tmp_path / "again.json")
    vp.write_vif_log(again, vif, adm, motion=mot, siti=st, psnr_hvs=None)
    assert open(again, "rb").read() == open(old, "rb").read()
    # the pass's tuple -> the log: the last element is PSNR-HVS's, SI/TI's the one before it
    from rtvqa_amd.engine import VIF_DTYPE
    v = np.zeros((3, 1), VIF_DTYPE)
    v["scale"][:, 0, :] = vif
    q = (None, None, v, adm[:, None], mot[:, None], st[:, None], rec[:, None])
    vp._write_feature_log(again, q, dict(vif=True, adm=True, motion=True, siti=True, psnr_hvs=True))
    assert open(again, "rb").read() == open(log, "rb").read()
    vp._write_feature_log(again, q[:-1], dict(vif=True, adm=True, motion=True, siti=True))
    assert open(again, "rb").read() == open(old, "rb").read()


def test_a_model_does_not_read_the_new_keys(tmp_path):
    from rtvqa_amd import vmaf_model
    from rtvqa_amd.engine import ADM_DTYPE

    class Model:
        features = ["vif_scale0", "adm2", "motion2"]

    vif = np.array([[0.5, 0.9, 0.95, 0.99], [0.7, 0.8, 0.97, 1.01]])
    adm = np.zeros(2, ADM_DTYPE)
    adm["adm2"] = [0.9, 0.95]
    mot = np.zeros(2, stream.MOTION_PASS_DTYPE)
    x = vmaf_model.feature_matrix(Model, {"vif_scale0": vif[:, 0], "adm2": adm["adm2"], "motion2": mot["motion2"], "psnr_hvs": [1.0, 2.0]})
    assert x.shape == (2, 3)
    vp.write_vif_log(str(tmp_path / "a.json"), vif, adm, motion=mot, siti=_siti(2), psnr_hvs=_records(2))
    names = list(json.load(open(str(tmp_path / "a.json")))["frames"][0]["metrics"])
    assert names[-4:] == ["si", "ti", "psnr_hvs", "psnr_hvsm"]


def test_config_key_psnr_hvs_is_a_bool():
    vp.validate_config(dict(GOOD))
    vp.validate_config(dict(GOOD, psnr_hvs=True))
    vp.validate_config(dict(GOOD, psnr_hvs=False, vif=True, adm=True, motion_feature=True, siti=True))
    for bad in (1, 0, "true", None, "only"):
        with pytest.raises(ValueError) as e:
            vp.validate_config(dict(GOOD, psnr_hvs=bad))
        assert str(e.value) == "psnr_hvs must be true or false."


def test_the_stream_request():
    p = [(16, 16, 0, 16, 1)]
    assert stream.Quality(p).psnr_hvs is False and stream.Quality(p, vif=True, adm=True, motion=True, siti=True).psnr_hvs is False
    assert stream.Quality(p, psnr_hvs=True).psnr_hvs is True and stream.Quality(p, psnr_hvs="only").psnr_hvs == "only"
    assert stream.Quality(p, psnr_hvs=True).ssim is True and stream.Quality(p, psnr_hvs="only").ssim is False
    assert stream.Quality(p, psnr_hvs=True).siti is False
    for bad in (1, "yes", None):
        with pytest.raises(ValueError):
            stream.Quality(p, psnr_hvs=bad)
    with pytest.raises(ValueError):
        stream.Quality(p, N.SSIM_MS, scales=True, psnr_hvs="only")
    z = np.zeros((0, 256), np.uint8)
    # an empty clip: without the request the tuples are what they were; with it ONE further last element, after SI/TI's
    for kw, length in ((dict(), 2), (dict(vif=True), 3), (dict(adm=True), 4), (dict(motion=True), 5), (dict(siti=True), 3),
                       (dict(vif=True, adm=True, motion=True, siti=True), 6)):
        q0, _ = stream.run(z, z, quality=stream.Quality(p, **kw))
        q1, _ = stream.run(z, z, quality=stream.Quality(p, psnr_hvs=True, **kw))
        assert len(q0) == length and len(q1) == length + 1, kw
        assert q1[-1].shape == (0, 1) and q1[-1].dtype.names == FIELDS
        for a, b in zip(q0, q1):
            assert (a is None and b is None) or (a.dtype == b.dtype and a.shape == b.shape)
    q, _ = stream.run(z, z, quality=stream.Quality(p, psnr_hvs="only"))
    assert len(q) == 3 and q[0] is None and q[1] is None and q[2].shape == (0, 1)
