"""ITU-T P.910 spatial and temporal information on the host side (no GPU): the NumPy restatement of tests/siti_reference.py
against known answers, the additive ABI (vqa_siti_submit, vqa_siti_wait, vqa_siti_metrics, VQA_K_SITI), the JSON log and the
row, the config key and the stream request."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import siti_reference as S
from rtvqa_amd import _native as N
from rtvqa_amd import stream
from rtvqa_amd import video_processing as vp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOOD = {"crf": 23, "vmaf_model_path": None, "resize_width": 64, "resize_height": 64, "frame_interval": 10}
FIELDS = ("grad_sum", "grad_sq", "diff_sum", "diff_sq", "si", "ti")


def _texture(h, w, seed, depth=8):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    v = 0.5 + 0.25 * np.sin(x / 7.0) * np.cos(y / 11.0) + 0.2 * np.sin((x + 2 * y) / 23.0) + 0.03 * rng.standard_normal((h, w))
    return np.clip(np.rint(v * ((1 << depth) - 1)), 0, (1 << depth) - 1).astype(np.int64)


def test_a_constant_plane_has_no_information():
    a = np.full((21, 30), 77)
    r = S.record(a, a)
    assert r["grad_fix"] == 0 and r["grad_sq"] == 0 and r["diff_sum"] == 0 and r["diff_sq"] == 0
    assert r["si"] == 0.0 and r["ti"] == 0.0


def test_a_horizontal_ramp_has_one_gradient_everywhere():
    h, w = 19, 40
    a = np.repeat(np.arange(w)[None, :], h, axis=0)
    q = S.sobel_q(a)
    assert (q == 64).all() and q.shape == (h - 2, w - 2)
    r = S.record(a)
    n_i = (h - 2) * (w - 2)
    assert r["grad_fix"] == 8 * n_i << 32 and r["grad_sum"] == 8.0 * n_i and r["grad_sq"] == 64 * n_i
    assert r["si"] == 0.0 and r["ti"] == 0.0
    # the transpose: gy takes gx's place
    assert (S.sobel_q(a.T) == 64).all()


def test_one_interior_sample_on_zeros():
    """the impulse is seen by its eight neighbours: |gx|, |gy| = (v, v) at the four corners, 2v at the four edge neighbours"""
    for v in (1, 200, 65535):
        a = np.zeros((16, 18), np.int64)
        a[7, 9] = v
        r = S.record(a)
        assert r["grad_sq"] == 24 * v * v == 4 * 2 * v * v + 4 * 4 * v * v


def test_a_brightness_shift_has_no_temporal_information():
    a = _texture(24, 33, 1)
    for c in (5, -3):
        r = S.record(a + c, a)
        assert r["diff_sum"] == c * 24 * 33 and r["diff_sq"] == c * c * 24 * 33 and r["ti"] == 0.0
    assert S.record(a)["ti"] == 0.0 and S.record(a)["diff_sq"] == 0      # no predecessor


def test_ten_bits_are_read_on_the_8_bit_scale():
    a, b = _texture(20, 28, 2), _texture(20, 28, 3)
    r8, r10 = S.record(b, a, 8), S.record(4 * b, 4 * a, 10)
    assert r10["grad_sq"] == 16 * r8["grad_sq"] and r10["diff_sq"] == 16 * r8["diff_sq"] and r10["diff_sum"] == 4 * r8["diff_sum"]
    assert r10["ti"] == r8["ti"] and r8["si"] > 0.0 and r8["ti"] > 0.0          # powers of two all the way: the same bits
    # si: each side rounds its own square roots to 2^-32, so the two agree to the quantum's bound of either side
    _, m, var = S.si_exact(b)
    assert abs(r10["si"] - r8["si"]) <= S.quantum_bar(m, var) + S.quantum_bar(4 * m, 16 * var, 10)
    assert abs(S.si_exact(4 * b, 10)[0] - S.si_exact(b)[0]) <= 1e-12


def test_the_quantum_on_a_plane_of_one_oblique_gradient():
    """R = x + y: q = 128 everywhere and the true SI is 0; what is left is the 2^-32 quantum on sqrt(128)"""
    y, x = np.mgrid[0:40, 0:56]
    r = S.record(x + y)
    assert (S.sobel_q(x + y) == 128).all()
    print("si of R = x + y: %.3e" % r["si"])
    assert r["si"] < 1e-4
    exact, m, var = S.si_exact(x + y)
    assert exact <= 1e-12 and r["si"] <= S.quantum_bar(m, var)


def test_the_two_forms_agree_and_prev0_is_the_frame_before():
    a = np.stack([_texture(20, 28, s) for s in range(4)])
    whole = S.series(a)
    assert whole[0]["ti"] == 0.0 and all(r["ti"] > 0 and r["si"] > 0 for r in whole[1:])
    assert S.series(a[1:], prev0=a[0]) == whole[1:]
    for i, r in enumerate(whole):
        exact, m, var = S.si_exact(a[i])
        assert abs(r["si"] - exact) <= S.quantum_bar(m, var)
        assert abs(r["ti"] - S.ti_exact(a[i], a[i - 1] if i else None)[0]) <= 1e-12
    with pytest.raises(ValueError):
        S.record(np.zeros((15, 40)))


def test_the_additive_abi():
    assert N.VQA_ABI_VERSION == 8
    assert C.sizeof(N.VqaSitiMetrics) == 48
    assert [getattr(N.VqaSitiMetrics, f).offset for f in FIELDS] == [0, 8, 16, 24, 32, 40]
    from rtvqa_amd.engine import SITI_DTYPE
    assert SITI_DTYPE.itemsize == 48 and [SITI_DTYPE.fields[f][1] for f in FIELDS] == [0, 8, 16, 24, 32, 40]
    assert SITI_DTYPE.names == FIELDS
    assert (N.K_SITI, N.K_LAST, N.K_END, N.K_MOTION) == (21, 22, 20, 19)
    assert N.K_IDS_KNOWN == tuple(range(14)) + (16, 17, 19, 21) and N.K_IDS_ALL == tuple(range(14)) + (16, 17, 19)
    assert N.SITI_MIN_DIM == S.MIN_DIM == 16
    txt = open(os.path.join(REPO, "include", "vqa.h")).read()
    assert re.search(r"VQA_K_SITI\s*=\s*21", txt) and re.search(r"VQA_K_LAST\s*=\s*22", txt) and re.search(r"VQA_K_END\s*=\s*20", txt)
    assert re.search(r"#define VQA_ABI_VERSION\s+8", txt)
    lib = N.load()
    assert "vqa_siti_submit" in N.SIGNATURES and "vqa_siti_wait" in N.SIGNATURES
    assert hasattr(lib, "vqa_siti_submit") and hasattr(lib, "vqa_siti_wait")     # both symbols are exported
    lib.vqa_kernel_name.restype = C.c_char_p
    assert lib.vqa_kernel_name(N.K_SITI) == b"k_siti"
    assert lib.vqa_kernel_name(N.K_END) == b"?" and lib.vqa_kernel_name(N.K_LAST) == b"?"
    assert lib.vqa_kernel_name(N.K_MOTION) == b"k_motion_sad"
    assert lib.vqa_abi_version() == 8
    # argument checks that need no device
    assert lib.vqa_siti_submit(None, None, None, 0, 0, 0, None, 0) == N.VQA_ERR_INVALID
    assert lib.vqa_siti_wait(None, None, 0) == N.VQA_ERR_INVALID
    assert lib.vqa_profile_read(None, N.K_SITI, None, None, 0) == N.VQA_ERR_INVALID


def test_the_header_struct_is_48_bytes_to_the_c_compiler(tmp_path):
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "vqa.h"\n'
           'int (*submit)(vqa_ctx *, const uint8_t *, const uint8_t *, int, int, int64_t, const vqa_plane_desc *, int) = vqa_siti_submit;\n'
           'int (*wait_)(vqa_ctx *, vqa_siti_metrics *, int) = vqa_siti_wait;\n'
           'int main(void){printf("%zu %zu %zu %zu %zu %zu %zu %d %d %d %d\\n", sizeof(vqa_siti_metrics), '
           'offsetof(vqa_siti_metrics, grad_sum), offsetof(vqa_siti_metrics, grad_sq), offsetof(vqa_siti_metrics, diff_sum), '
           'offsetof(vqa_siti_metrics, diff_sq), offsetof(vqa_siti_metrics, si), offsetof(vqa_siti_metrics, ti), '
           'VQA_K_SITI, VQA_K_LAST, VQA_K_END, VQA_ABI_VERSION);return submit == 0 || wait_ == 0;}\n')
    (tmp_path / "s.c").write_text(src)
    lib_dir = os.path.dirname(N.LIB_PATH)
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), "-o", str(tmp_path / "s"), str(tmp_path / "s.c"),
                           "-L", lib_dir, "-l:" + os.path.basename(N.LIB_PATH), "-Wl,-rpath," + lib_dir,
                           "-Wl,--allow-shlib-undefined"])
    assert subprocess.check_output([str(tmp_path / "s")]).decode().split() == ["48", "0", "8", "16", "24", "32", "40", "21", "22", "20", "8"]


def _siti_records(n, seed=0):
    from rtvqa_amd.engine import SITI_DTYPE
    rng = np.random.default_rng(seed)
    rec = np.zeros(n, SITI_DTYPE)
    rec["si"], rec["ti"] = 20.0 + 60.0 * rng.random(n), 30.0 * rng.random(n)
    rec["ti"][0] = 0.0
    return rec


def test_the_json_log_and_what_the_row_takes_from_it(tmp_path):
    from rtvqa_amd.engine import ADM_DTYPE
    vif = np.array([[0.5, 0.9, 0.95, 0.99], [0.7, 0.8, 0.97, 1.01], [0.6, 0.85, 0.96, 1.0]])
    adm = np.zeros(3, ADM_DTYPE)
    adm["adm2"], adm["scale"] = [0.9, 0.95, 0.85], 0.9
    mot = np.zeros(3, stream.MOTION_PASS_DTYPE)
    mot["motion"], mot["motion2"] = [0.0, 2.0, 1.0], [0.0, 1.0, 1.0]
    rec = _siti_records(3)
    old, log, only = str(tmp_path / "old.json"), str(tmp_path / "vmaf.json"), str(tmp_path / "siti.json")
    vp.write_vif_log(old, vif, adm, motion=mot)
    vp.write_vif_log(log, vif, adm, motion=mot, siti=rec)
    doc0, doc = json.load(open(old)), json.load(open(log))
    assert "\"si\"" not in json.dumps(doc0) and "\"ti\"" not in json.dumps(doc0) and "vmaf" not in json.dumps(doc)
    names0 = list(doc0["frames"][0]["metrics"])
    assert names0[-2:] == ["motion2", "motion"]
    assert list(doc["frames"][1]["metrics"]) == names0 + ["si", "ti"] == list(doc["pooled_metrics"])
    for i in range(3):
        m = doc["frames"][i]["metrics"]
        assert {k: m[k] for k in names0} == doc0["frames"][i]["metrics"]
        assert m["si"] == float(rec["si"][i]) and m["ti"] == float(rec["ti"][i])
    assert {k: doc["pooled_metrics"][k] for k in names0} == doc0["pooled_metrics"]
    for k in ("si", "ti"):
        p, x = doc["pooled_metrics"][k], rec[k]
        assert sorted(p) == ["harmonic_mean", "max", "mean", "min"]
        assert p["min"] == x.min() and p["max"] == x.max() and abs(p["mean"] - x.mean()) <= 1e-14
        assert abs(p["harmonic_mean"] - (3.0 / (1.0 / (x + 1.0)).sum() - 1.0)) <= 1e-13
    vp.write_vif_log(only, siti=rec)
    assert list(json.load(open(only))["frames"][0]["metrics"]) == ["si", "ti"]
    pl, sl = tmp_path / "psnr.log", tmp_path / "ssim.log"
    pl.write_text("n:1 mse_avg:1.00 psnr_avg:48.13 \n")
    sl.write_text("n:1 Y:0.990000 All:0.990000 (20.000000)\n")
    base = ["Bitrate (kbps)", "Resolution (px)", "Frame Rate (fps)", "CRF", "PSNR", "SSIM"]
    feats = ["VIF_scale0", "VIF_scale1", "VIF_scale2", "VIF_scale3", "ADM2", "ADM_scale0", "ADM_scale1", "ADM_scale2", "ADM_scale3",
             "MOTION2", "MOTION"]
    m = vp.extract_metrics_from_logs(str(pl), str(sl), log, "x", 23, 1000, "64x64", 30.0)
    assert list(m) == base + feats + ["SI", "TI"]
    assert m["SI"] == float(rec["si"].max()) and m["TI"] == float(rec["ti"].max())      # P.910: the maxima, not the means
    assert m["SI"] != doc["pooled_metrics"]["si"]["mean"]
    assert list(vp.extract_metrics_from_logs(str(pl), str(sl), only, "x", 23, 1000, "64x64", 30.0)) == base + ["SI", "TI"]
    # rows and logs without siti are what they were
    m0 = vp.extract_metrics_from_logs(str(pl), str(sl), old, "x", 23, 1000, "64x64", 30.0)
    assert list(m0) == base + feats and {k: m[k] for k in m0} == m0
    again = str(tmp_path / "again.json")
    vp.write_vif_log(again, vif, adm, motion=mot, siti=None)
    assert open(again, "rb").read() == open(old, "rb").read()


def test_a_model_scores_the_same_with_si_and_ti_in_the_log(tmp_path):
    """si and ti come after the motion keys and before vmaf; the model never reads them"""
    from rtvqa_amd import vmaf_model
    from rtvqa_amd.engine import ADM_DTYPE

    class Model:
        features = ["vif_scale0", "adm2", "motion2"]

    vif = np.array([[0.5, 0.9, 0.95, 0.99], [0.7, 0.8, 0.97, 1.01]])
    adm = np.zeros(2, ADM_DTYPE)
    adm["adm2"] = [0.9, 0.95]
    mot = np.zeros(2, stream.MOTION_PASS_DTYPE)
    x = vmaf_model.feature_matrix(Model, {"vif_scale0": vif[:, 0], "adm2": adm["adm2"], "motion2": mot["motion2"], "si": [1.0, 2.0]})
    assert x.shape == (2, 3)
    vp.write_vif_log(str(tmp_path / "a.json"), vif, adm, motion=mot, siti=_siti_records(2))
    names = list(json.load(open(str(tmp_path / "a.json")))["frames"][0]["metrics"])
    assert names[-4:] == ["motion2", "motion", "si", "ti"]


def test_config_key_siti_is_a_bool():
    vp.validate_config(dict(GOOD))
    vp.validate_config(dict(GOOD, siti=True))
    vp.validate_config(dict(GOOD, siti=False, vif=True, adm=True, motion_feature=True))
    for bad in (1, 0, "true", None, "only"):
        with pytest.raises(ValueError) as e:
            vp.validate_config(dict(GOOD, siti=bad))
        assert str(e.value) == "siti must be true or false."


def test_the_stream_request():
    p = [(16, 16, 0, 16, 1)]
    assert stream.Quality(p).siti is False and stream.Quality(p, vif=True, adm=True, motion=True).siti is False
    assert stream.Quality(p, siti=True).siti is True and stream.Quality(p, siti="only").siti == "only"
    assert stream.Quality(p, siti=True).ssim is True and stream.Quality(p, siti="only").ssim is False
    assert stream.Quality(p, siti=True).motion is False
    for bad in (1, "yes", None):
        with pytest.raises(ValueError):
            stream.Quality(p, siti=bad)
    with pytest.raises(ValueError):
        stream.Quality(p, N.SSIM_MS, scales=True, siti="only")
    z = np.zeros((0, 256), np.uint8)
    # an empty clip: without siti the tuples are what they were; with it ONE further last element
    for kw, length in ((dict(), 2), (dict(vif=True), 3), (dict(adm=True), 4), (dict(motion=True), 5), (dict(vif=True, adm=True, motion=True), 5)):
        q0, _ = stream.run(z, z, quality=stream.Quality(p, **kw))
        q1, _ = stream.run(z, z, quality=stream.Quality(p, siti=True, **kw))
        assert len(q0) == length and len(q1) == length + 1, kw
        assert q1[-1].shape == (0, 1) and q1[-1].dtype.names == FIELDS
        for a, b in zip(q0, q1):
            assert (a is None and b is None) or (a.dtype == b.dtype and a.shape == b.shape)
    q, _ = stream.run(z, z, quality=stream.Quality(p, siti="only"))
    assert len(q) == 3 and q[0] is None and q[1] is None and q[2].shape == (0, 1)
    q, _ = stream.run(z, z, quality=stream.Quality(p, N.SSIM_MS, scales=True, siti=True))
    assert len(q) == 5 and q[4].dtype.names == FIELDS
