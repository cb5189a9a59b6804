"""VIF on four scales on the host side (no GPU): the float64 reference of tests/vif_reference.py against known answers, the
additive ABI (vqa_vif_submit, vqa_vif_wait, vqa_vif_metrics, VQA_K_VIF), the JSON log and the config key."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import vif_reference as V
from rtvqa_amd import _native as N
from rtvqa_amd import video_processing as vp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOOD = {"crf": 23, "vmaf_model_path": None, "resize_width": 64, "resize_height": 64, "frame_interval": 10}


def _texture(h, w, seed, depth=8):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    v = 0.5 + 0.25 * np.sin(x / 7.0) * np.cos(y / 11.0) + 0.2 * np.sin((x + 2 * y) / 23.0) + 0.03 * rng.standard_normal((h, w))
    return np.clip(np.rint(v * ((1 << depth) - 1)), 0, (1 << depth) - 1).astype(np.int64)


@pytest.mark.parametrize("depth", [8, 10, 16])
def test_identical_planes_give_one_on_every_scale(depth):
    a = _texture(97, 120, 1, depth)
    num, den, scale, vif = V.vif(a, a, depth)
    assert np.abs(scale - 1.0).max() <= 1e-9, scale
    assert abs(vif - 1.0) <= 1e-9
    assert (num <= den + 1e-9 * den).all()


def test_constant_planes_in_closed_form():
    """s1 = s2 = 0 everywhere: den = 1 and num = 1 - 0 * smi per sample, so den_s is the level's sample count"""
    a, b = np.full((47, 35), 100), np.full((47, 35), 140)
    num, den, scale, vif = V.vif(a, b)
    counts = [h * w for h, w in V.level_dims(47, 35)]
    assert np.allclose(den, counts, rtol=0, atol=1e-6) and np.allclose(num, counts, rtol=0, atol=1e-6)
    assert np.abs(scale - 1.0).max() <= 1e-9 and abs(vif - 1.0) <= 1e-9


def test_level_dims_floor():
    assert V.level_dims(47, 35) == [(47, 35), (23, 17), (11, 8), (5, 4)]
    x = np.zeros((47, 35))
    dims = [x.shape]
    for s in range(1, 4):
        x = V.next_level(x, s)
        dims.append(x.shape)
    assert dims == V.level_dims(47, 35)
    assert V.level_dims(16, 16)[-1] == (2, 2)
    with pytest.raises(ValueError):
        V.vif(np.zeros((15, 40)), np.zeros((15, 40)))
    V.vif(np.zeros((16, 16)), np.zeros((16, 16)))


def test_taps():
    assert [len(V.taps(s)) for s in range(4)] == [17, 9, 5, 3]
    for s in range(4):
        t = V.taps(s)
        assert abs(t.sum() - 1.0) <= 1e-15 and (t == t[::-1]).all() and t.argmax() == len(t) // 2
    # scale 3 by hand: sd = 3/5, exp(-1 / (2 * .36)) on both sides of 1
    e = np.exp(-1.0 / 0.72)
    assert np.allclose(V.taps(3), np.array([e, 1.0, e]) / (1.0 + 2.0 * e), rtol=0, atol=1e-15)


def test_the_border_rule_by_hand():
    """the two sides differ: -1 reads 1 (the edge sample is not repeated), n reads n - 1 (it is)"""
    assert [V.border_index(i, 16) for i in (-8, -2, -1, 0, 15, 16, 17, 23)] == [8, 2, 1, 0, 15, 15, 14, 8]
    # 16 x 16 ramp along the rows, 3 taps (a, b, a): out[i] = a x[left] + b x[i] + a x[right]
    x = np.tile(np.arange(16, dtype=np.float64)[:, None] * 10.0, (1, 16))
    t = V.taps(3)
    a, b = t[0], t[1]
    out = V.filt(x, t)
    assert np.allclose(out[0], a * 10.0 + b * 0.0 + a * 10.0, rtol=0, atol=1e-12)        # row -1 reads row 1
    assert np.allclose(out[15], a * 140.0 + b * 150.0 + a * 150.0, rtol=0, atol=1e-12)   # row 16 reads row 15
    assert np.allclose(out[7], 70.0, rtol=0, atol=1e-12)
    # and along the columns, 17 taps on 16 samples: column -8 reads 8, column 23 reads 8
    y = np.tile(np.arange(16, dtype=np.float64)[None, :], (16, 1))
    t0 = V.taps(0)
    o0 = V.filt(y, t0)
    want0 = sum(t0[k] * abs(k - 8) for k in range(17))
    want15 = sum(t0[k] * (15 + k - 8 if 15 + k - 8 < 16 else 2 * 16 - (15 + k - 8) - 1) for k in range(17))
    assert np.allclose(o0[:, 0], want0, rtol=0, atol=1e-12) and np.allclose(o0[:, 15], want15, rtol=0, atol=1e-12)


def test_scale_0_falls_as_the_blur_widens():
    a = _texture(120, 150, 3).astype(np.float64)
    got = []
    for s in (3, 2, 1, 0):   # 3, 5, 9, 17 taps
        b = np.clip(np.rint(V.filt(a, V.taps(s))), 0, 255)
        got.append(V.vif(a, b)[2][0])
    assert all(x > y for x, y in zip(got, got[1:])), got
    assert got[0] < 1.0


def test_the_additive_abi():
    assert N.VQA_ABI_VERSION == 8
    assert C.sizeof(N.VqaVifMetrics) == 104
    assert [getattr(N.VqaVifMetrics, f).offset for f in ("num", "den", "scale", "vif")] == [0, 32, 64, 96]
    from rtvqa_amd.engine import VIF_DTYPE
    assert VIF_DTYPE.itemsize == 104 and [VIF_DTYPE.fields[f][1] for f in ("num", "den", "scale", "vif")] == [0, 32, 64, 96]
    assert (N.K_VIF, N.K_VIF_DECIMATE, N.K_COUNT_ALL) == (12, 13, 14)
    assert N.VIF_LEVELS == V.LEVELS and N.VIF_MIN_DIM == V.MIN_DIM
    txt = open(os.path.join(REPO, "include", "vqa.h")).read()
    assert re.search(r"VQA_K_VIF\s*=\s*12", txt) and re.search(r"VQA_K_VIF_DECIMATE\s*=\s*13", txt)
    assert re.search(r"typedef struct vqa_vif_metrics \{\s*double num\[4\], den\[4\];[^}]*double scale\[4\];[^}]*double vif;[^}]*\}"
                     r" vqa_vif_metrics;", txt)
    lib = N.load()
    assert "vqa_vif_submit" in N.SIGNATURES and "vqa_vif_wait" in N.SIGNATURES
    lib.vqa_kernel_name.restype = C.c_char_p
    assert lib.vqa_kernel_name(N.K_VIF) == b"k_vif_stats" and lib.vqa_kernel_name(N.K_VIF_DECIMATE) == b"k_vif_decimate"
    assert lib.vqa_kernel_name(N.K_COUNT_ALL) == b"?"
    # argument checks that need no device
    assert lib.vqa_vif_submit(None, None, None, 0, 0, 0, 0, None, 0) == N.VQA_ERR_INVALID
    assert lib.vqa_vif_wait(None, None, 0) == N.VQA_ERR_INVALID


def test_the_header_struct_is_104_bytes_to_the_c_compiler(tmp_path):
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "vqa.h"\nint main(void){printf("%zu %zu %d %d\\n", '
           'sizeof(vqa_vif_metrics), offsetof(vqa_vif_metrics, vif), VQA_K_VIF, VQA_K_COUNT_ALL);return 0;}\n')
    (tmp_path / "m.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), "-o", str(tmp_path / "m"), str(tmp_path / "m.c")])
    assert subprocess.check_output([str(tmp_path / "m")]).decode().split() == ["104", "96", "12", "14"]


def test_the_json_log_and_what_the_row_takes_from_it(tmp_path):
    scale = np.array([[0.5, 0.9, 0.95, 0.99], [0.7, 0.8, 0.97, 1.01], [0.6, 0.85, 0.96, 1.0]])
    log = str(tmp_path / "vmaf.json")
    vp.write_vif_log(log, scale)
    doc = json.load(open(log))
    assert sorted(doc) == ["frames", "pooled_metrics"]
    assert "vmaf" not in json.dumps(doc)
    assert [f["frameNum"] for f in doc["frames"]] == [0, 1, 2]
    assert doc["frames"][1]["metrics"] == {"vif_scale0": 0.7, "vif_scale1": 0.8, "vif_scale2": 0.97, "vif_scale3": 1.01}
    for s in range(4):
        p = doc["pooled_metrics"]["vif_scale%d" % s]
        assert sorted(p) == ["harmonic_mean", "max", "mean", "min"]
        x = scale[:, s]
        assert p["min"] == x.min() and p["max"] == x.max() and abs(p["mean"] - x.mean()) <= 1e-15
        assert abs(p["harmonic_mean"] - (3.0 / (1.0 / (x + 1.0)).sum() - 1.0)) <= 1e-15
        assert p["min"] <= p["harmonic_mean"] <= p["mean"]
    pl, sl = tmp_path / "psnr.log", tmp_path / "ssim.log"
    pl.write_text("n:1 mse_avg:1.00 psnr_avg:48.13 \n")
    sl.write_text("n:1 Y:0.990000 All:0.990000 (20.000000)\n")
    m = vp.extract_metrics_from_logs(str(pl), str(sl), log, "x", 23, 1000, "64x64", 30.0)
    assert list(m) == ["Bitrate (kbps)", "Resolution (px)", "Frame Rate (fps)", "CRF", "PSNR", "SSIM",
                       "VIF_scale0", "VIF_scale1", "VIF_scale2", "VIF_scale3"]
    assert "VMAF" not in m
    assert [m["VIF_scale%d" % s] for s in range(4)] == [doc["pooled_metrics"]["vif_scale%d" % s]["mean"] for s in range(4)]
    # without the file the row is what it was
    m0 = vp.extract_metrics_from_logs(str(pl), str(sl), str(tmp_path / "none.json"), "x", 23, 1000, "64x64", 30.0)
    assert list(m0) == ["Bitrate (kbps)", "Resolution (px)", "Frame Rate (fps)", "CRF", "PSNR", "SSIM"]
    # a log that is not this JSON (libvmaf's XML) adds nothing
    (tmp_path / "x.xml").write_text("<VMAF version=\"x\"></VMAF>\n")
    assert list(vp.extract_metrics_from_logs(str(pl), str(sl), str(tmp_path / "x.xml"), "x", 23, 1000, "64x64", 30.0)) == list(m0)


def test_config_key_vif_is_a_bool():
    vp.validate_config(dict(GOOD))
    vp.validate_config(dict(GOOD, vif=True))
    vp.validate_config(dict(GOOD, vif=False))
    for bad in (1, 0, "true", None, "yes"):
        with pytest.raises(ValueError) as e:
            vp.validate_config(dict(GOOD, vif=bad))
        assert str(e.value) == "vif must be true or false."


def test_the_stream_request():
    from rtvqa_amd import stream
    p = [(16, 16, 0, 16, 1)]
    assert stream.Quality(p).vif is False
    assert stream.Quality(p, vif=True).vif is True and stream.Quality(p, vif="only").vif == "only"
    for bad in (1, "yes", None):
        with pytest.raises(ValueError):
            stream.Quality(p, vif=bad)
    with pytest.raises(ValueError):
        stream.Quality(p, N.SSIM_MS, scales=True, vif="only")
    # an empty clip: the tuple keeps its shape
    q, _ = stream.run(np.zeros((0, 256), np.uint8), np.zeros((0, 256), np.uint8), quality=stream.Quality(p, vif=True))
    assert len(q) == 3 and q[2].shape == (0, 1) and q[2].dtype.names == ("num", "den", "scale", "vif")
    q, _ = stream.run(np.zeros((0, 256), np.uint8), np.zeros((0, 256), np.uint8), quality=stream.Quality(p, vif="only"))
    assert q[0] is None and q[1] is None and q[2].shape == (0, 1)
