"""ADM on four scales on the host side (no GPU): the float64 reference of tests/adm_reference.py against known answers, the
additive ABI (vqa_adm_submit, vqa_adm_wait, vqa_adm_metrics, VQA_K_ADM), the JSON log, the config key and the stream request;
and, for every pair the GPU parity tests compare, that the reference's own float32 run stays within 5e-5 of its float64 run."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import adm_cases as K
import adm_reference as A
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


def test_the_csf_weights():
    want = [(0.0173815342, 0.0058906866), (0.0319848145, 0.0142990667), (0.0433726647, 0.0243969129), (0.0456734100, 0.0313127351)]
    for s in range(4):
        hv, d = A.rf(s)
        assert abs(hv - want[s][0]) <= 1e-9 and abs(d - want[s][1]) <= 1e-9, (s, hv, d)


def test_the_dwt_index_rule_by_hand():
    # even length 8: output 0 reads |−1| = 1, 0, 1, 2; output 3 reads 5, 6, 7, 8 -> 2 * 8 - 8 - 1 = 7
    assert A.dwt_index(0, 8) == [1, 0, 1, 2] and A.dwt_index(1, 8) == [1, 2, 3, 4] and A.dwt_index(3, 8) == [5, 6, 7, 7]
    # odd length 7: four outputs; output 3 reads 5, 6, 7 -> 6, 8 -> 5
    assert A.dwt_index(3, 7) == [5, 6, 6, 5]
    assert A.dwt_index(0, 2) == [1, 0, 1, 1]
    x = np.arange(7, dtype=np.float64)[:, None] * np.ones((1, 8))
    L = A._pass(x, A.LO, 0)
    assert L.shape == (4, 8)
    lo = A.LO
    assert np.allclose(L[0], lo[0] * 1 + lo[1] * 0 + lo[2] * 1 + lo[3] * 2, rtol=0, atol=1e-15)
    assert np.allclose(L[3], lo[0] * 5 + lo[1] * 6 + lo[2] * 6 + lo[3] * 5, rtol=0, atol=1e-15)
    assert abs(sum(A.LO) - np.sqrt(2.0)) <= 1e-14 and abs(sum(A.HI)) <= 1e-14
    a, v, h, d = A.dwt(np.full((9, 12), 37.0))
    assert a.shape == (5, 6)
    assert np.allclose(a, 74.0, rtol=0, atol=1e-11)
    assert max(np.abs(v).max(), np.abs(h).max(), np.abs(d).max()) <= 1e-11
    # the vertical pass comes first: h answers to a change along the rows, v along the columns
    rows = np.repeat((np.arange(16) % 2 * 50.0)[:, None], 16, axis=1)
    a, v, h, d = A.dwt(rows)
    assert np.abs(h).max() > 10 and np.abs(v).max() <= 1e-11 and np.abs(d).max() <= 1e-11


@pytest.mark.parametrize("depth", [8, 10, 16])
def test_identical_planes_give_one_on_every_scale(depth):
    a = _texture(97, 120, 1, depth)
    num, den, scale, adm2 = A.adm(a, a, depth)
    assert np.abs(scale - 1.0).max() <= 1e-9, scale
    assert abs(adm2 - 1.0) <= 1e-9


def test_constant_planes_in_closed_form():
    a, b = np.full((47, 35), 100), np.full((47, 35), 140)
    num, den, scale, adm2 = A.adm(a, b)
    want = [3.0 * np.cbrt(A.region(bh, bw)[4] / 32.0) for bh, bw in A.level_dims(47, 35)]
    assert np.allclose(den, want, rtol=0, atol=1e-9) and np.allclose(num, want, rtol=0, atol=1e-9)
    assert abs(adm2 - 1.0) <= 1e-9


def _band_terms(ref, dist):
    """per scale and band: (num_band - c, den_band - c)"""
    x, y = ref.astype(np.float64) - 128.0, dist.astype(np.float64) - 128.0
    out = []
    for s in range(4):
        xa, xv, xh, xd = A.dwt(x)
        ya, yv, yh, yd = A.dwt(y)
        o, t = (xh, xv, xd), (yh, yv, yd)
        rfs = A.rf(s)
        w = (rfs[0], rfs[0], rfs[1])
        r, flag, _ = A.decouple(o, t)
        r = A._apply_flag(r, t, flag)
        thr = A._neighbour_sum(sum(np.abs(w[b] * (t[b] - r[b])) for b in range(3)))
        top, bottom, left, right, _area = A.region(*o[0].shape)
        for b in range(3):
            n = np.cbrt((np.maximum(np.abs(w[b] * r[b]) - thr, 0)[top:bottom, left:right] ** 3).sum())
            dn = np.cbrt((np.abs(w[b] * o[b])[top:bottom, left:right] ** 3).sum())
            out.append((n, dn))
        x, y = xa, ya
    return out


def test_a_halved_and_a_doubled_image_in_closed_form():
    """ref even-valued, D = R / 2 + 64: y = x / 2 exactly, every detail band is halved: k = 1/2, r = t, no additive part, no
    threshold: num_band - c = (den_band - c) / 2.  D = 2 R - 128 (kept in range): y = 2 x, the angle test holds, r = min(100 o,
    t) = t: the factor is 2 - enhancement is counted."""
    r = (_texture(80, 112, 4) // 2) * 2
    for n, dn in _band_terms(r, r // 2 + 64):
        assert dn > 0 and abs(n - 0.5 * dn) <= 1e-9 * dn
    r = 64 + _texture(80, 112, 4) // 2          # 64 .. 191: 2 r - 128 stays in 0 .. 254
    for n, dn in _band_terms(r, 2 * r - 128):
        assert dn > 0 and abs(n - 2.0 * dn) <= 1e-9 * dn
    num, den, scale, adm2 = A.adm(r, 2 * r - 128)
    assert (scale > 1.0).all() and adm2 > 1.0


def test_adm2_falls_as_a_blur_widens():
    a = _texture(120, 150, 3).astype(np.float64)
    got = []
    for s in (3, 2, 1, 0):   # 3, 5, 9, 17 taps
        b = np.clip(np.rint(V.filt(a, V.taps(s))), 0, 255)
        got.append(A.adm(a, b)[3])
    assert all(x > y for x, y in zip(got, got[1:])), got
    assert got[0] < 1.0


def test_level_dims_ceil_and_the_minimum_plane():
    assert A.level_dims(47, 35) == [(24, 18), (12, 9), (6, 5), (3, 3)]
    assert A.level_dims(16, 16) == [(8, 8), (4, 4), (2, 2), (1, 1)]
    x = np.zeros((47, 35))
    for want in A.level_dims(47, 35):
        x = A.dwt(x)[0]
        assert x.shape == want
    assert A.region(54, 96) == (4, 50, 9, 87, 46 * 78) and A.region(1, 1) == (0, 1, 0, 1, 1) and A.region(4, 4)[4] == 16
    assert [A.border_index(i, 5) for i in (-1, 0, 4, 5)] == [1, 0, 4, 4] and A.border_index(-1, 1) == 0
    with pytest.raises(ValueError):
        A.adm(np.zeros((15, 40)), np.zeros((15, 40)))
    A.adm(np.zeros((16, 16)), np.zeros((16, 16)))


def test_float32_stays_within_half_the_bar_on_every_gpu_parity_pair():
    """the decoupling's angle test is a discontinuity; the GPU parity pairs are chosen so that the reference's own float32 run
    does not flip a sample that matters: within 5e-5 (half the GPU bar) of float64 on every scale and on adm2"""
    worst = ("", 0.0)
    for tag, r, d, depth in K.parity_pairs():
        a, b = A.adm(r, d, depth), A.adm(r, d, depth, dtype=np.float32)
        e = max(np.abs(a[2] - b[2]).max(), abs(a[3] - b[3]))
        worst = max(worst, (tag, e), key=lambda x: x[1])
        assert e <= 5e-5, (tag, e)
    print("worst float32 deviation", worst)


def test_the_margin_report():
    a = _texture(64, 80, 5)
    b = K.distort(a, "sharp", 8, 1)
    num, den, scale, adm2, unsure, lo, hi = A.adm(a, b, margin=2.0 ** -20)
    assert unsure.shape == (5,) and unsure[4] == unsure[:4].sum()
    assert (lo[:4] <= scale + 1e-15).all() and (scale <= hi[:4] + 1e-15).all() and lo[4] <= adm2 <= hi[4]
    assert (hi - lo)[unsure == 0].max(initial=0.0) <= 1e-15     # no unsure sample, no spread
    wide = A.adm(a, b, margin=1e-2)
    assert wide[4][4] >= unsure[4] and (wide[6] - wide[5] >= hi - lo - 1e-15).all()


def test_the_additive_abi():
    assert N.VQA_ABI_VERSION == 8
    assert C.sizeof(N.VqaAdmMetrics) == 104
    assert [getattr(N.VqaAdmMetrics, f).offset for f in ("num", "den", "scale", "adm2")] == [0, 32, 64, 96]
    from rtvqa_amd.engine import ADM_DTYPE
    assert ADM_DTYPE.itemsize == 104 and [ADM_DTYPE.fields[f][1] for f in ("num", "den", "scale", "adm2")] == [0, 32, 64, 96]
    assert (N.K_ADM, N.K_ADM_REDUCE, N.K_COUNT_EXT, N.K_COUNT_ALL, N.K_COUNT) == (16, 17, 18, 14, 12)
    assert N.K_IDS == tuple(range(14)) + (16, 17)
    assert N.ADM_LEVELS == A.LEVELS and N.ADM_MIN_DIM == A.MIN_DIM
    txt = open(os.path.join(REPO, "include", "vqa.h")).read()
    assert re.search(r"VQA_K_ADM\s*=\s*16", txt) and re.search(r"VQA_K_ADM_REDUCE\s*=\s*17", txt) and re.search(r"VQA_K_COUNT_EXT\s*=\s*18", txt)
    assert re.search(r"VQA_K_COUNT_ALL\s*=\s*14", txt) and re.search(r"#define VQA_ABI_VERSION\s+8", txt)
    assert re.search(r"typedef struct vqa_adm_metrics \{\s*double num\[4\], den\[4\];[^}]*double scale\[4\];[^}]*double adm2;[^}]*\}"
                     r" vqa_adm_metrics;", txt)
    lib = N.load()
    assert "vqa_adm_submit" in N.SIGNATURES and "vqa_adm_wait" in N.SIGNATURES
    lib.vqa_kernel_name.restype = C.c_char_p
    assert lib.vqa_kernel_name(N.K_ADM) == b"k_adm_scale" and lib.vqa_kernel_name(N.K_ADM_REDUCE) == b"k_adm_reduce"
    assert lib.vqa_kernel_name(14) == b"?" and lib.vqa_kernel_name(15) == b"?" and lib.vqa_kernel_name(N.K_COUNT_EXT) == b"?"
    assert lib.vqa_kernel_name(N.K_VIF) == b"k_vif_stats" and lib.vqa_kernel_name(0) == b"k_bgr2gray_hist"
    # argument checks that need no device
    assert lib.vqa_adm_submit(None, None, None, 0, 0, 0, 0, None, 0) == N.VQA_ERR_INVALID
    assert lib.vqa_adm_wait(None, None, 0) == N.VQA_ERR_INVALID
    assert lib.vqa_profile_read(None, N.K_ADM, None, None, 0) == N.VQA_ERR_INVALID


def test_the_header_struct_is_104_bytes_to_the_c_compiler(tmp_path):
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "vqa.h"\nint main(void){printf("%zu %zu %zu %zu %zu %d %d %d\\n", '
           'sizeof(vqa_adm_metrics), offsetof(vqa_adm_metrics, num), offsetof(vqa_adm_metrics, den), offsetof(vqa_adm_metrics, scale), '
           'offsetof(vqa_adm_metrics, adm2), VQA_K_ADM, VQA_K_COUNT_ALL, VQA_K_COUNT_EXT);return 0;}\n')
    (tmp_path / "m.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), "-o", str(tmp_path / "m"), str(tmp_path / "m.c")])
    assert subprocess.check_output([str(tmp_path / "m")]).decode().split() == ["104", "0", "32", "64", "96", "16", "14", "18"]


def _records(n, seed=0):
    from rtvqa_amd.engine import ADM_DTYPE
    rng = np.random.default_rng(seed)
    rec = np.zeros(n, ADM_DTYPE)
    rec["scale"] = 0.8 + 0.3 * rng.random((n, 4))
    rec["adm2"] = 0.8 + 0.3 * rng.random(n)
    return rec


def test_the_json_log_and_what_the_row_takes_from_it(tmp_path):
    vif = np.array([[0.5, 0.9, 0.95, 0.99], [0.7, 0.8, 0.97, 1.01], [0.6, 0.85, 0.96, 1.0]])
    rec = _records(3)
    names = ["adm2"] + ["adm_scale%d" % s for s in range(4)]
    # called as before, it writes what it wrote before
    old, log, only = str(tmp_path / "old.json"), str(tmp_path / "vmaf.json"), str(tmp_path / "adm.json")
    vp.write_vif_log(old, vif)
    doc0 = json.load(open(old))
    assert list(doc0["frames"][0]["metrics"]) == ["vif_scale%d" % s for s in range(4)] and list(doc0["pooled_metrics"]) == list(doc0["frames"][0]["metrics"])
    vp.write_vif_log(log, vif, rec)
    doc = json.load(open(log))
    assert sorted(doc) == ["frames", "pooled_metrics"] and "vmaf" not in json.dumps(doc)
    assert [f["frameNum"] for f in doc["frames"]] == [0, 1, 2]
    assert list(doc["frames"][1]["metrics"]) == ["vif_scale%d" % s for s in range(4)] + names
    for i in range(3):
        assert {k: v for k, v in doc["frames"][i]["metrics"].items() if k.startswith("vif")} == doc0["frames"][i]["metrics"]
        assert doc["frames"][i]["metrics"]["adm2"] == float(rec["adm2"][i])
        assert [doc["frames"][i]["metrics"]["adm_scale%d" % s] for s in range(4)] == [float(x) for x in rec["scale"][i]]
    assert {k: v for k, v in doc["pooled_metrics"].items() if k.startswith("vif")} == doc0["pooled_metrics"]
    for k in names:
        p = doc["pooled_metrics"][k]
        assert sorted(p) == ["harmonic_mean", "max", "mean", "min"]
        x = rec["adm2"] if k == "adm2" else rec["scale"][:, int(k[-1])]
        assert p["min"] == x.min() and p["max"] == x.max() and abs(p["mean"] - x.mean()) <= 1e-15
        assert abs(p["harmonic_mean"] - (3.0 / (1.0 / (x + 1.0)).sum() - 1.0)) <= 1e-15
    vp.write_vif_log(only, None, rec)
    assert list(json.load(open(only))["frames"][0]["metrics"]) == names
    pl, sl = tmp_path / "psnr.log", tmp_path / "ssim.log"
    pl.write_text("n:1 mse_avg:1.00 psnr_avg:48.13 \n")
    sl.write_text("n:1 Y:0.990000 All:0.990000 (20.000000)\n")
    base = ["Bitrate (kbps)", "Resolution (px)", "Frame Rate (fps)", "CRF", "PSNR", "SSIM"]
    cols = ["ADM2", "ADM_scale0", "ADM_scale1", "ADM_scale2", "ADM_scale3"]
    m = vp.extract_metrics_from_logs(str(pl), str(sl), log, "x", 23, 1000, "64x64", 30.0)
    assert list(m) == base + ["VIF_scale0", "VIF_scale1", "VIF_scale2", "VIF_scale3"] + cols
    assert "VMAF" not in m
    assert [m[c] for c in cols] == [doc["pooled_metrics"][k]["mean"] for k in names]
    assert list(vp.extract_metrics_from_logs(str(pl), str(sl), only, "x", 23, 1000, "64x64", 30.0)) == base + cols
    # rows from logs without ADM are what they were
    m0 = vp.extract_metrics_from_logs(str(pl), str(sl), old, "x", 23, 1000, "64x64", 30.0)
    assert list(m0) == base + ["VIF_scale0", "VIF_scale1", "VIF_scale2", "VIF_scale3"]
    assert list(vp.extract_metrics_from_logs(str(pl), str(sl), str(tmp_path / "none.json"), "x", 23, 1000, "64x64", 30.0)) == base


def test_config_key_adm_is_a_bool():
    vp.validate_config(dict(GOOD))
    vp.validate_config(dict(GOOD, adm=True))
    vp.validate_config(dict(GOOD, adm=False, vif=True))
    for bad in (1, 0, "true", None, "yes"):
        with pytest.raises(ValueError) as e:
            vp.validate_config(dict(GOOD, adm=bad))
        assert str(e.value) == "adm must be true or false."


def test_the_stream_request():
    from rtvqa_amd import stream
    p = [(16, 16, 0, 16, 1)]
    assert stream.Quality(p).adm is False and stream.Quality(p, vif=True).adm is False
    assert stream.Quality(p, adm=True).adm is True and stream.Quality(p, adm="only").adm == "only"
    for bad in (1, "yes", None):
        with pytest.raises(ValueError):
            stream.Quality(p, adm=bad)
    with pytest.raises(ValueError):
        stream.Quality(p, N.SSIM_MS, scales=True, adm="only")
    z = np.zeros((0, 256), np.uint8)
    fields = ("num", "den", "scale", "adm2")
    # an empty clip: the tuple keeps its shape; the fourth element exists only when ADM is requested
    q, _ = stream.run(z, z, quality=stream.Quality(p))
    assert len(q) == 2
    q, _ = stream.run(z, z, quality=stream.Quality(p, vif=True))
    assert len(q) == 3 and q[2].dtype.names == ("num", "den", "scale", "vif")
    q, _ = stream.run(z, z, quality=stream.Quality(p, adm=True))
    assert len(q) == 4 and q[0].shape == (0, 1) and q[2] is None and q[3].shape == (0, 1) and q[3].dtype.names == fields
    q, _ = stream.run(z, z, quality=stream.Quality(p, vif=True, adm=True))
    assert len(q) == 4 and q[2].dtype.names == ("num", "den", "scale", "vif") and q[3].dtype.names == fields
    q, _ = stream.run(z, z, quality=stream.Quality(p, adm="only"))
    assert q[0] is None and q[1] is None and q[2] is None and q[3].shape == (0, 1)
    q, _ = stream.run(z, z, quality=stream.Quality(p, N.SSIM_MS, scales=True, adm=True))
    assert len(q) == 6 and q[4] is None and q[5].dtype.names == fields
