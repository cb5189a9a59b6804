"""VMAF's motion feature on the host side (no GPU): the float64 reference of tests/motion_reference.py against known answers,
the additive ABI (vqa_motion_submit, vqa_motion_wait, vqa_motion_metrics, VQA_K_MOTION), the JSON log and the row, the config
keys, the stream request and the stream plan's halo slot for the reference feed."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import motion_reference as M
from rtvqa_amd import _native as N
from rtvqa_amd import stream, tails
from rtvqa_amd import video_processing as vp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOOD = {"crf": 23, "vmaf_model_path": None, "resize_width": 64, "resize_height": 64, "frame_interval": 10}


def _texture(h, w, seed, depth=8):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    v = 0.5 + 0.25 * np.sin(x / 7.0) * np.cos(y / 11.0) + 0.2 * np.sin((x + 2 * y) / 23.0) + 0.03 * rng.standard_normal((h, w))
    return np.clip(np.rint(v * ((1 << depth) - 1)), 0, (1 << depth) - 1).astype(np.int64)


def test_the_border_rule_and_the_blur_by_loops():
    assert [M.border_index(i, 5) for i in (-2, -1, 0, 4, 5, 6)] == [2, 1, 0, 4, 4, 3]
    x = np.random.default_rng(0).standard_normal((19, 23))
    assert np.abs(M.blur(x) - M.blur_loops(x)).max() <= 1e-14
    # the vertical pass comes first: mathematically the order does not matter, the two orders agree to rounding
    assert np.abs(M.blur(x) - M.blur(x.T).T).max() <= 1e-14
    # one impulse in the interior spreads as the outer product of the taps
    z = np.zeros((16, 16))
    z[8, 7] = 1.0
    assert np.allclose(M.blur(z)[6:11, 5:10], np.outer(M.TAPS, M.TAPS), rtol=0, atol=1e-17)


@pytest.mark.parametrize("depth", [8, 10, 16])
def test_identical_frames_give_zero(depth):
    a = _texture(37, 52, 1, depth)
    assert M.sad(a, a, depth) == 0.0
    assert (M.motion(np.stack([a, a, a]), depth) == 0.0).all()


def test_a_constant_against_a_constant_in_closed_form():
    s = sum(M.TAPS)
    for c, d in ((100, 40), (7, -7), (0, 255)):
        a, b = np.full((21, 30), c), np.full((21, 30), c + d)
        m = M.motion(np.stack([a, b]))
        assert m[0] == 0.0 and abs(m[1] - abs(d) * s * s) <= 1e-12, (c, d, m)
    # at 10 bits a step of d is d / 4 on the 8-bit scale
    a, b = np.full((16, 16), 400), np.full((16, 16), 440)
    assert abs(M.motion(np.stack([a, b]), 10)[1] - 10.0 * s * s) <= 1e-12


def test_a_shifted_horizontal_ramp_on_the_interior():
    """x[i, j] = slope * j against the same ramp shifted by k columns: the blur of a ramp is a ramp (times the tap sum, twice)
    away from the borders, so |difference| = k * slope * (tap sum)^2 on the interior"""
    h, w, k, slope = 24, 64, 3, 2
    j = np.arange(w + k)
    ramp = np.repeat((slope * j)[None, :], h, axis=0)
    a, b = ramp[:, :w], ramp[:, k:]
    d = np.abs(M.blur(M.samples(b)) - M.blur(M.samples(a)))
    s = sum(M.TAPS)
    assert np.abs(d[:, 2:-2] - k * slope * s * s).max() <= 1e-12
    # the whole-plane motion is therefore k * slope * s^2 up to the two border columns on either side
    m = M.motion(np.stack([a, b]))[1]
    assert abs(m - k * slope * s * s) <= 4.0 / w * k * slope


def test_prev0_is_the_frame_before():
    a = np.stack([_texture(20, 28, s) for s in range(4)])
    whole = M.motion(a)
    assert whole[0] == 0.0 and (whole[1:] > 0).all()
    assert np.array_equal(M.motion(a[1:], prev0=a[0]), whole[1:])
    assert M.motion(a[2:3], prev0=a[1])[0] == whole[2]
    with pytest.raises(ValueError):
        M.sad(np.zeros((15, 40)), np.zeros((15, 40)))


def test_the_motion2_rule():
    m = [0.0, 3.0, 1.0, 4.0, 2.0]
    want = [0.0, 1.0, 1.0, 2.0, 2.0]
    assert list(M.motion2(m)) == want and list(tails.motion2(np.array(m))) == want
    assert list(M.motion2([5.0])) == [5.0] and list(tails.motion2(np.array([5.0]))) == [5.0]
    assert list(M.motion2([0.0])) == [0.0] and len(tails.motion2(np.zeros(0))) == 0
    assert list(tails.motion2(np.array([0.0, 2.0]))) == [0.0, 2.0]        # the first is 0 whenever motion[0] is, the last keeps its own
    # per plane, frame-major
    two = np.array([[0.0, 9.0], [3.0, 1.0], [1.0, 4.0]])
    assert tails.motion2(two).tolist() == [[0.0, 1.0], [1.0, 1.0], [1.0, 4.0]]
    rec = np.zeros((3, 2), [("sad", np.float64), ("motion", np.float64)])
    rec["motion"], rec["sad"] = two, two * 100
    out = stream.motion_records(rec)
    assert out.dtype.names == ("sad", "motion", "motion2") and out["motion2"].tolist() == tails.motion2(two).tolist()
    assert out["sad"].tolist() == (two * 100).tolist()


def test_the_additive_abi():
    assert N.VQA_ABI_VERSION == 8
    assert C.sizeof(N.VqaMotionMetrics) == 16
    assert [getattr(N.VqaMotionMetrics, f).offset for f in ("sad", "motion")] == [0, 8]
    from rtvqa_amd.engine import MOTION_DTYPE
    assert MOTION_DTYPE.itemsize == 16 and [MOTION_DTYPE.fields[f][1] for f in ("sad", "motion")] == [0, 8]
    assert (N.K_MOTION, N.K_END, N.K_COUNT_EXT, N.K_COUNT_ALL, N.K_COUNT) == (19, 20, 18, 14, 12)
    assert N.K_IDS_ALL == tuple(range(14)) + (16, 17, 19)
    assert N.MOTION_MIN_DIM == M.MIN_DIM
    txt = open(os.path.join(REPO, "include", "vqa.h")).read()
    assert re.search(r"VQA_K_MOTION\s*=\s*19", txt) and re.search(r"VQA_K_END\s*=\s*20", txt)
    assert re.search(r"VQA_K_COUNT_EXT\s*=\s*18", txt) and re.search(r"VQA_K_COUNT_ALL\s*=\s*14", txt) and re.search(r"VQA_K_COUNT\s*=\s*12", txt)
    assert re.search(r"#define VQA_ABI_VERSION\s+8", txt)
    assert re.search(r"typedef struct vqa_motion_metrics \{\s*double sad;[^}]*double motion;[^}]*\} vqa_motion_metrics;", txt)
    for t in M.TAPS:
        assert ("%.9f" % t) in txt
    lib = N.load()
    assert "vqa_motion_submit" in N.SIGNATURES and "vqa_motion_wait" in N.SIGNATURES
    assert hasattr(lib, "vqa_motion_submit") and hasattr(lib, "vqa_motion_wait")     # both symbols are exported
    lib.vqa_kernel_name.restype = C.c_char_p
    assert lib.vqa_kernel_name(N.K_MOTION) == b"k_motion_sad"
    assert lib.vqa_kernel_name(18) == b"?" and lib.vqa_kernel_name(N.K_END) == b"?" and lib.vqa_kernel_name(14) == b"?"
    assert lib.vqa_kernel_name(N.K_ADM) == b"k_adm_scale" and lib.vqa_kernel_name(0) == b"k_bgr2gray_hist"
    assert lib.vqa_abi_version() == 8
    # argument checks that need no device
    assert lib.vqa_motion_submit(None, None, None, 0, 0, 0, None, 0) == N.VQA_ERR_INVALID
    assert lib.vqa_motion_wait(None, None, 0) == N.VQA_ERR_INVALID
    assert lib.vqa_profile_read(None, N.K_MOTION, None, None, 0) == N.VQA_ERR_INVALID


def test_the_header_struct_is_16_bytes_to_the_c_compiler(tmp_path):
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "vqa.h"\n'
           'int (*submit)(vqa_ctx *, const uint8_t *, const uint8_t *, int, int, int64_t, const vqa_plane_desc *, int) = vqa_motion_submit;\n'
           'int (*wait_)(vqa_ctx *, vqa_motion_metrics *, int) = vqa_motion_wait;\n'
           'int main(void){printf("%zu %zu %zu %d %d %d %d %d %d\\n", sizeof(vqa_motion_metrics), offsetof(vqa_motion_metrics, sad), '
           'offsetof(vqa_motion_metrics, motion), VQA_K_MOTION, VQA_K_END, VQA_K_COUNT, VQA_K_COUNT_ALL, VQA_K_COUNT_EXT, '
           'VQA_ABI_VERSION);return submit == 0 || wait_ == 0;}\n')
    (tmp_path / "m.c").write_text(src)
    lib_dir = os.path.dirname(N.LIB_PATH)
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), "-o", str(tmp_path / "m"), str(tmp_path / "m.c"),
                           "-L", lib_dir, "-l:" + os.path.basename(N.LIB_PATH), "-Wl,-rpath," + lib_dir,
                           "-Wl,--allow-shlib-undefined"])
    assert subprocess.check_output([str(tmp_path / "m")]).decode().split() == ["16", "0", "8", "19", "20", "12", "14", "18", "8"]


def _motion_records(n, seed=0):
    rng = np.random.default_rng(seed)
    rec = np.zeros(n, stream.MOTION_PASS_DTYPE)
    rec["motion"] = 5.0 * rng.random(n)
    rec["motion"][0] = 0.0
    rec["sad"] = rec["motion"] * 64 * 64
    rec["motion2"] = tails.motion2(rec["motion"])
    return rec


def test_the_json_log_and_what_the_row_takes_from_it(tmp_path):
    from rtvqa_amd.engine import ADM_DTYPE
    vif = np.array([[0.5, 0.9, 0.95, 0.99], [0.7, 0.8, 0.97, 1.01], [0.6, 0.85, 0.96, 1.0]])
    adm = np.zeros(3, ADM_DTYPE)
    adm["adm2"], adm["scale"] = [0.9, 0.95, 0.85], 0.9
    mot = _motion_records(3)
    old, log, only = str(tmp_path / "old.json"), str(tmp_path / "vmaf.json"), str(tmp_path / "motion.json")
    vp.write_vif_log(old, vif, adm)
    doc0 = json.load(open(old))
    assert "motion" not in json.dumps(doc0) and "vmaf" not in json.dumps(doc0)
    vp.write_vif_log(log, vif, adm, motion=mot)
    doc = json.load(open(log))
    assert "vmaf" not in json.dumps(doc)
    names0 = list(doc0["frames"][0]["metrics"])
    assert list(doc["frames"][1]["metrics"]) == names0 + ["motion2", "motion"] and list(doc["pooled_metrics"]) == names0 + ["motion2", "motion"]
    for i in range(3):
        m = doc["frames"][i]["metrics"]
        assert {k: m[k] for k in names0} == doc0["frames"][i]["metrics"]
        assert m["motion"] == float(mot["motion"][i]) and m["motion2"] == float(mot["motion2"][i])
    assert {k: doc["pooled_metrics"][k] for k in names0} == doc0["pooled_metrics"]
    for k in ("motion", "motion2"):
        p, x = doc["pooled_metrics"][k], mot[k]
        assert sorted(p) == ["harmonic_mean", "max", "mean", "min"]
        assert p["min"] == x.min() and p["max"] == x.max() and abs(p["mean"] - x.mean()) <= 1e-15
        assert abs(p["harmonic_mean"] - (3.0 / (1.0 / (x + 1.0)).sum() - 1.0)) <= 1e-15
    vp.write_vif_log(only, None, None, motion=mot)
    assert list(json.load(open(only))["frames"][0]["metrics"]) == ["motion2", "motion"]
    pl, sl = tmp_path / "psnr.log", tmp_path / "ssim.log"
    pl.write_text("n:1 mse_avg:1.00 psnr_avg:48.13 \n")
    sl.write_text("n:1 Y:0.990000 All:0.990000 (20.000000)\n")
    base = ["Bitrate (kbps)", "Resolution (px)", "Frame Rate (fps)", "CRF", "PSNR", "SSIM"]
    feats = ["VIF_scale0", "VIF_scale1", "VIF_scale2", "VIF_scale3", "ADM2", "ADM_scale0", "ADM_scale1", "ADM_scale2", "ADM_scale3"]
    m = vp.extract_metrics_from_logs(str(pl), str(sl), log, "x", 23, 1000, "64x64", 30.0)
    assert list(m) == base + feats + ["MOTION2", "MOTION"] and "VMAF" not in m
    assert m["MOTION2"] == doc["pooled_metrics"]["motion2"]["mean"] and m["MOTION"] == doc["pooled_metrics"]["motion"]["mean"]
    assert list(vp.extract_metrics_from_logs(str(pl), str(sl), only, "x", 23, 1000, "64x64", 30.0)) == base + ["MOTION2", "MOTION"]
    # rows from logs without motion are what they were
    m0 = vp.extract_metrics_from_logs(str(pl), str(sl), old, "x", 23, 1000, "64x64", 30.0)
    assert list(m0) == base + feats and {k: m[k] for k in m0} == m0


def test_config_key_motion_feature_is_a_bool():
    vp.validate_config(dict(GOOD))
    vp.validate_config(dict(GOOD, motion_feature=True))
    vp.validate_config(dict(GOOD, motion_feature=False, vif=True, adm=True))
    vp.validate_config(dict(GOOD, motion_feature=True, motion="sad"))      # "motion" stays the complexity half's key
    for bad in (1, 0, "true", None, "yes"):
        with pytest.raises(ValueError) as e:
            vp.validate_config(dict(GOOD, motion_feature=bad))
        assert str(e.value) == "motion_feature must be true or false."


def test_the_stream_request():
    p = [(16, 16, 0, 16, 1)]
    assert stream.Quality(p).motion is False and stream.Quality(p, vif=True, adm=True).motion is False
    assert stream.Quality(p, motion=True).motion is True and stream.Quality(p, motion="only").motion == "only"
    assert stream.Quality(p, motion=True).ssim is True and stream.Quality(p, motion="only").ssim is False
    for bad in (1, "yes", None):
        with pytest.raises(ValueError):
            stream.Quality(p, motion=bad)
    with pytest.raises(ValueError):
        stream.Quality(p, N.SSIM_MS, scales=True, motion="only")
    z = np.zeros((0, 256), np.uint8)
    fields = ("sad", "motion", "motion2")
    # an empty clip: the tuple keeps its shape; the motion records come last, after the VIF and ADM places
    q, _ = stream.run(z, z, quality=stream.Quality(p, adm=True))
    assert len(q) == 4
    q, _ = stream.run(z, z, quality=stream.Quality(p, motion=True))
    assert len(q) == 5 and q[0].shape == (0, 1) and q[2] is None and q[3] is None and q[4].shape == (0, 1) and q[4].dtype.names == fields
    q, _ = stream.run(z, z, quality=stream.Quality(p, vif=True, adm=True, motion=True))
    assert len(q) == 5 and q[2].dtype.names == ("num", "den", "scale", "vif") and q[3].dtype.names == ("num", "den", "scale", "adm2")
    assert q[4].dtype.names == fields
    q, _ = stream.run(z, z, quality=stream.Quality(p, motion="only"))
    assert q[0] is None and q[1] is None and q[2] is None and q[3] is None and q[4].shape == (0, 1)
    q, _ = stream.run(z, z, quality=stream.Quality(p, N.SSIM_MS, scales=True, motion=True))
    assert len(q) == 7 and q[4] is None and q[5] is None and q[6].dtype.names == fields


@pytest.mark.parametrize("n,cap", [(10, 1), (10, 3), (10, 7), (10, 10), (10, 64), (1, 1), (65, 64)])
def test_the_plan_gives_the_reference_feed_a_halo_slot(n, cap):
    """with motion every chunk carries the reference frame before its first one in slot 0 of ITS OWN buffer: prev0 of chunk k is
    the last frame of chunk k - 1, never a pointer into that chunk's buffer set"""
    plain = stream.plan_chunks(n, True, None, 0, 0, cap)
    plans = stream.plan_chunks(n, True, None, 0, 0, cap, motion=True)
    assert len(plans) == len(plain) == -(-n // cap)
    assert stream.plan_chunks(n, True, None, 0, 0, cap, motion=False) == plain
    last = None
    for p, p0 in zip(plans, plain):
        assert "rslot" not in p0 and p0["rcopies"] == [(0, p0["q0"], p0["qn"], 1)]
        assert {k: v for k, v in p.items() if k not in ("rslot", "rhalo", "rcopies")} == {k: v for k, v in p0.items() if k != "rcopies"}
        assert p["rslot"] == 1
        body = (1, p["q0"], p["qn"], 1)
        if p["k"] == 0:
            assert p["q0"] == 0 and p["rhalo"] is False and p["rcopies"] == [body]
        else:
            assert p["rhalo"] is True and p["rcopies"] == [(0, last, 1, 1), body] and last == p["q0"] - 1
        last = p["q0"] + p["qn"] - 1
        assert max(slot + cnt for slot, _s, cnt, _t in p["rcopies"]) <= min(cap, n) + 1
    assert last == n - 1
    # the complexity half's halo and the split plans are untouched by the flag
    a = stream.plan_chunks(40, True, 4, 0, 9, 8, split=True)
    b = stream.plan_chunks(40, True, 4, 0, 9, 8, split=True, motion=True)
    for pa, pb in zip(a, b):
        assert pa["copies"] == pb["copies"] and pa["qcopies"] == pb["qcopies"] and pb["rslot"] == 1
