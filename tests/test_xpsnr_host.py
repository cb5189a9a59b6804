"""Host: the NumPy restatement of XPSNR (tests/xpsnr_reference.py) pinned by hand-computed answers, the shared cases shown to
be non-vacuous, and the Python layers around the kernels - config key, layout refusals, log and row - through their stub paths.
No GPU."""
import ctypes as C
import json
import math

import numpy as np
import pytest

import xpsnr_cases as XC
import xpsnr_reference as R
from rtvqa_amd import _native as N
from rtvqa_amd import stream
from rtvqa_amd import video_processing as vp

FIELDS = ("sse", "wsse", "xpsnr", "block", "nbx", "nby")
GOOD = {"crf": 23, "resize_width": 64, "resize_height": 64, "frame_interval": 10}


# ---- (a) the block size ------------------------------------------------------------------------------------------------------
def test_block_sizes():
    from rtvqa_amd.engine import xpsnr_grid
    for (h, w), want in (((16, 16), 4), ((135, 241), 8), ((1080, 1920), 64), ((1154, 2050), 68), ((2160, 3840), 128)):
        assert R.block_size(w, h) == want, (h, w)
        assert xpsnr_grid(w, h) == (want, -(-w // want), -(-h // want))
    assert R.geometry(1920, 1080)["bv"] == 1 and R.geometry(2048, 1152)["bv"] == 1 and R.geometry(2050, 1154)["bv"] == 2
    # the size limits: 2^28 samples at 8 bits give B = 728 (the header's bound)
    assert R.block_size(16384, 16384) == 728


# ---- (b) a plane without activity: plain PSNR, shifted ---------------------------------------------------------------------------
def test_a_linear_ramp_has_no_activity():
    y, x = np.mgrid[0:16, 0:16]
    r = (x + y).astype(np.int64)
    rng = np.random.default_rng(1)
    d = r + rng.integers(1, 4, r.shape)
    out = R.frame([r], [d], None, 8)
    assert (out["sa"] == 0).all() and (out["ta"] == 0).all()
    a_min = 2.0 ** (8 - 6)
    assert out["act"] == [a_min] * 16
    avg = R.average(16, 16, 8)
    assert abs((out["xpsnr"][0] - R.psnr(r, d, 8)) - 10.0 * math.log10(a_min / avg)) <= 1e-12
    # the same at 10 bits: a_min and avg follow the depth
    out10 = R.frame([r * 4], [d * 4], None, 10)
    assert out10["act"] == [16.0] * 16
    assert abs((out10["xpsnr"][0] - R.psnr(r * 4, d * 4, 10)) - 10.0 * math.log10(16.0 / R.average(16, 16, 10))) <= 1e-12


# ---- (c) one isolated sample -------------------------------------------------------------------------------------------------------
def test_one_sample_on_a_block_corner():
    """a sample of height v at (8, 8) of a flat 16 x 16 field, the first sample of block (2, 2) at B = 4: |f| is 12 v at the
    sample, 2 v at its four edge neighbours and v at its four corner neighbours - 24 v in all, over the four blocks its
    3 x 3 footprint touches"""
    v = 7
    r = np.full((16, 16), 50, np.int64)
    r[8, 8] += v
    sa, ta = R.act_words(r, None)
    assert sa.shape == (4, 4) and int(sa.sum()) == 24 * v == 12 * v + 4 * 2 * v + 4 * v
    want = np.zeros((4, 4), np.int64)
    want[2, 2] = 12 * v + 2 * v + 2 * v + v     # (8, 8); (8, 9) and (9, 8); (9, 9)
    want[2, 1] = 2 * v + v                      # (8, 7); (9, 7)
    want[1, 2] = 2 * v + v                      # (7, 8); (7, 9)
    want[1, 1] = v                              # (7, 7)
    assert (sa == want).all() and (ta == 0).all()
    # against a flat predecessor: |G - Gp| = v at the one sample
    sa2, ta2 = R.act_words(r, np.full((16, 16), 50, np.int64))
    assert (sa2 == sa).all() and int(ta2[2, 2]) == v and int(ta2.sum()) == v


# ---- (d) the counts -----------------------------------------------------------------------------------------------------------------
def test_origin_counts():
    n = R.counts(16, 16)                        # B = 4: corner blocks lose a row and a column, edge blocks one of them
    assert n.tolist() == [[9, 12, 12, 9], [12, 16, 16, 12], [12, 16, 16, 12], [9, 12, 12, 9]]
    n = R.counts(67, 33)                        # B = 4: 17 x 9 blocks; the last block holds 3 columns (64..66), 1 row (32)
    assert n.shape == (9, 17) and int(n.sum()) == 65 * 31
    assert n[0, 0] == 9 and n[0, 1] == 12 and n[1, 1] == 16 and n[1, 16] == 4 * 2 and n[8, 0] == 0 and n[8, 16] == 0
    # above HD: G is 1025 x 577 for 2050 x 1154 and for 2051 x 1155 alike, 34 grid samples to a block
    for w, h in ((2050, 1154), (2051, 1155)):
        g = R.geometry(w, h)
        assert (g["B"], g["bv"], g["gw"], g["gh"], g["nbx"], g["nby"]) == (68, 2, 1025, 577, 31, 17)
        n = R.counts(w, h)
        assert int(n.sum()) == 1023 * 575
        assert n[0, 0] == 33 * 33 and n[0, 1] == 33 * 34 and n[1, 1] == 34 * 34
        assert n[0, 30] == 33 * (1025 - 30 * 34 - 1) and n[16, 30] == (577 - 16 * 34 - 1) * (1025 - 30 * 34 - 1)
    # a last block that holds only the ignored column: W = 2 * 34 * 31 + 1, no origin falls into block column 31
    w, h = 2 * 34 * 31 + 1, 1156
    g = R.geometry(w, h)
    assert g["B"] == 68 and g["nbx"] == 32 and g["gw"] == 34 * 31
    n = R.counts(w, h)
    assert (n[:, 31] == 0).all() and n[1, 30] == 34 * 33


# ---- (e) the shared cases are not vacuous ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(16, 16), (33, 67), (135, 241)], ids=["16x16", "33x67", "135x241"])
def test_the_shared_cases_exercise_the_weights(shape):
    h, w = shape
    ref, dist, prev0 = XC.clip(2, h, w, "mono", 8, seed=3)
    a_min = 4.0
    first = R.frame(ref[1], dist[1], None, 8)              # the clean frame, taken as one with no predecessor
    second = R.frame(ref[1], dist[1], ref[0][0], 8)        # the same frame after its predecessor
    for out in (first, second):
        a = np.array(out["act"])
        assert (a > a_min).sum() * 4 >= a.size             # at least a quarter of the blocks are weighted
        assert a.max() / a.min() >= 4.0
    assert (np.array(first["act"]) == a_min).any()         # a block at the floor
    assert (second["ta"] > 0).sum() * 2 > second["ta"].size   # temporal activity in most blocks
    assert first["xpsnr"][0] != R.psnr(ref[1][0], dist[1][0], 8)


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def test_the_additive_abi():
    from rtvqa_amd.engine import XPSNR_DTYPE
    assert N.VQA_ABI_VERSION == 8
    assert (N.K_TERMINUS, N.K_XPSNR_ACT, N.K_XPSNR_SSE, N.K_BOUND) == (33, 34, 35, 36)
    assert N.K_IDS_GIVEN == N.K_IDS_TOLD + (34, 35) and N.K_TERMINUS not in N.K_IDS_GIVEN
    assert C.sizeof(N.VqaXpsnrMetrics) == 40 == XPSNR_DTYPE.itemsize and XPSNR_DTYPE.names == FIELDS
    assert [XPSNR_DTYPE.fields[k][1] for k in FIELDS] == [0, 8, 16, 24, 28, 32]
    assert [getattr(N.VqaXpsnrMetrics, k).offset for k in FIELDS] == [0, 8, 16, 24, 28, 32]
    for sym in ("vqa_xpsnr_submit", "vqa_xpsnr_wait"):
        assert sym in N.SIGNATURES
    lib = N.load()
    lib.vqa_kernel_name.restype = C.c_char_p
    assert [lib.vqa_kernel_name(k) for k in (34, 35)] == [b"k_xpsnr_act", b"k_xpsnr_sse"]
    assert lib.vqa_kernel_name(33) == b"?" and lib.vqa_kernel_name(36) == b"?" and lib.vqa_kernel_name(32) == b"k_cambi_topk"


# ---- (f) config, refusals, log and row ---------------------------------------------------------------------------------------------
def test_config_key():
    vp.validate_config(dict(GOOD))
    vp.validate_config(dict(GOOD, xpsnr=True))
    vp.validate_config(dict(GOOD, xpsnr=False, cambi=True, gmsd=True, vif=True))
    for bad in (1, 0, "true", None, "only"):
        with pytest.raises(ValueError) as e:
            vp.validate_config(dict(GOOD, xpsnr=bad))
        assert str(e.value) == "xpsnr must be true or false."


def test_layouts_that_have_no_luma_grid_are_refused_before_any_upload(tmp_path):
    from rtvqa_amd.engine import bgr_planes, check_xpsnr_planes, yuv_planes
    for chroma in ("mono", "420", "422", "444"):
        for depth in (8, 10):
            check_xpsnr_planes(yuv_planes(33, 67, chroma, depth))
    with pytest.raises(ValueError):
        check_xpsnr_planes(bgr_planes(32, 32))
    with pytest.raises(ValueError):
        stream.Quality(bgr_planes(32, 32), xpsnr=True)
    # chroma of another ratio: a quarter wide, a third high, larger than the luma
    for cw, ch in ((16, 32), (64, 22), (128, 64)):
        with pytest.raises(ValueError):
            check_xpsnr_planes([(64, 64, 0, 64, 1), (cw, ch, 4096, cw, 1)])
    with pytest.raises(ValueError):
        check_xpsnr_planes(yuv_planes(30, 30, "420"))          # chroma planes of 15 x 15
    z = np.zeros((2, 32, 32, 3), np.uint8)
    logs = [str(tmp_path / k) for k in ("p.log", "s.log", "v.json")]
    with pytest.raises(ValueError):
        vp.run_ffmpeg_metrics(z, z, *logs, xpsnr=True)                           # bgr24
    with pytest.raises(ValueError):
        vp.frame_xpsnr(z, z, "bgr24")


def _records(n):
    from rtvqa_amd.engine import XPSNR_DTYPE
    rec = np.zeros(n, XPSNR_DTYPE)
    rec["xpsnr"] = [41.5, np.inf, 120.0][:n]
    return rec


def _cambi(n):
    from rtvqa_amd.engine import CAMBI_DTYPE
    rec = np.zeros(n, CAMBI_DTYPE)
    rec["cambi"] = [0.125, 0.0, 0.25][:n]
    return rec


def test_the_json_log_and_what_the_row_takes_from_it(tmp_path):
    from rtvqa_amd.engine import ADM_DTYPE, VIF_DTYPE
    vif = np.array([[0.5, 0.9, 0.95, 0.99], [0.7, 0.8, 0.97, 1.01], [0.6, 0.85, 0.96, 1.0]])
    adm = np.zeros(3, ADM_DTYPE)
    adm["adm2"], adm["scale"] = [0.9, 0.95, 0.85], 0.9
    rec, cam = _records(3), _cambi(3)
    old, log, only = str(tmp_path / "old.json"), str(tmp_path / "vmaf.json"), str(tmp_path / "xpsnr.json")
    vp.write_vif_log(old, vif, adm, cambi=cam)
    vp.write_vif_log(log, vif, adm, cambi=cam, xpsnr=rec)
    doc0, doc = json.load(open(old)), json.load(open(log))
    assert "xpsnr" not in json.dumps(doc0)
    names0 = list(doc0["frames"][0]["metrics"])
    assert names0[-1] == "cambi"
    assert list(doc["frames"][1]["metrics"]) == names0 + ["xpsnr"] == list(doc["pooled_metrics"])     # after cambi
    capped = [41.5, 100.0, 100.0]                                                                     # min(value, 100.0)
    for i in range(3):
        m = doc["frames"][i]["metrics"]
        assert {k: m[k] for k in names0} == doc0["frames"][i]["metrics"] and m["xpsnr"] == capped[i]
    assert {k: doc["pooled_metrics"][k] for k in names0} == doc0["pooled_metrics"]
    p = doc["pooled_metrics"]["xpsnr"]
    assert sorted(p) == ["harmonic_mean", "max", "mean", "min"]
    assert p["min"] == 41.5 and p["max"] == 100.0 and abs(p["mean"] - np.mean(capped)) <= 1e-13
    vp.write_vif_log(only, xpsnr=rec)
    assert list(json.load(open(only))["frames"][0]["metrics"]) == ["xpsnr"]
    pl, sl = tmp_path / "psnr.log", tmp_path / "ssim.log"
    pl.write_text("n:1 mse_avg:1.00 psnr_avg:48.13 \n")
    sl.write_text("n:1 Y:0.990000 All:0.990000 (20.000000)\n")
    m0 = vp.extract_metrics_from_logs(str(pl), str(sl), old, "x", 23, 1000, "64x64", 30.0)
    m = vp.extract_metrics_from_logs(str(pl), str(sl), log, "x", 23, 1000, "64x64", 30.0)
    assert list(m0)[-1] == "CAMBI" and list(m) == list(m0) + ["XPSNR"]                                # after CAMBI
    assert {k: m[k] for k in m0} == m0 and abs(m["XPSNR"] - np.mean(capped)) <= 1e-13
    base = ["Bitrate (kbps)", "Resolution (px)", "Frame Rate (fps)", "CRF", "PSNR", "SSIM"]
    assert list(vp.extract_metrics_from_logs(str(pl), str(sl), only, "x", 23, 1000, "64x64", 30.0)) == base + ["XPSNR"]
    # logs without the key are what they were, byte for byte
    again = str(tmp_path / "again.json")
    vp.write_vif_log(again, vif, adm, cambi=cam, xpsnr=None)
    assert open(again, "rb").read() == open(old, "rb").read()
    # the pass's tuple -> the log: the last element is XPSNR's [n, p], CAMBI's the one before it
    v = np.zeros((3, 1), VIF_DTYPE)
    v["scale"][:, 0, :] = vif
    q = (None, None, v, adm[:, None], cam[:, None], rec[:, None])
    vp._write_feature_log(again, q, dict(vif=True, adm=True, motion=False, siti=False, psnr_hvs=False, ciede=False, gmsd=False, cambi=True, xpsnr=True))
    assert open(again, "rb").read() == open(log, "rb").read()
    vp._write_feature_log(again, q[:-1], dict(vif=True, adm=True, motion=False, siti=False, psnr_hvs=False, ciede=False, gmsd=False, cambi=True))
    assert open(again, "rb").read() == open(old, "rb").read()
    vp._write_feature_log(again, (None, None, rec[:, None]), dict(vif=False, adm=False, motion=False, siti=False, psnr_hvs=False, ciede=False, gmsd=False, cambi=False, xpsnr=True))
    assert open(again, "rb").read() == open(only, "rb").read()


def test_a_model_does_not_read_the_new_key():
    from rtvqa_amd import vmaf_model

    class Model:
        features = ["vif_scale0", "adm2", "motion2"]

    x = vmaf_model.feature_matrix(Model, {"vif_scale0": [0.5, 0.7], "adm2": [0.9, 0.95], "motion2": [0.0, 1.0], "xpsnr": [40.0, 41.0]})
    assert x.shape == (2, 3)


def test_the_stream_request():
    p = [(16, 16, 0, 16, 1), (16, 16, 256, 16, 1), (16, 16, 512, 16, 1)]
    every = dict(vif=True, adm=True, motion=True, siti=True, psnr_hvs=True, ciede=True, gmsd=True, cambi=True)
    assert stream.Quality(p).xpsnr is False and stream.Quality(p, **every).xpsnr is False
    assert stream.Quality(p, xpsnr=True).xpsnr is True and stream.Quality(p, xpsnr="only").xpsnr == "only"
    assert stream.Quality(p, xpsnr=True).ssim is True and stream.Quality(p, xpsnr="only").ssim is False
    assert stream.Quality(p, xpsnr=True).cambi is False
    for bad in (1, "yes", None):
        with pytest.raises(ValueError):
            stream.Quality(p, xpsnr=bad)
    with pytest.raises(ValueError):
        stream.Quality(p, N.SSIM_MS, scales=True, xpsnr="only")
    z = np.zeros((0, 768), np.uint8)
    # an empty clip: without the request the tuples are what they were; with it ONE further last element, after CAMBI's
    for kw, length in ((dict(), 2), (dict(vif=True), 3), (dict(cambi=True), 3), (dict(gmsd=True, cambi=True), 4), (every, 10)):
        q0, _ = stream.run(z, z, quality=stream.Quality(p, **kw))
        q1, _ = stream.run(z, z, quality=stream.Quality(p, xpsnr=True, **kw))
        assert len(q0) == length and len(q1) == length + 1, kw
        assert q1[-1].shape == (0, 3) and q1[-1].dtype.names == FIELDS
        for a, b in zip(q0, q1):
            assert (a is None and b is None) or (a.dtype == b.dtype and a.shape == b.shape)
    q, _ = stream.run(z, z, quality=stream.Quality(p, xpsnr="only"))
    assert len(q) == 3 and q[0] is None and q[1] is None and q[2].shape == (0, 3)
    # the request asks for the reference feed's halo, as motion and siti do
    plain = stream.plan_chunks(10, True, None, 0, 0, 4, False, motion=False)
    halo = stream.plan_chunks(10, True, None, 0, 0, 4, False, motion=True)
    assert "rhalo" not in plain[1] and halo[1]["rhalo"] is True and halo[0]["rhalo"] is False
