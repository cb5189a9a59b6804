"""Host: the float64 NumPy restatement of the VCA features (tests/vca_reference.py) pinned against SciPy's DCT and by
hand-computed answers, the quantised integer form against the plain form, an fp32 emulation of the device's two chains against
the bar, and the Python layers around the kernels - ABI, config key, log and row - through their stub paths.  No GPU."""
import ctypes as C
import json

import numpy as np
import pytest

import vca_cases as VC
import vca_reference as R
from rtvqa_amd import _native as N
from rtvqa_amd import stream
from rtvqa_amd import video_processing as vp

FIELDS = ("e_sum", "h_sum", "l_sum", "nbx", "nby", "e", "h", "l")
GOOD = {"crf": 23, "resize_width": 64, "resize_height": 64, "frame_interval": 10}


# ---- (a) the transform against SciPy ------------------------------------------------------------------------------------------
def test_the_transform_against_scipy():
    fft = pytest.importorskip("scipy.fft")
    rng = np.random.default_rng(1)
    for depth in (8, 10, 16):
        for _ in range(4):
            x = rng.integers(0, 1 << depth, (32, 32)).astype(np.float64)
            want = fft.dctn(x, type=2, norm="ortho")
            assert np.abs(R.dct_block(x) - want).max() <= 1e-12 * (1 << depth) * 32
    assert np.abs(R.T @ R.T.T - np.eye(32)).max() <= 1e-14                      # orthonormal
    assert R.T[0, 0] == np.sqrt(1.0 / 32.0) and abs(R.T[1, 0] - 0.25 * np.cos(np.pi / 64.0)) <= 1e-16


def test_the_weights():
    assert R.W[0, 0] == 0.0 and R.W[0, 1] == R.W[1, 0] == np.e                  # uv = 0: exp(1); the DC is left out
    assert R.W[31, 31] == np.exp(abs((961.0 / 1024.0) ** 2 - 1.0)) and (R.W == R.W.T).all()
    assert R.W[1:, 1:].min() >= 1.0 and R.W.max() == np.e


# ---- (b) hand answers ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", (8, 10, 12, 16))
def test_a_flat_block(depth):
    sc = 1.0 / (1 << (depth - 8))
    for v in (0, 1, 128 << (depth - 8), (1 << depth) - 1):
        f = R.features(np.full((1, 32, 32), v, np.int64), depth)
        assert abs(f["l"][0] - np.sqrt(32.0 * v * sc)) <= 1e-12 * max(1.0, f["l"][0])
        assert f["e"][0] <= R.bar(0.0) * 1e-6                                   # far within the bar of 0
        assert int(f["S"][0, 0, 0]) == 1024 * v
    # L_k = 64 for a flat 8-bit block of 128; the quantised form is within half a step of qL_k, 2^-25 sqrt(sc / 32)
    assert abs(R.features(np.full((1, 32, 32), 128, np.int64), 8, quantise=True)["l"][0] - 64.0) <= 2.0 ** -25 * np.sqrt(1.0 / 32.0)
    assert abs(R.features(np.full((1, 32, 32), 128, np.int64), 8)["l"][0] - 64.0) <= 64.0 * 2.0 ** -51


def test_one_cosine_lands_on_one_coefficient():
    u, v = 3, 5
    x = 40.0 * np.outer(R.T[u], R.T[v])                                          # D = 40 at (u, v), 0 elsewhere
    d = R.dct_block(x)
    assert abs(d[u, v] - 40.0) <= 1e-12 and np.abs(np.where(np.arange(32)[:, None] * 32 + np.arange(32) == u * 32 + v, 0, d)).max() <= 1e-12
    assert abs((np.abs(d) * R.W).sum() - 40.0 * np.exp(abs((15.0 / 1024.0) ** 2 - 1.0))) <= 1e-10


def test_a_remainder_strip_changes_nothing():
    rng = np.random.default_rng(2)
    big = rng.integers(0, 256, (2, 33, 65))
    a, b = R.features(big, 8, quantise=True), R.features(big[:, :32, :64], 8, quantise=True)
    assert R.grid(33, 65) == (1, 2) == R.grid(32, 64) and R.grid(1080, 1920) == (33, 60)
    for k in ("e_sum", "h_sum", "l_sum", "qh", "S"):
        assert np.array_equal(a[k], b[k]), k


def test_a_static_pair_and_the_symmetry_of_h():
    rng = np.random.default_rng(3)
    p, q = rng.integers(0, 1024, (2, 64, 96))
    for quantise in (False, True):
        assert R.features(np.stack([p, p]), 10, p, quantise)["h"].tolist() == [0.0, 0.0]
        ab, ba = R.features(np.stack([p, q]), 10, None, quantise), R.features(np.stack([q, p]), 10, None, quantise)
        assert ab["h"][0] == 0.0 and ab["h"][1] == ba["h"][1] > 0.0
        assert R.features(q[None], 10, p, quantise)["h"][0] == ab["h"][1]        # prev0 is the frame before


def test_every_depth_reads_on_the_8_bit_scale():
    rng = np.random.default_rng(4)
    x = rng.integers(0, 256, (2, 32, 64))
    base = R.features(x, 8, quantise=True)
    for depth in (10, 12, 16):
        f = R.features(x << (depth - 8), depth, quantise=True)
        for k in ("e", "h"):
            assert np.abs(f[k] - base[k]).max() <= 1e-6, (depth, k)             # (the quantum is the same 2^-16 on this scale)
        assert np.abs(f["l"] - base["l"]).max() <= 1e-6


# ---- (c) the integer words and the device's arithmetic ---------------------------------------------------------------------------
def _clips():
    for chroma, (h, w), depth in VC.SHAPES:
        for kind in VC.CONTENT:
            frames, prev0 = VC.clip(kind, 2, h, w, chroma, depth, seed=h + w + depth)
            for p in range(len(frames[0])):
                yield "%s %s %dx%d %d" % (kind, chroma, h, w, depth), np.stack([f[p] for f in frames]), prev0[p], depth


def test_the_quantised_form_stays_far_inside_the_bar_and_its_words_inside_their_bounds():
    for tag, stack, prev, depth in _clips():
        a, b = R.features(stack, depth, prev), R.features(stack, depth, prev, quantise=True)
        for k in ("e", "h", "l"):
            assert (np.abs(a[k] - b[k]) <= 0.01 * R.bar(a[k])).all(), (tag, k)
        assert b["qh"].max() < 1 << 37 and b["S"].max() < 1 << 26 and b["l_sum"].max() < 1 << 55


def _emulate(block, depth):
    """H_k as k_vca_blocks forms it: the block's rounded mean taken off, T and w in fp32, two fma chains of 32 terms in fp32 in
    ascending index order (the device permutes the order of the second; any fixed order has the same bound), |D| w summed in
    float64"""
    s = int(block.sum())
    x = (block - ((s + 512) >> 10)).astype(np.float32)
    t = R.T.astype(np.float32)
    p = np.zeros((32, 32), np.float32)
    for y in range(32):                              # P[x][u] += X[y][x] T[u][y]: the product is exact in the fma
        p = (p.astype(np.float64) + np.outer(x[y], t[:, y]).astype(np.float64)).astype(np.float32)
    d = np.zeros((32, 32), np.float32)
    for xx in range(32):                             # Dt[v][u] += T[v][x] P[x][u]
        d = (d.astype(np.float64) + np.outer(t[:, xx], p[xx]).astype(np.float64)).astype(np.float32)
    return float((np.abs(d.T).astype(np.float64) * R.W.astype(np.float32).astype(np.float64)).sum())


def test_an_fp32_emulation_of_the_device_chain_stays_inside_the_bar():
    worst = 0.0
    for tag, stack, _prev, depth in _clips():
        if stack.shape[1:] not in ((32, 32), (33, 65), (40, 72)):
            continue
        sc = 1.0 / (1 << (depth - 8))
        want = R.blocks(stack[0])[0] * sc / 1024.0
        nby, nbx = want.shape
        for by in range(nby):
            for bx in range(nbx):
                got = _emulate(stack[0][by * 32:by * 32 + 32, bx * 32:bx * 32 + 32], depth) * sc / 1024.0
                gap = abs(got - want[by, bx])
                worst = max(worst, gap / max(1.0, abs(want[by, bx])))
                assert gap <= 0.25 * R.bar(want[by, bx]), (tag, by, bx, gap)
    print("worst emulated gap / max(1, |value|): %.3e" % worst)


# ---- (d) the ABI -------------------------------------------------------------------------------------------------------------------
def test_the_additive_abi():
    from rtvqa_amd.engine import VCA_DTYPE
    assert N.VQA_ABI_VERSION == 8
    assert (N.K_FINIS, N.K_VCA_BLOCKS, N.K_VCA_SUM, N.K_CLOSE) == (38, 39, 40, 41)
    assert N.K_IDS_OPEN == N.K_IDS_SHOWN + (39, 40) and N.K_FINIS not in N.K_IDS_OPEN
    assert C.sizeof(N.VqaVcaMetrics) == 56 == VCA_DTYPE.itemsize and VCA_DTYPE.names == FIELDS
    assert [VCA_DTYPE.fields[k][1] for k in FIELDS] == [0, 8, 16, 24, 28, 32, 40, 48]
    assert [getattr(N.VqaVcaMetrics, k).offset for k in FIELDS] == [0, 8, 16, 24, 28, 32, 40, 48]
    for sym in ("vqa_vca_submit", "vqa_vca_wait"):
        assert sym in N.SIGNATURES
    lib = N.load()
    assert lib.vqa_abi_version() == 8
    lib.vqa_kernel_name.restype = C.c_char_p
    assert lib.vqa_kernel_name(39) == b"k_vca_blocks" and lib.vqa_kernel_name(40) == b"k_vca_sum"
    assert lib.vqa_kernel_name(38) == b"?" and lib.vqa_kernel_name(41) == b"?" and lib.vqa_kernel_name(36) == b"?"
    assert lib.vqa_kernel_name(37) == b"k_haarpsi"


def test_the_layout_rules_before_anything_is_uploaded():
    from rtvqa_amd.engine import bgr_planes, check_vca_planes, gray_planes, vca_grid, yuv_planes
    check_vca_planes(gray_planes(32, 32))
    check_vca_planes(yuv_planes(64, 96, "420", 10))
    for bad in (gray_planes(31, 64), gray_planes(64, 31), yuv_planes(62, 62, "420", 8), bgr_planes(64, 64)):
        with pytest.raises(ValueError):
            check_vca_planes(bad)
    assert vca_grid(1920, 1080) == (60, 33) and vca_grid(65, 33) == (2, 1)


# ---- (e) config, log and row ------------------------------------------------------------------------------------------------------
def test_config_key():
    vp.validate_config(dict(GOOD))
    vp.validate_config(dict(GOOD, vca=True))
    vp.validate_config(dict(GOOD, vca=False, haarpsi=True, xpsnr=True, vif=True))
    for bad in (1, 0, "true", None, "only"):
        with pytest.raises(ValueError) as e:
            vp.validate_config(dict(GOOD, vca=bad))
        assert str(e.value) == "vca must be true or false."


def _records(n):
    from rtvqa_amd.engine import VCA_DTYPE
    rec = np.zeros(n, VCA_DTYPE)
    rec["e"], rec["h"], rec["l"] = [52.5, 60.25, 40.0][:n], [0.0, 7.75, 20.25][:n], [64.0, 63.5, 65.5][:n]
    return rec


def test_the_json_log_and_what_the_row_takes_from_it(tmp_path):
    from rtvqa_amd.engine import HAARPSI_DTYPE
    hps = np.zeros(3, HAARPSI_DTYPE)
    hps["haarpsi"] = [0.875, 1.0, 0.25]
    vif = np.array([[0.5, 0.9, 0.95, 0.99], [0.7, 0.8, 0.97, 1.01], [0.6, 0.85, 0.96, 1.0]])
    rec = _records(3)
    old, log, only = str(tmp_path / "old.json"), str(tmp_path / "vmaf.json"), str(tmp_path / "vca.json")
    vp.write_vif_log(old, vif, haarpsi=hps)
    vp.write_vif_log(log, vif, haarpsi=hps, vca=rec)
    doc0, doc = json.load(open(old)), json.load(open(log))
    assert "vca" not in json.dumps(doc0)
    names0 = list(doc0["frames"][0]["metrics"])
    assert names0[-1] == "haarpsi"
    assert list(doc["frames"][1]["metrics"]) == names0 + ["vca_e", "vca_h", "vca_l"] == list(doc["pooled_metrics"])
    for i in range(3):
        m = doc["frames"][i]["metrics"]
        assert {k: m[k] for k in names0} == doc0["frames"][i]["metrics"]
        assert (m["vca_e"], m["vca_h"], m["vca_l"]) == (rec["e"][i], rec["h"][i], rec["l"][i])
    assert {k: doc["pooled_metrics"][k] for k in names0} == doc0["pooled_metrics"]
    p = doc["pooled_metrics"]["vca_h"]
    assert sorted(p) == ["harmonic_mean", "max", "mean", "min"]
    assert p["min"] == 0.0 and p["max"] == 20.25 and abs(p["mean"] - 28.0 / 3.0) <= 1e-14     # frame 0's 0 is included
    vp.write_vif_log(only, vca=rec)
    assert list(json.load(open(only))["frames"][0]["metrics"]) == ["vca_e", "vca_h", "vca_l"]
    pl, sl = tmp_path / "psnr.log", tmp_path / "ssim.log"
    pl.write_text("n:1 mse_avg:1.00 psnr_avg:48.13 \n")
    sl.write_text("n:1 Y:0.990000 All:0.990000 (20.000000)\n")
    m0 = vp.extract_metrics_from_logs(str(pl), str(sl), old, "x", 23, 1000, "64x64", 30.0)
    m = vp.extract_metrics_from_logs(str(pl), str(sl), log, "x", 23, 1000, "64x64", 30.0)
    assert list(m0)[-1] == "HAARPSI" and list(m) == list(m0) + ["VCA_E", "VCA_H", "VCA_L"]          # after HAARPSI
    assert {k: m[k] for k in m0} == m0 and abs(m["VCA_H"] - 28.0 / 3.0) <= 1e-14 and abs(m["VCA_L"] - 193.0 / 3.0) <= 1e-13
    base = ["Bitrate (kbps)", "Resolution (px)", "Frame Rate (fps)", "CRF", "PSNR", "SSIM"]
    assert list(vp.extract_metrics_from_logs(str(pl), str(sl), only, "x", 23, 1000, "64x64", 30.0)) == base + ["VCA_E", "VCA_H", "VCA_L"]
    # logs without the key are what they were, byte for byte
    again = str(tmp_path / "again.json")
    vp.write_vif_log(again, vif, haarpsi=hps, vca=None)
    assert open(again, "rb").read() == open(old, "rb").read()
    # the pass's tuple -> the log: the last element is VCA's [n, p], HaarPSI's the one before it
    from rtvqa_amd.engine import VIF_DTYPE
    v = np.zeros((3, 1), VIF_DTYPE)
    v["scale"][:, 0, :] = vif
    q = (None, None, v, hps[:, None], rec[:, None])
    vp._write_feature_log(again, q, dict(vif=True, adm=False, haarpsi=True, vca=True))
    assert open(again, "rb").read() == open(log, "rb").read()
    vp._write_feature_log(again, q[:-1], dict(vif=True, adm=False, haarpsi=True))
    assert open(again, "rb").read() == open(old, "rb").read()
    vp._write_feature_log(again, (None, None, rec[:, None]), dict(vif=False, adm=False, vca=True))
    assert open(again, "rb").read() == open(only, "rb").read()


def test_a_model_does_not_read_the_new_keys():
    from rtvqa_amd import vmaf_model

    class Model:
        features = ["vif_scale0", "adm2", "motion2"]

    x = vmaf_model.feature_matrix(Model, {"vif_scale0": [0.5, 0.7], "adm2": [0.9, 0.95], "motion2": [0.0, 1.0], "vca_e": [50.0, 60.0]})
    assert x.shape == (2, 3)


def test_the_stream_request():
    p = [(32, 32, 0, 32, 1), (32, 32, 1024, 32, 1), (32, 32, 2048, 32, 1)]
    every = dict(vif=True, adm=True, motion=True, siti=True, psnr_hvs=True, ciede=True, gmsd=True, cambi=True, xpsnr=True,
                 haarpsi=True)
    assert stream.Quality(p).vca is False and stream.Quality(p, **every).vca is False
    assert stream.Quality(p, vca=True).vca is True and stream.Quality(p, vca="only").vca == "only"
    assert stream.Quality(p, vca=True).ssim is True and stream.Quality(p, vca="only").ssim is False
    assert stream.Quality(p, vca=True).haarpsi is False
    for bad in (1, "yes", None):
        with pytest.raises(ValueError):
            stream.Quality(p, vca=bad)
    with pytest.raises(ValueError):
        stream.Quality(p, N.SSIM_MS, scales=True, vca="only")
    with pytest.raises(ValueError):
        stream.Quality([(31, 32, 0, 31, 1)], vca=True)                               # below one block
    with pytest.raises(ValueError):
        stream.Quality([(32, 32, c, 96, 3) for c in range(3)], vca=True)             # packed
    stream.Quality([(16, 16, 0, 16, 1)])                                             # (without the request nothing is checked)
    z = np.zeros((0, 3072), np.uint8)
    # an empty clip: without the request the tuples are what they were; with it ONE further last element, after HaarPSI's
    for kw, length in ((dict(), 2), (dict(vif=True), 3), (dict(haarpsi=True), 3), (dict(gmsd=True, haarpsi=True), 4), (every, 12)):
        q0, _ = stream.run(z, z, quality=stream.Quality(p, **kw))
        q1, _ = stream.run(z, z, quality=stream.Quality(p, vca=True, **kw))
        assert len(q0) == length and len(q1) == length + 1, kw
        assert q1[-1].shape == (0, 3) and q1[-1].dtype.names == FIELDS
        for a, b in zip(q0, q1):
            assert (a is None and b is None) or (a.dtype == b.dtype and a.shape == b.shape)
    q, _ = stream.run(z, z, quality=stream.Quality(p, vca="only", vca_blocks=True))
    assert len(q) == 3 and q[0] is None and q[1] is None
    rec, maps = q[2]
    assert rec.shape == (0, 3) and len(maps) == 3 and maps[0]["qh"].shape == (0, 1, 1) and maps[0]["s"].dtype == np.uint64
