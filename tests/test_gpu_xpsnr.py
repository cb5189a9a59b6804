"""GPU: XPSNR (vqa_xpsnr_submit / vqa_xpsnr_wait) through the C ABI, the engine, the one-pass stream and the reference-shaped
entry points, against the NumPy restatement of tests/xpsnr_reference.py (written from the definition in include/vqa.h).

The bars were fixed before the kernels first ran.  Everything the device produces is an integer: every word of the weight map
(sa, ta, n per block, sse per plane and block) is EQUAL to the restatement's.  wsse is a sum of nbx nby positive terms, each one
division of exactly converted integers, added in ascending k and scaled once: one rounding per division, per add and per scale,
all terms positive, so the host and the restatement - which do the same operations in the same order - may differ by at most
(nbx nby + 4) 2^-53 relative (in practice they are equal).  xpsnr is within 1e-12 dB: the logarithms are two libraries'."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import xpsnr_cases as XC
import xpsnr_reference as R

pytestmark = pytest.mark.gpu

FIELDS = ("sse", "wsse", "xpsnr", "block", "nbx", "nby")
MATRIX = XC.matrix()


def _planes(h, w, chroma, depth):
    from rtvqa_amd.engine import yuv_planes
    return yuv_planes(h, w, chroma, depth)


def _check(rec, blk, ref, dist, prev0, depth, tag):
    """rec [n, p], blk: the map of xpsnr_wait; ref / dist: lists of frames (lists of planes); prev0: planes or None"""
    n, npl = rec.shape
    h, w = ref[0][0].shape
    g = R.geometry(w, h)
    nb = g["nbx"] * g["nby"]
    for i in range(n):
        prev = ref[i - 1][0] if i > 0 else (prev0[0] if prev0 is not None else None)
        want = R.frame(ref[i], dist[i], prev, depth)
        assert (blk["sa"][i].astype(np.int64) == want["sa"]).all(), (tag, i, "sa")
        assert (blk["ta"][i].astype(np.int64) == want["ta"]).all(), (tag, i, "ta")
        assert (blk["n"][i].astype(np.int64) == want["n"]).all(), (tag, i, "n")
        assert (blk["sse"][i].astype(np.int64) == want["sse"]).all(), (tag, i, "sse")
        a = np.array(want["act"]).reshape(g["nby"], g["nbx"])
        raised = np.maximum(blk["act"][i], 2.0 ** (depth - 6))
        assert (np.where(want["n"] > 0, raised, 2.0 ** (depth - 6)) == a).all(), (tag, i, "act")
        for p in range(npl):
            r = rec[i, p]
            assert (int(r["block"]), int(r["nbx"]), int(r["nby"])) == (g["B"], g["nbx"], g["nby"])
            assert int(r["sse"]) == want["total"][p], (tag, i, p)
            gap = abs(float(r["wsse"]) - want["wsse"][p])
            print("%s frame %d plane %d xpsnr %.12f (ref %.12f) wsse gap %.2e rel" % (tag, i, p, r["xpsnr"], want["xpsnr"][p],
                                                                                      gap / max(want["wsse"][p], 1e-300)))
            assert gap <= (nb + 4) * 2.0 ** -53 * want["wsse"][p], (tag, i, p, gap)
            if math.isinf(want["xpsnr"][p]):
                assert float(r["wsse"]) == 0.0 and math.isinf(float(r["xpsnr"])) and r["xpsnr"] > 0
            else:
                assert abs(float(r["xpsnr"]) - want["xpsnr"][p]) <= 1e-12, (tag, i, p)


@pytest.mark.parametrize("chroma,shape,depth", MATRIX, ids=["%s-%dx%d-%d" % (c, s[0], s[1], d) for c, s, d in MATRIX])
def test_every_word_on_every_shape_layout_and_depth(engine, chroma, shape, depth):
    h, w = shape
    ref, dist, prev0 = XC.clip(2, h, w, chroma, depth, seed=h + w + depth)
    planes = _planes(h, w, chroma, depth)
    r, d, p0 = XC.pack(ref, depth), XC.pack(dist, depth), XC.pack([prev0], depth)
    rec, blk = engine.xpsnr(r, d, planes, prev0=p0, blocks=True)
    assert rec.dtype.names == FIELDS and rec.shape == (2, len(planes))
    _check(rec, blk, ref, dist, prev0, depth, "%s %dx%d %d bits" % (chroma, h, w, depth))
    assert (blk["ta"][0] > 0).any() and (blk["ta"][1] > 0).any()
    # without a predecessor: frame 0's ta is 0, every other word as before
    rec0, blk0 = engine.xpsnr(r, d, planes, blocks=True)
    _check(rec0, blk0, ref, dist, None, depth, "no prev0")
    assert (blk0["ta"][0] == 0).all() and (blk0["sa"] == blk["sa"]).all() and rec0[1].tobytes() == rec[1].tobytes()
    assert engine.xpsnr(r, d, planes, prev0=p0).tobytes() == rec.tobytes()          # without the map: the same records


@pytest.mark.parametrize("shape,depth", [(XC.BIG_SHAPES[0], 8), (XC.BIG_SHAPES[1], 8), (XC.BIG_SHAPES[1], 10)],
                         ids=["1154x2050-8", "1155x2051-8", "1155x2051-10"])
def test_the_two_by_two_path_above_hd(engine, shape, depth):
    """B = 68 is 34 on the activity grid: blocks cut across the 64 x 32 tiles; the odd plane's last row and column are ignored"""
    h, w = shape
    ref, dist, prev0 = XC.clip(2, h, w, "mono", depth, seed=h + depth)
    planes = _planes(h, w, "mono", depth)
    rec, blk = engine.xpsnr(XC.pack(ref, depth), XC.pack(dist, depth), planes, prev0=XC.pack([prev0], depth), blocks=True)
    assert int(rec[0, 0]["block"]) == 68 and blk["sa"].shape == (2, 17, 31)
    _check(rec, blk, ref, dist, prev0, depth, "%dx%d %d bits" % (h, w, depth))


def test_identical_pairs_and_the_range_ends(engine):
    for depth in XC.DEPTHS:
        h, w = XC.SMALL
        ref, _dist, prev0 = XC.clip(1, h, w, "444", depth, seed=depth)
        planes = _planes(h, w, "444", depth)
        r = XC.pack(ref, depth)
        rec, blk = engine.xpsnr(r, r, planes, prev0=XC.pack([prev0], depth), blocks=True)
        assert (rec["sse"] == 0).all() and (rec["wsse"] == 0.0).all() and np.isposinf(rec["xpsnr"]).all()
        assert (blk["sse"] == 0).all() and (blk["sa"] > 0).any()
        _check(rec, blk, ref, ref, prev0, depth, "identical %d bits" % depth)
        # flat 0 against flat peak: no activity, every a_k = a_min, the largest squared error there is
        peak = (1 << depth) - 1
        zero, full = [[np.zeros((h, w), np.int64)]], [[np.full((h, w), peak, np.int64)]]
        mono = _planes(h, w, "mono", depth)
        rec, blk = engine.xpsnr(XC.pack(zero, depth), XC.pack(full, depth), mono, blocks=True)
        assert (blk["sa"] == 0).all() and (blk["ta"] == 0).all() and int(rec[0, 0]["sse"]) == h * w * peak * peak
        _check(rec, blk, zero, full, None, depth, "ends %d bits" % depth)
        rec, blk = engine.xpsnr(XC.pack(full, depth), XC.pack(zero, depth), mono, prev0=XC.pack(zero, depth), blocks=True)
        _check(rec, blk, full, zero, zero[0], depth, "ends with prev %d bits" % depth)
        assert (blk["ta"].astype(np.int64) == blk["n"].astype(np.int64) * peak).all()


def _same(a, b):
    return a[0].tobytes() == b[0].tobytes() and all(np.array_equal(a[1][k], b[1][k]) for k in ("sa", "ta", "n", "sse"))


def test_batches_positions_prev0_and_memory_kinds_give_the_same_words(engine):
    h, w = XC.YUV_SHAPE
    ref, dist, prev0 = XC.clip(5, h, w, "420", 8, seed=11)
    planes = _planes(h, w, "420", 8)
    r, d, p0 = XC.pack(ref, 8), XC.pack(dist, 8), XC.pack([prev0], 8)
    whole = engine.xpsnr(r, d, planes, prev0=p0, blocks=True)
    assert _same(engine.xpsnr(r, d, planes, prev0=p0, blocks=True), whole)                      # run to run
    _check(whole[0], whole[1], ref, dist, prev0, 8, "batch of 5")

    def one(k, got, pos):
        return got[0][pos].tobytes() == whole[0][k].tobytes() and all(
            np.array_equal(got[1][key][pos], whole[1][key][k]) for key in ("sa", "ta", "n", "sse"))

    # a pair alone, its predecessor given explicitly: the words it has in the batch, where the predecessor is in the batch
    for k in (0, 2, 4):
        pk = p0 if k == 0 else r[k - 1:k]
        assert one(k, engine.xpsnr(r[k:k + 1], d[k:k + 1], planes, prev0=pk, blocks=True), 0), k
    # first, in the middle and last in a batch of 5, frame 1 before it each time (as prev0, or as the frame in front of it)
    for pos, order in ((0, [2, 0, 1, 3, 4]), (2, [0, 1, 2, 3, 4]), (4, [0, 3, 4, 1, 2])):
        assert order[pos] == 2 and (pos == 0 or order[pos - 1] == 1)
        assert one(2, engine.xpsnr(r[order], d[order], planes, prev0=r[1:2], blocks=True), pos), order
    # device and pinned memory
    dr, dd, dp = engine.upload(r), engine.upload(d), engine.upload(p0)
    assert _same(engine.xpsnr(dr, dd, planes, prev0=dp, blocks=True), whole)
    assert one(2, engine.xpsnr(dr.slice(2, 3), dd.slice(2, 3), planes, prev0=dr.frame(1), blocks=True), 0)
    pr, pd, pp = engine.alloc_pinned(r.shape), engine.alloc_pinned(d.shape), engine.alloc_pinned(p0.shape)
    pr[...], pd[...], pp[...] = r, d, p0
    assert engine.is_pinned(pr)
    assert _same(engine.xpsnr(pr, pd, planes, prev0=pp, blocks=True), whole)
    for a in (pr, pd, pp):
        engine.free_pinned(a)
    with pytest.raises(TypeError):
        engine.xpsnr(dr, dd, planes, prev0=p0)                                                     # prev0 lives elsewhere


def _submit(engine, f, d, planes, prev0=None):
    from rtvqa_amd import _native as N
    from rtvqa_amd.engine import plane_descs
    fb = f.shape[1] * f.dtype.itemsize
    return engine.lib.vqa_xpsnr_submit(engine.ctx, f.ctypes.data, d.ctypes.data, prev0.ctypes.data if prev0 is not None else None,
                                       N.VQA_MEM_HOST, f.shape[0], fb, fb, plane_descs(planes), len(planes))


def test_the_state_machine_and_the_refusals(engine):
    from rtvqa_amd import _native as N
    from rtvqa_amd.engine import bgr_planes, gray_planes, plane_descs, yuv420p_planes
    h, w = 64, 96
    ref, dist, prev0 = XC.clip(2, h, w, "420", 8, seed=8)
    planes = _planes(h, w, "420", 8)
    f, d, p0 = XC.pack(ref, 8), XC.pack(dist, 8), XC.pack([prev0], 8)
    want, bwant = engine.xpsnr(f, d, planes, prev0=p0, blocks=True)
    gwant, qwant = engine.gmsd(f, d, planes), engine.quality(f, d, planes)
    nb = int(want[0, 0]["nbx"]) * int(want[0, 0]["nby"])
    nwords = 2 * nb * (3 + 3)
    xout, gout, qout = (N.VqaXpsnrMetrics * 6)(), (N.VqaGmsdMetrics * 6)(), (N.VqaPlaneMetrics * 6)()
    sout, words = (N.VqaSitiMetrics * 6)(), (C.c_uint64 * nwords)()
    lib, ctx = engine.lib, engine.ctx
    assert lib.vqa_xpsnr_wait(ctx, xout, 6, None, 0) == N.VQA_ERR_STATE              # wait without submit
    assert _submit(engine, f, d, planes, p0) == N.VQA_OK
    assert _submit(engine, f, d, planes, p0) == N.VQA_ERR_STATE                      # submit while pending
    assert lib.vqa_quality_wait(ctx, qout, 6) == N.VQA_ERR_STATE                     # a wait of another kind
    assert lib.vqa_gmsd_wait(ctx, gout, 6) == N.VQA_ERR_STATE
    assert lib.vqa_siti_wait(ctx, sout, 6) == N.VQA_ERR_STATE
    assert lib.vqa_trim(ctx) == N.VQA_ERR_STATE
    assert lib.vqa_xpsnr_wait(ctx, xout, 5, None, 0) == N.VQA_ERR_STATE              # a wrong entry count
    for bad in (nwords - 1, nwords + 1, 0, nb):                                      # a wrong n_block_words: the batch survives
        assert lib.vqa_xpsnr_wait(ctx, xout, 6, words, bad) == N.VQA_ERR_INVALID
    assert lib.vqa_xpsnr_wait(ctx, xout, 6, words, nwords) == N.VQA_OK
    assert bytes(xout) == want.tobytes()
    got = np.frombuffer(words, np.uint64).reshape(2, 6 * nb)
    tri = got[:, :3 * nb].reshape(2, -1, 3)
    assert np.array_equal(tri[..., 0], bwant["sa"].reshape(2, -1)) and np.array_equal(tri[..., 1], bwant["ta"].reshape(2, -1))
    assert np.array_equal(tri[..., 2], bwant["n"].reshape(2, -1)) and np.array_equal(got[:, 3 * nb:], bwant["sse"].reshape(2, -1))
    assert lib.vqa_xpsnr_wait(ctx, xout, 6, None, 0) == N.VQA_ERR_STATE
    # the converse: an XPSNR wait with only a GMSD or a quality batch pending; each survives
    fb = f.shape[1]
    pd = plane_descs(planes)
    assert lib.vqa_gmsd_submit(ctx, f.ctypes.data, d.ctypes.data, N.VQA_MEM_HOST, 2, fb, fb, pd, 3) == N.VQA_OK
    assert lib.vqa_xpsnr_wait(ctx, xout, 6, None, 0) == N.VQA_ERR_STATE
    assert lib.vqa_gmsd_wait(ctx, gout, 6) == N.VQA_OK and bytes(gout) == gwant.tobytes()
    # in flight next to a quality, a GMSD and an SI/TI batch from one upload: each wait collects its own, in any order
    df, dd, dp = engine.upload(f), engine.upload(d), engine.upload(p0)
    swant = engine.siti(df, planes, dp)
    for order in (("xpsnr", "quality", "gmsd", "siti"), ("siti", "gmsd", "xpsnr", "quality")):
        engine.quality_submit(df, dd, planes)
        engine.siti_submit(df, planes, dp)
        engine.xpsnr_submit(df, dd, planes, dp)
        engine.gmsd_submit(df, dd, planes)
        wants = {"xpsnr": want, "quality": qwant, "gmsd": gwant, "siti": swant}
        for kind in order:
            assert getattr(engine, kind + "_wait")().tobytes() == wants[kind].tobytes(), (order, kind)
    engine.xpsnr_submit(df, dd, planes, dp)
    engine.drain()                                                                   # a pending batch is waited out
    assert lib.vqa_xpsnr_wait(ctx, xout, 6, None, 0) == N.VQA_ERR_STATE
    # planes below 16, packed BGR, chroma of another ratio: a failed submit leaves nothing in flight
    for hh, ww in ((15, 16), (16, 15)):
        z = np.zeros((2, hh * ww), np.uint8)
        assert _submit(engine, z, z, gray_planes(hh, ww)) == N.VQA_ERR_UNSUPPORTED, (hh, ww)
        assert lib.vqa_xpsnr_wait(ctx, xout, 2, None, 0) == N.VQA_ERR_STATE
    z = np.zeros((1, 30 * 30 * 3 // 2), np.uint8)                                    # 4:2:0 at 30: the chroma planes are 15
    assert _submit(engine, z, z, yuv420p_planes(30, 30)) == N.VQA_ERR_UNSUPPORTED
    z = np.zeros((1, 32 * 32 * 3), np.uint8)
    assert _submit(engine, z, z, bgr_planes(32, 32)) == N.VQA_ERR_UNSUPPORTED        # bgr24
    z = np.zeros((1, 64 * 64 + 16 * 32), np.uint8)
    assert _submit(engine, z, z, [(64, 64, 0, 64, 1), (16, 32, 4096, 16, 1)]) == N.VQA_ERR_UNSUPPORTED   # a quarter wide
    small = np.zeros((1, 64), np.uint8)                                              # more than 2^28 samples: a descriptor check
    assert _submit(engine, small, small, [(16385, 16384, 0, 16385, 1)]) == N.VQA_ERR_UNSUPPORTED
    assert lib.vqa_xpsnr_submit(ctx, f.ctypes.data, None, None, N.VQA_MEM_HOST, 2, fb, fb, pd, 3) == N.VQA_ERR_INVALID
    assert lib.vqa_xpsnr_submit(ctx, f.ctypes.data, d.ctypes.data, None, N.VQA_MEM_HOST, 2, fb - 1, fb, pd, 3) == N.VQA_ERR_INVALID
    z8 = np.zeros((1, 32 * 32 * 3), np.uint8)
    with pytest.raises(ValueError):
        engine.xpsnr(z8, z8, bgr_planes(32, 32))
    with pytest.raises(ValueError):
        engine.xpsnr(z8[:, :1024], z8[:, :1024], _planes(32, 32, "mono", 10))         # a dtype that does not match the depth
    # nothing is pending and the ctx computes as before; trim gives the feature's buffers back and it re-grows them
    assert lib.vqa_xpsnr_wait(ctx, xout, 6, None, 0) == N.VQA_ERR_STATE
    engine.trim()
    assert engine.xpsnr(f, d, planes, prev0=p0).tobytes() == want.tobytes()
    assert engine.quality(f, d, planes).tobytes() == qwant.tobytes()


def test_one_pass_entry_points(tmp_path):
    """frame_xpsnr at two batch sizes whose chunk seams fall inside the clip (frame q0 of a later chunk sees frame q0 - 1),
    run_ffmpeg_metrics(.., xpsnr=True) and config "xpsnr": true on a 6-frame 135 x 241 .y4m pair: the psnr / ssim logs are
    byte for byte those of a plain run, the log's values are the pooled restatement's, and the row gains XPSNR after CAMBI"""
    import rtvqa_amd
    from rtvqa_amd import frames, synth
    from rtvqa_amd import video_processing as vp
    (h, w), n = XC.YUV_SHAPE, 6
    ref, dist, _prev0 = XC.clip(n, h, w, "420", 8, seed=6)
    dist[2] = ref[2]                                             # one identical frame: inf in the record, 100.0 in the log
    planes = _planes(h, w, "420", 8)
    r, d = XC.pack(ref, 8), XC.pack(dist, 8)
    want = [R.frame(ref[i], dist[i], ref[i - 1][0] if i else None, 8) for i in range(n)]
    with rtvqa_amd.Engine(0) as eng:
        whole = eng.xpsnr(r, d, planes)
    for i in range(n):
        for p in range(3):
            if i == 2:
                assert np.isposinf(whole["xpsnr"][i, p])
            else:
                assert abs(whole["xpsnr"][i, p] - want[i]["xpsnr"][p]) <= 1e-12
    for bs in (2, 4):
        x, ws, sizes, block = vp.frame_xpsnr(r, d, "yuv420p", h, w, batch_size=bs)
        assert x.shape == (n, 3) and sizes == [(q[0], q[1]) for q in planes] and block == 8
        assert x.tobytes() == np.ascontiguousarray(whole["xpsnr"]).tobytes(), bs
        assert ws.tobytes() == np.ascontiguousarray(whole["wsse"]).tobytes(), bs
    pr, pd = str(tmp_path / "ref.y4m"), str(tmp_path / "enc.y4m")
    frames.write_y4m(pr, r, h, w)
    frames.write_y4m(pd, d, h, w)
    logs = {k: [str(tmp_path / ("%s_%s.log" % (k, t))) for t in ("psnr", "ssim", "vmaf")] for k in ("plain", "xpsnr", "feat", "both")}
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["plain"], batch_size=4) is None
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["xpsnr"], batch_size=4, xpsnr=True) is None
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["feat"], batch_size=4, gmsd=True, cambi=True) is None
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["both"], batch_size=2, gmsd=True, cambi=True, xpsnr=True) is None
    assert not os.path.exists(logs["plain"][2])
    for k in (0, 1):
        for kind in ("xpsnr", "feat", "both"):
            assert open(logs["plain"][k], "rb").read() == open(logs[kind][k], "rb").read(), (kind, k)
    doc, feat, both = (json.load(open(logs[k][2])) for k in ("xpsnr", "feat", "both"))
    assert list(doc["frames"][0]["metrics"]) == ["xpsnr"] == list(doc["pooled_metrics"])
    names = list(feat["frames"][0]["metrics"])
    assert names[-1] == "cambi" and "xpsnr" not in json.dumps(feat)
    assert list(both["frames"][0]["metrics"]) == names + ["xpsnr"]
    capped = [min(want[i]["xpsnr"][0], 100.0) for i in range(n)]
    assert capped[2] == 100.0
    for i in range(n):
        for dc in (doc, both):
            assert abs(dc["frames"][i]["metrics"]["xpsnr"] - capped[i]) <= 1e-12
            assert dc["frames"][i]["metrics"]["xpsnr"] == min(float(whole["xpsnr"][i, 0]), 100.0)
        assert {k: both["frames"][i]["metrics"][k] for k in names} == feat["frames"][i]["metrics"]
    assert {k: both["pooled_metrics"][k] for k in names} == feat["pooled_metrics"]
    assert abs(doc["pooled_metrics"]["xpsnr"]["mean"] - np.mean(capped)) <= 1e-12
    bgr = synth.s_natural(n, h, w, seed=12)
    cfg = {"crf": 23, "resize_width": 64, "resize_height": 64, "frame_interval": 1, "batch_size": 4}

    def row(name, **kw):
        return vp.process_video_and_extract_metrics(pr, pd, dict(cfg, **kw), csv_file=str(tmp_path / (name + ".csv")),
                                                    column_order="fixed", encoded_bgr=bgr)

    def same(a, b):
        return a == b or (a != a and b != b)

    # no other feature key: XPSNR is the only added column, right after SSIM (row3 below has it after CAMBI)
    row0, row1 = row("row0"), row("row1", xpsnr=True)
    k0 = list(row0)
    at = k0.index("SSIM") + 1
    assert list(row1) == k0[:at] + ["XPSNR"] + k0[at:] and all(same(row0[k], row1[k]) for k in k0)
    assert abs(row1["XPSNR"] - np.mean(capped)) <= 1e-12
    row2, row3 = row("row2", cambi=True, batch_size=2), row("row3", cambi=True, xpsnr=True, batch_size=2)
    k2 = list(row2)
    at = k2.index("CAMBI") + 1
    assert list(row3) == k2[:at] + ["XPSNR"] + k2[at:] and all(same(row2[k], row3[k]) for k in k2)
    assert row3["XPSNR"] == row1["XPSNR"]
    # the same call without the key, and with it false: the same file, byte for byte, with no new column
    row("row0b", xpsnr=False)
    assert open(str(tmp_path / "row0.csv"), "rb").read() == open(str(tmp_path / "row0b.csv"), "rb").read()
    assert b"XPSNR" not in open(str(tmp_path / "row0.csv"), "rb").read()
    assert b"CAMBI,XPSNR" in open(str(tmp_path / "row3.csv"), "rb").read()
    with pytest.raises(ValueError):
        vp.frame_xpsnr(bgr, bgr, "bgr24")


def test_profile_counts_one_launch_for_the_luma_and_one_per_plane_group():
    import rtvqa_amd
    from rtvqa_amd import _native as N
    h, w = XC.YUV_SHAPE
    ref, dist, _p = XC.clip(3, h, w, "420", 8, seed=9)
    planes = _planes(h, w, "420", 8)
    f, d = XC.pack(ref, 8), XC.pack(dist, 8)
    with rtvqa_amd.Engine(0) as eng:
        eng.lib.vqa_kernel_name.restype = C.c_char_p
        assert eng.lib.vqa_kernel_name(N.K_XPSNR_ACT) == b"k_xpsnr_act" and eng.lib.vqa_kernel_name(N.K_XPSNR_SSE) == b"k_xpsnr_sse"
        eng.profile(True)
        eng.xpsnr(f, d, planes)
        prof = eng.profile_read(reset=True)
        assert prof["k_xpsnr_act"][1] == 1 and prof["k_xpsnr_sse"][1] == 2 and "k_siti" not in prof and "k_gmsd" not in prof, prof
        assert prof["k_xpsnr_act"][0] > 0.0 and prof["k_xpsnr_sse"][0] > 0.0
        eng.gmsd(f, d, planes)
        assert "k_xpsnr_act" not in eng.profile_read(reset=True)
        ms, cnt = C.c_double(0), C.c_int64(0)
        for bad in (N.K_TERMINUS, N.K_BOUND):                              # ids 33 and 36 are unknown
            assert eng.lib.vqa_kernel_name(bad) == b"?"
            assert eng.lib.vqa_profile_read(eng.ctx, bad, C.byref(ms), C.byref(cnt), 0) == N.VQA_ERR_INVALID
