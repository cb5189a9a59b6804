"""GPU: VCA's texture features (vqa_vca_submit / vqa_vca_wait) through the C ABI, the engine, the one-pass stream and the
reference-shaped entry points, against the float64 NumPy restatement of tests/vca_reference.py (written from the definition in
include/vqa.h).

The bar was fixed before the kernels first ran: on E, h, L and every block's H_k / 1024 on the 8-bit scale,
1e-4 max(1, |restated value|), measured against the UNQUANTISED restatement.  DESIGN.md 4n derives the kernel's own bound
(two fp32 chains of 32 terms on samples with the block's mean taken off, plus the quantum 2^-(24 - depth)) and records the
error seen on the MI355X (E and the blocks within 5.5e-6, h within 2.5e-6, L within 8e-11 of its value).  S_k and l_sum depend on integers and one double sqrt only: they are tested for EQUALITY, l_sum
against the quantised restatement.  Everything that leaves the GPU is an integer, so the position-independence tests compare
bytes."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import vca_cases as VC
import vca_reference as R

pytestmark = pytest.mark.gpu

FIELDS = ("e_sum", "h_sum", "l_sum", "nbx", "nby", "e", "h", "l")
WORST = {"e": 0.0, "h": 0.0, "l": 0.0, "block": 0.0}


def _planes(h, w, chroma, depth):
    from rtvqa_amd.engine import yuv_planes
    return yuv_planes(h, w, chroma, depth)


def _check(rec, maps, frames, prev0, depth, tag):
    """rec [n, p], maps: vca_wait's; frames: lists of planes; prev0: planes or None"""
    n, npl = rec.shape
    sc = 1.0 / (1 << (depth - 8))
    for p in range(npl):
        stack = np.stack([f[p] for f in frames])
        prev = prev0[p] if prev0 is not None else None
        want = R.features(stack, depth, prev)
        wq = R.features(stack, depth, prev, quantise=True)
        nby, nbx = R.grid(*stack.shape[1:])
        assert (rec[:, p]["nbx"] == nbx).all() and (rec[:, p]["nby"] == nby).all()
        assert np.array_equal(maps[p]["s"].astype(np.int64), want["S"]), (tag, p, "S")
        assert np.array_equal(rec[:, p]["l_sum"].astype(np.int64), wq["l_sum"]), (tag, p, "l_sum")
        assert np.array_equal(rec[:, p]["e_sum"], maps[p]["qh"].reshape(n, -1).sum(axis=1)), (tag, p, "e_sum")
        hb = maps[p]["qh"].astype(np.float64) / float(1 << (24 - depth)) * sc / 1024.0
        wb = want["H"] * sc / 1024.0
        gap = np.abs(hb - wb)
        WORST["block"] = max(WORST["block"], float((gap / R.bar(wb) * 1e-4).max()))
        assert (gap <= R.bar(wb)).all(), (tag, p, "H_k", float(gap.max()))
        for key in ("e", "h", "l"):
            g = np.abs(rec[:, p][key] - want[key])
            WORST[key] = max(WORST[key], float((g / R.bar(want[key]) * 1e-4).max()))
            print("%s plane %d %s %s (ref %s) gap %.3e" % (tag, p, key, rec[:, p][key], want[key], g.max()))
            assert (g <= R.bar(want[key])).all(), (tag, p, key, float(g.max()))
        if prev0 is None:
            assert int(rec[0, p]["h_sum"]) == 0 and float(rec[0, p]["h"]) == 0.0


@pytest.mark.parametrize("chroma,shape,depth", VC.SHAPES, ids=["%s-%dx%d-%d" % (c, s[0], s[1], d) for c, s, d in VC.SHAPES])
def test_every_feature_on_every_shape_depth_and_content(engine, chroma, shape, depth):
    h, w = shape
    planes = _planes(h, w, chroma, depth)
    for kind in VC.CONTENT:
        frames, prev0 = VC.clip(kind, 2, h, w, chroma, depth, seed=h + w + depth)
        f, p0 = VC.pack(frames, depth), VC.pack([prev0], depth)
        tag = "%s %s %dx%d %d bits" % (kind, chroma, h, w, depth)
        rec, maps = engine.vca(f, planes, prev0=p0, blocks=True)
        assert rec.dtype.names == FIELDS and rec.shape == (2, len(planes))
        _check(rec, maps, frames, prev0, depth, tag)
        rec0, maps0 = engine.vca(f, planes, blocks=True)
        _check(rec0, maps0, frames, None, depth, tag + " no prev0")
        assert rec0[1].tobytes() == rec[1].tobytes() and all(np.array_equal(a["qh"], b["qh"]) for a, b in zip(maps, maps0))
        assert engine.vca(f, planes, prev0=p0).tobytes() == rec.tobytes()          # without the map: the same records
        if kind == "static":
            assert (rec["h_sum"] == 0).all() and (rec["h"] == 0.0).all() and (rec["e_sum"] > 0).all()
        if kind in ("flat0", "flatpeak"):
            v = 0 if kind == "flat0" else (1 << depth) - 1
            assert (rec["e_sum"] == 0).all(), tag                  # the mean is taken off first: a flat block transforms zeros
            assert np.abs(rec["l"] - np.sqrt(32.0 * v / (1 << (depth - 8)))).max() <= 1e-9
    print("worst gaps so far, in units of the 8-bit scale at a bar of 1e-4:", WORST)


def test_an_odd_row_stride_and_a_padded_layout(engine):
    h, w = 70, 134
    frames, prev0 = VC.clip("noise", 2, h, w, "420", 8, seed=3)
    want = engine.vca(VC.pack(frames, 8), _planes(h, w, "420", 8), prev0=VC.pack([prev0], 8), blocks=True)
    for pad in (1, 5):                                             # luma rows of 135 and 139 bytes, chroma rows of 68 and 72
        f, planes = VC.pack_padded(frames, 8, pad)
        p0, _ = VC.pack_padded([prev0], 8, pad)
        got = engine.vca(f, planes, prev0=p0, blocks=True)
        assert got[0].tobytes() == want[0].tobytes()
        assert all(np.array_equal(a[k], b[k]) for a, b in zip(got[1], want[1]) for k in ("qh", "s"))
    fr10 = VC.clip("noise", 2, 40, 72, "444", 10, seed=4)[0]
    f16, planes16 = VC.pack_padded(fr10, 10, 3)
    tight = engine.vca(VC.pack(fr10, 10), _planes(40, 72, "444", 10))
    assert engine.vca(f16, planes16).tobytes() == tight.tobytes()


def _same(a, b):
    return a[0].tobytes() == b[0].tobytes() and all(np.array_equal(x[k], y[k]) for x, y in zip(a[1], b[1]) for k in ("qh", "s"))


def test_batches_positions_prev0_and_memory_kinds_give_the_same_words(engine):
    from rtvqa_amd.engine import DeviceFrames, gray_planes
    h, w = 70, 134
    frames, prev0 = VC.clip("noise", 5, h, w, "420", 8, seed=11)
    planes = _planes(h, w, "420", 8)
    r, p0 = VC.pack(frames, 8), VC.pack([prev0], 8)
    whole = engine.vca(r, planes, prev0=p0, blocks=True)
    assert _same(engine.vca(r, planes, prev0=p0, blocks=True), whole)                       # run to run
    _check(whole[0], whole[1], frames, prev0, 8, "batch of 5")

    def one(k, got, pos):
        return got[0][pos].tobytes() == whole[0][k].tobytes() and all(
            np.array_equal(x[key][pos], y[key][k]) for x, y in zip(got[1], whole[1]) for key in ("qh", "s"))

    # n = 1: a frame alone, its predecessor given explicitly, has the words it has in the batch; n = 2 likewise
    for k in (0, 2, 4):
        pk = p0 if k == 0 else r[k - 1:k]
        assert one(k, engine.vca(r[k:k + 1], planes, prev0=pk, blocks=True), 0), k
    two = engine.vca(r[2:4], planes, prev0=r[1:2], blocks=True)
    assert one(2, two, 0) and one(3, two, 1)
    # first, in the middle and last in a batch of 5, frame 1 before it each time (as prev0, or as the frame in front of it)
    for pos, order in ((0, [2, 0, 1, 3, 4]), (2, [0, 1, 2, 3, 4]), (4, [0, 3, 4, 1, 2])):
        assert order[pos] == 2 and (pos == 0 or order[pos - 1] == 1)
        assert one(2, engine.vca(r[order], planes, prev0=r[1:2], blocks=True), pos), order
    # without a predecessor only frame 0's h changes
    bare = engine.vca(r, planes, blocks=True)
    assert (bare[0][0]["h_sum"] == 0).all() and bare[0][1:].tobytes() == whole[0][1:].tobytes()
    assert (bare[0][0]["e_sum"] == whole[0][0]["e_sum"]).all() and (whole[0][0]["h_sum"] > 0).all()
    # device and pinned memory
    dr, dp = engine.upload(r), engine.upload(p0)
    assert _same(engine.vca(dr, planes, prev0=dp, blocks=True), whole)
    assert one(2, engine.vca(dr.slice(2, 3), planes, prev0=dr.frame(1), blocks=True), 0)
    pr, pp = engine.alloc_pinned(r.shape), engine.alloc_pinned(p0.shape)
    pr[...], pp[...] = r, p0
    assert engine.is_pinned(pr)
    assert _same(engine.vca(pr, planes, prev0=pp, blocks=True), whole)
    for a in (pr, pp):
        engine.free_pinned(a)
    with pytest.raises(TypeError):
        engine.vca(dr, planes, prev0=p0)                                                       # prev0 lives elsewhere
    # every second frame of the resident clip: frame_stride does the stepping
    odd = DeviceFrames(dr.ptr + dr.frame_stride, 2, dr.h, dr.w, frame_stride=2 * dr.frame_stride, row_stride=dr.row_stride,
                       owner=dr, channels=dr.channels)
    assert engine.vca(odd, planes).tobytes() == engine.vca(r[1::2][:2], planes).tobytes()
    # a 75 x 93 window at (9, 13) of resident 120 x 160 gray frames: nothing outside the window is read
    g = np.random.default_rng(5).integers(0, 256, (3, 120, 160)).astype(np.uint8)
    win = engine.upload(g).roi(9, 9 + 75, 13, 13 + 93)
    cut = np.ascontiguousarray(g[:, 9:84, 13:106]).reshape(3, -1)
    alone = engine.vca(cut, gray_planes(75, 93))
    assert engine.vca(win, [(93, 75, 0, 160, 1)]).tobytes() == alone.tobytes()
    assert engine.vca(g.reshape(3, -1), [(93, 75, 9 * 160 + 13, 160, 1)]).tobytes() == alone.tobytes()


def _submit(engine, f, planes, prev0=None):
    from rtvqa_amd import _native as N
    from rtvqa_amd.engine import plane_descs
    fb = f.shape[1] * f.dtype.itemsize
    return engine.lib.vqa_vca_submit(engine.ctx, f.ctypes.data, prev0.ctypes.data if prev0 is not None else None,
                                     N.VQA_MEM_HOST, f.shape[0], fb, plane_descs(planes), len(planes))


def test_the_state_machine_and_the_refusals(engine):
    from rtvqa_amd import _native as N
    from rtvqa_amd.engine import bgr_planes, gray_planes, plane_descs, yuv420p_planes
    h, w = 64, 96
    frames, prev0 = VC.clip("noise", 2, h, w, "420", 8, seed=8)
    planes = _planes(h, w, "420", 8)
    f, p0 = VC.pack(frames, 8), VC.pack([prev0], 8)
    want, mwant = engine.vca(f, planes, prev0=p0, blocks=True)
    swant = engine.siti(f, planes, p0)
    nb = 6 + 1 + 1                                                                   # 3 x 2 luma blocks, one per chroma plane
    nwords = 2 * 2 * nb
    vout, sout, gout = (N.VqaVcaMetrics * 6)(), (N.VqaSitiMetrics * 6)(), (N.VqaGmsdMetrics * 6)()
    words = (C.c_uint64 * nwords)()
    lib, ctx = engine.lib, engine.ctx
    assert lib.vqa_vca_wait(ctx, vout, 6, None, 0) == N.VQA_ERR_STATE                # wait without submit
    assert _submit(engine, f, planes, p0) == N.VQA_OK
    assert _submit(engine, f, planes, p0) == N.VQA_ERR_STATE                         # submit while pending
    assert lib.vqa_siti_wait(ctx, sout, 6) == N.VQA_ERR_STATE                        # a wait of another kind
    assert lib.vqa_gmsd_wait(ctx, gout, 6) == N.VQA_ERR_STATE
    assert lib.vqa_trim(ctx) == N.VQA_ERR_STATE
    assert lib.vqa_vca_wait(ctx, vout, 5, None, 0) == N.VQA_ERR_STATE                # a wrong entry count
    for bad in (nwords - 1, nwords + 1, 0, nb):                                      # a wrong n_block_words: the batch survives
        assert lib.vqa_vca_wait(ctx, vout, 6, words, bad) == N.VQA_ERR_INVALID
    assert lib.vqa_vca_wait(ctx, vout, 6, words, nwords) == N.VQA_OK
    assert bytes(vout) == want.tobytes()
    got = np.frombuffer(words, np.uint64).reshape(2, nb, 2)
    assert np.array_equal(got[:, :6, 0].reshape(2, 2, 3), mwant[0]["qh"]) and np.array_equal(got[:, 6, 1], mwant[1]["s"].reshape(2))
    assert np.array_equal(got[:, 7, 0], mwant[2]["qh"].reshape(2))
    assert lib.vqa_vca_wait(ctx, vout, 6, None, 0) == N.VQA_ERR_STATE
    # the converse: a VCA wait with only an SI/TI batch pending; it survives
    fb = f.shape[1]
    pd = plane_descs(planes)
    assert lib.vqa_siti_submit(ctx, f.ctypes.data, p0.ctypes.data, N.VQA_MEM_HOST, 2, fb, pd, 3) == N.VQA_OK
    assert lib.vqa_vca_wait(ctx, vout, 6, None, 0) == N.VQA_ERR_STATE
    assert lib.vqa_siti_wait(ctx, sout, 6) == N.VQA_OK and bytes(sout) == swant.tobytes()
    # in flight next to an SI/TI batch, whose host staging it shares, from host and from device frames: each wait collects its own
    df, dp = engine.upload(f), engine.upload(p0)
    for a, b in ((f, p0), (df, dp)):
        for order in (("vca", "siti"), ("siti", "vca")):
            engine.siti_submit(a, planes, b)
            engine.vca_submit(a, planes, b)
            wants = {"vca": want, "siti": swant}
            for kind in order:
                assert getattr(engine, kind + "_wait")().tobytes() == wants[kind].tobytes(), (order, kind)
    engine.vca_submit(df, planes, dp)
    engine.drain()                                                                   # a pending batch is waited out
    assert lib.vqa_vca_wait(ctx, vout, 6, None, 0) == N.VQA_ERR_STATE
    # planes below 32 x 32, packed BGR: a failed submit leaves nothing in flight
    for hh, ww in ((31, 32), (32, 31)):
        z = np.zeros((2, hh * ww), np.uint8)
        assert _submit(engine, z, gray_planes(hh, ww)) == N.VQA_ERR_UNSUPPORTED, (hh, ww)
        assert lib.vqa_vca_wait(ctx, vout, 2, None, 0) == N.VQA_ERR_STATE
    z = np.zeros((1, 62 * 62 * 3 // 2), np.uint8)                                    # 4:2:0 at 62: the chroma planes are 31
    assert _submit(engine, z, yuv420p_planes(62, 62)) == N.VQA_ERR_UNSUPPORTED
    z = np.zeros((1, 32 * 32 * 3), np.uint8)
    assert _submit(engine, z, bgr_planes(32, 32)) == N.VQA_ERR_UNSUPPORTED           # bgr24
    small = np.zeros((1, 64), np.uint8)                                              # more than 2^28 samples: a descriptor check
    assert _submit(engine, small, [(16385, 16384, 0, 16385, 1)]) == N.VQA_ERR_UNSUPPORTED
    assert _submit(engine, small.view(np.uint16), [(8193, 8192, 0, 2 * 8193, 2, 10)]) == N.VQA_ERR_UNSUPPORTED
    assert lib.vqa_vca_submit(ctx, None, None, N.VQA_MEM_HOST, 2, fb, pd, 3) == N.VQA_ERR_INVALID
    assert lib.vqa_vca_submit(ctx, f.ctypes.data, None, N.VQA_MEM_HOST, 2, fb - 1, pd, 3) == N.VQA_ERR_INVALID
    with pytest.raises(ValueError):
        engine.vca(z, bgr_planes(32, 32))
    with pytest.raises(ValueError):
        engine.vca(np.zeros((1, 31 * 40), np.uint8), gray_planes(31, 40))
    with pytest.raises(ValueError):
        engine.vca(z[:, :1024], _planes(32, 32, "mono", 10))                          # a dtype that does not match the depth
    # nothing is pending and the ctx computes as before; trim gives the feature's buffers and tables back and it re-grows them
    assert lib.vqa_vca_wait(ctx, vout, 6, None, 0) == N.VQA_ERR_STATE
    engine.trim()
    assert engine.vca(f, planes, prev0=p0).tobytes() == want.tobytes()
    assert engine.siti(f, planes, p0).tobytes() == swant.tobytes()


def test_one_pass_entry_points(tmp_path):
    """frame_vca at two batch sizes whose chunk seams fall inside the clip (frame q0 of a later chunk sees frame q0 - 1),
    run_ffmpeg_metrics(.., vca=True) and config "vca": true on a 6-frame 70 x 134 .y4m pair: the psnr / ssim logs are byte for
    byte those of a plain run, the log's values are the records', and the row gains VCA_E, VCA_H, VCA_L after HAARPSI"""
    import rtvqa_amd
    from rtvqa_amd import frames as F
    from rtvqa_amd import synth
    from rtvqa_amd import video_processing as vp
    h, w, n = 70, 134, 6
    ref, _p = VC.clip("noise", n, h, w, "420", 8, seed=6)
    ref[3] = ref[2]                                              # a repeated frame: h = 0 there
    planes = _planes(h, w, "420", 8)
    r = VC.pack(ref, 8)
    d = np.ascontiguousarray(r[::-1])                            # the distorted stream is never read by VCA
    with rtvqa_amd.Engine(0) as eng:
        whole, wmaps = eng.vca(r, planes, blocks=True)
    assert (whole["h_sum"][0] == 0).all() and (whole["h_sum"][3] == 0).all() and (whole["h_sum"][1] > 0).all()
    for bs in (2, 4):
        out = vp.frame_vca(r, "yuv420p", h, w, batch_size=bs)
        e, hh, l, sizes = out
        assert e.shape == (n, 3) and sizes == [(q[0], q[1]) for q in planes]
        for got, key in ((e, "e"), (hh, "h"), (l, "l")):
            assert got.tobytes() == np.ascontiguousarray(whole[key]).tobytes(), (bs, key)
    e, hh, l, sizes, maps = vp.frame_vca(r, "yuv420p", h, w, batch_size=4, blocks=True)
    assert all(np.array_equal(a[k], b[k]) for a, b in zip(maps, wmaps) for k in ("qh", "s"))
    pr, pd = str(tmp_path / "ref.y4m"), str(tmp_path / "enc.y4m")
    F.write_y4m(pr, r, h, w)
    F.write_y4m(pd, d, h, w)
    logs = {k: [str(tmp_path / ("%s_%s.log" % (k, t))) for t in ("psnr", "ssim", "vmaf")] for k in ("plain", "vca", "feat", "both")}
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["plain"], batch_size=4) is None
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["vca"], batch_size=4, vca=True) is None
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["feat"], batch_size=4, gmsd=True, haarpsi=True) is None
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["both"], batch_size=2, gmsd=True, haarpsi=True, vca=True) is None
    assert not os.path.exists(logs["plain"][2])
    for k in (0, 1):
        for kind in ("vca", "feat", "both"):
            assert open(logs["plain"][k], "rb").read() == open(logs[kind][k], "rb").read(), (kind, k)
    doc, feat, both = (json.load(open(logs[k][2])) for k in ("vca", "feat", "both"))
    assert list(doc["frames"][0]["metrics"]) == ["vca_e", "vca_h", "vca_l"] == list(doc["pooled_metrics"])
    names = list(feat["frames"][0]["metrics"])
    assert names[-1] == "haarpsi" and "vca_e" not in json.dumps(feat)
    assert list(both["frames"][0]["metrics"]) == names + ["vca_e", "vca_h", "vca_l"]
    for i in range(n):
        for dc in (doc, both):
            for key in ("e", "h", "l"):
                assert dc["frames"][i]["metrics"]["vca_" + key] == float(whole[key][i, 0])
        assert {k: both["frames"][i]["metrics"][k] for k in names} == feat["frames"][i]["metrics"]
    assert {k: both["pooled_metrics"][k] for k in names} == feat["pooled_metrics"]
    for key in ("e", "h", "l"):
        assert abs(doc["pooled_metrics"]["vca_" + key]["mean"] - np.mean(whole[key][:, 0])) <= 1e-12 * max(1.0, np.mean(whole[key][:, 0]))
    bgr = synth.s_natural(n, h, w, seed=12)
    cfg = {"crf": 23, "resize_width": 64, "resize_height": 64, "frame_interval": 1, "batch_size": 4}

    def row(name, **kw):
        return vp.process_video_and_extract_metrics(pr, pd, dict(cfg, **kw), csv_file=str(tmp_path / (name + ".csv")),
                                                    column_order="fixed", encoded_bgr=bgr)

    def same(a, b):
        return a == b or (a != a and b != b)

    row0, row1 = row("row0"), row("row1", vca=True)
    k0 = list(row0)
    at = k0.index("SSIM") + 1
    assert list(row1) == k0[:at] + ["VCA_E", "VCA_H", "VCA_L"] + k0[at:] and all(same(row0[k], row1[k]) for k in k0)
    assert row1["VCA_H"] == doc["pooled_metrics"]["vca_h"]["mean"] and row1["VCA_E"] == doc["pooled_metrics"]["vca_e"]["mean"]
    assert row1["VCA_L"] == doc["pooled_metrics"]["vca_l"]["mean"]
    row2, row3 = row("row2", haarpsi=True, batch_size=2), row("row3", haarpsi=True, vca=True, batch_size=2)
    k2 = list(row2)
    at = k2.index("HAARPSI") + 1
    assert list(row3) == k2[:at] + ["VCA_E", "VCA_H", "VCA_L"] + k2[at:] and all(same(row2[k], row3[k]) for k in k2)
    assert row3["VCA_E"] == row1["VCA_E"]
    row("row0b", vca=False)
    assert open(str(tmp_path / "row0.csv"), "rb").read() == open(str(tmp_path / "row0b.csv"), "rb").read()
    assert b"VCA_" not in open(str(tmp_path / "row0.csv"), "rb").read()
    assert b"HAARPSI,VCA_E,VCA_H,VCA_L" in open(str(tmp_path / "row3.csv"), "rb").read()
    with pytest.raises(ValueError):
        vp.frame_vca(bgr, "bgr24")
    with pytest.raises(ValueError):
        vp.validate_config(dict(cfg, vca=1))


def test_profile_counts_one_launch_per_plane_group_and_one_sum():
    import rtvqa_amd
    from rtvqa_amd import _native as N
    h, w = 70, 134
    frames, _p = VC.clip("noise", 3, h, w, "420", 8, seed=9)
    planes = _planes(h, w, "420", 8)
    f = VC.pack(frames, 8)
    with rtvqa_amd.Engine(0) as eng:
        eng.lib.vqa_kernel_name.restype = C.c_char_p
        assert eng.lib.vqa_kernel_name(N.K_VCA_BLOCKS) == b"k_vca_blocks" and eng.lib.vqa_kernel_name(N.K_VCA_SUM) == b"k_vca_sum"
        eng.profile(True)
        eng.vca(f, planes)
        prof = eng.profile_read(reset=True)
        assert prof["k_vca_blocks"][1] == 2 and prof["k_vca_sum"][1] == 1 and "k_siti" not in prof, prof
        assert prof["k_vca_blocks"][0] > 0.0 and prof["k_vca_sum"][0] > 0.0
        eng.siti(f, planes)
        assert "k_vca_blocks" not in eng.profile_read(reset=True)
        ms, cnt = C.c_double(0), C.c_int64(0)
        for bad in (N.K_BOUND, N.K_FINIS, N.K_CLOSE):                            # ids 36, 38 and 41 are unknown
            assert eng.lib.vqa_kernel_name(bad) == b"?"
            assert eng.lib.vqa_profile_read(eng.ctx, bad, C.byref(ms), C.byref(cnt), 0) == N.VQA_ERR_INVALID
