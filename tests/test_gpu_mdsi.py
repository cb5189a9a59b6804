"""GPU: MDSI (vqa_mdsi_submit / vqa_mdsi_wait) through the C ABI, the engine, the one-pass stream and the reference-shaped entry
points, against the two NumPy restatements of tests/mdsi_reference.py (written from the definition in include/vqa.h).

What is asserted was fixed before the kernels first ran.  The four words must EQUAL the quantised restatement's: every double
operation up to g = rint(GCS 2^24) is an IEEE add, multiply, divide or square root in the order the header states, and everything
after g is a function of integers.  dev must lie within the case's own bar of the UNQUANTISED float64 form:
mdsi_reference.derived_bar, twice the mean per-sample change of |GCS|^(1/4) under a change of 2^-25 plus 3 * 2^-29 - between
2.0e-8 and 1.9e-7 on these cases, which tests/test_mdsi_host.py admits one by one (largest gap there 2.4e-8).  Largest gap seen
on an MI355X: 2.36e-8 against a bar of 1.82e-7 (texture_flat, gray, 33 x 67)."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import mdsi_cases as MC
import mdsi_reference as R

pytestmark = pytest.mark.gpu

FIELDS = ("sum_pos", "sum_neg", "n_neg", "sum_dev", "count", "factor", "reserved", "dev", "mdsi")
WORST = {"gap": 0.0, "bar": 0.0, "tag": ""}
MATRIX = MC.matrix()


def _words(g):
    return int(g["sum_pos"]), int(g["sum_neg"]), int(g["n_neg"]), int(g["sum_dev"])


def _one(engine, r, d, layout, h, w, depth):
    return engine.mdsi(MC.pack([r], layout, depth), MC.pack([d], layout, depth), MC.engine_planes(layout, h, w, depth))[0]


def _check_one(g, r, d, layout, depth, tag, float_too=True):
    model = MC.MODEL[layout]
    h, w = r[0].shape
    f, hd, wd = R.grid(h, w)
    assert int(g["count"]) == hd * wd and int(g["factor"]) == f and int(g["reserved"]) == 0
    want = R.mdsi_quantised(r, d, model, depth)
    print(tag, "words", _words(g), "restatement", want)
    assert _words(g) == want, tag
    dev, mdsi = R.pool_words(want, hd * wd)
    assert float(g["dev"]) == dev and float(g["mdsi"]) == mdsi == math.sqrt(math.sqrt(float(g["dev"])))
    if float_too:
        gcs = R.gcs_float(r, d, model, depth)
        fdev, fmdsi = R.pool_float(gcs)
        bar, gap = R.derived_bar(gcs), abs(float(g["dev"]) - fdev)
        print(tag, "dev %.10f (float64 %.10f) gap %.2e bar %.2e mdsi %.6f (float64 %.6f)" % (g["dev"], fdev, gap, bar, g["mdsi"], fmdsi))
        if gap > WORST["gap"]:
            WORST.update(gap=gap, bar=bar, tag=tag)
        assert bar <= MC.BAR_LIMIT and gap <= bar, (tag, gap, bar)


@pytest.mark.parametrize("case", MATRIX, ids=[MC.case_id(c) for c in MATRIX])
def test_parity_on_every_content_layout_shape_and_depth(engine, case):
    name, layout, (h, w), depth = case
    r, d = MC.pair(name, layout, h, w, depth)
    g = _one(engine, r, d, layout, h, w, depth)
    assert g.dtype.names == FIELDS and int(g["factor"]) == MC.FACTORS[(h, w)]
    _check_one(g, r, d, layout, depth, MC.case_id(case))
    if name == "noise":
        assert int(g["n_neg"]) > 0                                            # the complex branch is exercised
    if name in ("identical", "flat_zero", "flat_peak"):
        assert _words(g) == (int(g["count"]) << 28, 0, 0, 0) and g["dev"] == 0.0 and g["mdsi"] == 0.0


def test_the_worst_gap_of_the_parity_matrix():
    """runs after the parity tests of this module (pytest keeps the file's order): the figure DESIGN.md 4q quotes"""
    print("parity matrix: largest dev gap %.3e against its bar %.3e (%s)" % (WORST["gap"], WORST["bar"], WORST["tag"]))


def test_exact_zero_and_asymmetry_on_the_device(engine):
    for layout, depth in (("bgr24", 8), ("yuv420p", 10), ("gray", 16)):
        for h, w in MC.SMALL + ((385, 391),):
            r, _ = MC.pair("noise", layout, h, w, depth)
            g = _one(engine, r, r, layout, h, w, depth)
            assert _words(g) == (int(g["count"]) << 28, 0, 0, 0) and g["dev"] == 0.0 and g["mdsi"] == 0.0, (layout, h, w)
    # removed edges are worse than added edges: the pair is ordered
    for h, w in ((67, 130), (16, 16)):
        r, d = MC.pair("texture_flat", "bgr24", h, w)
        a, b = _one(engine, r, d, "bgr24", h, w, 8), _one(engine, d, r, "bgr24", h, w, 8)
        assert a["mdsi"] > b["mdsi"] + 0.05, (h, w, a["mdsi"], b["mdsi"])
        assert abs(a["mdsi"] - R.mdsi_float(r, d, "bgr")[1]) <= 1e-6 and abs(b["mdsi"] - R.mdsi_float(d, r, "bgr")[1]) <= 1e-6
    # a gray YUV clip: the same words at 4:4:4, 4:2:2 and 4:2:0
    (y, _, _), (yd, _, _) = MC.pair("natural", "yuv444p", 33, 67)
    got = []
    for layout in ("yuv444p", "yuv422p", "yuv420p"):
        sizes = MC.plane_sizes(layout, 33, 67)
        r = [y] + [np.full(s, 128, np.int64) for s in sizes[1:]]
        d = [yd] + [np.full(s, 128, np.int64) for s in sizes[1:]]
        got.append(_one(engine, r, d, layout, 33, 67, 8).tobytes())
    assert got[0] == got[1] == got[2]


def _clip(layout, h, w, depth, n):
    """n distinct admitted frame pairs (mdsi_cases.slice_pool's kinds) -> (ref, dist, planes, the frames as plane tuples)"""
    names = ("natural", "noise", "texture_flat", "noise", "natural", "noise", "natural", "noise")   # (texture_flat takes no seed)
    pairs = [MC.pair(names[k % 8], layout, h, w, depth, seed=11 + k) for k in range(n)]
    rs, ds = [p[0] for p in pairs], [p[1] for p in pairs]
    return MC.pack(rs, layout, depth), MC.pack(ds, layout, depth), MC.engine_planes(layout, h, w, depth), rs, ds


def test_batches_positions_and_memory_kinds_give_the_same_bytes(engine):
    """the same pair at several places of batches of 1, 3 and 8, from host, pinned and device memory; frame_mdsi in chunks of 1, 3
    and 64; a strided view and an unaligned region of interest of resident frames"""
    from rtvqa_amd import video_processing as vp
    from rtvqa_amd.engine import DeviceFrames
    h, w, layout, n = 33, 67, "yuv420p", 8
    r, d, planes, rs, ds = _clip(layout, h, w, 8, n)
    whole = engine.mdsi(r, d, planes)
    assert whole.shape == (n,) and len({x.tobytes() for x in whole}) == n
    for i in (0, 1, 2):
        _check_one(whole[i], rs[i], ds[i], layout, 8, "clip frame %d" % i, float_too=False)
    assert engine.mdsi(r, d, planes).tobytes() == whole.tobytes()             # run to run
    one = whole[5:6].tobytes()
    assert engine.mdsi(r[5:6], d[5:6], planes).tobytes() == one               # a batch of 1
    for order in ([5, 0, 5], [1, 5, 2], [5, 1, 2, 3, 5, 6, 7, 5]):            # batches of 3 and 8
        got = engine.mdsi(r[order], d[order], planes)
        for pos, k in enumerate(order):
            assert got[pos].tobytes() == whole[k].tobytes(), (order, pos)
    dr, dd = engine.upload(r), engine.upload(d)
    assert engine.mdsi(dr, dd, planes).tobytes() == whole.tobytes()
    assert engine.mdsi(dr.slice(5, 6), dd.slice(5, 6), planes).tobytes() == one
    pr, pd = engine.alloc_pinned(r.shape), engine.alloc_pinned(d.shape)
    pr[...], pd[...] = r, d
    assert engine.is_pinned(pr)
    assert engine.mdsi(pr, pd, planes).tobytes() == whole.tobytes()
    for src in ((r, d), (pr, pd), (dr, dd)):
        for bs in (1, 3, 64):
            score, dev = vp.frame_mdsi(src[0], src[1], layout, h, w, batch_size=bs)
            assert score.shape == (n,)
            assert score.tobytes() == np.ascontiguousarray(whole["mdsi"]).tobytes(), (type(src[0]), bs)
            assert dev.tobytes() == np.ascontiguousarray(whole["dev"]).tobytes(), (type(src[0]), bs)
    engine.free_pinned(pr)
    engine.free_pinned(pd)
    # every second frame of the resident clips: frame_stride does the stepping
    odd = [DeviceFrames(x.ptr + x.frame_stride, 4, x.h, x.w, frame_stride=2 * x.frame_stride, row_stride=x.row_stride, owner=x,
                        channels=x.channels) for x in (dr, dd)]
    assert engine.mdsi(odd[0], odd[1], planes).tobytes() == whole[1::2].tobytes()
    # a window of resident 60 x 80 4:4:4 frames (uploaded as [n, 3 * 60, 80]; the window's plane k starts k * 60 rows further
    # down) at (9, 13), 35 x 45: odd origin, odd size; against the same samples as frames of their own and the restatement
    H, W, (y0, x0, hh, ww) = 60, 80, (9, 13, 35, 45)
    g, gd, _, grs, gds = _clip("yuv444p", H, W, 8, 3)
    cut_r = [tuple(p[y0:y0 + hh, x0:x0 + ww] for p in f) for f in grs]
    cut_d = [tuple(p[y0:y0 + hh, x0:x0 + ww] for p in f) for f in gds]
    own = MC.engine_planes("yuv444p", hh, ww)
    alone = engine.mdsi(MC.pack(cut_r, "yuv444p"), MC.pack(cut_d, "yuv444p"), own)
    for i in range(3):
        _check_one(alone[i], cut_r[i], cut_d[i], "yuv444p", 8, "window frame %d" % i, float_too=False)
    dg, dgd = engine.upload(g.reshape(3, 3 * H, W)), engine.upload(gd.reshape(3, 3 * H, W))
    roi = [(ww, hh, k * H * W, W, 1) for k in range(3)]
    a, b = dg.roi(y0, y0 + hh, x0, x0 + ww), dgd.roi(y0, y0 + hh, x0, x0 + ww)
    assert engine.mdsi(a, b, roi).tobytes() == alone.tobytes()
    assert engine.mdsi(g, gd, [(ww, hh, k * H * W + y0 * W + x0, W, 1) for k in range(3)]).tobytes() == alone.tobytes()


def test_the_stream_runs_mdsi_beside_and_instead_of_ssim(engine):
    from rtvqa_amd import stream
    h, w, layout, n = 33, 67, "yuv420p", 5
    r, d, planes, _, _ = _clip(layout, h, w, 8, n)
    want, qwant = engine.mdsi(r, d, planes), engine.quality(r, d, planes)
    q0, _ = stream.run(d, r, quality=stream.Quality(planes), batch_size=2, engine=engine)
    q1, _ = stream.run(d, r, quality=stream.Quality(planes, mdsi=True), batch_size=2, engine=engine)
    q2, _ = stream.run(d, r, quality=stream.Quality(planes, mdsi="only"), batch_size=3, engine=engine)
    q3, _ = stream.run(d, r, quality=stream.Quality(planes, gmsd=True, brisque=True, mdsi=True), batch_size=2, engine=engine)
    assert len(q1) == len(q0) + 1 and q1[-1].tobytes() == want.tobytes() == q2[-1].tobytes() == q3[-1].tobytes()
    for a, b in zip(q0, q1):
        assert a.tobytes() == b.tobytes()
    assert q2[0] is None and q2[1] is None and len(q2) == 3 and len(q3) == 5
    assert np.array_equal(q1[0], qwant["sse"])
    bgr, bgd, bp, _, _ = _clip("bgr24", 33, 67, 8, 3)
    q4, _ = stream.run(bgd, bgr, quality=stream.Quality(bp, mdsi="only"), engine=engine)
    assert q4[-1].tobytes() == engine.mdsi(bgr, bgd, bp, model=1).tobytes()       # the model follows from the planes
    gy, gyd, gp, _, _ = _clip("gray", 33, 67, 8, 3)
    q5, _ = stream.run(gyd, gy, quality=stream.Quality(gp, mdsi=True), engine=engine)
    assert q5[-1].tobytes() == engine.mdsi(gy, gyd, gp).tobytes()


def _submit(engine, f, d, planes, n=None, model=0):
    from rtvqa_amd import _native as N
    from rtvqa_amd.engine import plane_descs
    fb = f.shape[1] * f.dtype.itemsize
    return engine.lib.vqa_mdsi_submit(engine.ctx, f.ctypes.data, d.ctypes.data, N.VQA_MEM_HOST, f.shape[0] if n is None else n,
                                      fb, fb, plane_descs(planes), len(planes), model)


def test_the_state_machine_and_the_refusals(engine):
    from rtvqa_amd import _native as N
    from rtvqa_amd.engine import plane_descs, yuv_planes
    f, d, planes, _, _ = _clip("yuv420p", 64, 96, 8, 2)
    want = engine.mdsi(f, d, planes)
    hwant, qwant = engine.gmsd(f, d, planes), engine.quality(f, d, planes)
    mout, gout, qout, eout = (N.VqaMdsiMetrics * 2)(), (N.VqaGmsdMetrics * 6)(), (N.VqaPlaneMetrics * 6)(), (N.VqaCiedeMetrics * 2)()
    lib, ctx = engine.lib, engine.ctx

    def idle():
        return lib.vqa_mdsi_wait(ctx, mout, 2) == N.VQA_ERR_STATE
    assert idle()                                                         # wait without submit
    # submit while pending; the other kinds' waits on an MDSI batch; the batch survives all of them
    assert _submit(engine, f, d, planes) == N.VQA_OK
    assert _submit(engine, f, d, planes) == N.VQA_ERR_STATE
    assert lib.vqa_quality_wait(ctx, qout, 6) == N.VQA_ERR_STATE
    assert lib.vqa_gmsd_wait(ctx, gout, 6) == N.VQA_ERR_STATE
    assert lib.vqa_ciede_wait(ctx, eout, 2) == N.VQA_ERR_STATE
    assert lib.vqa_trim(ctx) == N.VQA_ERR_STATE
    assert lib.vqa_mdsi_wait(ctx, mout, 6) == N.VQA_ERR_STATE             # a wrong entry count: one entry per FRAME
    assert lib.vqa_mdsi_wait(ctx, mout, 2) == N.VQA_OK
    assert bytes(mout) == want.tobytes()
    # a wait with another kind pending; that batch survives
    fb = f.shape[1]
    pd = plane_descs(planes)
    assert lib.vqa_gmsd_submit(ctx, f.ctypes.data, d.ctypes.data, N.VQA_MEM_HOST, 2, fb, fb, pd, 3) == N.VQA_OK
    assert idle()
    assert lib.vqa_gmsd_wait(ctx, gout, 6) == N.VQA_OK and bytes(gout) == hwant.tobytes()
    # in flight next to a quality and a GMSD batch from one upload: each wait collects its own, in any order
    df, dd = engine.upload(f), engine.upload(d)
    for order in (("mdsi", "quality", "gmsd"), ("gmsd", "mdsi", "quality")):
        engine.quality_submit(df, dd, planes)
        engine.gmsd_submit(df, dd, planes)
        engine.mdsi_submit(df, dd, planes)
        wants = {"mdsi": want, "quality": qwant, "gmsd": hwant}
        for kind in order:
            assert getattr(engine, kind + "_wait")().tobytes() == wants[kind].tobytes(), (order, kind)
    engine.quality_submit(f, d, planes)          # host frames share the staging of a pending quality batch
    engine.mdsi_submit(f, d, planes)
    assert engine.mdsi_wait().tobytes() == want.tobytes() and engine.quality_wait().tobytes() == qwant.tobytes()
    # the refusals: each leaves nothing in flight, and the next valid submit works
    Y, U, V = planes
    z16 = np.zeros((2, 64 * 96 * 3), np.uint16)
    p10 = yuv_planes(64, 96, "420", 10)
    refused = [
        (f, planes[:1], {"model": N.MDSI_YUV709}, N.VQA_ERR_INVALID),                       # one plane with the wrong model
        (f, planes[:1], {"model": N.MDSI_BGR}, N.VQA_ERR_INVALID),
        (f, planes, {"model": N.MDSI_GRAY}, N.VQA_ERR_INVALID),                             # three planes with the gray model
        (f, planes[:2], {}, N.VQA_ERR_INVALID),                                             # two planes
        (f, planes + [V], {}, N.VQA_ERR_INVALID),                                           # four
        (f, [Y, U, (V[0] - 1,) + V[1:]], {}, N.VQA_ERR_INVALID),                            # U and V geometries differ
        (f, [Y, U, V[:3] + (V[3] + 2, V[4])], {}, N.VQA_ERR_INVALID),                       # (their row strides too)
        (f, [Y, (40, 32, U[2], 40, 1), (40, 32, V[2], 40, 1)], {}, N.VQA_ERR_INVALID),      # neither full nor ceil-half
        (f, [Y, (48, 30, U[2], 48, 1), (48, 30, V[2], 48, 1)], {}, N.VQA_ERR_INVALID),
        (f, planes, {"model": N.MDSI_BGR}, N.VQA_ERR_INVALID),                              # B, G, R must share one geometry
        (f, planes, {"model": 3}, N.VQA_ERR_INVALID),                                       # an unknown model
        (f, planes, {"model": -1}, N.VQA_ERR_INVALID),
        (z16, p10[:1] + [p[:5] for p in p10[1:]], {}, N.VQA_ERR_INVALID),                   # mixed depths
        (f, [(16, 15, 0, 16, 1), (8, 8, 240, 8, 1), (8, 8, 304, 8, 1)], {}, N.VQA_ERR_UNSUPPORTED),   # luma 15 rows x 16
        (f, [(15, 16, 0, 15, 1)], {"model": N.MDSI_GRAY}, N.VQA_ERR_UNSUPPORTED),                     # too small
        (f, [(16385, 16384, 0, 16385, 1)] * 3, {"model": N.MDSI_BGR}, N.VQA_ERR_UNSUPPORTED),         # more than 2^28 samples
    ]
    for k, (buf, pl, kw, status) in enumerate(refused):
        assert _submit(engine, buf, buf, pl, n=1, **kw) == status, k
        assert idle(), k
    assert lib.vqa_mdsi_submit(ctx, f.ctypes.data, d.ctypes.data, N.VQA_MEM_HOST, 2, fb - 1, fb, pd, 3, 0) == N.VQA_ERR_INVALID
    assert lib.vqa_mdsi_submit(ctx, f.ctypes.data, None, N.VQA_MEM_HOST, 2, fb, fb, pd, 3, 0) == N.VQA_ERR_INVALID
    assert idle()
    # a 16 x 16 4:2:0 frame is measured: its 8 x 8 chroma planes are no limit
    z = np.zeros((1, 16 * 16 * 3 // 2), np.uint8)
    assert _submit(engine, z, z, yuv_planes(16, 16, "420", 8)) == N.VQA_OK and lib.vqa_mdsi_wait(ctx, mout, 1) == N.VQA_OK
    assert mout[0].sum_pos == 256 << 28 and mout[0].mdsi == 0.0
    assert engine.mdsi(f, d, planes).tobytes() == want.tobytes()
    engine.trim()
    assert engine.mdsi(f, d, planes).tobytes() == want.tobytes()
    assert engine.quality(f, d, planes).tobytes() == qwant.tobytes()


def test_one_pass_entry_points(tmp_path):
    """run_ffmpeg_metrics(.., mdsi=True) and config "mdsi": true on a 5-frame 72 x 88 .y4m pair: the psnr / ssim logs are byte for
    byte those of a plain run, the log's values are Engine.mdsi's, and the row gains MDSI after the BRISQUE columns with every
    other column as without the key"""
    import rtvqa_amd
    from rtvqa_amd import frames, synth
    from rtvqa_amd import video_processing as vp
    h, w, n = 72, 88, 5
    r, d, planes, _, _ = _clip("yuv420p", h, w, 8, n)
    d[2] = r[2]                                                  # one identical frame: exactly 0 in the record and the log
    pr, pd = str(tmp_path / "ref.y4m"), str(tmp_path / "enc.y4m")
    frames.write_y4m(pr, r, h, w)
    frames.write_y4m(pd, d, h, w)
    logs = {k: [str(tmp_path / ("%s_%s.log" % (k, t))) for t in ("psnr", "ssim", "vmaf")] for k in ("plain", "mdsi", "feat", "both")}
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["plain"], batch_size=4) is None
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["mdsi"], batch_size=4, mdsi=True) is None
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["feat"], batch_size=4, gmsd=True, brisque=True) is None
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["both"], batch_size=2, gmsd=True, brisque=True, mdsi=True) is None
    assert not os.path.exists(logs["plain"][2])
    for k in (0, 1):
        for kind in ("mdsi", "feat", "both"):
            assert open(logs["plain"][k], "rb").read() == open(logs[kind][k], "rb").read(), (kind, k)
    with rtvqa_amd.Engine(0) as eng:
        want = eng.mdsi(r, d, planes)
    assert want["mdsi"][2] == 0.0 and want["dev"][2] == 0.0 and (want["mdsi"][[0, 1, 3, 4]] > 0).all()
    doc, feat, both = (json.load(open(logs[k][2])) for k in ("mdsi", "feat", "both"))
    assert list(doc["frames"][0]["metrics"]) == ["mdsi"] == list(doc["pooled_metrics"])
    names = list(feat["frames"][0]["metrics"])
    assert names[-1] == "brisque_35" and "mdsi" not in json.dumps(feat)
    assert list(both["frames"][0]["metrics"]) == names + ["mdsi"]
    for i in range(n):
        for dc in (doc, both):
            assert dc["frames"][i]["metrics"]["mdsi"] == float(want["mdsi"][i])
        assert {k: both["frames"][i]["metrics"][k] for k in names} == feat["frames"][i]["metrics"]
    assert {k: both["pooled_metrics"][k] for k in names} == feat["pooled_metrics"]
    bgr = synth.s_natural(n, h, w, seed=12)
    cfg = {"crf": 23, "resize_width": 64, "resize_height": 64, "frame_interval": 1, "batch_size": 4}

    def row(name, **kw):
        return vp.process_video_and_extract_metrics(pr, pd, dict(cfg, **kw), csv_file=str(tmp_path / (name + ".csv")),
                                                    column_order="fixed", encoded_bgr=bgr)

    def same(a, b):
        return a == b or (a != a and b != b)

    row0, row1 = row("row0"), row("row1", mdsi=True)
    k0 = list(row0)
    at = k0.index("SSIM") + 1
    assert list(row1) == k0[:at] + ["MDSI"] + k0[at:] and all(same(row0[k], row1[k]) for k in k0)
    assert abs(row1["MDSI"] - want["mdsi"].mean()) <= 1e-15
    row2, row3 = row("row2", brisque=True, batch_size=2), row("row3", brisque=True, mdsi=True, batch_size=2)
    k2 = list(row2)
    at = k2.index("BRISQUE_SIGMA2") + 1
    assert list(row3) == k2[:at] + ["MDSI"] + k2[at:] and all(same(row2[k], row3[k]) for k in k2)
    assert row3["MDSI"] == row1["MDSI"]
    # the same call without the key, and with it false: the same file, byte for byte, with no new column
    row("row0b", mdsi=False)
    assert open(str(tmp_path / "row0.csv"), "rb").read() == open(str(tmp_path / "row0b.csv"), "rb").read()
    assert b"MDSI" not in open(str(tmp_path / "row0.csv"), "rb").read()
    assert b"BRISQUE_SIGMA2,MDSI" in open(str(tmp_path / "row3.csv"), "rb").read()


def test_profile_names_the_two_kernels():
    import rtvqa_amd
    from rtvqa_amd import _native as N
    f, d, planes, _, _ = _clip("yuv420p", 72, 88, 8, 3)
    with rtvqa_amd.Engine(0) as eng:
        eng.lib.vqa_kernel_name.restype = C.c_char_p
        assert eng.lib.vqa_kernel_name(48) == b"k_mdsi_map" and eng.lib.vqa_kernel_name(49) == b"k_mdsi_dev"
        assert eng.lib.vqa_kernel_name(47) == b"?" and eng.lib.vqa_kernel_name(50) == b"?"
        eng.profile(True)
        eng.mdsi(f, d, planes)
        ms, cnt = C.c_double(0), C.c_int64(0)
        for k in (N.K_MDSI_MAP, N.K_MDSI_DEV):
            assert eng.lib.vqa_profile_read(eng.ctx, k, C.byref(ms), C.byref(cnt), 0) == N.VQA_OK
            assert cnt.value == 1 and ms.value > 0.0                      # one launch each for all planes of all frames
        prof = eng.profile_read(reset=True)
        assert prof["k_mdsi_map"][1] == 1 and prof["k_mdsi_dev"][1] == 1 and "k_gmsd" not in prof, prof
        eng.gmsd(f, d, planes)
        prof = eng.profile_read(reset=True)
        assert "k_mdsi_map" not in prof and "k_mdsi_dev" not in prof
        for bad in (N.K_EDGE, N.K_BRINK):                                  # ids 47 and 50 are unknown
            assert eng.lib.vqa_profile_read(eng.ctx, bad, C.byref(ms), C.byref(cnt), 0) == N.VQA_ERR_INVALID
