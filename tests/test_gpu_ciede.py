"""GPU: CIEDE2000 (vqa_ciede_submit / vqa_ciede_wait) through the C ABI, the engine, the one-pass stream and the reference-shaped
entry points, against the float64 NumPy restatement of tests/ciede_reference.py (written from the definition in include/vqa.h).

The bar was fixed before the kernel first ran: |de_mean - ref| <= 1e-4 ref + 2^-21 - the family's relative bar (VIF, ADM,
PSNR-HVS) plus the fixed-point term the header derives (half a 2^-20 quantum).  The contents are those tests/test_ciede_host.py
admits.  Largest gap seen on an MI355X: see DESIGN.md 4i."""
import ctypes as C
import json

import numpy as np
import pytest

import ciede_cases as CC
import ciede_reference as R
import motion_cases as K

pytestmark = pytest.mark.gpu

WORST = {"gap": 0.0, "tag": ""}
FIELDS = ("de_sum", "de_mean", "ciede2000")


def _check(got, ref, dist, planes, depth, model, weights, tag):
    fr, fd = R.split_planes(ref, planes), R.split_planes(dist, planes)
    h, w = planes[0][1], planes[0][0]
    assert got.shape == (len(fr),) and got.dtype.names == FIELDS
    for i in range(len(fr)):
        want = R.de_mean(fr[i], fd[i], depth, model, weights)
        g = float(got[i]["de_mean"])
        gap = abs(g - want) / want if want > 0 else abs(g)
        print("%s frame %d: de_mean %.9g (ref %.9g) gap %.2e, ciede2000 %.4f" % (tag, i, g, want, gap, got[i]["ciede2000"]))
        if gap > WORST["gap"]:
            WORST.update(gap=gap, tag=tag)
        assert abs(g - want) <= CC.GPU_BAR * want + R.quantum_bar(), (tag, i, g, want)
        # the record is the host formula of its own sum
        assert g == float(got[i]["de_sum"]) / (h * w)
        assert float(got[i]["ciede2000"]) == R.score(g) or abs(float(got[i]["ciede2000"]) - R.score(g)) <= 1e-12 * abs(R.score(g))


@pytest.mark.parametrize("geom,depth,layout,distortion", CC.matrix(), ids=CC.matrix_ids())
def test_parity_on_every_shape_and_sample_type(engine, geom, depth, layout, distortion):
    r, d, planes = CC.case(geom, depth, layout, distortion)
    model = CC.model_of(layout)
    assert engine.ciede_model(planes) == model
    for weights in CC.WEIGHTS:
        got = engine.ciede(r, d, planes, weights=weights)
        _check(got, r, d, planes, depth, model, weights, "%dx%d %s %s k=%s" % (geom[0], geom[1], layout, distortion, weights))


def test_the_worst_gap_of_the_parity_matrix():
    """runs after the parity tests of this module (pytest keeps the file's order): the figure DESIGN.md 4i quotes"""
    print("parity matrix: largest relative gap on de_mean %.3e (%s)" % (WORST["gap"], WORST["tag"]))


def test_exact_answers_on_the_device(engine):
    for (geom, depth, layout) in CC.GRID:
        r, d, planes = CC.case(geom, depth, layout, "noise4")
        same = engine.ciede(r, r.copy(), planes)
        assert same.tobytes()[:8] == bytes(8) and (same["de_mean"] == 0).all() and (same["ciede2000"] == np.inf).all()   # exactly 0
        a, b = engine.ciede(r, d, planes), engine.ciede(d, r, planes)
        assert a.tobytes() == b.tobytes(), (geom, layout)                                         # the pair is symmetric
        assert engine.ciede(r, d, planes, weights=(1.0, 1.0, 1.0)).tobytes() == a.tobytes()
        assert engine.ciede(r, d, planes, weights=None).tobytes() == a.tobytes()                  # NULL = (1, 1, 1)
        assert engine.ciede(r, d, planes, weights=(0.65, 1.0, 4.0)).tobytes() != a.tobytes()
    # a luma-only offset on a gray clip (U = V = 128 s): replication is invisible, 4:4:4 and 4:2:0 give the same bits
    # (the contents are ciede_cases.gray_offset's, admitted with the matrix)
    for depth in sorted({d for d, _ in CC.GRAY}):
        recs = []
        for chroma in ("444", "420"):
            assert (depth, chroma) in CC.GRAY
            f, g, pl = CC.gray_offset(depth, chroma)
            recs.append(engine.ciede(f, g, pl))
            _check(recs[-1], f, g, pl, depth, R.YUV709, (1.0, 1.0, 1.0), "gray+5 %d bits %s" % (depth, chroma))
        assert recs[0].tobytes() == recs[1].tobytes(), depth


def test_batches_positions_and_memory_kinds_give_the_same_bits(engine):
    """the same pair at several places of batches of 1, 3 and 8, from host, pinned and device memory; frame_ciede in chunks; a
    strided view and a region of interest of resident frames that lands on the sample-by-sample path"""
    from rtvqa_amd import video_processing as vp
    from rtvqa_amd.engine import DeviceFrames
    h, w, layout, n = 72, 88, "yuv420p", 8
    r, d, planes = CC.pair_clip(layout, h, w, 8, seed=11, n=n)
    whole = engine.ciede(r, d, planes)
    assert engine.ciede(r, d, planes).tobytes() == whole.tobytes()          # run to run
    one = whole[5:6].tobytes()
    assert engine.ciede(r[5:6], d[5:6], planes).tobytes() == one             # a batch of 1
    for order in ([5, 0, 5], [1, 5, 2], [5, 1, 2, 3, 5, 6, 7, 5]):           # batches of 3 and 8
        got = engine.ciede(r[order], d[order], planes)
        for pos, k in enumerate(order):
            assert got[pos].tobytes() == whole[k].tobytes(), (order, pos)
    dr, dd = engine.upload(r), engine.upload(d)
    assert engine.ciede(dr, dd, planes).tobytes() == whole.tobytes()
    assert engine.ciede(dr.slice(5, 6), dd.slice(5, 6), planes).tobytes() == one
    pr, pd = engine.alloc_pinned(r.shape), engine.alloc_pinned(d.shape)
    pr[...], pd[...] = r, d
    assert engine.is_pinned(pr)
    assert engine.ciede(pr, pd, planes).tobytes() == whole.tobytes()
    for src in ((r, d), (pr, pd), (dr, dd)):
        for bs in (1, 3, 64):
            score, mean = vp.frame_ciede(src[0], src[1], layout, h, w, batch_size=bs)
            assert score.shape == (n,)
            assert score.tobytes() == np.ascontiguousarray(whole["ciede2000"]).tobytes(), (type(src[0]), bs)
            assert mean.tobytes() == np.ascontiguousarray(whole["de_mean"]).tobytes(), (type(src[0]), bs)
    engine.free_pinned(pr)
    engine.free_pinned(pd)
    # every second frame of the resident clips: frame_stride does the stepping
    odd = [DeviceFrames(x.ptr + x.frame_stride, 4, x.h, x.w, frame_stride=2 * x.frame_stride, row_stride=x.row_stride, owner=x,
                        channels=x.channels) for x in (dr, dd)]
    assert engine.ciede(odd[0], odd[1], planes).tobytes() == whole[1::2].tobytes()
    # windows of resident 60 x 80 4:4:4 frames (uploaded as [n, 3 * 60, 80]; the window's plane k starts k * 60 rows further down):
    # (9, 13) with 45 columns is unaligned (sample by sample), (8, 16) with 48 columns is aligned (one load per row); each against
    # the same samples as a frame of their own (ciede_cases.roi_cut: those contents are admitted with the matrix)
    H, W = CC.ROI_FRAME
    g3, gd3 = CC.roi_source()
    g, gd = g3.reshape(CC.ROI_N, -1), gd3.reshape(CC.ROI_N, -1)
    dg, dgd = engine.upload(g3), engine.upload(gd3)
    assert CC.ROIS == [(9, 13, 35, 45), (8, 16, 36, 48)]
    for (y0, x0, hh, ww) in CC.ROIS:
        roi = [(ww, hh, k * H * W, W, 1) for k in range(3)]
        cut = CC.roi_cut((y0, x0, hh, ww))
        own = cut[2]
        alone = engine.ciede(cut[0], cut[1], own)
        a, b = dg.roi(y0, y0 + hh, x0, x0 + ww), dgd.roi(y0, y0 + hh, x0, x0 + ww)
        assert engine.ciede(a, b, roi).tobytes() == alone.tobytes()
        assert engine.ciede(g, gd, [(ww, hh, k * H * W + y0 * W + x0, W, 1) for k in range(3)]).tobytes() == alone.tobytes()
        _check(alone, cut[0], cut[1], own, 8, R.YUV709, (1.0, 1.0, 1.0), "roi %d,%d" % (y0, x0))
        # the same bytes one byte off any alignment: the other load path, the same bits
        moved = []
        for x in cut[:2]:
            buf = np.zeros(x.size + 1, np.uint8)
            buf[1:] = x.reshape(-1)
            moved.append(buf[1:].reshape(x.shape))
        assert moved[0].ctypes.data % 2 == 1 and engine.ciede(moved[0], moved[1], own).tobytes() == alone.tobytes()


def _submit(engine, f, d, planes, n=None, model=0, weights=None):
    from rtvqa_amd import _native as N
    from rtvqa_amd.engine import plane_descs
    fb = K.flat(f).shape[1] * f.dtype.itemsize
    k = (C.c_double * 3)(*weights) if weights is not None else None
    return engine.lib.vqa_ciede_submit(engine.ctx, f.ctypes.data, d.ctypes.data, N.VQA_MEM_HOST, f.shape[0] if n is None else n,
                                       fb, fb, plane_descs(planes), len(planes), model, k)


def test_the_state_machine_and_the_refusals(engine):
    from rtvqa_amd import _native as N
    from rtvqa_amd.engine import plane_descs, yuv_planes
    f, d, planes = CC.pair_clip("yuv420p", 64, 96, 8, seed=8, n=2, kind="noise")
    want = engine.ciede(f, d, planes)
    hwant, qwant = engine.psnr_hvs(f, d, planes), engine.quality(f, d, planes)
    eout, hout, qout = (N.VqaCiedeMetrics * 2)(), (N.VqaPsnrHvsMetrics * 6)(), (N.VqaPlaneMetrics * 6)()
    lib, ctx = engine.lib, engine.ctx

    def idle():
        return lib.vqa_ciede_wait(ctx, eout, 2) == N.VQA_ERR_STATE
    assert idle()                                                         # wait without submit
    # submit while pending; the other kinds' waits on a CIEDE2000 batch; the batch survives all of them
    assert _submit(engine, f, d, planes) == N.VQA_OK
    assert _submit(engine, f, d, planes) == N.VQA_ERR_STATE
    assert lib.vqa_quality_wait(ctx, qout, 6) == N.VQA_ERR_STATE
    assert lib.vqa_psnr_hvs_wait(ctx, hout, 6) == N.VQA_ERR_STATE
    assert lib.vqa_trim(ctx) == N.VQA_ERR_STATE
    assert lib.vqa_ciede_wait(ctx, eout, 6) == N.VQA_ERR_STATE           # a wrong entry count: one entry per FRAME
    assert lib.vqa_ciede_wait(ctx, eout, 2) == N.VQA_OK
    assert bytes(eout) == want.tobytes()
    # a wait with another kind pending; that batch survives
    fb = K.flat(f).shape[1]
    pd = plane_descs(planes)
    assert lib.vqa_psnr_hvs_submit(ctx, f.ctypes.data, d.ctypes.data, N.VQA_MEM_HOST, 2, fb, fb, pd, 3) == N.VQA_OK
    assert idle()
    assert lib.vqa_psnr_hvs_wait(ctx, hout, 6) == N.VQA_OK and bytes(hout) == hwant.tobytes()
    # in flight next to a quality and a PSNR-HVS batch from one upload: each wait collects its own, in any order
    df, dd = engine.upload(f), engine.upload(d)
    for order in (("ciede", "quality", "psnr_hvs"), ("psnr_hvs", "ciede", "quality")):
        engine.quality_submit(df, dd, planes)
        engine.psnr_hvs_submit(df, dd, planes)
        engine.ciede_submit(df, dd, planes)
        wants = {"ciede": want, "quality": qwant, "psnr_hvs": hwant}
        for kind in order:
            assert getattr(engine, kind + "_wait")().tobytes() == wants[kind].tobytes(), (order, kind)
    engine.quality_submit(f, d, planes)          # host frames share the staging of a pending quality batch
    engine.ciede_submit(f, d, planes)
    assert engine.ciede_wait().tobytes() == want.tobytes() and engine.quality_wait().tobytes() == qwant.tobytes()
    # the refusals: each leaves nothing in flight, and the next valid submit works
    Y, U, V = planes
    z16 = np.zeros((2, 64 * 96 * 3), np.uint16)
    p10 = yuv_planes(64, 96, "420", 10)
    nan = float("nan")
    refused = [
        (f, planes[:2], {}, N.VQA_ERR_INVALID),                                             # two planes
        (f, planes + [V], {}, N.VQA_ERR_INVALID),                                           # four
        (f, [Y, U, (V[0] - 1,) + V[1:]], {}, N.VQA_ERR_INVALID),                            # U and V geometries differ
        (f, [Y, U, V[:3] + (V[3] + 2, V[4])], {}, N.VQA_ERR_INVALID),                       # (their row strides too)
        (f, [Y, (40, 32, U[2], 40, 1), (40, 32, V[2], 40, 1)], {}, N.VQA_ERR_INVALID),      # neither full nor ceil-half
        (f, [Y, (48, 30, U[2], 48, 1), (48, 30, V[2], 48, 1)], {}, N.VQA_ERR_INVALID),
        (f, planes, {"model": N.CIEDE_BGR}, N.VQA_ERR_INVALID),                             # B, G, R must share one geometry
        (f, planes, {"model": 2}, N.VQA_ERR_INVALID),
        (z16, p10[:1] + [p[:5] for p in p10[1:]], {}, N.VQA_ERR_INVALID),                   # mixed depths
        (f, [(16, 15, 0, 16, 1), (8, 8, 240, 8, 1), (8, 8, 304, 8, 1)], {}, N.VQA_ERR_UNSUPPORTED),   # luma 15 rows x 16
        (f, [(15, 16, 0, 15, 1), (8, 8, 240, 8, 1), (8, 8, 304, 8, 1)], {}, N.VQA_ERR_UNSUPPORTED),
        (f, [(16385, 16384, 0, 16385, 1)] * 3, {}, N.VQA_ERR_UNSUPPORTED),                  # more than 2^28 pixels
        (f, planes, {"weights": (0.0, 1.0, 1.0)}, N.VQA_ERR_INVALID),
        (f, planes, {"weights": (1.0, -1.0, 1.0)}, N.VQA_ERR_INVALID),
        (f, planes, {"weights": (1.0, 1.0, nan)}, N.VQA_ERR_INVALID),
        (f, planes, {"weights": (float("inf"), 1.0, 1.0)}, N.VQA_ERR_INVALID),
    ]
    for k, (buf, pl, kw, status) in enumerate(refused):
        assert _submit(engine, buf, buf, pl, n=1, **kw) == status, k
        assert idle(), k
    assert lib.vqa_ciede_submit(ctx, f.ctypes.data, d.ctypes.data, N.VQA_MEM_HOST, 2, fb - 1, fb, pd, 3, 0, None) == N.VQA_ERR_INVALID
    assert lib.vqa_ciede_submit(ctx, f.ctypes.data, None, N.VQA_MEM_HOST, 2, fb, fb, pd, 3, 0, None) == N.VQA_ERR_INVALID
    assert idle()
    # a 16 x 16 4:2:0 frame is measured: its 8 x 8 chroma planes are no limit
    z = np.zeros((1, 16 * 16 * 3 // 2), np.uint8)
    assert _submit(engine, z, z, yuv_planes(16, 16, "420", 8)) == N.VQA_OK and lib.vqa_ciede_wait(ctx, eout, 1) == N.VQA_OK
    assert engine.ciede(f, d, planes).tobytes() == want.tobytes()
    engine.trim()
    assert engine.ciede(f, d, planes).tobytes() == want.tobytes()
    assert engine.quality(f, d, planes).tobytes() == qwant.tobytes()


def test_one_pass_entry_points(tmp_path):
    """run_ffmpeg_metrics(.., psnr_hvs=True, ciede=True) on a 72 x 88 4:2:0 clip of 5 frames in chunks of 2: the log's ciede2000
    values are frame_ciede's; every other key of the log and the psnr / ssim files are those of a run without ciede, byte for byte;
    process_video_and_extract_metrics with "ciede": true gains CIEDE2000 after PSNR_HVSM and nothing else changes"""
    from rtvqa_amd import frames, synth
    from rtvqa_amd import video_processing as vp
    h, w, n = 72, 88, 5
    r, d, planes = CC.pair_clip("yuv420p", h, w, 8, seed=6, n=n)
    d[2] = r[2]                                                  # one identical frame: inf in the record, 100.0 in the log
    pr, pd = str(tmp_path / "ref.y4m"), str(tmp_path / "enc.y4m")
    frames.write_y4m(pr, r, h, w)
    frames.write_y4m(pd, d, h, w)
    logs = {k: [str(tmp_path / ("%s_%s.log" % (k, t))) for t in ("psnr", "ssim", "vmaf")] for k in ("hvs", "both", "only", "k")}
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["hvs"], batch_size=2, psnr_hvs=True) is None
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["both"], batch_size=2, psnr_hvs=True, ciede=True) is None
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["only"], batch_size=3, ciede=True) is None
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["k"], batch_size=3, ciede=True, ciede_weights=(0.65, 1.0, 4.0)) is None
    for k in (0, 1):
        for kind in ("both", "only", "k"):
            assert open(logs["hvs"][k], "rb").read() == open(logs[kind][k], "rb").read(), (kind, k)
    score, mean = vp.frame_ciede(r, d, "yuv420p", h, w, batch_size=2)
    assert score[2] == np.inf and mean[2] == 0.0 and np.isfinite(score[[0, 1, 3, 4]]).all()         # nothing capped here
    hvs, both, only, kk = (json.load(open(logs[k][2])) for k in ("hvs", "both", "only", "k"))
    names = list(hvs["frames"][0]["metrics"])
    assert names == ["psnr_hvs", "psnr_hvsm"] and "ciede2000" not in json.dumps(hvs)
    assert list(both["frames"][0]["metrics"]) == names + ["ciede2000"] == list(both["pooled_metrics"])
    assert list(only["frames"][0]["metrics"]) == ["ciede2000"]
    cap = np.minimum(score, 100.0)
    for i in range(n):
        assert both["frames"][i]["metrics"]["ciede2000"] == float(cap[i]) == only["frames"][i]["metrics"]["ciede2000"]
        assert {k: both["frames"][i]["metrics"][k] for k in names} == hvs["frames"][i]["metrics"]
    assert both["frames"][2]["metrics"]["ciede2000"] == 100.0
    assert {k: both["pooled_metrics"][k] for k in names} == hvs["pooled_metrics"]
    sk, _ = vp.frame_ciede(r, d, "yuv420p", h, w, weights=(0.65, 1.0, 4.0))
    assert [fr["metrics"]["ciede2000"] for fr in kk["frames"]] == [float(x) for x in np.minimum(sk, 100.0)]
    assert sk[0] != score[0]
    with pytest.raises(ValueError, match="ciede needs three planes"):
        vp.frame_ciede(r[:, :h * w], d[:, :h * w], "gray", h, w)
    bgr = synth.s_natural(n, h, w, seed=12)
    cfg = {"crf": 23, "resize_width": 64, "resize_height": 64, "frame_interval": 1, "batch_size": 2}

    def row(name, **kw):
        return vp.process_video_and_extract_metrics(pr, pd, dict(cfg, **kw), csv_file=str(tmp_path / (name + ".csv")),
                                                    column_order="fixed", encoded_bgr=bgr)

    def same(a, b):
        return a == b or (a != a and b != b)

    row0, row1 = row("row0", psnr_hvs=True), row("row1", psnr_hvs=True, ciede=True)
    k0 = list(row0)
    at = k0.index("PSNR_HVSM") + 1
    assert list(row1) == k0[:at] + ["CIEDE2000"] + k0[at:]
    assert all(same(row0[k], row1[k]) for k in k0)
    assert abs(row1["CIEDE2000"] - cap.mean()) <= 1e-12
    row("row0b", psnr_hvs=True, ciede=False)
    assert open(str(tmp_path / "row0.csv"), "rb").read() == open(str(tmp_path / "row0b.csv"), "rb").read()
    assert b"CIEDE2000" not in open(str(tmp_path / "row0.csv"), "rb").read()
    assert b"PSNR_HVSM,CIEDE2000" in open(str(tmp_path / "row1.csv"), "rb").read()
    rk = row("row2", ciede=True, ciede_weights=[0.65, 1, 4])
    assert abs(rk["CIEDE2000"] - np.minimum(sk, 100.0).mean()) <= 1e-12 and "PSNR_HVS" not in rk


def test_profile_counts_one_launch_per_submit():
    import rtvqa_amd
    from rtvqa_amd import _native as N
    f, d, planes = CC.pair_clip("yuv420p", 72, 88, 8, seed=9, n=3)
    with rtvqa_amd.Engine(0) as eng:
        eng.lib.vqa_kernel_name.restype = C.c_char_p
        assert eng.lib.vqa_kernel_name(N.K_CIEDE) == b"k_ciede" and eng.lib.vqa_kernel_name(N.K_PAST) == b"?"
        assert eng.lib.vqa_kernel_name(25) is not None
        eng.profile(True)
        eng.ciede(f, d, planes)
        ms, cnt = C.c_double(0), C.c_int64(0)
        assert eng.lib.vqa_profile_read(eng.ctx, N.K_CIEDE, C.byref(ms), C.byref(cnt), 0) == N.VQA_OK
        assert cnt.value == 1 and ms.value > 0.0                          # one launch for the three planes of all frames
        prof = eng.profile_read(reset=True)
        assert prof["k_ciede"][1] == 1 and "k_psnr_hvs" not in prof, prof
        eng.ciede(f, d, planes)
        eng.ciede(f, d, planes, weights=(0.65, 1.0, 4.0))
        assert eng.profile_read(reset=True)["k_ciede"][1] == 2
        eng.psnr_hvs(f, d, planes)
        assert "k_ciede" not in eng.profile_read(reset=True)
        for bad in (N.K_PAST, N.K_BEYOND):                                 # ids 24 and 26 are unknown
            assert eng.lib.vqa_profile_read(eng.ctx, bad, C.byref(ms), C.byref(cnt), 0) == N.VQA_ERR_INVALID
