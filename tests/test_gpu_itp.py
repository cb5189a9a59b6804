"""GPU: dE_ITP (vqa_itp_submit / vqa_itp_wait) through the C ABI, the engine, the one-pass stream and the reference-shaped entry
points, against the float64 NumPy restatement of tests/itp_reference.py (written from the definition in include/vqa.h).

The bar was fixed before the kernel first ran: de_mean and de_max within 2^-20 of the UNQUANTISED float64 restatement - half of it
is the quantum's half (derived: every pixel is rounded to 2^-20 once), the other half is room for last-ulp differences between the
device's pow / exp and NumPy's.  Word equality with the quantised restatement is NOT demanded (one such ulp may flip one rint);
what is demanded byte for byte is that the same pair gives the same two words wherever it runs.  Largest gap seen on an MI355X:
see DESIGN.md 4r."""
import ctypes as C
import json

import numpy as np
import pytest

import itp_cases as IC
import itp_reference as R

pytestmark = pytest.mark.gpu

WORST = {"mean": 0.0, "max": 0.0, "tag_mean": "", "tag_max": ""}
FIELDS = ("sum_q", "max_q", "de_sum", "de_mean", "de_max")


def _check(got, want, h, w, tag):
    """records of the device against the restatement's, and the record against its own words"""
    assert got.shape == (len(want),) and got.dtype.names == FIELDS
    for i, ref in enumerate(want):
        g_mean, g_max = float(got[i]["de_mean"]), float(got[i]["de_max"])
        gap_mean, gap_max = abs(g_mean - ref["de_mean"]), abs(g_max - ref["de_max"])
        print("%s frame %d: de_mean %.12g (ref %.12g, gap %.2e) de_max %.12g (ref %.12g, gap %.2e) words %s the quantised ref's"
              % (tag, i, g_mean, ref["de_mean"], gap_mean, g_max, ref["de_max"], gap_max,
                 "=" if (int(got[i]["sum_q"]), int(got[i]["max_q"])) == (ref["sum_q"], ref["max_q"]) else "!="))
        if gap_mean > WORST["mean"]:
            WORST.update(mean=gap_mean, tag_mean="%s frame %d" % (tag, i))
        if gap_max > WORST["max"]:
            WORST.update(max=gap_max, tag_max="%s frame %d" % (tag, i))
        assert gap_mean <= R.BAR and gap_max <= R.BAR, (tag, i, g_mean, ref["de_mean"], g_max, ref["de_max"])
        # the record is the host formula of its own words
        assert float(got[i]["de_sum"]) == int(got[i]["sum_q"]) / R.FIX
        assert g_mean == float(got[i]["de_sum"]) / (h * w) and g_max == int(got[i]["max_q"]) / R.FIX


@pytest.mark.parametrize("geom,depth,layout,content,tname,transfer,full", IC.matrix(), ids=IC.matrix_ids())
def test_parity_on_every_shape_content_and_transfer(engine, geom, depth, layout, content, tname, transfer, full):
    h, w = geom
    n = max(IC.COUNTS)
    r, d, planes = IC.clip(content, layout, h, w, depth, n, full_range=full)
    model = IC.model_of(layout)
    assert engine.itp_model(planes) == model
    want = IC.reference(r, d, planes, depth, model, transfer, full, key=(geom, depth, layout, content, transfer, full))
    got = engine.itp(r, d, planes, transfer=tname, full_range=full)
    tag = "%dx%d %s %s %s %s" % (w, h, layout, content, tname, "full" if full else "limited")
    _check(got, want, h, w, tag)
    for m in IC.COUNTS:                                                   # n = 1 and n = 3: the same words
        assert engine.itp(r[:m], d[:m], planes, transfer=tname, full_range=full).tobytes() == got[:m].tobytes(), m
    if content == "equal":
        assert got.tobytes() == bytes(got.nbytes)                         # both words, and every double, exactly 0
    if content == "graystep" and tname == "pq":
        answer = IC.graystep_answer(layout, depth, full)
        assert (np.abs(got["de_mean"] - answer) <= R.BAR).all() and (np.abs(got["de_max"] - answer) <= R.BAR).all()
        if (depth, layout, full) == (10, "yuv420p10le", False):
            assert answer == 720.0 / 876.0
    if content == "extremes":
        assert (got["de_max"] < 6800.0).all() and (got["de_mean"] > 100.0).all()   # black against peak: hundreds of JNDs, far below the bound
    if layout == "bgr24":                                                 # the range does not reach B, G, R
        assert engine.itp(r, d, planes, transfer=tname, full_range=True).tobytes() == got.tobytes()


def test_the_worst_gap_of_the_parity_matrix():
    """runs after the parity tests of this module (pytest keeps the file's order): the figure DESIGN.md 4r quotes"""
    print("parity matrix: largest gap %.3e on de_mean (%s), %.3e on de_max (%s); bar %.3e"
          % (WORST["mean"], WORST["tag_mean"], WORST["max"], WORST["tag_max"], R.BAR))


def test_the_pair_is_symmetric_and_the_switches_matter(engine):
    (h, w), depth, layout = IC.RANGES_ON
    r, d, planes = IC.clip("noise3", layout, h, w, depth, 2)
    a = engine.itp(r, d, planes)
    assert engine.itp(d, r, planes).tobytes() == a.tobytes()                  # every step is symmetric in the pair
    assert engine.itp(r, d, planes, transfer="pq", full_range=False).tobytes() == a.tobytes()
    assert engine.itp(r, d, planes, model=0, transfer=0).tobytes() == a.tobytes()
    assert engine.itp(r, d, planes, transfer="hlg").tobytes() != a.tobytes()
    assert engine.itp(r, d, planes, full_range=True).tobytes() != a.tobytes()


def test_batches_positions_memory_kinds_and_views_give_the_same_words(engine):
    """the same pair alone and at each place of a batch of 3, from host, pinned and device memory; every second frame of a
    resident clip through the frame stride; the one-load-per-row path against the same samples through a view that cannot take
    it; windows of resident frames against the same samples as frames of their own"""
    from rtvqa_amd import video_processing as vp
    from rtvqa_amd.engine import DeviceFrames
    (h, w), depth, layout = IC.VECTOR
    n = 4
    r, d, planes = IC.clip("noise3", layout, h, w, depth, n, seed=3)
    whole = engine.itp(r, d, planes)
    _check(whole, IC.reference(r, d, planes, depth, R.YUV2020, R.PQ, False), h, w, "64x36 batch")
    assert engine.itp(r, d, planes).tobytes() == whole.tobytes()            # run to run
    one = whole[1:2].tobytes()
    assert engine.itp(r[1:2], d[1:2], planes).tobytes() == one               # alone
    for order in ([1, 0, 2], [0, 1, 3], [2, 3, 1]):                          # in a batch of 3, at each position
        got = engine.itp(r[order], d[order], planes)
        for pos, k in enumerate(order):
            assert got[pos].tobytes() == whole[k].tobytes(), (order, pos)
    dr, dd = engine.upload(r), engine.upload(d)
    assert engine.itp(dr, dd, planes).tobytes() == whole.tobytes()
    assert engine.itp(dr.slice(1, 2), dd.slice(1, 2), planes).tobytes() == one
    pr, pd = engine.alloc_pinned(r.shape, np.uint16), engine.alloc_pinned(d.shape, np.uint16)
    pr[...], pd[...] = r, d
    assert engine.is_pinned(pr)
    assert engine.itp(pr, pd, planes).tobytes() == whole.tobytes()
    for src in ((r, d), (pr, pd), (dr, dd)):
        for bs in (1, 3, 64):
            mean, mx = vp.frame_delta_itp(src[0], src[1], layout, h, w, batch_size=bs)
            assert mean.tobytes() == np.ascontiguousarray(whole["de_mean"]).tobytes(), (type(src[0]), bs)
            assert mx.tobytes() == np.ascontiguousarray(whole["de_max"]).tobytes(), (type(src[0]), bs)
    engine.free_pinned(pr)
    engine.free_pinned(pd)
    # every second frame of the resident clips: frame_stride does the stepping
    odd = [DeviceFrames(x.ptr + x.frame_stride, 2, x.h, x.w, frame_stride=2 * x.frame_stride, row_stride=x.row_stride, owner=x,
                        channels=x.channels, itemsize=x.itemsize) for x in (dr, dd)]
    assert engine.itp(odd[0], odd[1], planes).tobytes() == whole[1::2].tobytes()
    # one sample of padding in front of every frame: every plane starts 2 bytes off the alignment of a row load, so the same
    # samples go sample by sample - the same words
    pad = [np.concatenate([np.zeros((n, 1), np.uint16), x], axis=1) for x in (r, d)]
    shifted = [(p[0], p[1], p[2] + 2) + tuple(p[3:]) for p in planes]
    assert engine.itp(pad[0], pad[1], shifted).tobytes() == whole.tobytes()
    dp = [engine.upload(x) for x in pad]
    assert engine.itp(dp[0], dp[1], shifted).tobytes() == whole.tobytes()
    # windows of the resident 64 x 36 frames read as 4:4:4 (uploaded as [n, 3 * 36, 64]; plane k starts 36 rows further down):
    # (5, 3) with 33 columns is unaligned and ragged (sample by sample), (4, 8) with 40 columns is aligned (one load per row)
    m = 2
    a3, b3, _ = IC.clip("noise3", "yuv444p10le", h, w, depth, m, seed=4)
    a3, b3 = a3.reshape(m, 3 * h, w), b3.reshape(m, 3 * h, w)
    da, db = engine.upload(a3), engine.upload(b3)
    for win in IC.ROIS:
        y0, x0, hh, ww = win
        roi = [(ww, hh, k * h * w * 2, w * 2, 2, depth) for k in range(3)]
        ca, own = IC.window_cut(a3, win, m)
        cb, _ = IC.window_cut(b3, win, m)
        alone = engine.itp(ca, cb, own)
        _check(alone, IC.reference(ca, cb, own, depth, R.YUV2020, R.PQ, False), hh, ww, "window %d,%d" % (y0, x0))
        assert engine.itp(da.roi(y0, y0 + hh, x0, x0 + ww), db.roi(y0, y0 + hh, x0, x0 + ww), roi).tobytes() == alone.tobytes()
        flat = [(ww, hh, (k * h * w + y0 * w + x0) * 2, w * 2, 2, depth) for k in range(3)]
        assert engine.itp(a3.reshape(m, -1), b3.reshape(m, -1), flat).tobytes() == alone.tobytes()


def test_in_flight_next_to_ciede_and_mdsi(engine):
    (h, w), depth, layout = IC.VECTOR
    r, d, planes = IC.clip("noise3", layout, h, w, depth, 3, seed=5)
    want = {"itp": engine.itp(r, d, planes, transfer="hlg"), "ciede": engine.ciede(r, d, planes), "mdsi": engine.mdsi(r, d, planes)}
    dr, dd = engine.upload(r), engine.upload(d)
    for src in ((dr, dd), (r, d)):                                        # resident frames; host frames share one staging
        for order in (("itp", "ciede", "mdsi"), ("mdsi", "itp", "ciede"), ("ciede", "mdsi", "itp")):
            engine.ciede_submit(src[0], src[1], planes)
            engine.itp_submit(src[0], src[1], planes, transfer="hlg")
            engine.mdsi_submit(src[0], src[1], planes)
            for kind in order:
                assert getattr(engine, kind + "_wait")().tobytes() == want[kind].tobytes(), (order, kind)


def _submit(engine, f, d, planes, n=None, model=0, transfer=0, full_range=0):
    from rtvqa_amd import _native as N
    from rtvqa_amd.engine import plane_descs
    fb = f.reshape(f.shape[0], -1).shape[1] * f.dtype.itemsize
    return engine.lib.vqa_itp_submit(engine.ctx, f.ctypes.data, d.ctypes.data, N.VQA_MEM_HOST, f.shape[0] if n is None else n,
                                     fb, fb, plane_descs(planes), len(planes), model, transfer, full_range)


def test_the_state_machine_and_the_refusals(engine):
    from rtvqa_amd import _native as N
    from rtvqa_amd.engine import plane_descs, yuv_planes
    f, d, planes = IC.clip("noise3", "yuv420p", 32, 48, 8, 2, seed=8)
    want = engine.itp(f, d, planes)
    cwant = engine.ciede(f, d, planes)
    iout, eout = (N.VqaItpMetrics * 2)(), (N.VqaCiedeMetrics * 2)()
    lib, ctx = engine.lib, engine.ctx

    def idle():
        return lib.vqa_itp_wait(ctx, iout, 2) == N.VQA_ERR_STATE
    assert idle()                                                         # wait without submit
    assert _submit(engine, f, d, planes) == N.VQA_OK
    assert _submit(engine, f, d, planes) == N.VQA_ERR_STATE              # submit while pending
    assert lib.vqa_ciede_wait(ctx, eout, 2) == N.VQA_ERR_STATE           # another kind's wait: the batch survives
    assert lib.vqa_trim(ctx) == N.VQA_ERR_STATE
    assert lib.vqa_itp_wait(ctx, iout, 6) == N.VQA_ERR_STATE             # a wrong entry count: one entry per FRAME
    assert lib.vqa_itp_wait(ctx, iout, 2) == N.VQA_OK
    assert bytes(iout) == want.tobytes()
    fb = f.shape[1]
    pd = plane_descs(planes)
    assert lib.vqa_ciede_submit(ctx, f.ctypes.data, d.ctypes.data, N.VQA_MEM_HOST, 2, fb, fb, pd, 3, 0, None) == N.VQA_OK
    assert idle()                                                         # a wait with only another kind pending
    assert lib.vqa_ciede_wait(ctx, eout, 2) == N.VQA_OK and bytes(eout) == cwant.tobytes()
    # the refusals: each leaves nothing in flight, and the next valid submit works
    Y, U, V = planes
    z16 = np.zeros((2, 32 * 48 * 3), np.uint16)
    p10 = yuv_planes(32, 48, "420", 10)
    refused = [
        (f, planes[:2], {}, N.VQA_ERR_INVALID),                                             # two planes
        (f, planes[:1], {}, N.VQA_ERR_INVALID),                                             # one
        (f, planes + [V], {}, N.VQA_ERR_INVALID),                                           # four
        (f, [Y, U, (V[0] - 1,) + V[1:]], {}, N.VQA_ERR_INVALID),                            # Cb and Cr geometries differ
        (f, [Y, U, V[:3] + (V[3] + 2, V[4])], {}, N.VQA_ERR_INVALID),                       # (their row strides too)
        (f, [Y, (20, 16, U[2], 20, 1), (20, 16, V[2], 20, 1)], {}, N.VQA_ERR_INVALID),      # neither full nor ceil-half
        (f, [Y, (24, 15, U[2], 24, 1), (24, 15, V[2], 24, 1)], {}, N.VQA_ERR_INVALID),
        (f, planes, {"model": N.ITP_BGR}, N.VQA_ERR_INVALID),                               # B, G, R must share one geometry
        (f, planes, {"model": 2}, N.VQA_ERR_INVALID),
        (f, planes, {"model": -1}, N.VQA_ERR_INVALID),
        (f, planes, {"transfer": 2}, N.VQA_ERR_INVALID),
        (f, planes, {"transfer": -1}, N.VQA_ERR_INVALID),
        (f, planes, {"full_range": 2}, N.VQA_ERR_INVALID),
        (f, planes, {"full_range": -1}, N.VQA_ERR_INVALID),
        (z16, p10[:1] + [p[:5] for p in p10[1:]], {}, N.VQA_ERR_INVALID),                   # mixed depths
        (f, [(16, 15, 0, 16, 1), (8, 8, 240, 8, 1), (8, 8, 304, 8, 1)], {}, N.VQA_ERR_UNSUPPORTED),   # luma 15 rows x 16
        (f, [(15, 16, 0, 15, 1), (8, 8, 240, 8, 1), (8, 8, 304, 8, 1)], {}, N.VQA_ERR_UNSUPPORTED),
        (f, [(16385, 16384, 0, 16385, 1)] * 3, {}, N.VQA_ERR_UNSUPPORTED),                  # more than 2^28 pixels
    ]
    for k, (buf, pl, kw, status) in enumerate(refused):
        assert _submit(engine, buf, buf, pl, n=1, **kw) == status, k
        assert idle(), k
    assert lib.vqa_itp_submit(ctx, f.ctypes.data, d.ctypes.data, N.VQA_MEM_HOST, 2, fb - 1, fb, pd, 3, 0, 0, 0) == N.VQA_ERR_INVALID
    assert lib.vqa_itp_submit(ctx, f.ctypes.data, None, N.VQA_MEM_HOST, 2, fb, fb, pd, 3, 0, 0, 0) == N.VQA_ERR_INVALID
    assert idle()
    with pytest.raises(ValueError, match="transfer must be 'pq' or 'hlg'"):
        engine.itp(f, d, planes, transfer="sdr")
    with pytest.raises(ValueError, match="full_range must be True or False"):
        engine.itp(f, d, planes, full_range="full")
    assert idle()
    # a 16 x 16 4:2:0 frame is measured: its 8 x 8 chroma planes are no limit
    z = np.zeros((1, 16 * 16 * 3 // 2), np.uint8)
    assert _submit(engine, z, z, yuv_planes(16, 16, "420", 8)) == N.VQA_OK and lib.vqa_itp_wait(ctx, iout, 1) == N.VQA_OK
    assert engine.itp(f, d, planes).tobytes() == want.tobytes()
    engine.trim()
    assert engine.itp(f, d, planes).tobytes() == want.tobytes()
    assert engine.ciede(f, d, planes).tobytes() == cwant.tobytes()


def test_one_pass_entry_points(engine, tmp_path):
    """Engine.itp, frame_delta_itp, a Quality(itp=True) pass and the delta_itp values of run_ffmpeg_metrics' log agree exactly; every
    other key of the log and the psnr / ssim files are those of a run without delta_itp, byte for byte; the row gains DELTA_ITP and
    DELTA_ITP_MAX after MDSI and nothing else changes; without the key nothing changes at all"""
    from rtvqa_amd import stream, synth
    from rtvqa_amd import video_processing as vp
    (h, w), depth, layout = IC.VECTOR
    n = 5
    r, d, planes = IC.clip("noise3", layout, h, w, depth, n, seed=6)
    d[2] = r[2]                                                  # one identical frame: exactly 0
    whole = engine.itp(r, d, planes)
    assert whole["sum_q"][2] == 0 and whole["max_q"][2] == 0 and (whole["sum_q"][[0, 1, 3, 4]] > 0).all()
    mean, mx = vp.frame_delta_itp(r, d, layout, h, w, batch_size=2)
    assert mean.tobytes() == np.ascontiguousarray(whole["de_mean"]).tobytes()
    assert mx.tobytes() == np.ascontiguousarray(whole["de_max"]).tobytes()
    q, _ = stream.run(d, r, quality=stream.Quality(planes, mdsi=True, itp=True), batch_size=2)
    assert q[-1].tobytes() == whole.tobytes() and q[-2].dtype.names[-1] == "mdsi"      # the last element, after MDSI's
    q, _ = stream.run(d, r, quality=stream.Quality(planes, itp="only", itp_transfer="hlg", itp_full_range=True), batch_size=3)
    assert q[0] is None and q[-1].tobytes() == engine.itp(r, d, planes, transfer="hlg", full_range=True).tobytes()
    kw = dict(layout=layout, height=h, width=w)
    logs = {k: [str(tmp_path / ("%s_%s.log" % (k, t))) for t in ("psnr", "ssim", "vmaf")] for k in ("plain", "md", "both", "only", "off")}
    assert vp.run_ffmpeg_metrics(r, d, *logs["plain"], batch_size=2, **kw) is None
    assert vp.run_ffmpeg_metrics(r, d, *logs["off"], batch_size=2, delta_itp=False, **kw) is None
    assert vp.run_ffmpeg_metrics(r, d, *logs["md"], batch_size=2, mdsi=True, **kw) is None
    assert vp.run_ffmpeg_metrics(r, d, *logs["both"], batch_size=2, mdsi=True, delta_itp=True, **kw) is None
    assert vp.run_ffmpeg_metrics(r, d, *logs["only"], batch_size=3, delta_itp=True, **kw) is None
    for k in (0, 1):
        for kind in ("md", "both", "only", "off"):
            assert open(logs["plain"][k], "rb").read() == open(logs[kind][k], "rb").read(), (kind, k)
    md, both, only = (json.load(open(logs[k][2])) for k in ("md", "both", "only"))
    assert list(md["frames"][0]["metrics"]) == ["mdsi"] and "delta_itp" not in json.dumps(md)
    assert list(both["frames"][0]["metrics"]) == ["mdsi", "delta_itp", "delta_itp_max"] == list(both["pooled_metrics"])
    assert list(only["frames"][0]["metrics"]) == ["delta_itp", "delta_itp_max"]
    for i in range(n):
        for doc in (both, only):
            assert doc["frames"][i]["metrics"]["delta_itp"] == float(whole["de_mean"][i])
            assert doc["frames"][i]["metrics"]["delta_itp_max"] == float(whole["de_max"][i])
        assert both["frames"][i]["metrics"]["mdsi"] == md["frames"][i]["metrics"]["mdsi"]
    assert both["pooled_metrics"]["mdsi"] == md["pooled_metrics"]["mdsi"]
    assert both["frames"][2]["metrics"]["delta_itp"] == 0.0
    hl = [str(tmp_path / ("hlg_%s.log" % t)) for t in ("psnr", "ssim", "vmaf")]
    vp.run_ffmpeg_metrics(r, d, *hl, delta_itp=True, delta_itp_transfer="hlg", delta_itp_full_range=True, **kw)
    assert [fr["metrics"]["delta_itp"] for fr in json.load(open(hl[2]))["frames"]] == [float(x) for x in q[-1]["de_mean"]]
    with pytest.raises(ValueError, match="delta_itp needs three planes"):
        vp.frame_delta_itp(r[:, :h * w], d[:, :h * w], "gray10le", h, w)
    # the row
    bgr = synth.s_natural(n, h, w, seed=12)
    cfg = {"crf": 23, "resize_width": 32, "resize_height": 32, "frame_interval": 1, "batch_size": 2, "pixfmt": layout}

    def row(name, **more):
        return vp.process_video_and_extract_metrics(r, d, dict(cfg, **more), csv_file=str(tmp_path / (name + ".csv")),
                                                    column_order="fixed", encoded_bgr=bgr)

    def same(a, b):
        return a == b or (a != a and b != b)

    row0, row1 = row("row0", mdsi=True), row("row1", mdsi=True, delta_itp=True)
    k0 = list(row0)
    at = k0.index("MDSI") + 1
    assert list(row1) == k0[:at] + ["DELTA_ITP", "DELTA_ITP_MAX"] + k0[at:]
    assert all(same(row0[k], row1[k]) for k in k0)
    assert abs(row1["DELTA_ITP"] - whole["de_mean"].mean()) <= 1e-12 and row1["DELTA_ITP_MAX"] == float(whole["de_max"].max())
    row("row0b", mdsi=True, delta_itp=False)
    assert open(str(tmp_path / "row0.csv"), "rb").read() == open(str(tmp_path / "row0b.csv"), "rb").read()
    assert b"DELTA_ITP" not in open(str(tmp_path / "row0.csv"), "rb").read()
    assert b"MDSI,DELTA_ITP,DELTA_ITP_MAX" in open(str(tmp_path / "row1.csv"), "rb").read()
    # all defaults: the key absent and the key false write the same files
    plain, off = row("plain"), row("off", delta_itp=False, delta_itp_transfer="hlg", delta_itp_range="full")
    assert list(plain) == list(off) and all(same(plain[k], off[k]) for k in plain) and "DELTA_ITP" not in plain
    assert open(str(tmp_path / "plain.csv"), "rb").read() == open(str(tmp_path / "off.csv"), "rb").read()
    rh = row("row2", delta_itp=True, delta_itp_transfer="hlg", delta_itp_range="full")
    assert abs(rh["DELTA_ITP"] - q[-1]["de_mean"].mean()) <= 1e-12 and "MDSI" not in rh


def test_profile_counts_one_launch_per_submit():
    import rtvqa_amd
    from rtvqa_amd import _native as N
    f, d, planes = IC.clip("noise3", "yuv420p", 32, 48, 8, 3, seed=9)
    with rtvqa_amd.Engine(0) as eng:
        eng.lib.vqa_kernel_name.restype = C.c_char_p
        assert eng.lib.vqa_kernel_name(N.K_ITP) == b"k_itp" and eng.lib.vqa_kernel_name(51) == b"k_itp"
        assert eng.lib.vqa_kernel_name(N.K_VERGE) == b"?" and eng.lib.vqa_kernel_name(52) == b"?"      # id 52 is unknown
        assert eng.lib.vqa_kernel_name(N.K_BRINK) == b"?"
        eng.profile(True)
        eng.itp(f, d, planes)
        ms, cnt = C.c_double(0), C.c_int64(0)
        assert eng.lib.vqa_profile_read(eng.ctx, N.K_ITP, C.byref(ms), C.byref(cnt), 0) == N.VQA_OK
        assert cnt.value == 1 and ms.value > 0.0                          # one launch for the three planes of all frames
        prof = eng.profile_read(reset=True)
        assert prof["k_itp"][1] == 1 and "k_ciede" not in prof, prof
        eng.itp(f, d, planes)
        eng.itp(f, d, planes, transfer="hlg")
        assert eng.profile_read(reset=True)["k_itp"][1] == 2
        eng.ciede(f, d, planes)
        assert "k_itp" not in eng.profile_read(reset=True)
        for bad in (N.K_BRINK, N.K_VERGE):                                 # ids 50 and 52 are unknown
            assert eng.lib.vqa_profile_read(eng.ctx, bad, C.byref(ms), C.byref(cnt), 0) == N.VQA_ERR_INVALID
