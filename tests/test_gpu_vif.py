"""GPU: VIF on four scales (vqa_vif_submit / vqa_vif_wait) through the C ABI, the engine, the one-pass stream and the
reference-shaped entry point, against the float64 reference of tests/vif_reference.py (written from the definition in
include/vqa.h).  Bar: 1e-4 absolute on every scale and on the combined value."""
import ctypes as C
import json

import numpy as np
import pytest

import vif_reference as V

pytestmark = pytest.mark.gpu

BAR = 1e-4
KINDS = ("blur", "noise", "quant", "sharp")


def _planes(layout, h, w):
    from rtvqa_amd import video_processing as vp
    return vp.LAYOUTS[layout][0](h, w)


def _natural(h, w, depth, seed):
    """one plane of synth.py's natural content (texture octaves, moving rectangles), scaled to `depth` bits"""
    from rtvqa_amd import synth
    g = synth.s_natural(1, h, w, seed=seed)[0][:, :, seed % 3].astype(np.int64)
    if depth > 8:
        rng = np.random.default_rng(seed)
        g = g * (1 << (depth - 8)) + rng.integers(0, 1 << (depth - 8), g.shape)   # the low bits carry content too
    return g


def _distort(a, kind, depth, seed):
    mx = (1 << depth) - 1
    rng = np.random.default_rng(seed + 99)
    f = a.astype(np.float64)
    if kind == "blur":
        b = V.filt(f, V.taps(2))
    elif kind == "noise":
        b = f + rng.standard_normal(a.shape) * 6 * (1 << (depth - 8))
    elif kind == "quant":
        q = 16 << (depth - 8)
        b = (a // q) * q + q // 2
    elif kind == "sharp":
        b = f + 0.8 * (f - V.filt(f, V.taps(2)))
    else:
        raise ValueError(kind)
    return np.clip(np.rint(b), 0, mx).astype(np.int64)


def _frames(layout, h, w, depth, kind, seed, n=1):
    """n frame pairs in `layout`: -> (ref, dist, planes) with [n, samples] arrays ([n, h, w, 3] for bgr24)"""
    planes = _planes(layout, h, w)
    dt = np.uint16 if depth > 8 else np.uint8
    isz = np.dtype(dt).itemsize
    size = max(p[2] + (p[1] - 1) * p[3] + (p[0] - 1) * p[4] + isz for p in planes) // isz
    out = [np.zeros((n, size), dt), np.zeros((n, size), dt)]
    for i in range(n):
        for k, p in enumerate(planes):
            pw, ph, off, rs, step = p[:5]
            a = _natural(ph, pw, depth, seed * 131 + i * 7 + k)
            pair = (a, _distort(a, kind, depth, seed + i))
            for o, v in zip(out, pair):
                view = np.lib.stride_tricks.as_strided(o[i, off // isz:], shape=(ph, pw), strides=(rs, step))
                view[...] = v
    if layout == "bgr24":
        out = [o.reshape(n, h, w, 3) for o in out]
    return out[0], out[1], planes


def _flat(a):
    return a.reshape(a.shape[0], -1)


def _plane_of(frame, p, isz):
    pw, ph, off, rs, step = p[:5]
    return np.lib.stride_tricks.as_strided(frame[off // isz:], shape=(ph, pw), strides=(rs, step)).astype(np.int64)


def _check(got, r, d, planes, depth, tag):
    """got: [n, p] VIF records; every scale and the combined value within BAR of the reference"""
    isz = r.dtype.itemsize
    worst = 0.0
    for i in range(got.shape[0]):
        for p, pl in enumerate(planes):
            num, den, scale, vif = V.vif(_plane_of(_flat(r)[i], pl, isz), _plane_of(_flat(d)[i], pl, isz), depth)
            es, ev = np.abs(got[i, p]["scale"] - scale).max(), abs(float(got[i, p]["vif"]) - vif)
            print(tag, "frame", i, "plane", p, "scale", np.round(scale, 6), "vif %.6f" % vif, "err scale %.2e vif %.2e" % (es, ev))
            worst = max(worst, es, ev)
            assert es <= BAR, (tag, i, p, got[i, p]["scale"], scale)
            assert ev <= BAR, (tag, i, p, float(got[i, p]["vif"]), vif)
            assert np.abs(got[i, p]["num"] - num).max() <= BAR * den.max() and np.abs(got[i, p]["den"] - den).max() <= BAR * den.max()
    print(tag, "worst", "%.2e" % worst)


# geometry (h, w), depth, layout
GRID = [((1080, 1920), 8, "yuv420p"), ((270, 480), 10, "yuv420p10le"), ((120, 160), 12, "yuv444p12le"), ((100, 140), 16, "gray16le"),
        ((163, 201), 8, "gray"), ((47, 35), 8, "gray"), ((16, 16), 8, "gray"), ((90, 110), 8, "bgr24")]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("geom,depth,layout", GRID, ids=["%dx%d-%s" % (g[0][0], g[0][1], g[2]) for g in GRID])
def test_parity_with_the_reference(engine, geom, depth, layout, kind):
    h, w = geom
    r, d, planes = _frames(layout, h, w, depth, kind, seed=h + depth)
    got = engine.vif(r, d, planes)
    assert got.shape == (1, len(planes))
    _check(got, r, d, planes, depth, "%dx%d %s %s" % (h, w, layout, kind))
    # the record is consistent with itself: quotients of its own sums, in double
    for p in range(len(planes)):
        g = got[0, p]
        assert np.array_equal(g["scale"], g["num"] / g["den"])
        assert float(g["vif"]) == g["num"].sum() / g["den"].sum() or abs(float(g["vif"]) - g["num"].sum() / g["den"].sum()) <= 1e-15


@pytest.mark.parametrize("kind", KINDS)
def test_a_region_of_interest_of_padded_device_frames(engine, kind):
    """a 75 x 93 window at (9, 13) of resident 120 x 160 frames: rows are 160 bytes apart, nothing outside the window is read
    (the border rule reflects inside the window)"""
    H, W, h, w, y0, x0 = 120, 160, 75, 93, 9, 13
    r, d, _ = _frames("gray", H, W, 8, kind, seed=5, n=2)
    roi = [(w, h, y0 * W + x0, W, 1)]
    dr, dd = engine.upload(r), engine.upload(d)
    got = engine.vif(dr, dd, roi)
    rr = np.ascontiguousarray(r.reshape(2, H, W)[:, y0:y0 + h, x0:x0 + w]).reshape(2, -1)
    dc = np.ascontiguousarray(d.reshape(2, H, W)[:, y0:y0 + h, x0:x0 + w]).reshape(2, -1)
    from rtvqa_amd.engine import gray_planes
    _check(got, rr, dc, gray_planes(h, w), 8, "roi " + kind)
    assert got.tobytes() == engine.vif(rr, dc, gray_planes(h, w)).tobytes()      # the window alone gives the same bits
    assert got.tobytes() == engine.vif(r, d, roi).tobytes()                      # and so does host memory


def test_identical_inputs(engine):
    for (h, w), depth, layout in GRID:
        r, _d, planes = _frames(layout, h, w, depth, "noise", seed=3)
        got = engine.vif(r, r, planes)
        print(layout, h, w, "1 - scale", (1.0 - got["scale"]).ravel(), "num - den", (got["num"] - got["den"]).max())
        assert np.abs(got["scale"] - 1.0).max() <= 1e-6
        assert abs(got["vif"] - 1.0).max() <= 1e-6
        assert (got["num"] <= got["den"] * (1.0 + 1e-6)).all()
    # a constant against a constant: den is the sample count of every level, every scale is 1
    from rtvqa_amd.engine import gray_planes
    a, b = np.full((1, 47 * 35), 100, np.uint8), np.full((1, 47 * 35), 140, np.uint8)
    got = engine.vif(a, b, gray_planes(47, 35))[0, 0]
    counts = [x * y for x, y in V.level_dims(47, 35)]
    assert np.allclose(got["den"], counts, rtol=0, atol=1e-3) and np.abs(got["scale"] - 1.0).max() <= 1e-6


def test_batches_and_positions_give_the_same_bits(engine):
    """the same pair at positions 0, 3 and 63 of batches of 1, 7 and 64, and frame_vif in chunks of 3 and 7"""
    from rtvqa_amd import video_processing as vp
    h, w, layout = 98, 130, "yuv420p"
    r, d, planes = _frames(layout, h, w, 8, "noise", seed=11, n=8)
    R, D = np.repeat(r, 8, axis=0), np.repeat(d, 8, axis=0)       # 64 frames: frame i is pair i // 8
    R[[0, 3, 63]], D[[0, 3, 63]] = r[5], d[5]
    one = engine.vif(r[5:6], d[5:6], planes)
    want = (one["num"].tobytes(), one["den"].tobytes())
    whole = engine.vif(R, D, planes)
    for pos in (0, 3, 63):
        assert (whole[pos:pos + 1]["num"].tobytes(), whole[pos:pos + 1]["den"].tobytes()) == want, pos
    seven = engine.vif(R[:7], D[:7], planes)
    for pos in (0, 3):
        assert (seven[pos:pos + 1]["num"].tobytes(), seven[pos:pos + 1]["den"].tobytes()) == want, pos
    assert seven.tobytes() == whole[:7].tobytes()
    assert engine.vif(R, D, planes).tobytes() == whole.tobytes()   # run to run
    for src_r, src_d in ((R[:17], D[:17]), (engine.upload(R[:17]), engine.upload(D[:17]))):
        for bs in (3, 7):
            scale, vif, sizes = vp.frame_vif(src_r, src_d, layout, h, w, batch_size=bs)
            assert scale.shape == (17, 3, 4) and vif.shape == (17, 3) and sizes == [(p[0], p[1]) for p in planes]
            assert scale.tobytes() == np.ascontiguousarray(whole[:17]["scale"]).tobytes(), bs
            assert vif.tobytes() == np.ascontiguousarray(whole[:17]["vif"]).tobytes(), bs


def _submit(engine, r, d, planes):
    from rtvqa_amd import _native as N
    from rtvqa_amd.engine import plane_descs
    fb = _flat(r).shape[1] * r.dtype.itemsize
    return engine.lib.vqa_vif_submit(engine.ctx, r.ctypes.data, d.ctypes.data, N.VQA_MEM_HOST, r.shape[0], fb, fb,
                                     plane_descs(planes), len(planes))


def test_the_state_machine_and_the_refusals(engine):
    from rtvqa_amd import _native as N
    from rtvqa_amd.engine import gray_planes, plane_descs, yuv420p_planes, yuv_planes
    r, d, planes = _frames("yuv420p", 64, 96, 8, "noise", seed=8)
    want = engine.vif(r, d, planes)
    qwant = engine.quality(r, d, planes)
    vout, qout = (N.VqaVifMetrics * 3)(), (N.VqaPlaneMetrics * 3)()
    # wait without submit
    assert engine.lib.vqa_vif_wait(engine.ctx, vout, 3) == N.VQA_ERR_STATE
    # submit while pending; a quality wait on a VIF batch; the batch survives both
    assert _submit(engine, r, d, planes) == N.VQA_OK
    assert _submit(engine, r, d, planes) == N.VQA_ERR_STATE
    assert engine.lib.vqa_quality_wait(engine.ctx, qout, 3) == N.VQA_ERR_STATE
    assert engine.lib.vqa_quality_wait_ms(engine.ctx, qout, None, 3) == N.VQA_ERR_STATE
    assert engine.lib.vqa_trim(engine.ctx) == N.VQA_ERR_STATE
    assert engine.lib.vqa_vif_wait(engine.ctx, vout, 2) == N.VQA_ERR_STATE      # a wrong entry count
    assert engine.lib.vqa_vif_wait(engine.ctx, vout, 3) == N.VQA_OK
    assert bytes(vout) == want.tobytes()
    # a VIF wait on a quality batch; the batch survives
    fb = _flat(r).shape[1]
    assert engine.lib.vqa_quality_submit(engine.ctx, r.ctypes.data, d.ctypes.data, N.VQA_MEM_HOST, 1, fb, fb, plane_descs(planes), 3,
                                         N.SSIM_GAUSS) == N.VQA_OK
    assert engine.lib.vqa_vif_wait(engine.ctx, vout, 3) == N.VQA_ERR_STATE
    assert engine.lib.vqa_quality_wait(engine.ctx, qout, 3) == N.VQA_OK
    assert bytes(qout) == qwant.tobytes()
    # both in flight on one upload (what the stream does): each wait collects its own
    dr, dd = engine.upload(r), engine.upload(d)
    engine.quality_submit(dr, dd, planes)
    engine.vif_submit(dr, dd, planes)
    assert engine.quality_wait().tobytes() == qwant.tobytes()
    assert engine.vif_wait().tobytes() == want.tobytes()
    # planes below 16
    for h, w in ((15, 40), (40, 15)):
        z = np.zeros((1, h * w), np.uint8)
        assert _submit(engine, z, z, gray_planes(h, w)) == N.VQA_ERR_UNSUPPORTED, (h, w)
    z = np.zeros((1, 30 * 30 * 3 // 2), np.uint8)                      # 4:2:0 at 30: the chroma planes are 15
    assert _submit(engine, z, z, yuv420p_planes(30, 30)) == N.VQA_ERR_UNSUPPORTED
    # what vqa_quality_submit refuses is refused the same way: mixed depths, bad depths, odd 16-bit strides
    z16 = np.zeros((1, 64 * 64 * 3 // 2), np.uint16)
    p10 = yuv_planes(64, 64, "420", 10)
    assert _submit(engine, z16, z16, p10) == N.VQA_OK
    assert engine.lib.vqa_vif_wait(engine.ctx, vout, 3) == N.VQA_OK
    assert _submit(engine, z16, z16, p10[:1] + [p[:5] for p in p10[1:]]) == N.VQA_ERR_INVALID
    assert _submit(engine, z16, z16, [p[:5] + (17,) for p in p10]) == N.VQA_ERR_INVALID
    assert _submit(engine, z16, z16, [(p[0], p[1], p[2], p[3] + 1, p[4], p[5]) for p in p10]) == N.VQA_ERR_INVALID
    assert engine.lib.vqa_vif_submit(engine.ctx, None, d.ctypes.data, N.VQA_MEM_HOST, 1, fb, fb, plane_descs(planes), 3) == N.VQA_ERR_INVALID
    assert engine.lib.vqa_vif_submit(engine.ctx, r.ctypes.data, d.ctypes.data, 7, 1, fb, fb, plane_descs(planes), 3) == N.VQA_ERR_INVALID
    # nothing is pending and the ctx computes as before
    assert engine.lib.vqa_vif_wait(engine.ctx, vout, 3) == N.VQA_ERR_STATE
    assert engine.vif(r, d, planes).tobytes() == want.tobytes()


def _free_bytes():
    import torch
    return torch.cuda.mem_get_info(0)[0]


def test_trim_returns_the_level_scratch():
    import rtvqa_amd
    h, w, n = 1080, 1920, 48
    r, d, planes = _frames("yuv420p", h, w, 8, "noise", seed=2)
    r, d = np.repeat(r, n, axis=0), np.repeat(d, n, axis=0)
    with rtvqa_amd.Engine(0) as eng:
        small = eng.vif(r[:1], d[:1], planes)
        eng.trim()
        base = _free_bytes()
        dr, dd = eng.upload(r), eng.upload(d)
        held = _free_bytes()
        eng.vif_submit(dr, dd, planes)
        from rtvqa_amd import _native as N
        assert eng.lib.vqa_trim(eng.ctx) == N.VQA_ERR_STATE
        big = eng.vif_wait()
        grown = _free_bytes()
        assert held - grown > (200 << 20), (held, grown)      # 48 x 1080p: 2.6 B per luma pixel = 261 MiB of levels
        eng.trim()
        dr._owner.free()
        dd._owner.free()
        after = _free_bytes()
        assert abs(after - base) <= (64 << 20), (base, held, grown, after)
        again = eng.vif(r[:1], d[:1], planes)
        assert small.tobytes() == again.tobytes() == big[:1].tobytes()


def test_the_other_modes_keep_their_results_next_to_vif():
    """Gaussian SSIM, MS-SSIM and a complexity batch before and after VIF batches on one ctx: the same bits"""
    import rtvqa_amd
    from rtvqa_amd import _native as N
    from rtvqa_amd import synth
    r, d, planes = _frames("yuv420p", 322, 386, 8, "noise", seed=4, n=3)
    bgr = synth.s_natural(5, 96, 128, seed=3)
    with rtvqa_amd.Engine(0) as eng:
        def others():
            g = eng.quality(r, d, planes, N.SSIM_GAUSS)
            ms = eng.quality(r, d, planes, N.SSIM_MS, scales=True)
            c = eng.complexity(bgr[1:], bgr[0])
            return [g.tobytes()] + [np.ascontiguousarray(x).tobytes() for x in ms] + [c.tobytes()]
        before = others()
        v1 = eng.vif(r, d, planes)
        after = others()
        assert before == after
        assert eng.vif(r, d, planes).tobytes() == v1.tobytes()
        _check(v1[:1], r[:1], d[:1], planes, 8, "next to the other modes")


def test_one_pass_entry_points(tmp_path):
    """run_ffmpeg_metrics(.., vif=True): the psnr / ssim logs are byte for byte those of the run without, plus the JSON;
    process_video_and_extract_metrics with "vif": true: the row gains VIF_scale0..3 and nothing else moves"""
    import rtvqa_amd
    from rtvqa_amd import frames, synth
    from rtvqa_amd import video_processing as vp
    h, w, n = 96, 128, 7
    r, d, planes = _frames("yuv420p", h, w, 8, "noise", seed=6, n=n)
    pr, pd = str(tmp_path / "ref.y4m"), str(tmp_path / "enc.y4m")
    frames.write_y4m(pr, r, h, w)
    frames.write_y4m(pd, d, h, w)
    logs = {k: [str(tmp_path / ("%s_%s.log" % (k, t))) for t in ("psnr", "ssim", "vmaf")] for k in ("plain", "vif")}
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["plain"], batch_size=3) is None
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["vif"], batch_size=3, vif=True) is None
    import os
    assert not os.path.exists(logs["plain"][2])
    for k in (0, 1):
        assert open(logs["plain"][k], "rb").read() == open(logs["vif"][k], "rb").read()
    doc = json.load(open(logs["vif"][2]))
    assert "vmaf" not in json.dumps(doc) and len(doc["frames"]) == n
    with rtvqa_amd.Engine(0) as eng:
        want = eng.vif(r, d, planes)
    for i in range(n):
        assert [doc["frames"][i]["metrics"]["vif_scale%d" % s] for s in range(4)] == [float(x) for x in want[i, 0]["scale"]]
    for s in range(4):
        assert abs(doc["pooled_metrics"]["vif_scale%d" % s]["mean"] - want[:, 0]["scale"][:, s].mean()) <= 1e-15
    _check(want[:2], r[:2], d[:2], planes, 8, "entry point")
    bgr = synth.s_natural(n, h, w, seed=12)
    cfg = {"crf": 23, "resize_width": 64, "resize_height": 64, "frame_interval": 1, "batch_size": 2}
    row0 = vp.process_video_and_extract_metrics(pr, pd, cfg, csv_file=str(tmp_path / "row0.csv"), column_order="fixed", encoded_bgr=bgr)
    row1 = vp.process_video_and_extract_metrics(pr, pd, dict(cfg, vif=True), csv_file=str(tmp_path / "row1.csv"), column_order="fixed",
                                                encoded_bgr=bgr)
    assert "VMAF" not in row1
    added = [k for k in row1 if k not in row0]
    assert added == ["VIF_scale0", "VIF_scale1", "VIF_scale2", "VIF_scale3"]
    assert list(row1)[:6] == list(row0)[:6] and list(row1)[6:10] == added and list(row1)[10:] == list(row0)[6:]
    for k in row0:
        assert row0[k] == row1[k] or (row0[k] != row0[k] and row1[k] != row1[k]), k
    for s in range(4):
        assert abs(row1["VIF_scale%d" % s] - want[:, 0]["scale"][:, s].mean()) <= 1e-15


def test_profile_shows_four_statistics_and_three_decimations_per_plane_group():
    import rtvqa_amd
    from rtvqa_amd import _native as N
    r, d, planes = _frames("yuv420p", 96, 128, 8, "noise", seed=9, n=3)
    with rtvqa_amd.Engine(0) as eng:
        eng.lib.vqa_kernel_name.restype = C.c_char_p
        assert eng.lib.vqa_kernel_name(N.K_VIF) == b"k_vif_stats"
        eng.profile(True)
        eng.vif(r, d, planes)
        prof = eng.profile_read(reset=True)
        assert prof["k_vif_stats"][1] == 8 and prof["k_vif_decimate"][1] == 6, prof       # luma; the two chroma planes together
        assert prof["k_vif_stats"][0] > 0 and prof["k_vif_decimate"][0] > 0
        rb, db, pb = _frames("bgr24", 40, 56, 8, "noise", seed=9, n=2)
        eng.vif(rb, db, pb)
        prof = eng.profile_read(reset=True)
        assert prof["k_vif_stats"][1] == 4 and prof["k_vif_decimate"][1] == 3, prof       # B, G, R are one group
        eng.quality(r, d, planes, N.SSIM_GAUSS)
        prof = eng.profile_read(reset=True)
        assert "k_vif_stats" not in prof and "k_vif_decimate" not in prof, prof
