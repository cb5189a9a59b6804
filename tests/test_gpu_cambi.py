"""GPU: CAMBI (vqa_cambi_submit / vqa_cambi_wait) through the C ABI, the engine, the one-pass stream and the reference-shaped
entry points, against the integer NumPy restatement of tests/cambi_reference.py (written from the definition in include/vqa.h).

There is no tolerance: every integer word of the record (top, k, masked at all five scales) must EQUAL the restatement's.  pool
and cambi are the host's formulas of those words: they are compared with the same formulas in Python at 1e-15."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import cambi_cases as CC
import cambi_reference as R
import motion_cases as K

pytestmark = pytest.mark.gpu

FIELDS = ("top", "k", "masked", "pool", "cambi")
MATRIX = CC.matrix()
SEEN = {}


def _mono(engine, p, depth):
    from rtvqa_amd.engine import mono_planes
    h, w = p.shape
    return engine.cambi(p.astype(CC.dtype_of(depth)).reshape(1, -1), mono_planes(h, w, depth))[0, 0]


def _check_one(g, p, depth, tag):
    want = R.cambi_words(p, depth)
    got = {k: [int(v) for v in g[k]] for k in ("top", "k", "masked")}
    print(tag, "masked", got["masked"], "top", got["top"], "cambi %.6f" % g["cambi"])
    assert got == want, (tag, got, want)
    pool, score = R.pool_and_score(got["top"], got["k"])
    assert max(abs(a - float(b)) for a, b in zip(pool, g["pool"])) <= 1e-15 and abs(score - float(g["cambi"])) <= 1e-15
    assert 0.0 <= float(g["cambi"]) <= 1.0
    return got


def _layout_clip(layout, h, w, depth, n, seed=0):
    """n frames in a layout whose planes are the banded contents in turn, a noise frame among them"""
    planes = K.planes_of(layout, h, w)
    dt = CC.dtype_of(depth)
    isz = np.dtype(dt).itemsize
    size = max(p[2] + (p[1] - 1) * p[3] + (p[0] - 1) * p[4] + isz for p in planes) // isz
    out = np.zeros((n, size), dt)
    names = CC.BANDED + ("noise",)
    for i in range(n):
        for k, p in enumerate(planes):
            pw, ph, off, rs, step = p[:5]
            view = np.lib.stride_tricks.as_strided(out[i, off // isz:], shape=(ph, pw), strides=(rs, step))
            view[...] = CC.plane(names[(i + k) % len(names)], ph, pw, depth, seed=seed + i)
    if layout == "bgr24":
        out = out.reshape(n, h, w, 3)
    return out, planes


def _check(got, frames, planes, depth, tag):
    for j, p in enumerate(planes):
        ps = K.plane_series(frames, p)
        for i in range(got.shape[0]):
            _check_one(got[i, j], ps[i], depth, "%s frame %d plane %d" % (tag, i, j))


@pytest.mark.parametrize("name,shape,depth", MATRIX, ids=["%s-%dx%d-%d" % (c, s[0], s[1], dp) for c, s, dp in MATRIX])
def test_every_word_on_every_content_shape_and_depth(engine, name, shape, depth):
    p = CC.plane(name, shape[0], shape[1], depth)
    g = _mono(engine, p, depth)
    assert g.dtype.names == FIELDS
    got = _check_one(g, p, depth, "%s %dx%d %d bits" % (name, shape[0], shape[1], depth))
    if name in CC.ZERO:                                            # exact zeros
        assert got["top"] == [0] * 5 and float(g["cambi"]) == 0.0 and all(float(v) == 0.0 for v in g["pool"])
        if name == "noise":
            assert got["masked"] == [0] * 5
        else:
            assert got["masked"][0] > shape[0] * shape[1] // 2    # a flat field: the mask is full but for the outer ring
    else:
        assert float(g["cambi"]) > 0.0
    if shape == (41, 71):
        n = [(-(-41 // (1 << s))) * (-(-71 // (1 << s))) for s in range(5)]
        SEEN[(name, depth)] = ([m / float(k) for m, k in zip(got["masked"], n)], float(g["cambi"]))


@pytest.mark.parametrize("depth", [8, 10])
def test_the_last_bin_of_the_histogram(engine, depth):
    """u = 65536 exactly at sixteen samples of scale 1 (cambi_cases.full_contrast; tests/test_cambi_host.py shows that the
    restatement has them): bin 65536 is why the histogram has 65537 bins"""
    p = CC.full_contrast(depth)
    y, m = R.scales(p, depth)[1]
    assert int((R.contrast(y, m) == 65536).sum()) == 16
    _check_one(_mono(engine, p, depth), p, depth, "full contrast %d bits" % depth)


@pytest.mark.parametrize("geom,depth,layout", [(CC.YUV_SHAPE, 8, "yuv420p"), (CC.BGR_SHAPE, 8, "bgr24"), (CC.YUV_SHAPE, 10, "yuv420p10le")],
                         ids=["135x241-yuv420p", "33x67-bgr24", "135x241-yuv420p10le"])
def test_every_word_on_layouts(engine, geom, depth, layout):
    """4:2:0 with odd chroma: three planes in two geometry groups of one submit; packed BGR: three planes at pixel step 3"""
    h, w = geom
    f, planes = _layout_clip(layout, h, w, depth, n=2)
    got = engine.cambi(f, planes)
    assert got.shape == (2, 3) and got.dtype.names == FIELDS
    _check(got, f, planes, depth, "%dx%d %s" % (h, w, layout))


def test_batches_positions_memory_kinds_and_views_give_the_same_words(engine):
    """one frame alone, first, last and in the middle of a batch of 5; from pageable, pinned and device memory; as a strided
    selection of frames and as a region of interest of a larger plane"""
    from rtvqa_amd.engine import mono_planes
    h, w = CC.YUV_SHAPE
    f, planes = _layout_clip("yuv420p", h, w, 8, n=5, seed=3)
    whole = engine.cambi(f, planes)
    assert engine.cambi(f, planes).tobytes() == whole.tobytes()                   # run to run
    assert len({whole[i].tobytes() for i in range(5)}) == 5                       # (five different frames)
    one = whole[2:3].tobytes()
    assert engine.cambi(f[2:3], planes).tobytes() == one                          # alone
    for order in ([2, 0, 1, 3, 4], [0, 1, 3, 4, 2], [0, 1, 2, 3, 4]):             # first, last, in the middle
        got = engine.cambi(f[order], planes)
        for pos, k in enumerate(order):
            assert got[pos].tobytes() == whole[k].tobytes(), (order, pos)
    df = engine.upload(f)
    assert engine.cambi(df, planes).tobytes() == whole.tobytes()
    assert engine.cambi(df.slice(2, 3), planes).tobytes() == one
    pf = engine.alloc_pinned(f.shape)
    pf[...] = f
    assert engine.is_pinned(pf)
    assert engine.cambi(pf, planes).tobytes() == whole.tobytes()
    engine.free_pinned(pf)
    # every other frame, through the frame stride (frame_bytes), without a copy of the selection
    fb = f.shape[1]
    lib, ctx = engine.lib, engine.ctx
    from rtvqa_amd import _native as N
    from rtvqa_amd.engine import plane_descs
    out = (N.VqaCambiMetrics * 9)()
    assert lib.vqa_cambi_submit(ctx, f.ctypes.data, N.VQA_MEM_HOST, 3, 2 * fb, plane_descs(planes), 3) == N.VQA_OK
    assert lib.vqa_cambi_wait(ctx, out, 9) == N.VQA_OK
    assert bytes(out) == whole[[0, 2, 4]].tobytes()
    # a region of interest: the 41 x 71 plane inside a 60 x 100 frame of noise, through offset and row stride
    p = CC.plane("dither", 41, 71, 8)
    big = np.random.default_rng(5).integers(0, 256, (1, 60, 100)).astype(np.uint8)
    big[0, 7:48, 13:84] = p
    roi = engine.cambi(big.reshape(1, -1), [(71, 41, 7 * 100 + 13, 100, 1)])
    assert roi.tobytes() == engine.cambi(p.astype(np.uint8).reshape(1, -1), mono_planes(41, 71, 8)).tobytes()


def _submit(engine, f, planes):
    from rtvqa_amd import _native as N
    from rtvqa_amd.engine import plane_descs
    fb = K.flat(f).shape[1] * f.dtype.itemsize
    return engine.lib.vqa_cambi_submit(engine.ctx, f.ctypes.data, N.VQA_MEM_HOST, f.shape[0], fb, plane_descs(planes), len(planes))


def test_the_state_machine_and_the_refusals(engine):
    from rtvqa_amd import _native as N
    from rtvqa_amd.engine import gray_planes, mono_planes, plane_descs, yuv420p_planes
    f, planes = _layout_clip("yuv420p", 64, 96, 8, n=2, seed=8)
    d = K.clip("yuv420p", 64, 96, 8, "noise", seed=8, n=2)[0]
    want, gwant, qwant = engine.cambi(f, planes), engine.gmsd(f, d, planes), engine.quality(f, d, planes)
    bout, gout, qout = (N.VqaCambiMetrics * 6)(), (N.VqaGmsdMetrics * 6)(), (N.VqaPlaneMetrics * 6)()
    vout = (N.VqaVifMetrics * 6)()
    lib, ctx = engine.lib, engine.ctx
    assert lib.vqa_cambi_wait(ctx, bout, 6) == N.VQA_ERR_STATE                   # wait without submit
    # submit while pending; the other kinds' waits on a CAMBI batch; the batch survives all of them
    assert _submit(engine, f, planes) == N.VQA_OK
    assert _submit(engine, f, planes) == N.VQA_ERR_STATE
    assert lib.vqa_quality_wait(ctx, qout, 6) == N.VQA_ERR_STATE
    assert lib.vqa_vif_wait(ctx, vout, 6) == N.VQA_ERR_STATE
    assert lib.vqa_gmsd_wait(ctx, gout, 6) == N.VQA_ERR_STATE
    assert lib.vqa_trim(ctx) == N.VQA_ERR_STATE
    assert lib.vqa_cambi_wait(ctx, bout, 5) == N.VQA_ERR_STATE                   # a wrong entry count
    assert lib.vqa_cambi_wait(ctx, bout, 6) == N.VQA_OK
    assert bytes(bout) == want.tobytes()
    # the converse: a CAMBI wait with only a GMSD or a quality batch pending; each survives
    fb = K.flat(f).shape[1]
    pd = plane_descs(planes)
    assert lib.vqa_gmsd_submit(ctx, f.ctypes.data, d.ctypes.data, N.VQA_MEM_HOST, 2, fb, fb, pd, 3) == N.VQA_OK
    assert lib.vqa_cambi_wait(ctx, bout, 6) == N.VQA_ERR_STATE
    assert lib.vqa_gmsd_wait(ctx, gout, 6) == N.VQA_OK and bytes(gout) == gwant.tobytes()
    assert lib.vqa_quality_submit(ctx, f.ctypes.data, d.ctypes.data, N.VQA_MEM_HOST, 2, fb, fb, pd, 3, N.SSIM_GAUSS) == N.VQA_OK
    assert lib.vqa_cambi_wait(ctx, bout, 6) == N.VQA_ERR_STATE
    assert lib.vqa_quality_wait(ctx, qout, 6) == N.VQA_OK and bytes(qout) == qwant.tobytes()
    # in flight next to a quality and a GMSD batch from one upload: each wait collects its own, in any order.  CAMBI reads
    # the SECOND stream's frames here, as the one-pass run does
    df, dd = engine.upload(d), engine.upload(f)
    wants = {"cambi": want, "quality": engine.quality(d, f, planes), "gmsd": engine.gmsd(d, f, planes)}
    for order in (("cambi", "quality", "gmsd"), ("gmsd", "cambi", "quality")):
        engine.quality_submit(df, dd, planes)
        engine.gmsd_submit(df, dd, planes)
        engine.cambi_submit(dd, planes)
        for kind in order:
            assert getattr(engine, kind + "_wait")().tobytes() == wants[kind].tobytes(), (order, kind)
    # the same from host memory: the quality batch has read its staged frames before CAMBI's overwrite them
    engine.quality_submit(f, d, planes)
    engine.cambi_submit(f, planes)
    assert engine.quality_wait().tobytes() == qwant.tobytes() and engine.cambi_wait().tobytes() == want.tobytes()
    # planes below 16: a failed submit leaves nothing in flight and the ctx usable
    for h, w in ((15, 16), (16, 15)):
        z = np.zeros((2, h * w), np.uint8)
        assert _submit(engine, z, gray_planes(h, w)) == N.VQA_ERR_UNSUPPORTED, (h, w)
        assert lib.vqa_cambi_wait(ctx, bout, 2) == N.VQA_ERR_STATE
    z = np.zeros((1, 30 * 30 * 3 // 2), np.uint8)                                # 4:2:0 at 30: the chroma planes are 15
    assert _submit(engine, z, yuv420p_planes(30, 30)) == N.VQA_ERR_UNSUPPORTED
    small = np.zeros((1, 64), np.uint8)                                          # more than 2^28 samples: a descriptor check
    assert _submit(engine, small, [(16385, 16384, 0, 16385, 1)]) == N.VQA_ERR_UNSUPPORTED
    assert lib.vqa_cambi_submit(ctx, None, N.VQA_MEM_HOST, 2, fb, pd, 3) == N.VQA_ERR_INVALID
    assert lib.vqa_cambi_submit(ctx, f.ctypes.data, N.VQA_MEM_HOST, 2, fb - 1, pd, 3) == N.VQA_ERR_INVALID
    assert lib.vqa_cambi_submit(ctx, f.ctypes.data, 7, 2, fb, pd, 3) == N.VQA_ERR_INVALID
    # a dtype that does not match the depth
    z8, z16 = np.zeros((1, 32 * 32), np.uint8), np.zeros((1, 32 * 32), np.uint16)
    with pytest.raises(ValueError):
        engine.cambi(z8, mono_planes(32, 32, 10))
    with pytest.raises(ValueError):
        engine.cambi(z16, gray_planes(32, 32))
    # nothing is pending and the ctx computes as before; trim gives the feature's buffers back and it re-grows them
    assert lib.vqa_cambi_wait(ctx, bout, 6) == N.VQA_ERR_STATE
    engine.trim()
    assert engine.cambi(f, planes).tobytes() == want.tobytes()
    assert engine.quality(f, d, planes).tobytes() == qwant.tobytes()


def test_one_pass_entry_points(tmp_path):
    """frame_cambi at two batch sizes, run_ffmpeg_metrics(.., cambi=True) and config "cambi": true on a 6-frame 135 x 241 .y4m
    pair: CAMBI measures the ENCODED stream; the psnr / ssim logs are byte for byte those of a plain run, the log's values are
    Engine.cambi of the first plane, and the row gains CAMBI after GMSD with every other column as without the key"""
    import rtvqa_amd
    from rtvqa_amd import frames, synth
    from rtvqa_amd import video_processing as vp
    (h, w), n = CC.YUV_SHAPE, 6
    d, planes = _layout_clip("yuv420p", h, w, 8, n=n, seed=6)
    r = K.clip("yuv420p", h, w, 8, "natural", seed=6, n=n)[0]
    pr, pd = str(tmp_path / "ref.y4m"), str(tmp_path / "enc.y4m")
    frames.write_y4m(pr, r, h, w)
    frames.write_y4m(pd, d, h, w)
    logs = {k: [str(tmp_path / ("%s_%s.log" % (k, t))) for t in ("psnr", "ssim", "vmaf")] for k in ("plain", "cambi", "feat", "both")}
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["plain"], batch_size=4) is None
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["cambi"], batch_size=4, cambi=True) is None
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["feat"], batch_size=4, ciede=True, gmsd=True) is None
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["both"], batch_size=2, ciede=True, gmsd=True, cambi=True) is None
    assert not os.path.exists(logs["plain"][2])
    for k in (0, 1):
        for kind in ("cambi", "feat", "both"):
            assert open(logs["plain"][k], "rb").read() == open(logs[kind][k], "rb").read(), (kind, k)
    with rtvqa_amd.Engine(0) as eng:
        want = eng.cambi(d, planes)
        assert eng.cambi(r, planes).tobytes() != want.tobytes()                   # (the reference stream would read otherwise)
    assert (want["cambi"][:, 0] > 0).sum() >= 4
    for bs in (2, 4):
        g, pool, sizes = vp.frame_cambi(d, "yuv420p", h, w, batch_size=bs)
        assert g.shape == (n, 3) and pool.shape == (n, 3, 5) and sizes == [(q[0], q[1]) for q in planes]
        assert g.tobytes() == np.ascontiguousarray(want["cambi"]).tobytes() and pool.tobytes() == np.ascontiguousarray(want["pool"]).tobytes()
    doc, feat, both = (json.load(open(logs[k][2])) for k in ("cambi", "feat", "both"))
    assert list(doc["frames"][0]["metrics"]) == ["cambi"] == list(doc["pooled_metrics"])
    names = list(feat["frames"][0]["metrics"])
    assert names[-1] == "gmsd" and "cambi" not in json.dumps(feat)
    assert list(both["frames"][0]["metrics"]) == names + ["cambi"]
    for i in range(n):
        for dc in (doc, both):
            assert dc["frames"][i]["metrics"]["cambi"] == float(want["cambi"][i, 0])
        assert {k: both["frames"][i]["metrics"][k] for k in names} == feat["frames"][i]["metrics"]
    assert {k: both["pooled_metrics"][k] for k in names} == feat["pooled_metrics"]
    bgr = synth.s_natural(n, h, w, seed=12)
    cfg = {"crf": 23, "resize_width": 64, "resize_height": 64, "frame_interval": 1, "batch_size": 4}

    def row(name, **kw):
        return vp.process_video_and_extract_metrics(pr, pd, dict(cfg, **kw), csv_file=str(tmp_path / (name + ".csv")),
                                                    column_order="fixed", encoded_bgr=bgr)

    def same(a, b):
        return a == b or (a != a and b != b)

    row0, row1 = row("row0"), row("row1", cambi=True)
    k0 = list(row0)
    at = k0.index("SSIM") + 1
    assert list(row1) == k0[:at] + ["CAMBI"] + k0[at:] and all(same(row0[k], row1[k]) for k in k0)
    assert abs(row1["CAMBI"] - want["cambi"][:, 0].mean()) <= 1e-15
    row2, row3 = row("row2", gmsd=True, batch_size=2), row("row3", gmsd=True, cambi=True, batch_size=2)
    k2 = list(row2)
    at = k2.index("GMSD") + 1
    assert list(row3) == k2[:at] + ["CAMBI"] + k2[at:] and all(same(row2[k], row3[k]) for k in k2)
    assert row3["CAMBI"] == row1["CAMBI"]
    # the same call without the key, and with it false: the same file, byte for byte, with no new column
    row("row0b", cambi=False)
    assert open(str(tmp_path / "row0.csv"), "rb").read() == open(str(tmp_path / "row0b.csv"), "rb").read()
    assert b"CAMBI" not in open(str(tmp_path / "row0.csv"), "rb").read()
    assert b"GMSD,CAMBI" in open(str(tmp_path / "row3.csv"), "rb").read()


def test_profile_counts_the_launches_per_plane_group():
    import rtvqa_amd
    from rtvqa_amd import _native as N
    h, w = CC.YUV_SHAPE
    f, planes = _layout_clip("yuv420p", h, w, 8, n=3, seed=9)
    names = {N.K_CAMBI_MASK: b"k_cambi_mask", N.K_CAMBI_DECIMATE: b"k_cambi_decimate", N.K_CAMBI_CONTRAST: b"k_cambi_contrast",
             N.K_CAMBI_TOPK: b"k_cambi_topk"}
    with rtvqa_amd.Engine(0) as eng:
        eng.lib.vqa_kernel_name.restype = C.c_char_p
        for kid, name in names.items():
            assert eng.lib.vqa_kernel_name(kid) == name
        assert eng.lib.vqa_kernel_name(N.K_LIMIT) == b"?" and eng.lib.vqa_kernel_name(N.K_TERMINUS) == b"?"
        eng.profile(True)
        eng.cambi(f, planes)
        prof = eng.profile_read(reset=True)
        # luma; the two chroma planes together: two groups
        assert prof["k_cambi_mask"][1] == 2 and prof["k_cambi_decimate"][1] == 2 and prof["k_cambi_contrast"][1] == 10, prof
        assert prof["k_cambi_topk"][1] == 20 and "k_gmsd" not in prof and all(v[0] > 0.0 for v in prof.values()), prof
        eng.gmsd(f, f, planes)
        assert not any(k.startswith("k_cambi") for k in eng.profile_read(reset=True))
        ms, cnt = C.c_double(0), C.c_int64(0)
        for bad in (N.K_LIMIT, N.K_TERMINUS):                              # ids 28 and 33 are unknown
            assert eng.lib.vqa_profile_read(eng.ctx, bad, C.byref(ms), C.byref(cnt), 0) == N.VQA_ERR_INVALID


def test_the_masked_shares_and_scores_of_the_contents():
    """runs after the parity tests of this module (pytest keeps the file's order): the figures DESIGN.md 4k quotes"""
    for (name, depth), (shares, score) in sorted(SEEN.items()):
        print("41x71 %-10s %2d bits: masked share per scale %s cambi %.6f" % (name, depth, " ".join("%.3f" % s for s in shares), score))
