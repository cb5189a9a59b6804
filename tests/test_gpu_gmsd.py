"""GPU: GMSD (vqa_gmsd_submit / vqa_gmsd_wait) through the C ABI, the engine, the one-pass stream and the reference-shaped entry
points, against the float64 NumPy restatement of tests/gmsd_reference.py (written from the definition in include/vqa.h).

The bar was fixed before the kernel first ran.  The kernel forms gms in double from exact integers, so what separates it from
the UNQUANTISED float64 restatement is the rounding u = rint(gms 2^24): every sample moves by at most 2^-25.  The mean moves by
at most that; the standard deviation is 1-Lipschitz in the root mean square of the per-sample changes times sqrt(N / (N - 1)),
at most 2^-25 * sqrt(64 / 63) on the smallest plane.  Both are below 2^-24 = 5.96e-8, the bar (gmsd_cases.BAR) on gmsd and on
gms_mean.  On the CPU the quantised restatement lies within 9.3e-9 of the float form on these cases (tests/test_gmsd_host.py).
Largest gap seen on an MI355X: 9.26e-9."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import gmsd_cases as GC
import gmsd_reference as R
import motion_cases as K

pytestmark = pytest.mark.gpu

FIELDS = ("sum_u", "sum_u2_lo", "sum_u2_hi", "count", "gms_mean", "gmsd")
WORST = {"gap": 0.0, "tag": ""}
MATRIX = GC.matrix()


def _mono(engine, r, d, depth):
    from rtvqa_amd.engine import mono_planes
    h, w = r.shape
    dt = GC.dtype_of(depth)
    return engine.gmsd(r.astype(dt).reshape(1, -1), d.astype(dt).reshape(1, -1), mono_planes(h, w, depth))[0, 0]


def _check_one(g, rp, dp, depth, tag):
    want, mean = R.gmsd(rp, dp, depth)
    gaps = (abs(float(g["gmsd"]) - want), abs(float(g["gms_mean"]) - mean))
    print(tag, "gmsd %.10f (ref %.10f) gms_mean %.10f (ref %.10f) gaps %.2e %.2e" % (g["gmsd"], want, g["gms_mean"], mean, *gaps))
    if max(gaps) > WORST["gap"]:
        WORST.update(gap=max(gaps), tag=tag)
    n = ((rp.shape[0] + 1) // 2) * ((rp.shape[1] + 1) // 2)
    assert int(g["count"]) == n
    assert gaps[0] <= GC.BAR and gaps[1] <= GC.BAR, (tag, gaps)
    # the record's two values are the host formulas of its own three words
    a, b = R.pool_words(int(g["sum_u"]), int(g["sum_u2_lo"]), int(g["sum_u2_hi"]), n)
    assert abs(a - float(g["gmsd"])) <= 1e-15 and abs(b - float(g["gms_mean"])) <= 1e-15


def _pair_clip(layout, h, w, depth, seed, n, kind="natural"):
    """n frame pairs in a layout: the suite's reference clip and the same clip with +-12 levels (8-bit scale) of noise"""
    r, planes = K.clip(layout, h, w, depth, kind, seed=seed, n=n)
    rng = np.random.default_rng(seed + 1)
    u, L = 1 << (depth - 8), (1 << depth) - 1
    d = np.clip(r.astype(np.int64) + rng.integers(-12, 13, r.shape) * u, 0, L)
    return r, d.astype(r.dtype), planes


def _check(got, ref, dist, planes, depth, tag):
    for j, p in enumerate(planes):
        rs, ds = K.plane_series(ref, p), K.plane_series(dist, p)
        for i in range(got.shape[0]):
            _check_one(got[i, j], rs[i], ds[i], depth, "%s frame %d plane %d" % (tag, i, j))


@pytest.mark.parametrize("name,shape,depth", MATRIX, ids=["%s-%dx%d-%d" % (c, s[0], s[1], dp) for c, s, dp in MATRIX])
def test_parity_on_every_content_shape_and_depth(engine, name, shape, depth):
    rp, dp = GC.pair(name, shape[0], shape[1], depth)
    g = _mono(engine, rp, dp, depth)
    assert g.dtype.names == FIELDS
    _check_one(g, rp, dp, depth, "%s %dx%d %d bits" % (name, shape[0], shape[1], depth))
    if name in ("identical", "flat_peak"):
        assert g["gmsd"] == 0.0 and g["gms_mean"] == 1.0


@pytest.mark.parametrize("geom,depth,layout", [(GC.YUV_SHAPE, 8, "yuv420p"), ((33, 67), 8, "bgr24"), (GC.YUV_SHAPE, 10, "yuv420p10le")],
                         ids=["135x241-yuv420p", "33x67-bgr24", "135x241-yuv420p10le"])
def test_parity_on_layouts(engine, geom, depth, layout):
    """4:2:0 with odd chroma: three planes in two geometry groups of one submit; packed BGR: three planes at pixel step 3"""
    h, w = geom
    r, d, planes = _pair_clip(layout, h, w, depth, seed=h + w, n=2)
    got = engine.gmsd(r, d, planes)
    assert got.shape == (2, 3) and got.dtype.names == FIELDS
    _check(got, r, d, planes, depth, "%dx%d %s" % (h, w, layout))


def test_the_worst_gap_of_the_parity_matrix():
    """runs after the parity tests of this module (pytest keeps the file's order): the figure DESIGN.md 4j quotes"""
    print("parity matrix: largest gap %.3e (%s), bar %.3e" % (WORST["gap"], WORST["tag"], GC.BAR))


def test_exact_answers_and_symmetry_on_the_device(engine):
    for depth in GC.DEPTHS:
        for shape in GC.SHAPES:
            r, _ = GC.pair("natural", shape[0], shape[1], depth)
            g = _mono(engine, r, r, depth)
            n = int(g["count"])
            assert g["gmsd"] == 0.0 and g["gms_mean"] == 1.0                          # exact zeros
            assert int(g["sum_u"]) == n << 24 and (int(g["sum_u2_hi"]) << 32) + int(g["sum_u2_lo"]) == n << 48
        for name in ("natural", "noise", "ends"):
            r, d = GC.pair(name, 33, 67, depth)
            a, b = _mono(engine, r, d, depth), _mono(engine, d, r, depth)
            assert a["gmsd"] == b["gmsd"] and a["gms_mean"] == b["gms_mean"], (name, depth)
    # flat 0 against the flat maximum on an EVEN plane (an odd one has a half-weight last row, a gradient of its own): only the
    # border ring of the 33 x 65 downsampled grid departs from 1, and there gms = c / (q + c) < 2^-3
    g = _mono(engine, *GC.pair("ends", 66, 130, 8), 8)
    ring = 2 * 33 + 2 * 65 - 4
    assert (33 * 65 - ring) << 24 < int(g["sum_u"]) < ((33 * 65 - ring) << 24) + ring * (1 << 21)
    # the same clip times 257 at 16 bits: q and T scale by 257^2 exactly, so gms differs by roundings of double only and a
    # sample's u by at most one step
    r, d = GC.pair("natural", 33, 67, 8)
    a, b = _mono(engine, r, d, 8), _mono(engine, r * 257, d * 257, 16)
    assert abs(a["gmsd"] - b["gmsd"]) <= GC.BAR and abs(a["gms_mean"] - b["gms_mean"]) <= GC.BAR


def test_batches_positions_and_memory_kinds_give_the_same_words(engine):
    """one pair alone, first, last and in the middle of a batch of 5; from pageable, pinned and device memory"""
    h, w = GC.YUV_SHAPE
    r, d, planes = _pair_clip("yuv420p", h, w, 8, seed=11, n=5)
    whole = engine.gmsd(r, d, planes)
    assert engine.gmsd(r, d, planes).tobytes() == whole.tobytes()                # run to run
    one = whole[2:3].tobytes()
    assert engine.gmsd(r[2:3], d[2:3], planes).tobytes() == one                   # alone
    for order in ([2, 0, 1, 3, 4], [0, 1, 3, 4, 2], [0, 1, 2, 3, 4]):            # first, last, in the middle
        got = engine.gmsd(r[order], d[order], planes)
        for pos, k in enumerate(order):
            assert got[pos].tobytes() == whole[k].tobytes(), (order, pos)
    dr, dd = engine.upload(r), engine.upload(d)
    assert engine.gmsd(dr, dd, planes).tobytes() == whole.tobytes()
    assert engine.gmsd(dr.slice(2, 3), dd.slice(2, 3), planes).tobytes() == one
    pr, pd = engine.alloc_pinned(r.shape), engine.alloc_pinned(d.shape)
    pr[...], pd[...] = r, d
    assert engine.is_pinned(pr)
    assert engine.gmsd(pr, pd, planes).tobytes() == whole.tobytes()
    engine.free_pinned(pr)
    engine.free_pinned(pd)


def _submit(engine, f, d, planes):
    from rtvqa_amd import _native as N
    from rtvqa_amd.engine import plane_descs
    fb = K.flat(f).shape[1] * f.dtype.itemsize
    return engine.lib.vqa_gmsd_submit(engine.ctx, f.ctypes.data, d.ctypes.data, N.VQA_MEM_HOST, f.shape[0], fb, fb,
                                      plane_descs(planes), len(planes))


def test_the_state_machine_and_the_refusals(engine):
    from rtvqa_amd import _native as N
    from rtvqa_amd.engine import gray_planes, mono_planes, plane_descs, yuv420p_planes
    f, d, planes = _pair_clip("yuv420p", 64, 96, 8, seed=8, n=2, kind="noise")
    want, hwant, qwant = engine.gmsd(f, d, planes), engine.psnr_hvs(f, d, planes), engine.quality(f, d, planes)
    gout, hout, qout = (N.VqaGmsdMetrics * 6)(), (N.VqaPsnrHvsMetrics * 6)(), (N.VqaPlaneMetrics * 6)()
    vout, eout = (N.VqaVifMetrics * 6)(), (N.VqaCiedeMetrics * 2)()
    lib, ctx = engine.lib, engine.ctx
    assert lib.vqa_gmsd_wait(ctx, gout, 6) == N.VQA_ERR_STATE                    # wait without submit
    # submit while pending; the other kinds' waits on a GMSD batch; the batch survives all of them
    assert _submit(engine, f, d, planes) == N.VQA_OK
    assert _submit(engine, f, d, planes) == N.VQA_ERR_STATE
    assert lib.vqa_quality_wait(ctx, qout, 6) == N.VQA_ERR_STATE
    assert lib.vqa_vif_wait(ctx, vout, 6) == N.VQA_ERR_STATE
    assert lib.vqa_psnr_hvs_wait(ctx, hout, 6) == N.VQA_ERR_STATE
    assert lib.vqa_ciede_wait(ctx, eout, 2) == N.VQA_ERR_STATE
    assert lib.vqa_trim(ctx) == N.VQA_ERR_STATE
    assert lib.vqa_gmsd_wait(ctx, gout, 5) == N.VQA_ERR_STATE                    # a wrong entry count
    assert lib.vqa_gmsd_wait(ctx, gout, 6) == N.VQA_OK
    assert bytes(gout) == want.tobytes()
    # the converse: a GMSD wait with only a PSNR-HVS or a quality batch pending; each survives
    fb = K.flat(f).shape[1]
    pd = plane_descs(planes)
    assert lib.vqa_psnr_hvs_submit(ctx, f.ctypes.data, d.ctypes.data, N.VQA_MEM_HOST, 2, fb, fb, pd, 3) == N.VQA_OK
    assert lib.vqa_gmsd_wait(ctx, gout, 6) == N.VQA_ERR_STATE
    assert lib.vqa_psnr_hvs_wait(ctx, hout, 6) == N.VQA_OK and bytes(hout) == hwant.tobytes()
    assert lib.vqa_quality_submit(ctx, f.ctypes.data, d.ctypes.data, N.VQA_MEM_HOST, 2, fb, fb, pd, 3, N.SSIM_GAUSS) == N.VQA_OK
    assert lib.vqa_gmsd_wait(ctx, gout, 6) == N.VQA_ERR_STATE
    assert lib.vqa_quality_wait(ctx, qout, 6) == N.VQA_OK and bytes(qout) == qwant.tobytes()
    # in flight next to a quality and a PSNR-HVS batch from one upload: each wait collects its own, in any order
    df, dd = engine.upload(f), engine.upload(d)
    for order in (("gmsd", "quality", "psnr_hvs"), ("psnr_hvs", "gmsd", "quality")):
        engine.quality_submit(df, dd, planes)
        engine.psnr_hvs_submit(df, dd, planes)
        engine.gmsd_submit(df, dd, planes)
        wants = {"gmsd": want, "quality": qwant, "psnr_hvs": hwant}
        for kind in order:
            assert getattr(engine, kind + "_wait")().tobytes() == wants[kind].tobytes(), (order, kind)
    # planes below 16: a failed submit leaves nothing in flight and the ctx usable
    for h, w in ((15, 16), (16, 15)):
        z = np.zeros((2, h * w), np.uint8)
        assert _submit(engine, z, z, gray_planes(h, w)) == N.VQA_ERR_UNSUPPORTED, (h, w)
        assert lib.vqa_gmsd_wait(ctx, gout, 2) == N.VQA_ERR_STATE
    z = np.zeros((1, 30 * 30 * 3 // 2), np.uint8)                                # 4:2:0 at 30: the chroma planes are 15
    assert _submit(engine, z, z, yuv420p_planes(30, 30)) == N.VQA_ERR_UNSUPPORTED
    small = np.zeros((1, 64), np.uint8)                                          # more than 2^28 samples: a descriptor check
    assert _submit(engine, small, small, [(16385, 16384, 0, 16385, 1)]) == N.VQA_ERR_UNSUPPORTED
    assert lib.vqa_gmsd_submit(ctx, f.ctypes.data, None, N.VQA_MEM_HOST, 2, fb, fb, pd, 3) == N.VQA_ERR_INVALID
    assert lib.vqa_gmsd_submit(ctx, f.ctypes.data, d.ctypes.data, N.VQA_MEM_HOST, 2, fb - 1, fb, pd, 3) == N.VQA_ERR_INVALID
    # a dtype that does not match the depth
    z8, z16 = np.zeros((1, 32 * 32), np.uint8), np.zeros((1, 32 * 32), np.uint16)
    with pytest.raises(ValueError):
        engine.gmsd(z8, z8, mono_planes(32, 32, 10))
    with pytest.raises(ValueError):
        engine.gmsd(z16, z16, gray_planes(32, 32))
    # nothing is pending and the ctx computes as before; trim gives the feature's buffers back and it re-grows them
    assert lib.vqa_gmsd_wait(ctx, gout, 6) == N.VQA_ERR_STATE
    engine.trim()
    assert engine.gmsd(f, d, planes).tobytes() == want.tobytes()
    assert engine.quality(f, d, planes).tobytes() == qwant.tobytes()


def test_one_pass_entry_points(tmp_path):
    """frame_gmsd at two batch sizes, run_ffmpeg_metrics(.., gmsd=True) and config "gmsd": true on a 6-frame 135 x 241 .y4m
    pair: the psnr / ssim logs are byte for byte those of a plain run, the log's values are Engine.gmsd of the first plane, and
    the row gains GMSD after CIEDE2000 with every other column as without the key"""
    import rtvqa_amd
    from rtvqa_amd import frames, synth
    from rtvqa_amd import video_processing as vp
    (h, w), n = GC.YUV_SHAPE, 6
    r, d, planes = _pair_clip("yuv420p", h, w, 8, seed=6, n=n)
    d[2] = r[2]                                                  # one identical frame: exactly 0 in the record and the log
    pr, pd = str(tmp_path / "ref.y4m"), str(tmp_path / "enc.y4m")
    frames.write_y4m(pr, r, h, w)
    frames.write_y4m(pd, d, h, w)
    logs = {k: [str(tmp_path / ("%s_%s.log" % (k, t))) for t in ("psnr", "ssim", "vmaf")] for k in ("plain", "gmsd", "feat", "both")}
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["plain"], batch_size=4) is None
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["gmsd"], batch_size=4, gmsd=True) is None
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["feat"], batch_size=4, psnr_hvs=True, ciede=True) is None
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["both"], batch_size=2, psnr_hvs=True, ciede=True, gmsd=True) is None
    assert not os.path.exists(logs["plain"][2])
    for k in (0, 1):
        for kind in ("gmsd", "feat", "both"):
            assert open(logs["plain"][k], "rb").read() == open(logs[kind][k], "rb").read(), (kind, k)
    with rtvqa_amd.Engine(0) as eng:
        want = eng.gmsd(r, d, planes)
    assert want["gmsd"][2, 0] == 0.0 and want["gms_mean"][2, 0] == 1.0 and (want["gmsd"][[0, 1, 3, 4, 5], 0] > 0).all()
    for bs in (2, 4):
        g, m, sizes = vp.frame_gmsd(r, d, "yuv420p", h, w, batch_size=bs)
        assert g.shape == (n, 3) and sizes == [(q[0], q[1]) for q in planes]
        assert g.tobytes() == np.ascontiguousarray(want["gmsd"]).tobytes() and m.tobytes() == np.ascontiguousarray(want["gms_mean"]).tobytes()
    doc, feat, both = (json.load(open(logs[k][2])) for k in ("gmsd", "feat", "both"))
    assert list(doc["frames"][0]["metrics"]) == ["gmsd"] == list(doc["pooled_metrics"])
    names = list(feat["frames"][0]["metrics"])
    assert names[-1] == "ciede2000" and "gmsd" not in json.dumps(feat)
    assert list(both["frames"][0]["metrics"]) == names + ["gmsd"]
    for i in range(n):
        for dc in (doc, both):
            assert dc["frames"][i]["metrics"]["gmsd"] == float(want["gmsd"][i, 0])
        assert {k: both["frames"][i]["metrics"][k] for k in names} == feat["frames"][i]["metrics"]
    assert {k: both["pooled_metrics"][k] for k in names} == feat["pooled_metrics"]
    bgr = synth.s_natural(n, h, w, seed=12)
    cfg = {"crf": 23, "resize_width": 64, "resize_height": 64, "frame_interval": 1, "batch_size": 4}

    def row(name, **kw):
        return vp.process_video_and_extract_metrics(pr, pd, dict(cfg, **kw), csv_file=str(tmp_path / (name + ".csv")),
                                                    column_order="fixed", encoded_bgr=bgr)

    def same(a, b):
        return a == b or (a != a and b != b)

    row0, row1 = row("row0"), row("row1", gmsd=True)
    k0 = list(row0)
    at = k0.index("SSIM") + 1
    assert list(row1) == k0[:at] + ["GMSD"] + k0[at:] and all(same(row0[k], row1[k]) for k in k0)
    assert abs(row1["GMSD"] - want["gmsd"][:, 0].mean()) <= 1e-15
    row2, row3 = row("row2", ciede=True, batch_size=2), row("row3", ciede=True, gmsd=True, batch_size=2)
    k2 = list(row2)
    at = k2.index("CIEDE2000") + 1
    assert list(row3) == k2[:at] + ["GMSD"] + k2[at:] and all(same(row2[k], row3[k]) for k in k2)
    assert row3["GMSD"] == row1["GMSD"]
    # the same call without the key, and with it false: the same file, byte for byte, with no new column
    row("row0b", gmsd=False)
    assert open(str(tmp_path / "row0.csv"), "rb").read() == open(str(tmp_path / "row0b.csv"), "rb").read()
    assert b"GMSD" not in open(str(tmp_path / "row0.csv"), "rb").read()
    assert b"CIEDE2000,GMSD" in open(str(tmp_path / "row3.csv"), "rb").read()


def test_profile_counts_one_launch_per_plane_group():
    import rtvqa_amd
    from rtvqa_amd import _native as N
    h, w = GC.YUV_SHAPE
    f, d, planes = _pair_clip("yuv420p", h, w, 8, seed=9, n=3)
    with rtvqa_amd.Engine(0) as eng:
        eng.lib.vqa_kernel_name.restype = C.c_char_p
        assert eng.lib.vqa_kernel_name(N.K_GMSD) == b"k_gmsd" and eng.lib.vqa_kernel_name(N.K_BEYOND) == b"?"
        eng.profile(True)
        eng.gmsd(f, d, planes)
        ms, cnt = C.c_double(0), C.c_int64(0)
        assert eng.lib.vqa_profile_read(eng.ctx, N.K_GMSD, C.byref(ms), C.byref(cnt), 0) == N.VQA_OK
        assert cnt.value == 2 and ms.value > 0.0                          # luma; the two chroma planes together
        prof = eng.profile_read(reset=True)
        assert prof["k_gmsd"][1] == 2 and "k_psnr_hvs" not in prof and "k_siti" not in prof, prof
        eng.psnr_hvs(f, d, planes)
        assert "k_gmsd" not in eng.profile_read(reset=True)
        for bad in (N.K_BEYOND, N.K_LIMIT):                                # ids 26 and 28 are unknown
            assert eng.lib.vqa_profile_read(eng.ctx, bad, C.byref(ms), C.byref(cnt), 0) == N.VQA_ERR_INVALID
