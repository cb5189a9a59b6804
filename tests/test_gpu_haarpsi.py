"""GPU: HaarPSI (vqa_haarpsi_submit / vqa_haarpsi_wait) through the C ABI, the engine, the one-pass stream and the
reference-shaped entry points, against the float64 NumPy restatement of tests/haarpsi_reference.py (written from the
definition in include/vqa.h).

The bar was fixed before the kernel first ran (include/vqa.h derives it): the kernel forms the local similarity in double from
exact integers, so what separates it from the UNQUANTISED float64 restatement is u = rint(2^30 sigmoid), which moves similarity
by at most 2^-31 and haarpsi by at most 32.7 times that, and alpha' for alpha, another 1.6e-8: below 3.2e-8 together, bar 4e-8
(haarpsi_cases.BAR) on haarpsi and on similarity.  den is an exact integer and equals the restatement's.  On the CPU the
quantised restatement lies within 8.0e-9 of the float form on these cases (tests/test_haarpsi_host.py).  Largest gap seen on an
MI355X: 7.95e-9."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import haarpsi_cases as HC
import haarpsi_reference as R
import motion_cases as K

pytestmark = pytest.mark.gpu

FIELDS = ("den", "num_lo", "num_hi", "similarity", "haarpsi")
WORST = {"gap": 0.0, "tag": ""}
MATRIX = HC.matrix()


def mono(engine, r, d, depth):
    from rtvqa_amd.engine import mono_planes
    h, w = r.shape
    dt = HC.dtype_of(depth)
    return engine.haarpsi(r.astype(dt).reshape(1, -1), d.astype(dt).reshape(1, -1), mono_planes(h, w, depth))[0, 0]


def check_one(g, rp, dp, depth, tag, worst=WORST):
    want, sim = R.haarpsi(rp, dp, depth)
    gaps = (abs(float(g["haarpsi"]) - want), abs(float(g["similarity"]) - sim))
    print(tag, "haarpsi %.10f (ref %.10f) similarity %.10f (ref %.10f) gaps %.2e %.2e" % (g["haarpsi"], want, g["similarity"], sim, *gaps))
    if max(gaps) > worst["gap"]:
        worst.update(gap=max(gaps), tag=tag)
    den, lo, hi = R.words(rp, dp, depth)
    assert int(g["den"]) == den, (tag, int(g["den"]), den)
    num = (int(g["num_hi"]) << 32) + int(g["num_lo"])
    assert abs(num - ((hi << 32) + lo)) <= den, tag    # every u within one step of the restatement's
    assert gaps[0] <= HC.BAR and gaps[1] <= HC.BAR, (tag, gaps)
    # the record's two values are the host formulas of its own three words
    a, b = R.pool_words(int(g["den"]), int(g["num_lo"]), int(g["num_hi"]))
    assert abs(a - float(g["haarpsi"])) <= 1e-14 and abs(b - float(g["similarity"])) <= 1e-15


def pair_clip(layout, h, w, depth, seed, n, kind="natural"):
    """n frame pairs in a layout: the suite's reference clip and the same clip with +-12 levels (8-bit scale) of noise; full-range
    noise against full-range noise for kind "noise" """
    r, planes = K.clip(layout, h, w, depth, kind, seed=seed, n=n)
    rng = np.random.default_rng(seed + 1)
    if kind == "noise":
        d, _ = K.clip(layout, h, w, depth, kind, seed=seed + 77, n=n)
        return r, d, planes
    u, L = 1 << (depth - 8), (1 << depth) - 1
    d = np.clip(r.astype(np.int64) + rng.integers(-12, 13, r.shape) * u, 0, L)
    return r, d.astype(r.dtype), planes


def check(got, ref, dist, planes, depth, tag):
    for j, p in enumerate(planes):
        rs, ds = K.plane_series(ref, p), K.plane_series(dist, p)
        for i in range(got.shape[0]):
            check_one(got[i, j], rs[i], ds[i], depth, "%s frame %d plane %d" % (tag, i, j))


@pytest.mark.parametrize("name,shape,depth", MATRIX, ids=["%s-%dx%d-%d" % (c, s[0], s[1], dp) for c, s, dp in MATRIX])
def test_parity_on_every_content_shape_and_depth(engine, name, shape, depth):
    rp, dp = HC.pair(name, shape[0], shape[1], depth)
    g = mono(engine, rp, dp, depth)
    assert g.dtype.names == FIELDS
    check_one(g, rp, dp, depth, "%s %dx%d %d bits" % (name, shape[0], shape[1], depth))
    if name == "identical":
        assert g["haarpsi"] == 1.0 and g["similarity"] == R.U1 / R.FIX
        assert (int(g["num_hi"]) << 32) + int(g["num_lo"]) == R.U1 * int(g["den"])


LAYOUT_CASES = [(HC.YUV_SHAPE, 8, "yuv420p", "natural"), (HC.YUV_SHAPE, 10, "yuv420p10le", "natural"),
                ((33, 47), 16, "yuv444p16le", "noise"), ((33, 47), 8, "bgr24", "natural")]


@pytest.mark.parametrize("geom,depth,layout,kind", LAYOUT_CASES, ids=["%dx%d-%s" % (g[0], g[1], lay) for g, _d, lay, _k in LAYOUT_CASES])
def test_parity_on_layouts(engine, geom, depth, layout, kind):
    """4:2:0 with odd chroma: three planes in two geometry groups of one submit; 16-bit 4:4:4 with full-range samples: the word
    bounds; packed BGR: three planes at pixel step 3"""
    h, w = geom
    r, d, planes = pair_clip(layout, h, w, depth, seed=h + w, n=2, kind=kind)
    got = engine.haarpsi(r, d, planes)
    assert got.shape == (2, 3) and got.dtype.names == FIELDS
    check(got, r, d, planes, depth, "%dx%d %s" % (h, w, layout))
    if depth == 16:
        assert int(K.flat(r).max()) > 65000 and int(got["num_hi"].max()) > 0


def test_the_worst_gap_of_the_parity_matrix():
    """runs after the parity tests of this module (pytest keeps the file's order): the figure DESIGN.md 4m quotes"""
    print("parity matrix: largest gap %.3e (%s), bar %.3e" % (WORST["gap"], WORST["tag"], HC.BAR))
    assert WORST["gap"] <= HC.BAR


def test_exact_answers_and_symmetry_on_the_device(engine):
    for depth in HC.DEPTHS:
        for shape in HC.SHAPES:
            r, _ = HC.pair("natural", shape[0], shape[1], depth)
            g = mono(engine, r, r, depth)
            assert g["haarpsi"] == 1.0 and g["similarity"] == R.U1 / R.FIX           # exactly 1
            assert (int(g["num_hi"]) << 32) + int(g["num_lo"]) == R.U1 * int(g["den"]) and int(g["den"]) > 0
        for name in ("natural", "noise"):
            r, d = HC.pair(name, 33, 47, depth)
            a, b = mono(engine, r, d, depth), mono(engine, d, r, depth)
            assert a.tobytes() == b.tobytes(), (name, depth)
    # the same clip times 257 at 16 bits: H and c_s scale by 257 and 257^2 exactly, so the similarities differ by roundings of
    # double only, every u by at most one step, and den by the factor
    r, d = HC.pair("natural", 33, 47, 8)
    a, b = mono(engine, r, d, 8), mono(engine, r * 257, d * 257, 16)
    assert int(b["den"]) == 257 * int(a["den"])
    assert abs(a["haarpsi"] - b["haarpsi"]) <= HC.BAR and abs(a["similarity"] - b["similarity"]) <= HC.BAR


def test_batches_positions_and_memory_kinds_give_the_same_words(engine):
    """one pair alone and at positions 0, 4 and 2 of a batch of 5; from pageable, pinned and device memory"""
    h, w = HC.YUV_SHAPE
    r, d, planes = pair_clip("yuv420p", h, w, 8, seed=11, n=5)
    whole = engine.haarpsi(r, d, planes)
    assert engine.haarpsi(r, d, planes).tobytes() == whole.tobytes()                # run to run
    one = whole[2:3].tobytes()
    assert engine.haarpsi(r[2:3], d[2:3], planes).tobytes() == one                   # alone
    for order in ([2, 0, 1, 3, 4], [0, 1, 3, 4, 2], [0, 1, 2, 3, 4]):               # first, last, in the middle
        got = engine.haarpsi(r[order], d[order], planes)
        for pos, k in enumerate(order):
            assert got[pos].tobytes() == whole[k].tobytes(), (order, pos)
    dr, dd = engine.upload(r), engine.upload(d)
    assert engine.haarpsi(dr, dd, planes).tobytes() == whole.tobytes()
    assert engine.haarpsi(dr.slice(2, 3), dd.slice(2, 3), planes).tobytes() == one
    pr, pd = engine.alloc_pinned(r.shape), engine.alloc_pinned(d.shape)
    pr[...], pd[...] = r, d
    assert engine.is_pinned(pr)
    assert engine.haarpsi(pr, pd, planes).tobytes() == whole.tobytes()
    engine.free_pinned(pr)
    engine.free_pinned(pd)


def _submit(engine, f, d, planes):
    from rtvqa_amd import _native as N
    from rtvqa_amd.engine import plane_descs
    fb = K.flat(f).shape[1] * f.dtype.itemsize
    return engine.lib.vqa_haarpsi_submit(engine.ctx, f.ctypes.data, d.ctypes.data, N.VQA_MEM_HOST, f.shape[0], fb, fb,
                                         plane_descs(planes), len(planes))


def test_the_state_machine_and_the_refusals(engine):
    from rtvqa_amd import _native as N
    from rtvqa_amd.engine import gray_planes, mono_planes, plane_descs, yuv420p_planes
    f, d, planes = pair_clip("yuv420p", 64, 96, 8, seed=8, n=2, kind="noise")
    want, gwant, qwant = engine.haarpsi(f, d, planes), engine.gmsd(f, d, planes), engine.quality(f, d, planes)
    wout, gout, qout = (N.VqaHaarpsiMetrics * 6)(), (N.VqaGmsdMetrics * 6)(), (N.VqaPlaneMetrics * 6)()
    vout, xout = (N.VqaVifMetrics * 6)(), (N.VqaXpsnrMetrics * 6)()
    lib, ctx = engine.lib, engine.ctx
    assert lib.vqa_haarpsi_wait(ctx, wout, 6) == N.VQA_ERR_STATE                 # wait without submit
    # submit while pending; the other kinds' waits on a HaarPSI batch; the batch survives all of them
    assert _submit(engine, f, d, planes) == N.VQA_OK
    assert _submit(engine, f, d, planes) == N.VQA_ERR_STATE
    assert lib.vqa_quality_wait(ctx, qout, 6) == N.VQA_ERR_STATE
    assert lib.vqa_vif_wait(ctx, vout, 6) == N.VQA_ERR_STATE
    assert lib.vqa_gmsd_wait(ctx, gout, 6) == N.VQA_ERR_STATE
    assert lib.vqa_xpsnr_wait(ctx, xout, 6, None, 0) == N.VQA_ERR_STATE
    assert lib.vqa_trim(ctx) == N.VQA_ERR_STATE
    assert lib.vqa_haarpsi_wait(ctx, wout, 5) == N.VQA_ERR_STATE                 # a wrong entry count
    assert lib.vqa_haarpsi_wait(ctx, wout, 6) == N.VQA_OK
    assert bytes(wout) == want.tobytes()
    # the converse: a HaarPSI wait with only a GMSD or a quality batch pending; each survives
    fb = K.flat(f).shape[1]
    pd = plane_descs(planes)
    assert lib.vqa_gmsd_submit(ctx, f.ctypes.data, d.ctypes.data, N.VQA_MEM_HOST, 2, fb, fb, pd, 3) == N.VQA_OK
    assert lib.vqa_haarpsi_wait(ctx, wout, 6) == N.VQA_ERR_STATE
    assert lib.vqa_gmsd_wait(ctx, gout, 6) == N.VQA_OK and bytes(gout) == gwant.tobytes()
    assert lib.vqa_quality_submit(ctx, f.ctypes.data, d.ctypes.data, N.VQA_MEM_HOST, 2, fb, fb, pd, 3, N.SSIM_GAUSS) == N.VQA_OK
    assert lib.vqa_haarpsi_wait(ctx, wout, 6) == N.VQA_ERR_STATE
    assert lib.vqa_quality_wait(ctx, qout, 6) == N.VQA_OK and bytes(qout) == qwant.tobytes()
    # in flight next to a quality and a GMSD batch from one upload: each wait collects its own, in any order
    df, dd = engine.upload(f), engine.upload(d)
    for order in (("haarpsi", "quality", "gmsd"), ("gmsd", "haarpsi", "quality")):
        engine.quality_submit(df, dd, planes)
        engine.gmsd_submit(df, dd, planes)
        engine.haarpsi_submit(df, dd, planes)
        wants = {"haarpsi": want, "quality": qwant, "gmsd": gwant}
        for kind in order:
            assert getattr(engine, kind + "_wait")().tobytes() == wants[kind].tobytes(), (order, kind)
    # planes below 16: a failed submit leaves nothing in flight and the ctx usable
    for h, w in ((15, 16), (16, 15)):
        z = np.zeros((2, h * w), np.uint8)
        assert _submit(engine, z, z, gray_planes(h, w)) == N.VQA_ERR_UNSUPPORTED, (h, w)
        assert lib.vqa_haarpsi_wait(ctx, wout, 2) == N.VQA_ERR_STATE
    z = np.zeros((1, 30 * 30 * 3 // 2), np.uint8)                                # 4:2:0 at 30: the chroma planes are 15
    assert _submit(engine, z, z, yuv420p_planes(30, 30)) == N.VQA_ERR_UNSUPPORTED
    small = np.zeros((1, 64), np.uint8)                                          # more than 2^28 samples: a descriptor check
    assert _submit(engine, small, small, [(16385, 16384, 0, 16385, 1)]) == N.VQA_ERR_UNSUPPORTED
    assert lib.vqa_haarpsi_submit(ctx, f.ctypes.data, None, N.VQA_MEM_HOST, 2, fb, fb, pd, 3) == N.VQA_ERR_INVALID
    assert lib.vqa_haarpsi_submit(ctx, f.ctypes.data, d.ctypes.data, N.VQA_MEM_HOST, 2, fb - 1, fb, pd, 3) == N.VQA_ERR_INVALID
    # a dtype that does not match the depth
    z8, z16 = np.zeros((1, 32 * 32), np.uint8), np.zeros((1, 32 * 32), np.uint16)
    with pytest.raises(ValueError):
        engine.haarpsi(z8, z8, mono_planes(32, 32, 10))
    with pytest.raises(ValueError):
        engine.haarpsi(z16, z16, gray_planes(32, 32))
    # nothing is pending and the ctx computes as before; trim gives the feature's buffers back and it re-grows them
    assert lib.vqa_haarpsi_wait(ctx, wout, 6) == N.VQA_ERR_STATE
    engine.trim()
    assert engine.haarpsi(f, d, planes).tobytes() == want.tobytes()
    assert engine.quality(f, d, planes).tobytes() == qwant.tobytes()


def test_one_pass_entry_points(tmp_path):
    """frame_haarpsi at two batch sizes, run_ffmpeg_metrics(.., haarpsi=True) and config "haarpsi": true on a 4-frame 135 x 241
    .y4m pair: the psnr / ssim logs are byte for byte those of a plain run, the log's values are Engine.haarpsi of the first
    plane after xpsnr, and the row gains HAARPSI after XPSNR with every other column as without the key"""
    import rtvqa_amd
    from rtvqa_amd import frames, synth
    from rtvqa_amd import video_processing as vp
    (h, w), n = HC.YUV_SHAPE, 4
    r, d, planes = pair_clip("yuv420p", h, w, 8, seed=6, n=n)
    d[2] = r[2]                                                  # one identical frame: exactly 1 in the record and the log
    pr, pd = str(tmp_path / "ref.y4m"), str(tmp_path / "enc.y4m")
    frames.write_y4m(pr, r, h, w)
    frames.write_y4m(pd, d, h, w)
    logs = {k: [str(tmp_path / ("%s_%s.log" % (k, t))) for t in ("psnr", "ssim", "vmaf")] for k in ("plain", "haar", "feat", "both")}
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["plain"], batch_size=4) is None
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["haar"], batch_size=4, haarpsi=True) is None
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["feat"], batch_size=4, gmsd=True, xpsnr=True) is None
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["both"], batch_size=3, gmsd=True, xpsnr=True, haarpsi=True) is None
    assert not os.path.exists(logs["plain"][2])
    for k in (0, 1):
        for kind in ("haar", "feat", "both"):
            assert open(logs["plain"][k], "rb").read() == open(logs[kind][k], "rb").read(), (kind, k)
    with rtvqa_amd.Engine(0) as eng:
        want = eng.haarpsi(r, d, planes)
    assert want["haarpsi"][2, 0] == 1.0 and (want["haarpsi"][[0, 1, 3], 0] < 1.0).all()
    for bs in (3, 4):
        v, s, sizes = vp.frame_haarpsi(r, d, "yuv420p", h, w, batch_size=bs)
        assert v.shape == (n, 3) and sizes == [(q[0], q[1]) for q in planes]
        assert v.tobytes() == np.ascontiguousarray(want["haarpsi"]).tobytes()
        assert s.tobytes() == np.ascontiguousarray(want["similarity"]).tobytes()
    doc, feat, both = (json.load(open(logs[k][2])) for k in ("haar", "feat", "both"))
    assert list(doc["frames"][0]["metrics"]) == ["haarpsi"] == list(doc["pooled_metrics"])
    names = list(feat["frames"][0]["metrics"])
    assert names[-1] == "xpsnr" and "haarpsi" not in json.dumps(feat)
    assert list(both["frames"][0]["metrics"]) == names + ["haarpsi"]
    for i in range(n):
        for dc in (doc, both):
            assert dc["frames"][i]["metrics"]["haarpsi"] == float(want["haarpsi"][i, 0])
        assert {k: both["frames"][i]["metrics"][k] for k in names} == feat["frames"][i]["metrics"]
    assert {k: both["pooled_metrics"][k] for k in names} == feat["pooled_metrics"]
    bgr = synth.s_natural(n, h, w, seed=12)
    cfg = {"crf": 23, "resize_width": 64, "resize_height": 64, "frame_interval": 1, "batch_size": 4}

    def row(name, **kw):
        return vp.process_video_and_extract_metrics(pr, pd, dict(cfg, **kw), csv_file=str(tmp_path / (name + ".csv")),
                                                    column_order="fixed", encoded_bgr=bgr)

    def same(a, b):
        return a == b or (a != a and b != b)

    row0, row1 = row("row0"), row("row1", haarpsi=True)
    k0 = list(row0)
    at = k0.index("SSIM") + 1
    assert list(row1) == k0[:at] + ["HAARPSI"] + k0[at:] and all(same(row0[k], row1[k]) for k in k0)
    assert abs(row1["HAARPSI"] - want["haarpsi"][:, 0].mean()) <= 1e-15
    row2, row3 = row("row2", xpsnr=True, batch_size=3), row("row3", xpsnr=True, haarpsi=True, batch_size=3)
    k2 = list(row2)
    at = k2.index("XPSNR") + 1
    assert list(row3) == k2[:at] + ["HAARPSI"] + k2[at:] and all(same(row2[k], row3[k]) for k in k2)
    assert row3["HAARPSI"] == row1["HAARPSI"]
    # the same call without the key, and with it false: the same file, byte for byte, with no new column
    row("row0b", haarpsi=False)
    assert open(str(tmp_path / "row0.csv"), "rb").read() == open(str(tmp_path / "row0b.csv"), "rb").read()
    assert b"HAARPSI" not in open(str(tmp_path / "row0.csv"), "rb").read()
    assert b"XPSNR,HAARPSI" in open(str(tmp_path / "row3.csv"), "rb").read()


def test_profile_counts_one_launch_per_plane_group():
    import rtvqa_amd
    from rtvqa_amd import _native as N
    h, w = HC.YUV_SHAPE
    f, d, planes = pair_clip("yuv420p", h, w, 8, seed=9, n=3)
    with rtvqa_amd.Engine(0) as eng:
        eng.lib.vqa_kernel_name.restype = C.c_char_p
        assert eng.lib.vqa_kernel_name(N.K_HAARPSI) == b"k_haarpsi"
        assert eng.lib.vqa_kernel_name(N.K_BOUND) == b"?" and eng.lib.vqa_kernel_name(N.K_FINIS) == b"?"
        eng.profile(True)
        eng.haarpsi(f, d, planes)
        ms, cnt = C.c_double(0), C.c_int64(0)
        assert eng.lib.vqa_profile_read(eng.ctx, N.K_HAARPSI, C.byref(ms), C.byref(cnt), 0) == N.VQA_OK
        assert cnt.value == 2 and ms.value > 0.0                          # luma; the two chroma planes together
        prof = eng.profile_read(reset=True)
        assert prof["k_haarpsi"][1] == 2 and "k_gmsd" not in prof and "k_siti" not in prof, prof
        eng.gmsd(f, d, planes)
        assert "k_haarpsi" not in eng.profile_read(reset=True)
        for bad in (N.K_BOUND, N.K_FINIS):                                 # ids 36 and 38 are unknown
            assert eng.lib.vqa_profile_read(eng.ctx, bad, C.byref(ms), C.byref(cnt), 0) == N.VQA_ERR_INVALID
