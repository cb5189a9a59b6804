"""GPU: PSNR-HVS and PSNR-HVS-M (vqa_psnr_hvs_submit / vqa_psnr_hvs_wait) through the C ABI, the engine, the one-pass stream and
the reference-shaped entry points, against the float64 NumPy restatement of tests/psnr_hvs_reference.py (written from the
definition in include/vqa.h).

The bar was fixed before the kernel first ran: |S - S_ref| <= 1e-4 S_ref + 2^-27 on both sums - the family's relative bar (VIF,
ADM) plus the fixed-point term the header derives (half a 2^-20 quantum per block over 64 coefficients).  The contents are those
tests/test_psnr_hvs_host.py admits.  Largest gaps seen on an MI355X: see DESIGN.md 4h."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import motion_cases as K
import psnr_hvs_cases as PC
import psnr_hvs_reference as R

pytestmark = pytest.mark.gpu

# geometry (h, w), depth, layout: the minimum (four blocks, one workgroup), remainders either way, two workgroups with a ragged
# second one (5 x 17 blocks), 4:2:0 whose 36 x 44 chroma leaves a remainder of 4, packed BGR (pixel step 3), and every sample type.
# Rows of 136, 88 (8 bits), 176 and 112 bytes (16 bits) take the one-load-per-row path, the others the sample-by-sample one.
GRID = [((16, 16), 8, "gray"), ((17, 23), 8, "gray"), ((40, 136), 8, "gray"), ((72, 88), 8, "yuv420p"),
        ((72, 88), 10, "yuv420p10le"), ((40, 56), 12, "yuv444p12le"), ((50, 70), 16, "gray16le"), ((40, 56), 8, "bgr24")]
IDS = ["%dx%d-%s" % (g[0][0], g[0][1], g[2]) for g in GRID]
WORST = {"gap": 0.0, "tag": ""}
FIELDS = ("s_hvs", "s_hvsm", "psnr_hvs", "psnr_hvsm")


def _pair_clip(layout, h, w, depth, seed, n, kind="natural"):
    """n frame pairs: the suite's reference clip and the same clip with a few levels of noise -> (ref, dist, planes)"""
    r, planes = K.clip(layout, h, w, depth, kind, seed=seed, n=n)
    rng = np.random.default_rng(seed + 1)
    u, L = 1 << (depth - 8), (1 << depth) - 1
    d = np.clip(r.astype(np.int64) + rng.integers(-4, 5, r.shape) * u + (rng.integers(0, u, r.shape) if depth > 8 else 0), 0, L)
    return r, d.astype(r.dtype), planes


def _check_one(g, rp, dp, depth, tag):
    s, sm, p, pm = R.psnr_hvs(rp, dp, depth)
    gs, gm = float(g["s_hvs"]), float(g["s_hvsm"])
    gaps = [abs(gs - s) / s if s > 0 else abs(gs), abs(gm - sm) / sm if sm > 0 else abs(gm)]
    print(tag, "S_hvs %.9g (ref %.9g) S_hvsm %.9g (ref %.9g) gaps %.2e %.2e, %.3f / %.3f dB" % (gs, s, gm, sm, gaps[0], gaps[1], p, pm))
    if max(gaps) > WORST["gap"]:
        WORST.update(gap=max(gaps), tag=tag)
    assert abs(gs - s) <= PC.GPU_BAR * s + R.quantum_bar(), (tag, gs, s)
    assert abs(gm - sm) <= PC.GPU_BAR * sm + R.quantum_bar(), (tag, gm, sm)
    assert gm <= gs
    # the dB values are the host formula of the record's own sums
    for v, x in ((float(g["psnr_hvs"]), gs), (float(g["psnr_hvsm"]), gm)):
        assert v == R.db(x, depth) or abs(v - R.db(x, depth)) <= 1e-12 * abs(v)


def _check(got, ref, dist, planes, depth, tag):
    for j, p in enumerate(planes):
        rs, ds = K.plane_series(ref, p), K.plane_series(dist, p)
        for i in range(got.shape[0]):
            _check_one(got[i, j], rs[i], ds[i], depth, "%s frame %d plane %d" % (tag, i, j))


@pytest.mark.parametrize("geom,depth,layout", GRID, ids=IDS)
def test_parity_on_every_shape_and_sample_type(engine, geom, depth, layout):
    h, w = geom
    r, d, planes = _pair_clip(layout, h, w, depth, seed=h + w, n=2)
    got = engine.psnr_hvs(r, d, planes)
    assert got.shape == (2, len(planes)) and got.dtype.names == FIELDS
    _check(got, r, d, planes, depth, "%dx%d %s" % (h, w, layout))


@pytest.mark.parametrize("name,depth", PC.matrix(), ids=["%s-%d" % c for c in PC.matrix()])
def test_parity_on_the_admitted_contents(engine, name, depth):
    from rtvqa_amd.engine import mono_planes
    h, w = PC.SHAPE
    rp, dp = PC.pair(name, h, w, depth)
    dt = np.uint16 if depth > 8 else np.uint8
    got = engine.psnr_hvs(rp.astype(dt).reshape(1, -1), dp.astype(dt).reshape(1, -1), mono_planes(h, w, depth))
    _check_one(got[0, 0], rp, dp, depth, "%s %d bits" % (name, depth))


def test_the_worst_gap_of_the_parity_matrix():
    """runs after the parity tests of this module (pytest keeps the file's order): the figure DESIGN.md 4h quotes"""
    print("parity matrix: largest relative gap on S %.3e (%s)" % (WORST["gap"], WORST["tag"]))


def test_exact_answers_on_the_device(engine):
    from rtvqa_amd.engine import gray_planes, mono_planes
    h, w = 40, 136
    for depth in (8, 10, 16):
        dt = np.uint16 if depth > 8 else np.uint8
        a, _ = PC.pair("natural", h, w, depth)
        pl = mono_planes(h, w, depth)
        f = a.astype(dt).reshape(1, -1)
        got = engine.psnr_hvs(f, f.copy(), pl)[0, 0]
        assert got.tobytes()[:16] == bytes(16)                                   # S bits are exactly 0
        assert got["psnr_hvs"] == np.inf and got["psnr_hvsm"] == np.inf
        # a constant offset: only the DC term, which is never masked
        for c in (3, -7, 100):
            b = np.clip(a, 200, (1 << depth) - 201)
            want = c * c * (25.735088 / 16.0) ** 2
            got = engine.psnr_hvs(b.astype(dt).reshape(1, -1), (b + c).astype(dt).reshape(1, -1), pl)[0, 0]
            print("offset %d at %d bits: S %.9g, want %.9g" % (c, depth, got["s_hvs"], want))
            assert abs(got["s_hvs"] - want) <= PC.GPU_BAR * want + R.quantum_bar()
            assert abs(got["s_hvsm"] - want) <= PC.GPU_BAR * want + R.quantum_bar()
    # a 17 x 23 plane gives the bits of its 16 x 16 crop
    r, d = PC.pair("natural", 17, 23, 8)
    whole = engine.psnr_hvs(r.astype(np.uint8).reshape(1, -1), d.astype(np.uint8).reshape(1, -1), gray_planes(17, 23))
    crop = engine.psnr_hvs(np.ascontiguousarray(r[:16, :16]).astype(np.uint8).reshape(1, -1),
                           np.ascontiguousarray(d[:16, :16]).astype(np.uint8).reshape(1, -1), gray_planes(16, 16))
    assert whole.tobytes() == crop.tobytes()
    # the pair is symmetric
    sw = engine.psnr_hvs(d.astype(np.uint8).reshape(1, -1), r.astype(np.uint8).reshape(1, -1), gray_planes(17, 23))
    assert sw.tobytes() == whole.tobytes()


def test_batches_positions_and_memory_kinds_give_the_same_bits(engine):
    """the same pair at several places of batches of 1, 3 and 8, from host, pinned and device memory; frame_psnr_hvs in chunks;
    a strided view and regions of interest of resident frames (both load paths)"""
    from rtvqa_amd import video_processing as vp
    from rtvqa_amd.engine import DeviceFrames, gray_planes
    h, w, layout, n = 72, 88, "yuv420p", 8
    r, d, planes = _pair_clip(layout, h, w, 8, seed=11, n=n)
    whole = engine.psnr_hvs(r, d, planes)
    assert engine.psnr_hvs(r, d, planes).tobytes() == whole.tobytes()          # run to run
    one = whole[5:6].tobytes()
    assert engine.psnr_hvs(r[5:6], d[5:6], planes).tobytes() == one             # a batch of 1
    for order in ([5, 0, 5], [1, 5, 2], [5, 1, 2, 3, 5, 6, 7, 5]):              # batches of 3 and 8
        got = engine.psnr_hvs(r[order], d[order], planes)
        for pos, k in enumerate(order):
            assert got[pos].tobytes() == whole[k].tobytes(), (order, pos)
    dr, dd = engine.upload(r), engine.upload(d)
    assert engine.psnr_hvs(dr, dd, planes).tobytes() == whole.tobytes()
    assert engine.psnr_hvs(dr.slice(5, 6), dd.slice(5, 6), planes).tobytes() == one
    pr, pd = engine.alloc_pinned(r.shape), engine.alloc_pinned(d.shape)
    pr[...], pd[...] = r, d
    assert engine.is_pinned(pr)
    assert engine.psnr_hvs(pr, pd, planes).tobytes() == whole.tobytes()
    for src in ((r, d), (pr, pd), (dr, dd)):
        for bs in (1, 3, 64):
            p, pm, s, sm, sizes = vp.frame_psnr_hvs(src[0], src[1], layout, h, w, batch_size=bs)
            assert p.shape == (n, 3) and sizes == [(q[0], q[1]) for q in planes]
            for got, k in ((p, "psnr_hvs"), (pm, "psnr_hvsm"), (s, "s_hvs"), (sm, "s_hvsm")):
                assert got.tobytes() == np.ascontiguousarray(whole[k]).tobytes(), (type(src[0]), bs, k)
    engine.free_pinned(pr)
    engine.free_pinned(pd)
    # every second frame of the resident clips: frame_stride does the stepping
    odd = [DeviceFrames(x.ptr + x.frame_stride, 4, x.h, x.w, frame_stride=2 * x.frame_stride, row_stride=x.row_stride, owner=x,
                        channels=x.channels) for x in (dr, dd)]
    assert engine.psnr_hvs(odd[0], odd[1], planes).tobytes() == whole[1::2].tobytes()
    # windows of resident 120 x 160 gray frames: nothing outside the window is read.  (9, 13) is unaligned (sample by sample),
    # (8, 16) with 96 columns is aligned (one load per row); each against the same samples as a plane of their own
    g, gd, _ = _pair_clip("gray", 120, 160, 8, seed=5, n=3)
    g3, gd3 = g.reshape(3, 120, 160), gd.reshape(3, 120, 160)
    dg, dgd = engine.upload(g3), engine.upload(gd3)
    for (y0, x0, hh, ww) in ((9, 13, 75, 93), (8, 16, 75, 96)):
        roi = [(ww, hh, 0, 160, 1)]
        cut = [np.ascontiguousarray(x[:, y0:y0 + hh, x0:x0 + ww]).reshape(3, -1) for x in (g3, gd3)]
        alone = engine.psnr_hvs(cut[0], cut[1], gray_planes(hh, ww))
        assert engine.psnr_hvs(dg.roi(y0, y0 + hh, x0, x0 + ww), dgd.roi(y0, y0 + hh, x0, x0 + ww), roi).tobytes() == alone.tobytes()
        assert engine.psnr_hvs(g, gd, [(ww, hh, y0 * 160 + x0, 160, 1)]).tobytes() == alone.tobytes()
        _check(alone, cut[0], cut[1], gray_planes(hh, ww), 8, "roi %d,%d" % (y0, x0))


def _submit(engine, f, d, planes, n=None):
    from rtvqa_amd import _native as N
    from rtvqa_amd.engine import plane_descs
    fb = K.flat(f).shape[1] * f.dtype.itemsize
    return engine.lib.vqa_psnr_hvs_submit(engine.ctx, f.ctypes.data, d.ctypes.data, N.VQA_MEM_HOST, f.shape[0] if n is None else n,
                                          fb, fb, plane_descs(planes), len(planes))


def test_the_state_machine_and_the_refusals(engine):
    from rtvqa_amd import _native as N
    from rtvqa_amd.engine import gray_planes, plane_descs, yuv420p_planes, yuv_planes
    f, d, planes = _pair_clip("yuv420p", 64, 96, 8, seed=8, n=2, kind="noise")
    want = engine.psnr_hvs(f, d, planes)
    vwant, qwant, swant = engine.vif(f, d, planes), engine.quality(f, d, planes), engine.siti(f, planes)
    hout, vout, qout, sout = (N.VqaPsnrHvsMetrics * 6)(), (N.VqaVifMetrics * 6)(), (N.VqaPlaneMetrics * 6)(), (N.VqaSitiMetrics * 6)()
    aout, mout = (N.VqaAdmMetrics * 6)(), (N.VqaMotionMetrics * 6)()
    lib, ctx = engine.lib, engine.ctx
    # wait without submit
    assert lib.vqa_psnr_hvs_wait(ctx, hout, 6) == N.VQA_ERR_STATE
    # submit while pending; the other kinds' waits on a PSNR-HVS batch; the batch survives all of them
    assert _submit(engine, f, d, planes) == N.VQA_OK
    assert _submit(engine, f, d, planes) == N.VQA_ERR_STATE
    assert lib.vqa_quality_wait(ctx, qout, 6) == N.VQA_ERR_STATE
    assert lib.vqa_vif_wait(ctx, vout, 6) == N.VQA_ERR_STATE
    assert lib.vqa_adm_wait(ctx, aout, 6) == N.VQA_ERR_STATE
    assert lib.vqa_motion_wait(ctx, mout, 6) == N.VQA_ERR_STATE
    assert lib.vqa_siti_wait(ctx, sout, 6) == N.VQA_ERR_STATE
    assert lib.vqa_trim(ctx) == N.VQA_ERR_STATE
    assert lib.vqa_psnr_hvs_wait(ctx, hout, 5) == N.VQA_ERR_STATE      # a wrong entry count
    assert lib.vqa_psnr_hvs_wait(ctx, hout, 6) == N.VQA_OK
    assert bytes(hout) == want.tobytes()
    # a PSNR-HVS wait on a quality, a VIF and an SI/TI batch; each survives
    fb = K.flat(f).shape[1]
    pd = plane_descs(planes)
    assert lib.vqa_quality_submit(ctx, f.ctypes.data, d.ctypes.data, N.VQA_MEM_HOST, 2, fb, fb, pd, 3, N.SSIM_GAUSS) == N.VQA_OK
    assert lib.vqa_psnr_hvs_wait(ctx, hout, 6) == N.VQA_ERR_STATE
    assert lib.vqa_quality_wait(ctx, qout, 6) == N.VQA_OK and bytes(qout) == qwant.tobytes()
    assert lib.vqa_vif_submit(ctx, f.ctypes.data, d.ctypes.data, N.VQA_MEM_HOST, 2, fb, fb, pd, 3) == N.VQA_OK
    assert lib.vqa_psnr_hvs_wait(ctx, hout, 6) == N.VQA_ERR_STATE
    assert lib.vqa_vif_wait(ctx, vout, 6) == N.VQA_OK and bytes(vout) == vwant.tobytes()
    assert lib.vqa_siti_submit(ctx, f.ctypes.data, None, N.VQA_MEM_HOST, 2, fb, pd, 3) == N.VQA_OK
    assert lib.vqa_psnr_hvs_wait(ctx, hout, 6) == N.VQA_ERR_STATE
    assert lib.vqa_siti_wait(ctx, sout, 6) == N.VQA_OK and bytes(sout) == swant.tobytes()
    # a PSNR-HVS batch in flight next to a quality and a VIF batch from one upload: each wait collects its own, in any order
    df, dd = engine.upload(f), engine.upload(d)
    for order in (("psnr_hvs", "quality", "vif"), ("vif", "psnr_hvs", "quality"), ("quality", "vif", "psnr_hvs")):
        engine.quality_submit(df, dd, planes)
        engine.vif_submit(df, dd, planes)
        engine.psnr_hvs_submit(df, dd, planes)
        wants = {"psnr_hvs": want, "quality": qwant, "vif": vwant}
        for kind in order:
            assert getattr(engine, kind + "_wait")().tobytes() == wants[kind].tobytes(), (order, kind)
    # host frames share the staging of a pending quality batch: the stream orders them
    engine.quality_submit(f, d, planes)
    engine.psnr_hvs_submit(f, d, planes)
    assert engine.psnr_hvs_wait().tobytes() == want.tobytes() and engine.quality_wait().tobytes() == qwant.tobytes()
    # planes below 16: a failed submit leaves nothing in flight and the ctx usable
    for h, w in ((15, 40), (40, 15)):
        z = np.zeros((2, h * w), np.uint8)
        assert _submit(engine, z, z, gray_planes(h, w)) == N.VQA_ERR_UNSUPPORTED, (h, w)
        assert lib.vqa_psnr_hvs_wait(ctx, hout, 2) == N.VQA_ERR_STATE
    z = np.zeros((2, 16 * 16), np.uint8)
    assert _submit(engine, z, z, gray_planes(16, 16)) == N.VQA_OK
    assert lib.vqa_psnr_hvs_wait(ctx, hout, 2) == N.VQA_OK
    z = np.zeros((1, 30 * 30 * 3 // 2), np.uint8)                      # 4:2:0 at 30: the chroma planes are 15
    assert _submit(engine, z, z, yuv420p_planes(30, 30)) == N.VQA_ERR_UNSUPPORTED
    # what vqa_vif_submit refuses is refused the same way: mixed depths, bad depths, odd 16-bit strides, short frame strides
    z16 = np.zeros((2, 64 * 64 * 3 // 2), np.uint16)
    p10 = yuv_planes(64, 64, "420", 10)
    assert _submit(engine, z16, z16, p10) == N.VQA_OK
    assert lib.vqa_psnr_hvs_wait(ctx, hout, 6) == N.VQA_OK
    assert _submit(engine, z16, z16, p10[:1] + [p[:5] for p in p10[1:]]) == N.VQA_ERR_INVALID          # mixed depths
    assert _submit(engine, z16, z16, [p[:5] + (17,) for p in p10]) == N.VQA_ERR_INVALID
    assert _submit(engine, z16, z16, [(p[0], p[1], p[2], p[3] + 1, p[4], p[5]) for p in p10]) == N.VQA_ERR_INVALID
    assert lib.vqa_psnr_hvs_submit(ctx, f.ctypes.data, d.ctypes.data, N.VQA_MEM_HOST, 2, fb - 1, fb, pd, 3) == N.VQA_ERR_INVALID
    assert lib.vqa_psnr_hvs_submit(ctx, f.ctypes.data, d.ctypes.data, N.VQA_MEM_HOST, 2, fb, fb - 1, pd, 3) == N.VQA_ERR_INVALID
    assert lib.vqa_psnr_hvs_submit(ctx, f.ctypes.data, None, N.VQA_MEM_HOST, 2, fb, fb, pd, 3) == N.VQA_ERR_INVALID
    assert lib.vqa_psnr_hvs_submit(ctx, f.ctypes.data, d.ctypes.data, 7, 2, fb, fb, pd, 3) == N.VQA_ERR_INVALID
    assert lib.vqa_psnr_hvs_submit(ctx, f.ctypes.data, d.ctypes.data, N.VQA_MEM_HOST, 2, fb, fb, pd, 5) == N.VQA_ERR_INVALID
    # a plane of more than 2^28 samples: a descriptor check, made before any sample is read
    small = np.zeros((1, 64), np.uint8)
    assert _submit(engine, small, small, [(16385, 16384, 0, 16385, 1)]) == N.VQA_ERR_UNSUPPORTED
    # nothing is pending and the ctx computes as before; trim gives the feature's buffers back and it re-grows them
    assert lib.vqa_psnr_hvs_wait(ctx, hout, 6) == N.VQA_ERR_STATE
    assert engine.psnr_hvs(f, d, planes).tobytes() == want.tobytes()
    engine.trim()
    assert engine.psnr_hvs(f, d, planes).tobytes() == want.tobytes()
    assert engine.quality(f, d, planes).tobytes() == qwant.tobytes() and engine.vif(f, d, planes).tobytes() == vwant.tobytes()


def test_one_pass_entry_points(tmp_path):
    """run_ffmpeg_metrics(.., psnr_hvs=True): the psnr / ssim logs are byte for byte those of a plain run and the log's values are
    Engine.psnr_hvs of the first plane (capped at 100 dB); process_video_and_extract_metrics with "psnr_hvs": true: PSNR_HVS and
    PSNR_HVSM after TI (at the end of the feature columns), every other column and file as without the key"""
    import rtvqa_amd
    from rtvqa_amd import frames, synth
    from rtvqa_amd import video_processing as vp
    h, w, n = 96, 128, 5
    r, d, planes = _pair_clip("yuv420p", h, w, 8, seed=6, n=n)
    d[2] = r[2]                                                  # one identical frame: inf in the record, 100.0 in the log
    pr, pd = str(tmp_path / "ref.y4m"), str(tmp_path / "enc.y4m")
    frames.write_y4m(pr, r, h, w)
    frames.write_y4m(pd, d, h, w)
    logs = {k: [str(tmp_path / ("%s_%s.log" % (k, t))) for t in ("psnr", "ssim", "vmaf")] for k in ("plain", "hvs", "feat", "both")}
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["plain"], batch_size=3) is None
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["hvs"], batch_size=3, psnr_hvs=True) is None
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["feat"], batch_size=3, vif=True, siti=True) is None
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["both"], batch_size=2, vif=True, siti=True, psnr_hvs=True) is None
    assert not os.path.exists(logs["plain"][2])
    for k in (0, 1):
        for kind in ("hvs", "feat", "both"):
            assert open(logs["plain"][k], "rb").read() == open(logs[kind][k], "rb").read(), (kind, k)
    with rtvqa_amd.Engine(0) as eng:
        want = eng.psnr_hvs(r, d, planes)[:, 0]
    assert want["psnr_hvs"][2] == np.inf and want["s_hvs"][2] == 0.0 and np.isfinite(want["psnr_hvs"][[0, 1, 3, 4]]).all()
    p, pm, s, sm, _ = vp.frame_psnr_hvs(r, d, "yuv420p", h, w, batch_size=2)
    assert p[:, 0].tobytes() == np.ascontiguousarray(want["psnr_hvs"]).tobytes() and p[2, 0] == np.inf      # nothing capped here
    assert sm[:, 0].tobytes() == np.ascontiguousarray(want["s_hvsm"]).tobytes()
    doc, feat, both = (json.load(open(logs[k][2])) for k in ("hvs", "feat", "both"))
    assert list(doc["frames"][0]["metrics"]) == ["psnr_hvs", "psnr_hvsm"] == list(doc["pooled_metrics"])
    names = list(feat["frames"][0]["metrics"])
    assert names[-2:] == ["si", "ti"] and "psnr_hvs" not in json.dumps(feat)
    assert list(both["frames"][0]["metrics"]) == names + ["psnr_hvs", "psnr_hvsm"]
    cap = {k: np.minimum(want[k], 100.0) for k in ("psnr_hvs", "psnr_hvsm")}
    for i in range(n):
        for dc in (doc, both):
            m = dc["frames"][i]["metrics"]
            assert m["psnr_hvs"] == float(cap["psnr_hvs"][i]) and m["psnr_hvsm"] == float(cap["psnr_hvsm"][i])
        assert {k: both["frames"][i]["metrics"][k] for k in names} == feat["frames"][i]["metrics"]
    assert doc["frames"][2]["metrics"]["psnr_hvs"] == 100.0
    assert {k: both["pooled_metrics"][k] for k in names} == feat["pooled_metrics"]
    bgr = synth.s_natural(n, h, w, seed=12)
    cfg = {"crf": 23, "resize_width": 64, "resize_height": 64, "frame_interval": 1, "batch_size": 2}

    def row(name, **kw):
        return vp.process_video_and_extract_metrics(pr, pd, dict(cfg, **kw), csv_file=str(tmp_path / (name + ".csv")),
                                                    column_order="fixed", encoded_bgr=bgr)

    def same(a, b):
        return a == b or (a != a and b != b)

    row0, row1 = row("row0"), row("row1", psnr_hvs=True)
    k0 = list(row0)
    at = k0.index("SSIM") + 1
    assert list(row1) == k0[:at] + ["PSNR_HVS", "PSNR_HVSM"] + k0[at:]          # no other feature: right after SSIM
    assert all(same(row0[k], row1[k]) for k in k0)
    assert abs(row1["PSNR_HVS"] - cap["psnr_hvs"].mean()) <= 1e-12 and abs(row1["PSNR_HVSM"] - cap["psnr_hvsm"].mean()) <= 1e-12
    row2, row3 = row("row2", vif=True, siti=True), row("row3", vif=True, siti=True, psnr_hvs=True)
    k2 = list(row2)
    at = k2.index("TI") + 1
    assert list(row3) == k2[:at] + ["PSNR_HVS", "PSNR_HVSM"] + k2[at:] and all(same(row2[k], row3[k]) for k in k2)
    assert row3["PSNR_HVS"] == row1["PSNR_HVS"] and row3["PSNR_HVSM"] == row1["PSNR_HVSM"]
    # the same call without the key, and with it false: the same file, byte for byte, with no new column
    row("row0b", psnr_hvs=False)
    assert open(str(tmp_path / "row0.csv"), "rb").read() == open(str(tmp_path / "row0b.csv"), "rb").read()
    assert b"PSNR_HVS" not in open(str(tmp_path / "row0.csv"), "rb").read()
    assert b"PSNR_HVS,PSNR_HVSM" in open(str(tmp_path / "row1.csv"), "rb").read()


def test_profile_counts_one_launch_per_plane_group():
    import rtvqa_amd
    from rtvqa_amd import _native as N
    f, d, planes = _pair_clip("yuv420p", 96, 128, 8, seed=9, n=3)
    with rtvqa_amd.Engine(0) as eng:
        eng.lib.vqa_kernel_name.restype = C.c_char_p
        assert eng.lib.vqa_kernel_name(N.K_PSNR_HVS) == b"k_psnr_hvs" and eng.lib.vqa_kernel_name(N.K_LAST) == b"?"
        eng.profile(True)
        eng.psnr_hvs(f, d, planes)
        ms, cnt = C.c_double(0), C.c_int64(0)
        assert eng.lib.vqa_profile_read(eng.ctx, N.K_PSNR_HVS, C.byref(ms), C.byref(cnt), 0) == N.VQA_OK
        assert cnt.value == 2 and ms.value > 0.0                          # luma; the two chroma planes together
        prof = eng.profile_read(reset=True)
        assert prof["k_psnr_hvs"][1] == 2 and "k_siti" not in prof and "k_vif_stats" not in prof, prof
        fb, db_, pb = _pair_clip("bgr24", 40, 56, 8, seed=9, n=2)
        eng.psnr_hvs(fb, db_, pb)
        prof = eng.profile_read(reset=True)
        assert prof["k_psnr_hvs"][1] == 1, prof                            # B, G, R are one group
        eng.vif(f, d, planes)
        assert "k_psnr_hvs" not in eng.profile_read(reset=True)
        for bad in (N.K_LAST, N.K_PAST):                                   # ids 22 and 24 are unknown
            assert eng.lib.vqa_profile_read(eng.ctx, bad, C.byref(ms), C.byref(cnt), 0) == N.VQA_ERR_INVALID
