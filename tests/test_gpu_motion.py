"""GPU: VMAF's motion feature (vqa_motion_submit / vqa_motion_wait) through the C ABI, the engine, the one-pass stream and the
reference-shaped entry points with a test-made model file, against the float64 reference of tests/motion_reference.py (written
from the definition in include/vqa.h).

The bar is the worst-case fp32 error include/vqa.h derives for in-range samples: per blurred sample 5 roundings in the vertical
pass, carried through the horizontal pass, 5 more there and the taps' own rounding to fp32 in either pass (12 units of 2^-17,
one unit being the largest rounding of a value below 256); two blurred samples, one rounding of their difference and the 2^-17
of the fixed-point quantum: 26 x 2^-17 = 1.98e-4 absolute on motion.  It was fixed before the kernel first ran.
Largest gap seen on an MI355X: see DESIGN.md 4f."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import motion_cases as K
import motion_reference as M
import vmaf_reference as R

pytestmark = pytest.mark.gpu

BAR = 26 * 2.0 ** -17
WORST = {"gap": 0.0, "tag": ""}


def _reference(frames, planes, depth, prev0=None):
    """[n, p] float64 motion of every plane"""
    cols = []
    for p in planes:
        s = K.plane_series(frames, p)
        p0 = K.plane_series(prev0[None], p)[0] if prev0 is not None else None
        cols.append(M.motion(s, depth, p0))
    return np.stack(cols, axis=1)


def _check(got, want, planes, tag):
    gap = np.abs(got["motion"] - want)
    print(tag, "motion", np.round(want.ravel(), 6).tolist(), "gap %.3e" % gap.max(), "bar %.3e" % BAR)
    if gap.max() > WORST["gap"]:
        WORST.update(gap=float(gap.max()), tag=tag)
    assert gap.max() <= BAR, (tag, gap)
    area = np.array([p[0] * p[1] for p in planes], np.float64)
    assert np.array_equal(got["motion"], got["sad"] / area)            # the record is consistent with itself
    assert (got["sad"] * 65536.0 == np.rint(got["sad"] * 65536.0)).all()      # multiples of the quantum


@pytest.mark.parametrize("kind", K.KINDS)
@pytest.mark.parametrize("geom,depth,layout,n", K.GRID, ids=K.IDS)
def test_parity_with_the_reference(engine, geom, depth, layout, n, kind):
    h, w = geom
    f, planes = K.clip(layout, h, w, depth, kind, seed=h + w, n=n)
    got = engine.motion(f, planes)
    assert got.shape == (n, len(planes))
    assert (got[0]["motion"] == 0.0).all() and (got[0]["sad"] == 0.0).all()       # no predecessor
    assert (got[1:]["motion"] > 0.0).all()
    _check(got, _reference(f, planes, depth), planes, "%dx%d %s %s" % (h, w, layout, kind))


def test_the_worst_gap_of_the_parity_matrix():
    """runs after the parity tests of this module (pytest keeps the file's order): the figure DESIGN.md 4f quotes"""
    print("largest gap of the parity matrix: %.3e (%s), bar %.3e" % (WORST["gap"], WORST["tag"], BAR))
    assert WORST["gap"] <= BAR


def test_identical_consecutive_frames_give_exactly_zero(engine):
    for (h, w), depth, layout, _n in K.GRID[1:]:
        f, planes = K.clip(layout, h, w, depth, "noise", seed=3, n=1)
        got = engine.motion(np.repeat(f, 3, axis=0), planes, prev0=f[0])
        assert (got["sad"] == 0.0).all() and (got["motion"] == 0.0).all(), layout
    # a constant against a constant: d (tap sum)^2, the taps as fp32
    from rtvqa_amd.engine import gray_planes
    a, b = np.full((1, 47 * 35), 100, np.uint8), np.full((1, 47 * 35), 140, np.uint8)
    got = engine.motion(b, gray_planes(47, 35), prev0=a[0])[0, 0]
    assert abs(float(got["motion"]) - 40.0 * sum(M.TAPS) ** 2) <= BAR


def test_prev0_given_or_not(engine):
    h, w, layout = 66, 98, "yuv420p"
    f, planes = K.clip(layout, h, w, 8, "natural", seed=5, n=6)
    whole = engine.motion(f, planes)
    assert (whole[0]["motion"] == 0.0).all()
    tail = engine.motion(f[1:], planes, prev0=f[0])
    assert tail.tobytes() == whole[1:].tobytes()             # motion[0] with prev0 is motion[1] of the clip prefixed by it
    assert engine.motion(f[3:4], planes, prev0=f[2]).tobytes() == whole[3:4].tobytes()
    none = engine.motion(f[1:], planes)
    assert (none[0]["motion"] == 0.0).all() and none[1:].tobytes() == whole[2:].tobytes()
    _check(tail, _reference(f[1:], planes, 8, prev0=f[0]), planes, "prev0")
    df = engine.upload(f)
    assert engine.motion(df.slice(1, 6), planes, prev0=df.frame(0)).tobytes() == whole[1:].tobytes()
    with pytest.raises(TypeError):
        engine.motion(df.slice(1, 6), planes, prev0=f[0])
    with pytest.raises(ValueError):
        engine.motion(f.astype(np.uint16), planes)
    with pytest.raises(ValueError):
        engine.motion(f, planes, prev0=f[0].astype(np.uint16))
    with pytest.raises(ValueError):
        engine.motion(f, planes, prev0=f[0][:-1])


def test_batches_positions_and_memory_kinds_give_the_same_bits(engine):
    """the same pair at different places of batches of different sizes; frame_motion in chunks of 1, 3, 7 and 64 from pageable,
    pinned and device-resident memory; a strided view and a region of interest of resident frames"""
    from rtvqa_amd import video_processing as vp
    from rtvqa_amd.engine import gray_planes
    h, w, layout, n = 98, 130, "yuv420p", 21
    f, planes = K.clip(layout, h, w, 8, "natural", seed=11, n=n)
    whole = engine.motion(f, planes)
    assert engine.motion(f, planes).tobytes() == whole.tobytes()          # run to run
    F = np.concatenate([f[4:6], f[:3], f[4:6], f[7:9], f[4:6]])            # the pair (4, 5) at places 1, 6 and 10
    got = engine.motion(F, planes)
    for pos in (1, 6, 10):
        assert got[pos].tobytes() == whole[5].tobytes(), pos
    assert engine.motion(f[5:6], planes, prev0=f[4]).tobytes() == whole[5:6].tobytes()
    df = engine.upload(f)
    assert engine.motion(df, planes).tobytes() == whole.tobytes()
    pinned = engine.alloc_pinned(f.shape)
    pinned[...] = f
    assert engine.is_pinned(pinned)
    want_m = np.ascontiguousarray(whole["motion"])
    for src in (f, pinned, df):
        for bs in (1, 3, 7, 64):
            m, m2, sizes = vp.frame_motion(src, layout, h, w, batch_size=bs)
            assert m.shape == (n, 3) and sizes == [(p[0], p[1]) for p in planes]
            assert m.tobytes() == want_m.tobytes(), (type(src), bs)
            assert np.array_equal(m2, np.stack([M.motion2(want_m[:, p]) for p in range(3)], axis=1))
    engine.free_pinned(pinned)
    # every second frame of the resident clip: frame_stride does the stepping
    from rtvqa_amd.engine import DeviceFrames
    odd = DeviceFrames(df.ptr + df.frame_stride, 10, df.h, df.w, frame_stride=2 * df.frame_stride, row_stride=df.row_stride,
                       owner=df, channels=df.channels)
    assert engine.motion(odd, planes).tobytes() == engine.motion(f[1::2][:10], planes).tobytes()
    # a 75 x 93 window at (9, 13) of resident 120 x 160 gray frames: nothing outside the window is read
    g, _ = K.clip("gray", 120, 160, 8, "natural", seed=5, n=3)
    dg = engine.upload(g.reshape(3, 120, 160))
    win = dg.roi(9, 9 + 75, 13, 13 + 93)
    roi = [(93, 75, 0, 160, 1)]
    cut = np.ascontiguousarray(g.reshape(3, 120, 160)[:, 9:84, 13:106]).reshape(3, -1)
    alone = engine.motion(cut, gray_planes(75, 93))
    assert engine.motion(win, roi).tobytes() == alone.tobytes()
    assert engine.motion(g, [(93, 75, 9 * 160 + 13, 160, 1)]).tobytes() == alone.tobytes()
    _check(alone, _reference(cut, gray_planes(75, 93), 8), gray_planes(75, 93), "roi")


def _submit(engine, f, planes, prev0=None):
    from rtvqa_amd import _native as N
    from rtvqa_amd.engine import plane_descs
    fb = K.flat(f).shape[1] * f.dtype.itemsize
    return engine.lib.vqa_motion_submit(engine.ctx, f.ctypes.data, prev0.ctypes.data if prev0 is not None else None,
                                        N.VQA_MEM_HOST, f.shape[0], fb, plane_descs(planes), len(planes))


def test_the_state_machine_and_the_refusals(engine):
    from rtvqa_amd import _native as N
    from rtvqa_amd.engine import gray_planes, plane_descs, yuv420p_planes, yuv_planes
    f, planes = K.clip("yuv420p", 64, 96, 8, "noise", seed=8, n=2)
    d, _ = K.clip("yuv420p", 64, 96, 8, "noise", seed=9, n=2)
    want = engine.motion(f, planes)
    awant, vwant, qwant = engine.adm(f, d, planes), engine.vif(f, d, planes), engine.quality(f, d, planes)
    mout, aout, vout, qout = (N.VqaMotionMetrics * 6)(), (N.VqaAdmMetrics * 6)(), (N.VqaVifMetrics * 6)(), (N.VqaPlaneMetrics * 6)()
    # wait without submit
    assert engine.lib.vqa_motion_wait(engine.ctx, mout, 6) == N.VQA_ERR_STATE
    # submit while pending; the other kinds' waits on a motion batch; the batch survives all of them
    assert _submit(engine, f, planes) == N.VQA_OK
    assert _submit(engine, f, planes) == N.VQA_ERR_STATE
    assert engine.lib.vqa_quality_wait(engine.ctx, qout, 6) == N.VQA_ERR_STATE
    assert engine.lib.vqa_vif_wait(engine.ctx, vout, 6) == N.VQA_ERR_STATE
    assert engine.lib.vqa_adm_wait(engine.ctx, aout, 6) == N.VQA_ERR_STATE
    assert engine.lib.vqa_trim(engine.ctx) == N.VQA_ERR_STATE
    assert engine.lib.vqa_set_option(engine.ctx, N.OPT_HYST_STATS, 0) == N.VQA_ERR_STATE
    assert engine.lib.vqa_motion_wait(engine.ctx, mout, 5) == N.VQA_ERR_STATE      # a wrong entry count
    assert engine.lib.vqa_motion_wait(engine.ctx, mout, 6) == N.VQA_OK
    assert bytes(mout) == want.tobytes()
    # a motion wait on a quality, a VIF and an ADM batch; each survives
    fb = K.flat(f).shape[1]
    assert engine.lib.vqa_quality_submit(engine.ctx, f.ctypes.data, d.ctypes.data, N.VQA_MEM_HOST, 2, fb, fb, plane_descs(planes), 3,
                                         N.SSIM_GAUSS) == N.VQA_OK
    assert engine.lib.vqa_motion_wait(engine.ctx, mout, 6) == N.VQA_ERR_STATE
    assert engine.lib.vqa_quality_wait(engine.ctx, qout, 6) == N.VQA_OK and bytes(qout) == qwant.tobytes()
    assert engine.lib.vqa_vif_submit(engine.ctx, f.ctypes.data, d.ctypes.data, N.VQA_MEM_HOST, 2, fb, fb, plane_descs(planes), 3) == N.VQA_OK
    assert engine.lib.vqa_motion_wait(engine.ctx, mout, 6) == N.VQA_ERR_STATE
    assert engine.lib.vqa_vif_wait(engine.ctx, vout, 6) == N.VQA_OK and bytes(vout) == vwant.tobytes()
    assert engine.lib.vqa_adm_submit(engine.ctx, f.ctypes.data, d.ctypes.data, N.VQA_MEM_HOST, 2, fb, fb, plane_descs(planes), 3) == N.VQA_OK
    assert engine.lib.vqa_motion_wait(engine.ctx, mout, 6) == N.VQA_ERR_STATE
    assert engine.lib.vqa_adm_wait(engine.ctx, aout, 6) == N.VQA_OK and bytes(aout) == awant.tobytes()
    # all four in flight on one upload (what the stream does): each wait collects its own, in any order
    df, dd = engine.upload(f), engine.upload(d)
    engine.quality_submit(df, dd, planes)
    engine.vif_submit(df, dd, planes)
    engine.adm_submit(df, dd, planes)
    engine.motion_submit(df, planes)
    assert engine.motion_wait().tobytes() == want.tobytes()
    assert engine.adm_wait().tobytes() == awant.tobytes()
    assert engine.quality_wait().tobytes() == qwant.tobytes()
    assert engine.vif_wait().tobytes() == vwant.tobytes()
    # planes below 16: a failed submit leaves nothing in flight and the ctx usable
    for h, w in ((15, 40), (40, 15)):
        z = np.zeros((2, h * w), np.uint8)
        assert _submit(engine, z, gray_planes(h, w)) == N.VQA_ERR_UNSUPPORTED, (h, w)
        assert engine.lib.vqa_motion_wait(engine.ctx, mout, 2) == N.VQA_ERR_STATE
    z = np.zeros((2, 16 * 16), np.uint8)
    assert _submit(engine, z, gray_planes(16, 16), prev0=z[0]) == N.VQA_OK
    assert engine.lib.vqa_motion_wait(engine.ctx, mout, 2) == N.VQA_OK
    z = np.zeros((1, 30 * 30 * 3 // 2), np.uint8)                      # 4:2:0 at 30: the chroma planes are 15
    assert _submit(engine, z, yuv420p_planes(30, 30)) == N.VQA_ERR_UNSUPPORTED
    # what vqa_vif_submit refuses is refused the same way: mixed depths, bad depths, odd 16-bit strides, a short frame stride
    z16 = np.zeros((2, 64 * 64 * 3 // 2), np.uint16)
    p10 = yuv_planes(64, 64, "420", 10)
    assert _submit(engine, z16, p10) == N.VQA_OK
    assert engine.lib.vqa_motion_wait(engine.ctx, mout, 6) == N.VQA_OK
    assert _submit(engine, z16, p10[:1] + [p[:5] for p in p10[1:]]) == N.VQA_ERR_INVALID
    assert _submit(engine, z16, [p[:5] + (17,) for p in p10]) == N.VQA_ERR_INVALID
    assert _submit(engine, z16, [(p[0], p[1], p[2], p[3] + 1, p[4], p[5]) for p in p10]) == N.VQA_ERR_INVALID
    assert engine.lib.vqa_motion_submit(engine.ctx, f.ctypes.data, None, N.VQA_MEM_HOST, 2, fb - 1, plane_descs(planes), 3) == N.VQA_ERR_INVALID
    assert engine.lib.vqa_motion_submit(engine.ctx, None, None, N.VQA_MEM_HOST, 2, fb, plane_descs(planes), 3) == N.VQA_ERR_INVALID
    assert engine.lib.vqa_motion_submit(engine.ctx, f.ctypes.data, None, 7, 2, fb, plane_descs(planes), 3) == N.VQA_ERR_INVALID
    assert engine.lib.vqa_motion_submit(engine.ctx, f.ctypes.data, None, N.VQA_MEM_HOST, 2, fb, plane_descs(planes), 5) == N.VQA_ERR_INVALID
    # nothing is pending and the ctx computes as before; trim gives the feature's buffers back and it re-grows them
    assert engine.lib.vqa_motion_wait(engine.ctx, mout, 6) == N.VQA_ERR_STATE
    assert engine.motion(f, planes).tobytes() == want.tobytes()
    engine.trim()
    assert engine.motion(f, planes).tobytes() == want.tobytes()
    assert engine.quality(f, d, planes).tobytes() == qwant.tobytes() and engine.adm(f, d, planes).tobytes() == awant.tobytes()


def _model_file(path, fmt, feats):
    """a seeded model of vmaf_v0.6.1's shape and magnitudes (about 200 support vectors, 6 features), its rho chosen so that the
    median frame of `feats` [n, 6] scores 50 through the JSON form"""
    rng = np.random.default_rng(7)
    sv, coef = rng.random((200, 6)), rng.uniform(-4.0, 4.0, 200)
    sv[rng.random(sv.shape) < 0.1] = 0.0
    slopes = [0.012020766332648465, 2.8098077502505414, 0.06264407466686016, 1.2227634563978586, 1.5360318811084146,
              1.7620864995501058, 2.08656468286432]
    intercepts = [-0.3092981927591963, -1.7993968597186747, -0.003017198086831897, -0.1728125095425364, -0.5294309090081222,
                  -0.7577185792093722, -1.083428597549764]
    ys = R.predict(feats, [1.0] + slopes[1:], [0.0] + intercepts[1:], None, 0.04, 0.0, coef, sv)
    rho = float(np.median(ys) - (50.0 * slopes[0] + intercepts[0]))
    with open(path, "w") as fh:
        fh.write(R.json_model(0.04, rho, coef, sv, slopes, intercepts, (0.0, 100.0)) if fmt == "json"
                 else R.libsvm_text(0.04, rho, coef, sv))
    return path


def test_one_pass_entry_points_with_a_model_file(tmp_path):
    """run_ffmpeg_metrics(.., vmaf_model_path): the psnr / ssim logs are byte for byte those of a plain run; the logged vif / adm
    values are those of a run without the model; every frame's vmaf is, bit for bit, vmaf_model.predict of the frame's logged
    features; process_video_and_extract_metrics with config vmaf_model_path: VMAF after SSIM = the pooled mean, MOTION2 and
    MOTION last, nothing else moves"""
    import adm_cases as A
    import rtvqa_amd
    from rtvqa_amd import frames, synth, vmaf_model
    from rtvqa_amd import video_processing as vp
    h, w, n = 96, 128, 7
    r, planes = K.clip("yuv420p", h, w, 8, "natural", seed=6, n=n)
    d = np.stack([K.flat(r)[i].copy() for i in range(n)])
    for i in range(n):
        for p in planes:
            pw, ph, off = p[:3]
            d[i, off:off + pw * ph] = A.distort(K.plane_of(r[i], p, 1), "blur" if i % 2 else "noise", 8, i).reshape(-1)
    pr, pd = str(tmp_path / "ref.y4m"), str(tmp_path / "enc.y4m")
    frames.write_y4m(pr, r, h, w)
    frames.write_y4m(pd, d, h, w)
    logs = {k: [str(tmp_path / ("%s_%s.log" % (k, t))) for t in ("psnr", "ssim", "vmaf")] for k in ("plain", "feat", "mot", "json", "text")}
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["plain"], batch_size=3) is None
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["feat"], batch_size=3, vif=True, adm=True) is None
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["mot"], batch_size=3, motion=True) is None
    feats = [[{**a["metrics"], **b["metrics"]}[k] for k in R.FEATURES_V061]
             for a, b in zip(json.load(open(logs["feat"][2]))["frames"], json.load(open(logs["mot"][2]))["frames"])]
    mj, mt = _model_file(str(tmp_path / "model.json"), "json", feats), _model_file(str(tmp_path / "model.txt"), "text", feats)
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["json"], mj, batch_size=3) is None
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["text"], vmaf_model_path=mt, batch_size=2) is None
    assert not os.path.exists(logs["plain"][2])
    for k in (0, 1):
        for kind in ("feat", "mot", "json", "text"):
            assert open(logs["plain"][k], "rb").read() == open(logs[kind][k], "rb").read(), (kind, k)
    feat, mot, doc, tdoc = (json.load(open(logs[k][2])) for k in ("feat", "mot", "json", "text"))
    assert "vmaf" not in json.dumps(feat) and "motion" not in json.dumps(feat) and "vmaf" not in json.dumps(mot)
    names = list(feat["frames"][0]["metrics"])
    assert list(mot["frames"][0]["metrics"]) == ["motion2", "motion"]
    assert list(doc["frames"][0]["metrics"]) == names + ["motion2", "motion", "vmaf"] == list(doc["pooled_metrics"])
    with rtvqa_amd.Engine(0) as eng:
        want = eng.motion(r, planes)[:, 0]["motion"]
    want2 = M.motion2(want)
    models = {"json": vmaf_model.load_model(mj), "text": vmaf_model.load_model(mt)}
    for tag, dc in (("json", doc), ("text", tdoc)):
        assert len(dc["frames"]) == n
        for i in range(n):
            m = dc["frames"][i]["metrics"]
            assert {k: m[k] for k in names} == feat["frames"][i]["metrics"]          # vif / adm as without the model
            assert m["motion"] == float(want[i]) == mot["frames"][i]["metrics"]["motion"] and m["motion2"] == float(want2[i])
            logged = [m[k] for k in R.FEATURES_V061]
            assert m["vmaf"] == vmaf_model.predict(models[tag], [logged])[0], (tag, i)      # bit for bit: no tolerance
        x = np.array([fr["metrics"]["vmaf"] for fr in dc["frames"]])
        p = dc["pooled_metrics"]["vmaf"]
        assert p["min"] == x.min() and p["max"] == x.max() and abs(p["mean"] - x.mean()) <= 1e-12
        assert {k: dc["pooled_metrics"][k] for k in names} == feat["pooled_metrics"]
    x = np.array([fr["metrics"]["vmaf"] for fr in doc["frames"]])
    print("vmaf per frame", np.round(x, 3).tolist(), "motion", np.round(want, 4).tolist())
    assert ((x >= 0.0) & (x <= 100.0)).all() and ((x > 0.0) & (x < 100.0)).any()
    gap = np.abs(want - M.motion(K.plane_series(r, planes[0])))
    assert gap.max() <= BAR and want[0] == 0.0 and (want[1:] > 0).all()
    bgr = synth.s_natural(n, h, w, seed=12)
    cfg = {"crf": 23, "resize_width": 64, "resize_height": 64, "frame_interval": 1, "batch_size": 2}
    row0 = vp.process_video_and_extract_metrics(pr, pd, dict(cfg, vif=True, adm=True), csv_file=str(tmp_path / "row0.csv"),
                                                column_order="fixed", encoded_bgr=bgr)
    row1 = vp.process_video_and_extract_metrics(pr, pd, dict(cfg, vif=True, adm=True, motion_feature=True),
                                                csv_file=str(tmp_path / "row1.csv"), column_order="fixed", encoded_bgr=bgr)
    row2 = vp.process_video_and_extract_metrics(pr, pd, dict(cfg, vmaf_model_path=mj), csv_file=str(tmp_path / "row2.csv"),
                                                column_order="fixed", encoded_bgr=bgr)
    assert "VMAF" not in row0 and "VMAF" not in row1 and "MOTION" not in row0
    k0 = list(row0)
    at = k0.index("ADM_scale3") + 1
    assert list(row1) == k0[:at] + ["MOTION2", "MOTION"] + k0[at:]
    k2 = list(row2)
    assert k2[k2.index("SSIM") + 1] == "VMAF" and [k for k in k2 if k != "VMAF"] == list(row1)
    for k in row0:
        assert row0[k] == row1[k] == row2[k] or (row0[k] != row0[k] and row1[k] != row1[k] and row2[k] != row2[k]), k
    assert row1["MOTION"] == row2["MOTION"] and abs(row1["MOTION"] - want.mean()) <= 1e-15 and abs(row1["MOTION2"] - want2.mean()) <= 1e-15
    assert row2["VMAF"] == doc["pooled_metrics"]["vmaf"]["mean"]
    # BGR frames, the halves sharing one upload, a model on resident frames
    rb, pb = K.clip("bgr24", h, w, 8, "natural", seed=2, n=5)
    db = synth.distort(rb)
    row3 = vp.process_video_and_extract_metrics(rb, db, dict(cfg, vmaf_model_path=mj), csv_file=str(tmp_path / "row3.csv"))
    with rtvqa_amd.Engine(0) as eng:
        row4 = vp.process_video_and_extract_metrics(eng.upload(rb), eng.upload(db), dict(cfg, vmaf_model_path=mj, batch_size=64),
                                                    csv_file=str(tmp_path / "row4.csv"))
        wb = eng.motion(rb, pb)[:, 0]["motion"]
    assert row3["VMAF"] == row4["VMAF"] and row3["MOTION"] == row4["MOTION"] and abs(row3["MOTION"] - wb.mean()) <= 1e-15


def test_profile_counts_one_launch_per_plane_group():
    import rtvqa_amd
    from rtvqa_amd import _native as N
    f, planes = K.clip("yuv420p", 96, 128, 8, "noise", seed=9, n=3)
    with rtvqa_amd.Engine(0) as eng:
        eng.lib.vqa_kernel_name.restype = C.c_char_p
        assert eng.lib.vqa_kernel_name(N.K_MOTION) == b"k_motion_sad" and eng.lib.vqa_kernel_name(18) == b"?"
        eng.profile(True)
        eng.motion(f, planes)
        ms, cnt = C.c_double(0), C.c_int64(0)
        assert eng.lib.vqa_profile_read(eng.ctx, N.K_MOTION, C.byref(ms), C.byref(cnt), 0) == N.VQA_OK
        assert cnt.value == 2 and ms.value > 0.0                          # luma; the two chroma planes together
        prof = eng.profile_read(reset=True)
        assert prof["k_motion_sad"][1] == 2 and "k_vif_stats" not in prof and "k_adm_scale" not in prof, prof
        fb, pb = K.clip("bgr24", 40, 56, 8, "noise", seed=9, n=2)
        eng.motion(fb, pb, prev0=fb[0])
        prof = eng.profile_read(reset=True)
        assert prof["k_motion_sad"][1] == 1, prof                          # B, G, R are one group
        eng.vif(f, f, planes)
        assert "k_motion_sad" not in eng.profile_read(reset=True)
        for bad in (14, 15, 18, N.K_END):
            assert eng.lib.vqa_profile_read(eng.ctx, bad, C.byref(ms), C.byref(cnt), 0) == N.VQA_ERR_INVALID
