"""GPU: BRISQUE's natural-scene statistics (vqa_brisque_submit / vqa_brisque_wait) through the C ABI, the engine, the one-pass
stream and the reference-shaped entry points, against the restatements of tests/brisque_reference.py (written from the
definition in include/vqa.h; pinned by tests/test_brisque_host.py).

Everything that leaves the GPU is an integer, so the same frame gives the same bytes in any batch, from any memory.  The words
are NOT compared for equality with the restatement's: u = rint(m 2^16) of a double m that two machines form in another order
may fall on either side of a tie.  Every moment the words state is held within its bar of the float64 restatement (the bars are
derived in brisque_reference.py from Q = 16 and the restatement's own moments, never from the library's); flags are equal; each
alpha is within one grid step (libm ties) of the restatement's host formulas applied to the library's own words, every other
feature within 1e-9 of them; and on admitted fits (test_brisque_host.py: the float64 alpha moves by at most 2 steps when every
moment moves by its bar) alpha is within the admitted steps plus one of the float64 alpha.  Uniform noise on planes of 2000
samples or more is the clamp case: its scale-0 GGD alpha is exactly 10.0."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import brisque_cases as BC
import brisque_reference as R
import motion_cases as K

pytestmark = pytest.mark.gpu

FIELDS = BC.FIELDS


def _check_record(rec, want, tag):
    """one record against the restatements of its plane (an entry of BC.restated)"""
    ph, pw = want["x"].shape
    ws = R.record_words(rec)
    got = R.word_moments(ws, ph, pw)
    BC.close_moments(got, want["moments"], tag)
    assert int(rec["flags"]) == want["flags"] and int(rec["reserved"]) == 0, (tag, "flags", int(rec["flags"]), want["flags"])
    ft = rec["features"].astype(np.float64)
    assert not np.isnan(ft).any() and np.isfinite(ft).all(), tag
    own, own_flags, own_ks = R.word_features(ws, ph, pw)
    assert own_flags == int(rec["flags"]), tag
    for f in range(10):
        s, o = divmod(f, 5)
        at = 18 * s + (0 if o == 0 else 2 + 4 * (o - 1))
        if own_ks[f] < 0:
            assert (ft[at:at + (2 if o == 0 else 4)] == 0).all(), (tag, f)
            continue
        k = int(round(ft[at] * 1000.0)) - 200
        assert abs(ft[at] - (200 + k) / 1000.0) < 1e-12 and abs(k - own_ks[f]) <= 1, (tag, f, ft[at], own_ks[f])
        if o == 0:
            assert abs(ft[at + 1] - own[at + 1]) <= 1e-9 * max(1.0, abs(own[at + 1])), (tag, f, "sigma2")
        else:
            al = ft[at]
            l2, r2 = own[at + 2], own[at + 3]
            assert abs(ft[at + 2] - l2) <= 1e-9 * max(1.0, l2) and abs(ft[at + 3] - r2) <= 1e-9 * max(1.0, r2), (tag, f, "l2 r2")
            mean = R.aggd_mean(np.sqrt(l2), np.sqrt(r2), al)          # (at the library's own alpha)
            assert abs(ft[at + 1] - mean) <= 1e-9 * max(1.0, abs(mean)), (tag, f, "mean", ft[at + 1], mean)
        span = want["spans"][f]
        if span is not None and span <= 2:
            assert abs(k - want["ks"][f]) <= span + 1, (tag, f, "admitted", k, want["ks"][f], span)
        elif tag[0] == "natural":                                                # named, never silent
            assert ("%dx%d-%s" % tag[1:4], tag[4], tag[5], f) in BC.NOT_ADMITTED, (tag, f, span)
    if want["x"].size >= 2000 and tag[0] == "noise":
        assert ft[0] == 10.0, (tag, ft[0])


@pytest.mark.parametrize("geom,depth,layout,n", BC.GRID, ids=BC.IDS)
def test_every_moment_flag_and_fit_on_every_geometry_depth_layout_and_content(engine, geom, depth, layout, n):
    h, w = geom
    for kind in BC.KINDS:
        f, planes = BC.clip(layout, h, w, depth, kind, n)
        want = BC.restated(layout, h, w, depth, kind, n)
        got = engine.brisque(f, planes)
        assert got.shape == (n, len(planes)) and got.dtype.names == FIELDS
        for i in range(n):
            for j in range(len(planes)):
                _check_record(got[i, j], want[i][j], (kind, h, w, layout, i, j))
        # from device memory, and frame by frame from both: the same bytes
        df = engine.upload(np.ascontiguousarray(f))
        assert engine.brisque(df, planes).tobytes() == got.tobytes(), (kind, "device")
        for i in range(n):
            assert engine.brisque(f[i:i + 1], planes).tobytes() == got[i:i + 1].tobytes(), (kind, "host frame", i)
            assert engine.brisque(df.slice(i, i + 1), planes).tobytes() == got[i:i + 1].tobytes(), (kind, "device frame", i)
        df._owner.free()
        if kind == "zeros":
            assert (got["flags"] == 0x3ff).all() and (got["features"] == 0).all()
            for k in FIELDS[:9]:
                assert (got[k] == 0).all(), k
        else:
            assert (got["sum_abs_u"] > 0).all() and (got["n_neg"] > 0).all() and (got["n_pos"] > 0).all()   # (not vacuous)


def test_known_answers(engine):
    """an impulse on a tile corner, whose window falls into four tiles of a 40 x 130 plane and whose pairs wrap nowhere; the
    same impulse in the plane's corner, whose pairs wrap on every side"""
    for depth, v in ((8, 200), (16, 65535)):
        for y, x in ((16, 64), (0, 0), (39, 129), (0, 129)):
            p = np.zeros((40, 130), np.int64)
            p[y, x] = v
            f, planes = BC.gray_frames([p], depth)
            rec = engine.brisque(f, planes)[0, 0]
            ws = R.record_words(rec)
            want = R.words(p, depth)
            # 49 + 14 non-zero m at most, none within a rounding tie of the double's last bits: the words are the restatement's
            assert ws == want, (depth, y, x)
            assert ws[0]["sum_abs_u"] > 0 and ws[0]["n_neg"][0] > 0


def test_single_flag_bits(engine):
    """rows of 0 and 255: with a period of two rows only the H fit of scale 0 degenerates, with a period of one V, D1 and D2 do
    too; the degenerate fits' features are 0, the others' are not, and everything equals the restatement's"""
    for period, bits in ((2, 0b00010), (1, 0b11110)):
        p = BC.rows(40, 56, period)
        f, planes = BC.gray_frames([p], 8)
        rec = engine.brisque(f, planes)[0, 0]
        ft, flags, ks = R.float_features(p, 8)
        assert int(rec["flags"]) == flags and flags & 0x1f == bits, (period, int(rec["flags"]), flags)
        want = dict(x=p, moments=R.float_moments(p, 8), features=ft, flags=flags, ks=ks, spans=[None] * 10)
        _check_record(rec, want, ("rows", period))
        got = rec["features"]
        assert got[0] > 0 and got[1] > 0                                         # the GGD of scale 0 is not degenerate
        for o in range(4):
            four = got[2 + 4 * o: 6 + 4 * o]
            assert ((four == 0).all() if bits >> (1 + o) & 1 else (four[[0, 2, 3]] > 0).all()), (period, o, four)
        assert int(rec["n_neg"][0][0]) == 0 and int(rec["n_pos"][0][0]) == 40 * 56


def test_batches_positions_memory_kinds_and_views_give_the_same_words(engine):
    from rtvqa_amd import _native as N
    from rtvqa_amd.engine import DeviceFrames, plane_descs, yuv_planes
    h, w = 66, 98
    f, planes = K.clip("yuv420p", h, w, 8, "natural", seed=3, n=8)
    whole = engine.brisque(f, planes)
    assert engine.brisque(f, planes).tobytes() == whole.tobytes()               # run to run
    assert len({whole[i].tobytes() for i in range(8)}) == 8
    one = whole[2].tobytes()
    assert engine.brisque(f[2:3], planes)[0].tobytes() == one
    for size in (3, 8):
        for pos in (0, 1, size - 1):
            order = [k for k in range(8) if k != 2][:size - 1]
            order.insert(pos, 2)
            got = engine.brisque(f[order], planes)
            for at, k in enumerate(order):
                assert got[at].tobytes() == whole[k].tobytes(), (size, pos, at)
    df = engine.upload(f)
    assert engine.brisque(df, planes).tobytes() == whole.tobytes()
    assert engine.brisque(df.slice(2, 3), planes)[0].tobytes() == one
    pf = engine.alloc_pinned(f.shape)
    pf[...] = f
    assert engine.brisque(pf, planes).tobytes() == whole.tobytes()
    engine.free_pinned(pf)
    odd = DeviceFrames(df.ptr + df.frame_stride, 3, df.h, df.w, frame_stride=2 * df.frame_stride, row_stride=df.row_stride,
                       owner=df, channels=df.channels)
    assert engine.brisque(odd, planes).tobytes() == whole[[1, 3, 5]].tobytes()
    out = (N.VqaBrisqueMetrics * 9)()
    fb = f.shape[1]
    assert engine.lib.vqa_brisque_submit(engine.ctx, f.ctypes.data, N.VQA_MEM_HOST, 3, 2 * fb, plane_descs(planes), 3) == N.VQA_OK
    assert engine.lib.vqa_brisque_wait(engine.ctx, out, 9) == N.VQA_OK
    assert bytes(out) == whole[[0, 2, 4]].tobytes()
    # a 41 x 71 window at (7, 13) of a 60 x 100 frame, through offset and row stride
    g = np.random.default_rng(5).integers(0, 256, (2, 60, 100)).astype(np.uint8)
    cut = np.ascontiguousarray(g[:, 7:48, 13:84]).reshape(2, -1)
    alone = engine.brisque(cut, yuv_planes(41, 71, "mono", 8))
    assert engine.brisque(g.reshape(2, -1), [(71, 41, 7 * 100 + 13, 100, 1)]).tobytes() == alone.tobytes()
    # packed bgr24: each channel is the plane it would be alone
    b = np.random.default_rng(6).integers(0, 256, (2, 40, 56, 3)).astype(np.uint8)
    packed = engine.brisque(b, K.planes_of("bgr24", 40, 56))
    for ch in range(3):
        mono = np.ascontiguousarray(b[..., ch]).reshape(2, -1)
        assert engine.brisque(mono, yuv_planes(40, 56, "mono", 8))[:, 0].tobytes() == np.ascontiguousarray(packed[:, ch]).tobytes()


def _submit(engine, f, planes):
    from rtvqa_amd import _native as N
    from rtvqa_amd.engine import plane_descs
    fb = K.flat(f).shape[1] * f.dtype.itemsize
    return engine.lib.vqa_brisque_submit(engine.ctx, f.ctypes.data, N.VQA_MEM_HOST, f.shape[0], fb, plane_descs(planes),
                                         len(planes))


def test_the_state_machine_and_the_refusals(engine):
    from rtvqa_amd import _native as N
    from rtvqa_amd.engine import gray_planes, plane_descs, yuv420p_planes, yuv_planes
    f, planes = K.clip("yuv420p", 64, 96, 8, "natural", seed=8, n=2)
    want, cwant, awant = engine.brisque(f, planes), engine.cambi(f, planes), engine.artifacts(f, planes)
    nout, bout = (N.VqaBrisqueMetrics * 6)(), (N.VqaCambiMetrics * 6)()
    lib, ctx = engine.lib, engine.ctx
    assert lib.vqa_brisque_wait(ctx, nout, 6) == N.VQA_ERR_STATE                 # wait without submit
    assert _submit(engine, f, planes) == N.VQA_OK
    assert _submit(engine, f, planes) == N.VQA_ERR_STATE                         # submit while pending
    assert lib.vqa_cambi_wait(ctx, bout, 6) == N.VQA_ERR_STATE                   # a wait of another kind
    assert lib.vqa_trim(ctx) == N.VQA_ERR_STATE
    assert lib.vqa_brisque_wait(ctx, nout, 5) == N.VQA_ERR_STATE                 # a wrong entry count
    assert lib.vqa_brisque_wait(ctx, nout, 6) == N.VQA_OK
    assert bytes(nout) == want.tobytes()
    # the converse: a BRISQUE wait with only a CAMBI batch pending; it survives
    fb = K.flat(f).shape[1]
    pd = plane_descs(planes)
    assert lib.vqa_cambi_submit(ctx, f.ctypes.data, N.VQA_MEM_HOST, 2, fb, pd, 3) == N.VQA_OK
    assert lib.vqa_brisque_wait(ctx, nout, 6) == N.VQA_ERR_STATE
    assert lib.vqa_cambi_wait(ctx, bout, 6) == N.VQA_OK and bytes(bout) == cwant.tobytes()
    # in flight next to a CAMBI and an artefacts batch, whose host staging it shares, from host and device frames
    df = engine.upload(f)
    for a in (f, df):
        for order in (("brisque", "cambi", "artifacts"), ("artifacts", "cambi", "brisque")):
            engine.cambi_submit(a, planes)
            engine.brisque_submit(a, planes)
            engine.artifacts_submit(a, planes)
            wants = {"brisque": want, "cambi": cwant, "artifacts": awant}
            for kind in order:
                assert getattr(engine, kind + "_wait")().tobytes() == wants[kind].tobytes(), (order, kind)
    engine.brisque_submit(df, planes)
    engine.drain()                                                               # a pending batch is waited out
    assert lib.vqa_brisque_wait(ctx, nout, 6) == N.VQA_ERR_STATE
    # planes below 16: a failed submit leaves nothing in flight
    for h, w in ((15, 16), (16, 15)):
        z = np.zeros((2, h * w), np.uint8)
        assert _submit(engine, z, gray_planes(h, w)) == N.VQA_ERR_UNSUPPORTED, (h, w)
        assert lib.vqa_brisque_wait(ctx, nout, 2) == N.VQA_ERR_STATE
    z = np.zeros((1, 30 * 30 * 3 // 2), np.uint8)                                # 4:2:0 at 30: the chroma planes are 15
    assert _submit(engine, z, yuv420p_planes(30, 30)) == N.VQA_ERR_UNSUPPORTED
    small = np.zeros((1, 64), np.uint8)                                          # more than 2^28 samples: a descriptor check
    assert _submit(engine, small, [(16385, 16384, 0, 16385, 1)]) == N.VQA_ERR_UNSUPPORTED
    assert lib.vqa_brisque_submit(ctx, None, N.VQA_MEM_HOST, 2, fb, pd, 3) == N.VQA_ERR_INVALID
    assert lib.vqa_brisque_submit(ctx, f.ctypes.data, N.VQA_MEM_HOST, 2, fb - 1, pd, 3) == N.VQA_ERR_INVALID
    assert lib.vqa_brisque_submit(ctx, f.ctypes.data, 7, 2, fb, pd, 3) == N.VQA_ERR_INVALID
    z8, z16 = np.zeros((1, 32 * 32), np.uint8), np.zeros((1, 32 * 32), np.uint16)
    with pytest.raises(ValueError):
        engine.brisque(z8, yuv_planes(32, 32, "mono", 10))                       # a dtype that does not match the depth
    with pytest.raises(ValueError):
        engine.brisque(z16, gray_planes(32, 32))
    assert lib.vqa_brisque_wait(ctx, nout, 6) == N.VQA_ERR_STATE
    engine.trim()
    assert engine.brisque(f, planes).tobytes() == want.tobytes()
    assert engine.cambi(f, planes).tobytes() == cwant.tobytes()


def test_one_pass_entry_points(tmp_path):
    """frame_brisque at two batch sizes, run_ffmpeg_metrics(.., brisque=True) with and without a test-made model and config
    "brisque": true on a 6-frame 66 x 98 .y4m pair: the ENCODED stream is measured, in the same pass as PSNR / SSIM, whose logs
    are byte for byte those of a plain run; the log's values are Engine.brisque of the first plane; the row gains BRISQUE_ALPHA,
    BRISQUE_SIGMA2 (and BRISQUE with a model) after NOISE"""
    import rtvqa_amd
    from rtvqa_amd import brisque_model as bm
    from rtvqa_amd import frames, synth
    from rtvqa_amd import video_processing as vp
    h, w, n = 66, 98, 6
    d, planes = K.clip("yuv420p", h, w, 8, "natural", seed=6, n=n)
    r = K.clip("yuv420p", h, w, 8, "noise", seed=7, n=n)[0]
    pr, pd = str(tmp_path / "ref.y4m"), str(tmp_path / "enc.y4m")
    frames.write_y4m(pr, r, h, w)
    frames.write_y4m(pd, d, h, w)
    mp, rp = tmp_path / "m.model", tmp_path / "m.range"
    mp.write_text(BC.model_text(np.random.default_rng(3)))
    rp.write_text(BC.range_text(np.full(36, -1.0), np.full(36, 11.0)))
    model = bm.load_model(str(mp), str(rp))
    logs = {k: [str(tmp_path / ("%s_%s.log" % (k, t))) for t in ("psnr", "ssim", "vmaf")]
            for k in ("plain", "bsq", "feat", "both", "scored")}
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["plain"], batch_size=4) is None
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["bsq"], batch_size=4, brisque=True) is None
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["feat"], batch_size=4, gmsd=True, artifacts=True) is None
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["both"], batch_size=2, gmsd=True, artifacts=True, brisque=True) is None
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["scored"], batch_size=4, brisque_model_path=str(mp),
                                 brisque_range_path=str(rp)) is None     # (both keys turn brisque on)
    assert not os.path.exists(logs["plain"][2])
    for k in (0, 1):
        for kind in ("bsq", "feat", "both", "scored"):
            assert open(logs["plain"][k], "rb").read() == open(logs[kind][k], "rb").read(), (kind, k)
    with rtvqa_amd.Engine(0) as eng:
        want = eng.brisque(d, planes)
        assert eng.brisque(r, planes).tobytes() != want.tobytes()                 # (the reference stream would read otherwise)
    for bs in (2, 4):
        ft, flags, sizes = vp.frame_brisque(d, "yuv420p", h, w, batch_size=bs)
        assert sizes == [(q[0], q[1]) for q in planes] and ft.shape == (n, 3, 36) and flags.shape == (n, 3)
        assert ft.tobytes() == np.ascontiguousarray(want["features"]).tobytes() and (flags == want["flags"]).all()
    doc, feat, both, scored = (json.load(open(logs[k][2])) for k in ("bsq", "feat", "both", "scored"))
    mine = ["brisque_%02d" % k for k in range(36)]
    assert list(doc["frames"][0]["metrics"]) == mine == list(doc["pooled_metrics"])
    assert list(scored["frames"][0]["metrics"]) == mine + ["brisque"]
    names = list(feat["frames"][0]["metrics"])
    assert names[-1] == "noise" and "brisque" not in json.dumps(feat)
    assert list(both["frames"][0]["metrics"]) == names + mine
    score = bm.predict(model, want["features"][:, 0])
    for i in range(n):
        for dc in (doc, both, scored):
            assert [dc["frames"][i]["metrics"][k] for k in mine] == want["features"][i, 0].tolist()
        assert scored["frames"][i]["metrics"]["brisque"] == float(score[i])
        assert {k: both["frames"][i]["metrics"][k] for k in names} == feat["frames"][i]["metrics"]
    assert {k: both["pooled_metrics"][k] for k in names} == feat["pooled_metrics"]
    bgr = synth.s_natural(n, h, w, seed=12)
    cfg = {"crf": 23, "resize_width": 64, "resize_height": 64, "frame_interval": 1, "batch_size": 4}

    def row(name, **kw):
        return vp.process_video_and_extract_metrics(pr, pd, dict(cfg, **kw), csv_file=str(tmp_path / (name + ".csv")),
                                                    column_order="fixed", encoded_bgr=bgr)

    def same(a, b):
        return a == b or (a != a and b != b)

    cols = ["BRISQUE_ALPHA", "BRISQUE_SIGMA2"]
    row0, row1 = row("row0"), row("row1", brisque=True)
    k0 = list(row0)
    at = k0.index("SSIM") + 1
    assert list(row1) == k0[:at] + cols + k0[at:] and all(same(row0[k], row1[k]) for k in k0)
    for col, key in zip(cols, (0, 1)):
        assert row1[col] == doc["pooled_metrics"]["brisque_%02d" % key]["mean"]
        mean = want["features"][:, 0, key].mean()
        assert abs(row1[col] - mean) <= 1e-12 * max(1.0, abs(mean))
    row2 = row("row2", artifacts=True, batch_size=2)
    row3 = row("row3", artifacts=True, batch_size=2, brisque_model_path=str(mp), brisque_range_path=str(rp))
    k2 = list(row2)
    at = k2.index("NOISE") + 1
    assert list(row3) == k2[:at] + cols + ["BRISQUE"] + k2[at:] and all(same(row2[k], row3[k]) for k in k2)
    assert row3["BRISQUE_ALPHA"] == row1["BRISQUE_ALPHA"]
    assert abs(row3["BRISQUE"] - score.mean()) <= 1e-12 * max(1.0, abs(score.mean()))
    row("row0b", brisque=False)
    assert open(str(tmp_path / "row0.csv"), "rb").read() == open(str(tmp_path / "row0b.csv"), "rb").read()
    assert b"BRISQUE" not in open(str(tmp_path / "row0.csv"), "rb").read()
    assert b"NOISE,BRISQUE_ALPHA,BRISQUE_SIGMA2,BRISQUE" in open(str(tmp_path / "row3.csv"), "rb").read()
    with pytest.raises(ValueError):
        vp.validate_config(dict(cfg, brisque=1))


def test_profile_counts_the_launches_per_plane_group():
    import rtvqa_amd
    from rtvqa_amd import _native as N
    f, planes = K.clip("yuv420p", 66, 98, 8, "noise", seed=9, n=3)
    with rtvqa_amd.Engine(0) as eng:
        eng.lib.vqa_kernel_name.restype = C.c_char_p
        assert eng.lib.vqa_kernel_name(N.K_BRISQUE_MSCN) == b"k_brisque_mscn"
        eng.profile(True)
        eng.brisque(f, planes)
        prof = eng.profile_read(reset=True)
        # two plane groups (luma, chroma): one half, two mscn and two seam launches each
        assert prof["k_brisque_half"][1] == 2 and prof["k_brisque_mscn"][1] == 4 and prof["k_brisque_seam"][1] == 4, prof
        assert prof["k_brisque_mscn"][0] > 0.0 and "k_artifacts" not in prof, prof
        eng.artifacts(f, planes)
        assert "k_brisque_mscn" not in eng.profile_read(reset=True)
        ms, cnt = C.c_double(0), C.c_int64(0)
        for bad in (N.K_CLOSE, N.K_STOP, N.K_EDGE):                              # ids 41, 43 and 47 are unknown
            assert eng.lib.vqa_kernel_name(bad) == b"?"
            assert eng.lib.vqa_profile_read(eng.ctx, bad, C.byref(ms), C.byref(cnt), 0) == N.VQA_ERR_INVALID
