"""GPU: no-reference blockiness, blur and noise (vqa_artifacts_submit / vqa_artifacts_wait) through the C ABI, the engine, the
one-pass stream and the reference-shaped entry points, against the NumPy restatement of tests/artifacts_reference.py (written
from the definition in include/vqa.h).

Everything that leaves the GPU is an integer: all 21 words must be EQUAL to the restatement's, and so must phase_h and phase_v.
Every double must be within 2 ulp of the restatement's value formed from the record's own words - the bar of SI/TI's test for
host formulas (both sides do the same IEEE operations in the same order; 2 ulp leaves room for a compiler's choice of an
equivalent form, nothing more).  Position-independence tests compare bytes."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import artifacts_cases as AC
import artifacts_reference as R
import motion_cases as K

pytestmark = pytest.mark.gpu

FIELDS = ("edge_h", "edge_v", "blur_f_h", "blur_v_h", "blur_f_v", "blur_v_v", "lap", "phase_h", "phase_v", "blockiness",
          "blockiness_max", "blur_h", "blur_v", "blur", "noise")


def _check_record(rec, plane, depth, tag):
    """one record against the restatement of one plane [h, w]"""
    h, w = plane.shape
    want = R.words(plane)
    got = R.record_words(rec)
    for k in R.WORDS:
        assert got[k] == want[k], (tag, k, got[k], want[k])
    fig = R.figures(got, h, w, depth)
    assert int(rec["phase_h"]) == fig["phase_h"] and int(rec["phase_v"]) == fig["phase_v"], (tag, "phase")
    for k in R.DOUBLES:
        u = R.ulps(float(rec[k]), fig[k])
        assert u <= 2.0, (tag, k, float(rec[k]), fig[k], u)
    return fig


def _check(rec, frames, planes, depth, tag):
    n, npl = rec.shape
    for j, p in enumerate(planes):
        series = K.plane_series(frames, p)
        for i in range(n):
            _check_record(rec[i, j], series[i], depth, "%s frame %d plane %d" % (tag, i, j))


@pytest.mark.parametrize("geom,depth,layout,n", AC.GRID, ids=AC.IDS)
def test_every_word_on_every_geometry_depth_layout_and_content(engine, geom, depth, layout, n):
    h, w = geom
    for kind in K.KINDS:
        f, planes = AC.clip(layout, h, w, depth, kind, seed=h + w + depth, n=n)
        got = engine.artifacts(f, planes)
        assert got.shape == (n, len(planes)) and got.dtype.names == FIELDS
        _check(got, f, planes, depth, "%s %dx%d %s" % (kind, h, w, layout))
        assert (got["lap"] > 0).all() and got["blur_f_h"].sum() > 0 and got["blur_f_v"].sum() > 0   # (not vacuous)


@pytest.mark.parametrize("depth", [8, 10, 16])
def test_known_answers(engine, depth):
    peak = (1 << depth) - 1
    h, w = 72, 136
    # flat planes at 0 and at the peak: every word and every figure exactly 0, nothing NaN
    f, planes = AC.gray_frames([np.zeros((h, w), np.int64), np.full((h, w), peak, np.int64)], depth)
    got = engine.artifacts(f, planes)
    for k in FIELDS:
        assert (got[k] == 0).all() and not np.isnan(got[k].astype(np.float64)).any(), k
    # blocks, blocks shifted by (3, 5), the ramp
    f, planes = AC.gray_frames([AC.blocks(h, w, depth), AC.blocks(h, w, depth, (3, 5)), AC.ramp(h, w)], depth)
    got = engine.artifacts(f, planes)[:, 0]
    for i in range(3):
        _check_record(got[i], f[i].reshape(h, w).astype(np.int64), depth, "known %d" % i)
    assert got[0]["blockiness"] == 1.0 and got[0]["blockiness_max"] == 1.0 and got[0]["phase_h"] == 0 and got[0]["phase_v"] == 0
    assert (got[0]["edge_h"][1:] == 0).all() and got[0]["edge_h"][0] > 0
    assert got[1]["phase_h"] == 3 and got[1]["phase_v"] == 5 and got[1]["blockiness_max"] == 1.0 and got[1]["blockiness"] == -1.0
    assert got[2]["blur_h"] == 1.0 and got[2]["blur_v"] == 0.0 and got[2]["blur"] == 1.0 and got[2]["noise"] == 0.0
    assert got[2]["lap"] == 0 and got[2]["blur_f_v"] == 0 and got[2]["blur_f_h"] == h * (w - 9)


def test_the_checkerboard_at_16_bits_has_the_closed_form(engine):
    """0 / 65535 on 64 x 96: every step and every dB9 is 65535, the largest value a sample can add to each word"""
    h, w, peak = 64, 96, 65535
    f, planes = AC.gray_frames([AC.checker(h, w, peak)], 16)
    got = engine.artifacts(f, planes)[0, 0]
    want = AC.checker_words(h, w, peak, R.counts)
    assert R.record_words(got) == want
    assert want == R.words(AC.checker(h, w, peak))
    assert R.ulps(float(got["blur"]), 1.0 / 9.0) <= 2.0 and got["blur_h"] == got["blur_v"]
    _check_record(got, AC.checker(h, w, peak), 16, "checker")


def test_an_impulse_on_a_tile_corner(engine):
    """one sample of v at (32, 64), the first sample of a tile of a 70 x 130 plane: its terms fall into four tiles"""
    h, w, v = 70, 130, 200
    p = AC.impulse(h, w, 32, 64, v)
    f, planes = AC.gray_frames([p], 8)
    got = engine.artifacts(f, planes)[0, 0]
    e = [v, v, 0, 0, 0, 0, 0, 0]                       # boundaries 64 and 65 (rows 32 and 33): phases 0 and 1
    assert R.record_words(got) == dict(edge_h=e, edge_v=e, blur_f_h=2 * v, blur_v_h=18 * v, blur_f_v=2 * v, blur_v_v=18 * v,
                                       lap=16 * v)
    _check_record(got, p, 8, "impulse")


def test_batches_positions_memory_kinds_and_views_give_the_same_words(engine):
    from rtvqa_amd import _native as N
    from rtvqa_amd.engine import DeviceFrames, plane_descs, yuv_planes
    h, w = 66, 98
    f, planes = AC.clip("yuv420p", h, w, 8, "natural", seed=3, n=8)
    whole = engine.artifacts(f, planes)
    assert engine.artifacts(f, planes).tobytes() == whole.tobytes()               # run to run
    assert len({whole[i].tobytes() for i in range(8)}) == 8
    # the same frame at positions 0, 1 and last of batches of 1, 3 and 8
    one = whole[2].tobytes()
    assert engine.artifacts(f[2:3], planes)[0].tobytes() == one
    for size in (3, 8):
        for pos in (0, 1, size - 1):
            order = [k for k in range(8) if k != 2][:size - 1]
            order.insert(pos, 2)
            got = engine.artifacts(f[order], planes)
            for at, k in enumerate(order):
                assert got[at].tobytes() == whole[k].tobytes(), (size, pos, at)
    # host, pinned and device memory, a slice and a strided view of the resident clip
    df = engine.upload(f)
    assert engine.artifacts(df, planes).tobytes() == whole.tobytes()
    assert engine.artifacts(df.slice(2, 3), planes)[0].tobytes() == one
    pf = engine.alloc_pinned(f.shape)
    pf[...] = f
    assert engine.artifacts(pf, planes).tobytes() == whole.tobytes()
    engine.free_pinned(pf)
    odd = DeviceFrames(df.ptr + df.frame_stride, 3, df.h, df.w, frame_stride=2 * df.frame_stride, row_stride=df.row_stride,
                       owner=df, channels=df.channels)
    assert engine.artifacts(odd, planes).tobytes() == whole[[1, 3, 5]].tobytes()
    out = (N.VqaArtifactsMetrics * 9)()
    fb = f.shape[1]
    assert engine.lib.vqa_artifacts_submit(engine.ctx, f.ctypes.data, N.VQA_MEM_HOST, 3, 2 * fb, plane_descs(planes), 3) == N.VQA_OK
    assert engine.lib.vqa_artifacts_wait(engine.ctx, out, 9) == N.VQA_OK
    assert bytes(out) == whole[[0, 2, 4]].tobytes()
    # a 41 x 71 window at (7, 13) of a 60 x 100 frame, through offset and row stride: rows that no load of four is aligned to
    g = np.random.default_rng(5).integers(0, 256, (2, 60, 100)).astype(np.uint8)
    cut = np.ascontiguousarray(g[:, 7:48, 13:84]).reshape(2, -1)
    alone = engine.artifacts(cut, yuv_planes(41, 71, "mono", 8))
    assert engine.artifacts(g.reshape(2, -1), [(71, 41, 7 * 100 + 13, 100, 1)]).tobytes() == alone.tobytes()
    _check(alone, cut, yuv_planes(41, 71, "mono", 8), 8, "window")


def _submit(engine, f, planes):
    from rtvqa_amd import _native as N
    from rtvqa_amd.engine import plane_descs
    fb = K.flat(f).shape[1] * f.dtype.itemsize
    return engine.lib.vqa_artifacts_submit(engine.ctx, f.ctypes.data, N.VQA_MEM_HOST, f.shape[0], fb, plane_descs(planes),
                                           len(planes))


def test_the_state_machine_and_the_refusals(engine):
    from rtvqa_amd import _native as N
    from rtvqa_amd.engine import gray_planes, plane_descs, yuv420p_planes, yuv_planes
    f, planes = AC.clip("yuv420p", 64, 96, 8, "natural", seed=8, n=2)
    want, cwant = engine.artifacts(f, planes), engine.cambi(f, planes)
    rout, bout = (N.VqaArtifactsMetrics * 6)(), (N.VqaCambiMetrics * 6)()
    lib, ctx = engine.lib, engine.ctx
    assert lib.vqa_artifacts_wait(ctx, rout, 6) == N.VQA_ERR_STATE               # wait without submit
    assert _submit(engine, f, planes) == N.VQA_OK
    assert _submit(engine, f, planes) == N.VQA_ERR_STATE                         # submit while pending
    assert lib.vqa_cambi_wait(ctx, bout, 6) == N.VQA_ERR_STATE                   # a wait of another kind
    assert lib.vqa_trim(ctx) == N.VQA_ERR_STATE
    assert lib.vqa_artifacts_wait(ctx, rout, 5) == N.VQA_ERR_STATE               # a wrong entry count
    assert lib.vqa_artifacts_wait(ctx, rout, 6) == N.VQA_OK
    assert bytes(rout) == want.tobytes()
    # the converse: an artefacts wait with only a CAMBI batch pending; it survives
    fb = K.flat(f).shape[1]
    pd = plane_descs(planes)
    assert lib.vqa_cambi_submit(ctx, f.ctypes.data, N.VQA_MEM_HOST, 2, fb, pd, 3) == N.VQA_OK
    assert lib.vqa_artifacts_wait(ctx, rout, 6) == N.VQA_ERR_STATE
    assert lib.vqa_cambi_wait(ctx, bout, 6) == N.VQA_OK and bytes(bout) == cwant.tobytes()
    # in flight next to a CAMBI batch, whose host staging it shares, from host and device frames: each wait collects its own
    df = engine.upload(f)
    for a in (f, df):
        for order in (("artifacts", "cambi"), ("cambi", "artifacts")):
            engine.cambi_submit(a, planes)
            engine.artifacts_submit(a, planes)
            wants = {"artifacts": want, "cambi": cwant}
            for kind in order:
                assert getattr(engine, kind + "_wait")().tobytes() == wants[kind].tobytes(), (order, kind)
    engine.artifacts_submit(df, planes)
    engine.drain()                                                               # a pending batch is waited out
    assert lib.vqa_artifacts_wait(ctx, rout, 6) == N.VQA_ERR_STATE
    # planes below 16: a failed submit leaves nothing in flight
    for h, w in ((15, 16), (16, 15)):
        z = np.zeros((2, h * w), np.uint8)
        assert _submit(engine, z, gray_planes(h, w)) == N.VQA_ERR_UNSUPPORTED, (h, w)
        assert lib.vqa_artifacts_wait(ctx, rout, 2) == N.VQA_ERR_STATE
    z = np.zeros((1, 30 * 30 * 3 // 2), np.uint8)                                # 4:2:0 at 30: the chroma planes are 15
    assert _submit(engine, z, yuv420p_planes(30, 30)) == N.VQA_ERR_UNSUPPORTED
    small = np.zeros((1, 64), np.uint8)                                          # more than 2^28 samples: a descriptor check
    assert _submit(engine, small, [(16385, 16384, 0, 16385, 1)]) == N.VQA_ERR_UNSUPPORTED
    assert lib.vqa_artifacts_submit(ctx, None, N.VQA_MEM_HOST, 2, fb, pd, 3) == N.VQA_ERR_INVALID
    assert lib.vqa_artifacts_submit(ctx, f.ctypes.data, N.VQA_MEM_HOST, 2, fb - 1, pd, 3) == N.VQA_ERR_INVALID
    assert lib.vqa_artifacts_submit(ctx, f.ctypes.data, 7, 2, fb, pd, 3) == N.VQA_ERR_INVALID
    z8, z16 = np.zeros((1, 32 * 32), np.uint8), np.zeros((1, 32 * 32), np.uint16)
    with pytest.raises(ValueError):
        engine.artifacts(z8, yuv_planes(32, 32, "mono", 10))                     # a dtype that does not match the depth
    with pytest.raises(ValueError):
        engine.artifacts(z16, gray_planes(32, 32))
    assert lib.vqa_artifacts_wait(ctx, rout, 6) == N.VQA_ERR_STATE
    engine.trim()
    assert engine.artifacts(f, planes).tobytes() == want.tobytes()
    assert engine.cambi(f, planes).tobytes() == cwant.tobytes()


def test_one_pass_entry_points(tmp_path):
    """frame_artifacts at two batch sizes, run_ffmpeg_metrics(.., artifacts=True) and config "artifacts": true on a 6-frame
    66 x 98 .y4m pair: the ENCODED stream is measured, in the same pass as PSNR / SSIM, whose logs are byte for byte those of a
    plain run; the log's values are Engine.artifacts of the first plane; the row gains BLOCKINESS, BLUR, NOISE after VCA_L"""
    import rtvqa_amd
    from rtvqa_amd import frames, synth
    from rtvqa_amd import video_processing as vp
    h, w, n = 66, 98, 6
    d, planes = AC.clip("yuv420p", h, w, 8, "natural", seed=6, n=n)
    r = AC.clip("yuv420p", h, w, 8, "noise", seed=7, n=n)[0]
    pr, pd = str(tmp_path / "ref.y4m"), str(tmp_path / "enc.y4m")
    frames.write_y4m(pr, r, h, w)
    frames.write_y4m(pd, d, h, w)
    logs = {k: [str(tmp_path / ("%s_%s.log" % (k, t))) for t in ("psnr", "ssim", "vmaf")] for k in ("plain", "art", "feat", "both")}
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["plain"], batch_size=4) is None
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["art"], batch_size=4, artifacts=True) is None
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["feat"], batch_size=4, gmsd=True, vca=True) is None
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["both"], batch_size=2, gmsd=True, vca=True, artifacts=True) is None
    assert not os.path.exists(logs["plain"][2])
    for k in (0, 1):
        for kind in ("art", "feat", "both"):
            assert open(logs["plain"][k], "rb").read() == open(logs[kind][k], "rb").read(), (kind, k)
    with rtvqa_amd.Engine(0) as eng:
        want = eng.artifacts(d, planes)
        assert eng.artifacts(r, planes).tobytes() != want.tobytes()               # (the reference stream would read otherwise)
    keys = ("blockiness", "blockiness_max", "phase_h", "phase_v", "blur", "noise")
    for bs in (2, 4):
        out, sizes = vp.frame_artifacts(d, "yuv420p", h, w, batch_size=bs)
        assert sorted(out) == sorted(keys) and sizes == [(q[0], q[1]) for q in planes]
        for key in keys:
            assert out[key].shape == (n, 3) and out[key].tobytes() == np.ascontiguousarray(want[key]).tobytes(), (bs, key)
    doc, feat, both = (json.load(open(logs[k][2])) for k in ("art", "feat", "both"))
    mine = ["blockiness", "blur", "noise"]
    assert list(doc["frames"][0]["metrics"]) == mine == list(doc["pooled_metrics"])
    names = list(feat["frames"][0]["metrics"])
    assert names[-1] == "vca_l" and "blockiness" not in json.dumps(feat)
    assert list(both["frames"][0]["metrics"]) == names + mine
    for i in range(n):
        for dc in (doc, both):
            for key in mine:
                assert dc["frames"][i]["metrics"][key] == float(want[key][i, 0])
        assert {k: both["frames"][i]["metrics"][k] for k in names} == feat["frames"][i]["metrics"]
    assert {k: both["pooled_metrics"][k] for k in names} == feat["pooled_metrics"]
    bgr = synth.s_natural(n, h, w, seed=12)
    cfg = {"crf": 23, "resize_width": 64, "resize_height": 64, "frame_interval": 1, "batch_size": 4}

    def row(name, **kw):
        return vp.process_video_and_extract_metrics(pr, pd, dict(cfg, **kw), csv_file=str(tmp_path / (name + ".csv")),
                                                    column_order="fixed", encoded_bgr=bgr)

    def same(a, b):
        return a == b or (a != a and b != b)

    cols = ["BLOCKINESS", "BLUR", "NOISE"]
    row0, row1 = row("row0"), row("row1", artifacts=True)
    k0 = list(row0)
    at = k0.index("SSIM") + 1
    assert list(row1) == k0[:at] + cols + k0[at:] and all(same(row0[k], row1[k]) for k in k0)
    for col, key in zip(cols, mine):
        assert row1[col] == doc["pooled_metrics"][key]["mean"]
        assert abs(row1[col] - want[key][:, 0].mean()) <= 1e-12 * max(1.0, abs(want[key][:, 0].mean()))
    row2, row3 = row("row2", vca=True, batch_size=2), row("row3", vca=True, artifacts=True, batch_size=2)
    k2 = list(row2)
    at = k2.index("VCA_L") + 1
    assert list(row3) == k2[:at] + cols + k2[at:] and all(same(row2[k], row3[k]) for k in k2)
    assert row3["NOISE"] == row1["NOISE"]
    row("row0b", artifacts=False)
    assert open(str(tmp_path / "row0.csv"), "rb").read() == open(str(tmp_path / "row0b.csv"), "rb").read()
    assert b"BLOCKINESS" not in open(str(tmp_path / "row0.csv"), "rb").read()
    assert b"VCA_L,BLOCKINESS,BLUR,NOISE" in open(str(tmp_path / "row3.csv"), "rb").read()
    with pytest.raises(ValueError):
        vp.validate_config(dict(cfg, artifacts=1))


def test_profile_counts_one_launch_per_plane_group():
    import rtvqa_amd
    from rtvqa_amd import _native as N
    f, planes = AC.clip("yuv420p", 66, 98, 8, "noise", seed=9, n=3)
    with rtvqa_amd.Engine(0) as eng:
        eng.lib.vqa_kernel_name.restype = C.c_char_p
        assert eng.lib.vqa_kernel_name(N.K_ARTIFACTS) == b"k_artifacts"
        eng.profile(True)
        eng.artifacts(f, planes)
        prof = eng.profile_read(reset=True)
        assert prof["k_artifacts"][1] == 2 and prof["k_artifacts"][0] > 0.0 and "k_cambi_mask" not in prof, prof
        eng.cambi(f, planes)
        assert "k_artifacts" not in eng.profile_read(reset=True)
        ms, cnt = C.c_double(0), C.c_int64(0)
        for bad in (N.K_CLOSE, N.K_STOP):                                        # ids 41 and 43 are unknown
            assert eng.lib.vqa_kernel_name(bad) == b"?"
            assert eng.lib.vqa_profile_read(eng.ctx, bad, C.byref(ms), C.byref(cnt), 0) == N.VQA_ERR_INVALID
