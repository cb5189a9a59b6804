"""GPU: a ladder rung through the pass.  A 4:2:0 clip of 9 frames at 48 x 32 against its 96 x 64 reference, batch_size 4 (three
chunks on two lanes): stream.run and run_ffmpeg_metrics with dist_planes / scale give, byte for byte, what the direct engine
calls and the unscaled entry points give on frames scaled beforehand (tests/scale_reference.py fed the library's tables) - the
rung is uploaded at its own size and resampled on the lane that measures it."""
import json
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import scale_cases as SC

pytestmark = pytest.mark.gpu

N_FRAMES, H, W, OH, OW = 9, 32, 48, 64, 96
FILTER = "bicubic"


@pytest.fixture(scope="module")
def clip():
    from rtvqa_amd import synth
    from rtvqa_amd.frames import bgr_to_yuv420p
    src = synth.s_natural(N_FRAMES, OH, OW, seed=11)
    bgr = synth.distort(synth.s_natural(N_FRAMES, H, W, seed=11))
    ref, rung = bgr_to_yuv420p(src), bgr_to_yuv420p(bgr)
    planes, out_planes = SC.planes_of("420", H, W), SC.planes_of("420", OH, OW)
    pre = SC.expected(rung, planes, out_planes, SC.frame_bytes(out_planes), FILTER, 8)
    assert pre.shape == ref.shape and (pre != SC.FILL).any()
    return dict(ref=ref, rung=rung, bgr=bgr, pre=pre, planes=planes, out_planes=out_planes)


def test_a_quality_only_pass_equals_the_engine_on_prescaled_frames(engine, clip):
    from rtvqa_amd import stream
    q = stream.Quality(clip["out_planes"], vif=True, gmsd=True, cambi=True, dist_planes=clip["planes"], scale=FILTER)
    got, _ = stream.run(clip["rung"], clip["ref"], quality=q, batch_size=4)
    rec = stream.records_by_kind(got, q)
    ref, pre, op = clip["ref"], clip["pre"], clip["out_planes"]
    want_q = engine.quality(ref, pre, op)
    assert rec["sse"].tobytes() == want_q["sse"].tobytes() and rec["ssim"].tobytes() == want_q["ssim"].tobytes()
    assert rec["vif"].tobytes() == engine.vif(ref, pre, op).tobytes()
    assert rec["gmsd"].tobytes() == engine.gmsd(ref, pre, op).tobytes()
    assert rec["cambi"].tobytes() == engine.cambi(pre, op).tobytes()            # the banding index AT THE REFERENCE'S geometry
    assert rec["cambi"].shape == (N_FRAMES, 3) and int(rec["sse"].sum()) > 0
    native = engine.cambi(clip["rung"], clip["planes"])                         # ... the rung itself is another measurement
    assert native.shape == rec["cambi"].shape
    # pinned and resident streams travel their own ways to the same bytes
    dev, _ = stream.run(engine.upload(clip["rung"]), engine.upload(ref), quality=q, batch_size=4)
    assert all(a is b or np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(dev, got))


def _run(vp, tmp, name, ref, dist, **kw):
    paths = [os.path.join(tmp, "%s_%s.log" % (name, k)) for k in ("psnr", "ssim", "vmaf")]
    vp.run_ffmpeg_metrics(ref, dist, *paths, layout="yuv420p", batch_size=4, vif=True, gmsd=True, cambi=True, **kw)
    return [open(p).read() for p in paths]


def test_run_ffmpeg_metrics_with_the_keys_equals_the_call_on_prescaled_frames(engine, clip, tmp_path):
    from rtvqa_amd import video_processing as vp
    tmp = str(tmp_path)
    scaled = _run(vp, tmp, "scaled", clip["ref"], clip["rung"], height=OH, width=OW, dist_height=H, dist_width=W, scale=FILTER)
    plain = _run(vp, tmp, "plain", clip["ref"], clip["pre"], height=OH, width=OW)
    assert scaled[0] == plain[0] and scaled[1] == plain[1] and scaled[0].count("\n") == N_FRAMES
    a, b = json.loads(scaled[2]), json.loads(plain[2])
    assert list(a)[-2:] == ["DIST_RES", "SCALE"] and a.pop("DIST_RES") == "%dx%d" % (W, H) and a.pop("SCALE") == FILTER
    assert a == b and "cambi" in a["pooled_metrics"] and "vif_scale0" in a["pooled_metrics"]
    # the stats lines are the engine's records on the prescaled frames
    q = engine.quality(clip["ref"], clip["pre"], clip["out_planes"])
    sizes = [(p[0], p[1]) for p in clip["out_planes"]]
    assert scaled[0] == vp.psnr_stats_lines(1, q["sse"], sizes, "yuv")
    # .y4m pairs bring their sizes in their headers
    from rtvqa_amd.frames import write_y4m
    rp, dp = os.path.join(tmp, "ref.y4m"), os.path.join(tmp, "rung.y4m")
    write_y4m(rp, clip["ref"], OH, OW)
    write_y4m(dp, clip["rung"], H, W)
    files = _run(vp, tmp, "y4m", rp, dp, scale=FILTER)
    assert files == scaled
    with pytest.raises(ValueError):                       # sizes that merely differ: nothing is scaled silently
        _run(vp, tmp, "differ", rp, dp)


def test_without_the_keys_an_equal_size_pair_is_what_it_was(engine, clip, tmp_path):
    from rtvqa_amd import video_processing as vp
    tmp = str(tmp_path)
    explicit = _run(vp, tmp, "explicit", clip["ref"], clip["pre"], height=OH, width=OW, dist_height=None, dist_width=None, scale=None)
    default = _run(vp, tmp, "default", clip["ref"], clip["pre"], height=OH, width=OW)
    assert explicit == default
    doc = json.loads(default[2])
    assert list(doc) == ["frames", "pooled_metrics"]
    q = engine.quality(clip["ref"], clip["pre"], clip["out_planes"])
    sizes = [(p[0], p[1]) for p in clip["out_planes"]]
    assert default[0] == vp.psnr_stats_lines(1, q["sse"], sizes, "yuv") and default[1] == vp.ssim_stats_lines(1, q["ssim"], sizes, "yuv")
    g = engine.gmsd(clip["ref"], clip["pre"], clip["out_planes"])
    assert [f["metrics"]["gmsd"] for f in doc["frames"]] == [float(v) for v in g[:, 0]["gmsd"]]


def test_qdist_next_to_a_native_size_bgr_stream(engine, clip):
    """the complexity half goes on reading the BGR stream at the rung's size; the quality half gets the scaled rung"""
    from rtvqa_amd import stream
    q = stream.Quality(clip["out_planes"], gmsd=True, dist_planes=clip["planes"], scale=FILTER)
    cx = stream.Complexity((64, 64), 1)
    got, series = stream.run(clip["bgr"], clip["ref"], quality=q, complexity=cx, batch_size=4, qdist=clip["rung"])
    rec = stream.records_by_kind(got, q)
    want_q = engine.quality(clip["ref"], clip["pre"], clip["out_planes"])
    assert rec["sse"].tobytes() == want_q["sse"].tobytes() and rec["ssim"].tobytes() == want_q["ssim"].tobytes()
    assert rec["gmsd"].tobytes() == engine.gmsd(clip["ref"], clip["pre"], clip["out_planes"]).tobytes()
    _none, alone = stream.run(clip["bgr"], complexity=cx, batch_size=4)
    for kind in stream.KINDS + ("temporal",):
        assert series[kind] == alone[kind] and len(series[kind]) >= N_FRAMES - 2, kind


def test_the_one_pass_row_carries_dist_res_and_scale_last(engine, clip, tmp_path):
    from rtvqa_amd import video_processing as vp
    cfg = {"crf": 23, "resize_width": 64, "resize_height": 64, "frame_interval": 1, "batch_size": 4, "pixfmt": "yuv420p",
           "height": OH, "width": OW, "gmsd": True, "cambi": True}
    row = vp.process_video_and_extract_metrics(clip["ref"], clip["rung"], dict(cfg, scale=FILTER, dist_height=H, dist_width=W),
                                               csv_file=str(tmp_path / "a.csv"), encoded_bgr=clip["bgr"])
    plain = vp.process_video_and_extract_metrics(clip["ref"], clip["pre"], cfg, csv_file=str(tmp_path / "b.csv"),
                                                 encoded_bgr=clip["bgr"])
    assert list(row)[-2:] == ["DIST_RES", "SCALE"] and row["DIST_RES"] == "%dx%d" % (W, H) and row["SCALE"] == FILTER
    assert list(row)[:-2] == list(plain) and all(row[k] == plain[k] or (row[k] != row[k] and plain[k] != plain[k]) for k in plain)
    head = open(str(tmp_path / "a.csv")).readline().strip().split(",")
    assert head[-2:] == ["DIST_RES", "SCALE"] and "DIST_RES" not in open(str(tmp_path / "b.csv")).readline()
    from rtvqa_amd import complexity_metrics as cm
    cm.release_buffers()


def test_the_combined_one_stream_form_is_refused(engine, clip):
    from rtvqa_amd import stream
    from rtvqa_amd.engine import bgr_planes
    src = np.zeros((N_FRAMES, OH, OW, 3), np.uint8)
    q = stream.Quality(bgr_planes(OH, OW), dist_planes=bgr_planes(H, W), scale=FILTER)
    with pytest.raises(ValueError, match="one BGR stream serves both halves"):
        stream.run(clip["bgr"], src, quality=q, complexity=stream.Complexity((64, 64), 1), batch_size=4)
    got, _ = stream.run(clip["bgr"], src, quality=q, batch_size=4)           # the quality half alone may
    assert got[0].shape == (N_FRAMES, 3)
    assert not getattr(engine, "_pending_k", None)


def test_frame_scale_returns_the_scaled_stream(engine, clip):
    from rtvqa_amd import video_processing as vp
    out = vp.frame_scale(clip["rung"], "yuv420p", H, W, OH, OW, FILTER, batch_size=4)
    assert out.dtype == np.uint8 and (out == clip["pre"]).all()
    wide = (clip["rung"].astype(np.uint16) << 2) | 3
    out10 = vp.frame_scale(wide, "yuv420p10le", H, W, OH, OW, "lanczos", batch_size=5)
    planes, op = SC.planes_of("420", H, W, 10), SC.planes_of("420", OH, OW, 10)
    want = SC.expected(np.ascontiguousarray(wide).view(np.uint8), planes, op, SC.frame_bytes(op), "lanczos", 10)
    assert out10.dtype == np.uint16 and (out10.view(np.uint8) == want).all()
    bgr = vp.frame_scale(clip["bgr"], "bgr24", None, None, OH, OW, "bilinear")
    bp, bo = SC.planes_of("bgr24", H, W), SC.planes_of("bgr24", OH, OW)
    assert (bgr == SC.expected(clip["bgr"].reshape(N_FRAMES, -1), bp, bo, OH * OW * 3, "bilinear", 8)).all()
