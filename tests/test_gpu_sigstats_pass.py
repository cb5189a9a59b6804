"""GPU: the signal statistics inside the one-pass entry points.  A short clip with a black frame, a frozen pair, a cut and bars
(tests/sigstats_cases.py::qc_clip) goes through run_ffmpeg_metrics(.., sigstats=True) and through
process_video_and_extract_metrics with "sigstats": true; the log and the row are checked against direct engine calls on the
REFERENCE stream and events.signal_events, for two batch sizes, and once with every other switch on too."""
import json
import os

import numpy as np
import pytest

import sigstats_cases as SC
import sigstats_reference as R
from rtvqa_amd import events
from rtvqa_amd import video_processing as vp

pytestmark = pytest.mark.gpu

H, W = 64, 96                                   # 4:2:0 chroma of 32 x 48: VCA's smallest plane
KEYS = ["y_min", "y_low", "y_avg", "y_high", "y_max", "y_dif", "out_of_range", "black", "frozen", "scene_score"]
COLS = ["Y_LOW", "Y_HIGH", "OUT_OF_RANGE", "BLACK_FRAMES", "FROZEN_FRAMES", "SCENE_CUTS", "CROP_TOP", "CROP_BOTTOM", "CROP_LEFT",
        "CROP_RIGHT"]


@pytest.fixture(scope="module")
def clip():
    """-> (ref, dist [n, samples] yuv420p, planes, the luma's [n, h, w], the box)"""
    luma, box = SC.qc_clip(H, W)
    rng = np.random.default_rng(9)

    def per_plane(k, ph, pw):
        return luma if k == 0 else rng.integers(100, 150, (len(luma), ph, pw))
    ref, planes = SC.pack("yuv420p", H, W, 8, per_plane)
    dist = np.clip(ref.astype(np.int64) + rng.integers(-3, 4, ref.shape), 0, 255).astype(np.uint8)
    return ref, dist, planes, luma, box


def _want(engine, ref, planes, **levels):
    rec = engine.sigstats(ref, planes, **levels)
    return rec, events.signal_events(rec, 8)


def _check_log(doc, rec, ev, n_px):
    assert list(doc["frames"][0]["metrics"])[-len(KEYS):] == KEYS
    for i, fr in enumerate(doc["frames"]):
        m, r = fr["metrics"], rec[i, 0]
        assert [m[k] for k in KEYS[:6]] == [float(r[k]) for k in ("min", "low", "mean", "high", "max", "dif")], i
        assert m["out_of_range"] == (int(r["under"]) + int(r["over_luma"])) / n_px
        assert (m["black"], m["frozen"], m["scene_score"]) == (float(ev["black"][i]), float(ev["frozen"][i]), float(ev["scene_score"][i]))
    assert doc["signal"] == {"black_frames": int(ev["black"].sum()), "frozen_frames": int(ev["frozen"].sum()),
                             "scene_cuts": len(ev["cuts"]), "crop": list(ev["crop"])}


def test_the_engine_sees_the_clip_as_it_was_made(engine, clip):
    ref, _dist, planes, luma, box = clip
    rec, ev = _want(engine, ref, planes)
    want = R.series(luma, 8)
    for i in range(len(luma)):
        assert not R.same_words(rec[i, 0], want[i]), (i, R.same_words(rec[i, 0], want[i]))
    assert ev["black_runs"] == [(2, 2)] and ev["frozen_runs"] == [(4, 4)] and ev["cuts"] == [2, 5] and ev["crop"] == box
    got = vp.frame_sigstats(ref, "yuv420p", H, W, batch_size=3)
    assert got.tobytes() == rec.tobytes()
    assert vp.frame_sigstats(ref, "yuv420p", H, W, batch_size=64, black_level=20, crop_level=30).tobytes() == \
        engine.sigstats(ref, planes, black_level=20, crop_level=30).tobytes()


@pytest.mark.parametrize("batch_size", [2, 5])
def test_run_ffmpeg_metrics(engine, clip, tmp_path, batch_size):
    ref, dist, planes, _luma, _box = clip
    rec, ev = _want(engine, ref, planes)
    logs = {k: [str(tmp_path / ("%s_%s.log" % (k, t))) for t in ("psnr", "ssim", "vmaf")] for k in ("plain", "sig", "siti", "both")}
    kw = dict(layout="yuv420p", height=H, width=W, batch_size=batch_size)
    assert vp.run_ffmpeg_metrics(ref, dist, *logs["plain"], **kw) is None
    assert not os.path.exists(logs["plain"][2])
    assert vp.run_ffmpeg_metrics(ref, dist, *logs["sig"], sigstats=True, **kw) is None
    doc = json.load(open(logs["sig"][2]))
    assert list(doc["frames"][0]["metrics"]) == KEYS and len(doc["frames"]) == len(ref)
    _check_log(doc, rec, ev, H * W)
    for k in (0, 1):                               # the stats files are those of a run without the flag
        assert open(logs["sig"][k], "rb").read() == open(logs["plain"][k], "rb").read()
    # next to another kind: its keys first, byte for byte what they were
    assert vp.run_ffmpeg_metrics(ref, dist, *logs["siti"], siti=True, **kw) is None
    assert vp.run_ffmpeg_metrics(ref, dist, *logs["both"], siti=True, sigstats=True, **kw) is None
    one, both = json.load(open(logs["siti"][2])), json.load(open(logs["both"][2]))
    assert list(both["frames"][0]["metrics"]) == ["si", "ti"] + KEYS and "signal" not in one
    assert [{k: f["metrics"][k] for k in ("si", "ti")} for f in both["frames"]] == [f["metrics"] for f in one["frames"]]
    _check_log(both, rec, ev, H * W)
    # other levels reach the kernels
    assert vp.run_ffmpeg_metrics(ref, dist, *logs["sig"], sigstats=True, sigstats_black=10, sigstats_crop=23, **kw) is None
    rec2, ev2 = _want(engine, ref, planes, black_level=10, crop_level=23)
    assert ev2["black_runs"] == [] and ev2["crop"] == (0, H - 1, 0, W - 1)
    _check_log(json.load(open(logs["sig"][2])), rec2, ev2, H * W)


@pytest.mark.parametrize("batch_size", [2, 5])
def test_process_video_and_extract_metrics(engine, clip, tmp_path, batch_size):
    """bgr24: the quality pair and the complexity half read the same frames; plane 0 is B"""
    _ref, _dist, _planes, luma, box = clip
    from rtvqa_amd.engine import bgr_planes
    ref = np.repeat(luma[..., None], 3, axis=3).astype(np.uint8)
    ref[..., 1] = np.clip(luma + 7, 0, 255)        # (G and R differ from B: the row reads plane 0)
    rng = np.random.default_rng(4)
    enc = np.clip(ref.astype(np.int64) + rng.integers(-2, 3, ref.shape), 0, 255).astype(np.uint8)
    rec, ev = _want(engine, ref, bgr_planes(H, W))
    want = R.series(luma, 8)
    assert not any(R.same_words(rec[i, 0], want[i]) for i in range(len(luma)))
    cfg = {"crf": 23, "resize_width": 64, "resize_height": 64, "frame_interval": 1, "batch_size": batch_size}
    row0 = vp.process_video_and_extract_metrics(ref, enc, dict(cfg), csv_file=str(tmp_path / "a.csv"), column_order="fixed")
    row = vp.process_video_and_extract_metrics(ref, enc, dict(cfg, sigstats=True), csv_file=str(tmp_path / "b.csv"), column_order="fixed")
    names0, names = list(row0), list(row)
    at = names.index("Y_LOW")
    assert names[at:at + len(COLS)] == COLS and names[:at] + names[at + len(COLS):] == names0
    assert {k: row[k] for k in names0} == row0
    assert row["Y_LOW"] == float(rec[:, 0]["low"].min()) and row["Y_HIGH"] == float(rec[:, 0]["high"].max())
    assert row["OUT_OF_RANGE"] == float(np.mean((rec[:, 0]["under"].astype(np.float64) + rec[:, 0]["over_luma"]) / (H * W)))
    assert [row[k] for k in COLS[3:]] == [1, 1, 2] + list(box)
    assert (int(ev["black"].sum()), int(ev["frozen"].sum()), ev["cuts"], ev["crop"]) == (1, 1, [2, 5], box)
    row2 = vp.process_video_and_extract_metrics(ref, enc, dict(cfg, sigstats=True, sigstats_crop=23, fsim=True),
                                                csv_file=str(tmp_path / "c.csv"), column_order="fixed")
    assert list(row2)[list(row2).index("FSIMC") + 1] == "Y_LOW" and [row2[k] for k in COLS[6:]] == [0, H - 1, 0, W - 1]


def test_with_every_other_switch_on(engine, clip, tmp_path):
    import test_gpu_stream_all_on as TA
    ref, dist, planes, _luma, _box = clip
    rec, ev = _want(engine, ref, planes)
    flags = {flag: True for flag in TA.FLAGS}
    logs = {k: [str(tmp_path / ("%s_%s.log" % (k, t))) for t in ("psnr", "ssim", "vmaf")] for k in ("all", "all+sig")}
    kw = dict(layout="yuv420p", height=H, width=W, batch_size=3)
    assert vp.run_ffmpeg_metrics(ref, dist, *logs["all"], **flags, **kw) is None
    assert vp.run_ffmpeg_metrics(ref, dist, *logs["all+sig"], sigstats=True, **flags, **kw) is None
    old, doc = json.load(open(logs["all"][2])), json.load(open(logs["all+sig"][2]))
    names0 = list(old["frames"][0]["metrics"])
    assert names0[-1] == "fsimc" and list(doc["frames"][0]["metrics"]) == names0 + KEYS
    for a, b in zip(old["frames"], doc["frames"]):       # (as text: a NaN a kind may give on the black frame equals itself)
        assert json.dumps({k: b["metrics"][k] for k in names0}) == json.dumps(a["metrics"])
    assert json.dumps({k: doc["pooled_metrics"][k] for k in names0}) == json.dumps(old["pooled_metrics"])
    _check_log(doc, rec, ev, H * W)
    for k in (0, 1):
        assert open(logs["all"][k], "rb").read() == open(logs["all+sig"][k], "rb").read()
