"""GPU: clip-wide sync through the reference-shaped entry points - frame_sync, run_ffmpeg_metrics and
process_video_and_extract_metrics with and without the `sync` keys.  All cases use yuv420p at 64 x 48: 20 unrelated reference
frames and 12 distorted frames made from ref[3:15] with +-2 of noise (sync_cases.pass_clip).  Signatures and words are compared
for equality with the restatement (tests/sync_reference.py); files are compared byte for byte."""
import csv
import json
import logging
import os

import numpy as np
import pytest

import sync_cases as SC
import sync_reference as R

pytestmark = pytest.mark.gpu

H, W = 48, 64
KW = dict(layout="yuv420p", height=H, width=W)


@pytest.fixture(scope="module")
def clip():
    ref, dist = SC.pass_clip(h=H, w=W)
    assert ref.shape == (20, H * W * 3 // 2) and dist.shape == (12, H * W * 3 // 2)
    rs = R.signatures(ref[:, :H * W].reshape(20, H, W))
    ds = R.signatures(dist[:, :H * W].reshape(12, H, W))
    return ref, dist, rs, ds, R.cross(ds, rs)


def test_frame_sync_finds_the_offset(engine, clip):
    from rtvqa_amd import video_processing as vp
    ref, dist, rs, ds, (diag, best) = clip
    res = vp.frame_sync(ref, dist, engine=engine, **KW)
    assert (res["ref_sig"] == rs).all() and (res["dist_sig"] == ds).all()
    assert (res["diag"] == diag).all() and (res["best"] == best).all()
    assert (res["offset"], res["overlap"], res["frames_off"]) == (3, 12, 0)
    assert res["trim"] == (3, 0, 12) and not res["ambiguous"] and res["runs"] == [(0, 12, 3)]
    for window in (1, 5, 12, 20):   # any window gives the same signatures
        again = vp.frame_sync(ref, dist, engine=engine, window=window, **KW)
        assert (again["ref_sig"] == rs).all() and (again["dist_sig"] == ds).all() and again["offset"] == 3, window
    dev = vp.frame_sync(engine.upload(ref), engine.upload(dist), engine=engine, window=7, **KW)
    assert (dev["ref_sig"] == rs).all() and (dev["dist_sig"] == ds).all() and dev["trim"] == (3, 0, 12)


def test_refine_gives_the_band_at_the_found_offset(engine, clip):
    from rtvqa_amd import video_processing as vp
    ref, dist = clip[:2]
    res = vp.frame_sync(ref, dist, refine=2, engine=engine, **KW)
    want = vp.frame_align(ref[3:15], dist, radius=2, engine=engine, **KW)
    assert (res["align"]["sse"] == want["sse"]).all() and res["align"]["offset"] == 0
    luma = lambda a: a[:, :H * W].astype(np.int64)   # noqa: E731
    direct = ((luma(dist) - luma(ref[3:15])) ** 2).sum(axis=1)
    assert (res["align"]["sse"][:, 2] == direct.astype(np.uint64)).all()   # column 0 of the band: the pairs at the found offset


def _run(tmp_path, tag, ref, enc, **kw):
    from rtvqa_amd import video_processing as vp
    logs = [str(tmp_path / ("%s_%s.log" % (k, tag))) for k in ("psnr", "ssim", "vmaf")]
    assert vp.run_ffmpeg_metrics(ref, enc, *logs, **dict(KW, **kw)) is None
    return logs


def _same_files(a, b):
    for x, y in zip(a[:2], b[:2]):
        assert open(x, "rb").read() == open(y, "rb").read()


def test_sync_apply_gives_the_files_of_the_trimmed_pair(engine, tmp_path, clip, caplog):
    from rtvqa_amd import sync as S
    ref, dist = clip[:2]
    plain = _run(tmp_path, "plain", ref[3:15], dist)
    with caplog.at_level(logging.WARNING):
        synced = _run(tmp_path, "sync", ref, dist, sync=True, sync_apply=True)
    assert any("trimmed" in r.getMessage() for r in caplog.records)
    _same_files(plain, synced)
    assert not os.path.exists(plain[2])   # no kind is on: no feature log, as before
    doc = json.load(open(synced[2]))
    assert list(doc)[-6:] == list(S.SYNC_KEYS)
    assert (doc["SYNC_OFFSET"], doc["SYNC_OVERLAP"], doc["SYNC_FRAMES_OFF"], doc["SYNC_APPLIED"]) == (3, 12, 0, 1)
    assert 0.0 <= doc["SYNC_DISTANCE"] < doc["SYNC_RUNNER_UP"]
    # next to a kind: the feature log differs by the six keys only
    plain = _run(tmp_path, "plain_g", ref[3:15], dist, gmsd=True)
    synced = _run(tmp_path, "sync_g", ref, dist, gmsd=True, sync=True, sync_apply=True, sync_min_overlap=6)
    _same_files(plain, synced)
    doc = json.load(open(synced[2]))
    assert not any(k.startswith("SYNC") for k in json.load(open(plain[2])))
    for k in S.SYNC_KEYS:
        del doc[k]
    assert open(plain[2]).read() == json.dumps(doc, indent=1) + "\n"
    # resident streams are sliced by DeviceFrames.slice
    dev = _run(tmp_path, "sync_d", engine.upload(ref), engine.upload(dist), sync=True, sync_apply=True)
    _same_files(plain, dev)


def test_an_aligned_pair_is_left_alone(tmp_path, clip):
    ref, dist = clip[:2]
    plain = _run(tmp_path, "plain", ref[3:15], dist)
    for apply in (False, True):
        synced = _run(tmp_path, "sync%d" % apply, ref[3:15], dist, sync=True, sync_apply=apply)
        _same_files(plain, synced)
        doc = json.load(open(synced[2]))
        assert (doc["SYNC_OFFSET"], doc["SYNC_OVERLAP"], doc["SYNC_APPLIED"]) == (0, 12, 0)


def test_without_sync_apply_unequal_lengths_stay_the_error(tmp_path, clip):
    ref, dist = clip[:2]
    with pytest.raises(ValueError, match="ref and dist must have the same shape"):
        _run(tmp_path, "plain", ref, dist)
    with pytest.raises(ValueError, match="ref and dist must have the same shape"):
        _run(tmp_path, "sync", ref, dist, sync=True)


def test_a_static_distorted_clip_is_ambiguous_and_not_applied(tmp_path, clip, caplog):
    ref = clip[0]
    static = np.repeat(ref[7:8], 20, axis=0)   # twenty times reference frame 7: every offset that pairs it fits as well
    still_ref = np.repeat(ref[7:8], 20, axis=0)
    plain = _run(tmp_path, "plain", still_ref, static)
    with caplog.at_level(logging.WARNING):
        synced = _run(tmp_path, "sync", still_ref, static, sync=True, sync_apply=True)
    assert any("ambiguous" in r.getMessage() for r in caplog.records)
    _same_files(plain, synced)
    doc = json.load(open(synced[2]))
    assert (doc["SYNC_OFFSET"], doc["SYNC_APPLIED"], doc["SYNC_DISTANCE"], doc["SYNC_RUNNER_UP"]) == (0, 0, 0.0, 0.0)


def _bgr(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, H, W, 3)).astype(np.uint8)


def test_the_row_of_the_one_pass_entry_point(tmp_path, clip):
    from rtvqa_amd import sync as S
    from rtvqa_amd import video_processing as vp
    ref, dist = clip[:2]
    cfg = {"crf": 23, "resize_width": 64, "resize_height": 64, "frame_interval": 1, "batch_size": 16, "pixfmt": "yuv420p",
           "height": H, "width": W}
    bgr = _bgr(20, 5)
    plain = vp.process_video_and_extract_metrics(ref[3:15], dist, cfg, csv_file=str(tmp_path / "plain.csv"), column_order="fixed",
                                                 encoded_bgr=bgr[:12])
    synced = vp.process_video_and_extract_metrics(ref, dist, dict(cfg, sync=True, sync_apply=True),
                                                  csv_file=str(tmp_path / "sync.csv"), column_order="fixed", encoded_bgr=bgr[:12])
    assert list(synced)[:-6] == list(plain) and list(synced)[-6:] == list(S.SYNC_KEYS)
    assert all(repr(synced[k]) == repr(plain[k]) for k in plain)   # (repr: a NaN equals a NaN)
    assert [synced[k] for k in ("SYNC_OFFSET", "SYNC_OVERLAP", "SYNC_FRAMES_OFF", "SYNC_APPLIED")] == [3, 12, 0, 1]
    rows = list(csv.reader(open(str(tmp_path / "sync.csv"))))
    assert rows[0][-6:] == list(S.SYNC_KEYS) and rows[1][-6:-4] == ["3", "12"] and rows[1][-1] == "1"
    # the encoded stream is the long one: BOTH its BGR frames and its pair stream are sliced by the distorted side's trim, and
    # the ALIGN_* columns stay last
    long_dist = SC.noisy(ref, 2, 77)
    want = vp.process_video_and_extract_metrics(ref[3:15], long_dist[3:15], dict(cfg, align=2), csv_file=str(tmp_path / "w.csv"),
                                                column_order="fixed", encoded_bgr=bgr[3:15])
    got = vp.process_video_and_extract_metrics(ref[3:15], long_dist, dict(cfg, align=2, sync=True, sync_apply=True),
                                               csv_file=str(tmp_path / "g.csv"), column_order="fixed", encoded_bgr=bgr)
    assert list(got)[-11:-5] == list(S.SYNC_KEYS) and [k for k in got if k not in S.SYNC_KEYS] == list(want)
    assert all(repr(got[k]) == repr(want[k]) for k in want)
    assert (got["SYNC_OFFSET"], got["SYNC_OVERLAP"], got["SYNC_APPLIED"]) == (-3, 12, 1)


def test_a_rung_of_its_own_size_is_synchronised(tmp_path, clip):
    """the 2 x 2 mean of the distorted frames, 32 x 24: frame_sync reads plane 0 of either stream at its own size.  The pass
    itself resamples every plane, and the resampler's floor is 16 x 16 - the 16 x 12 chroma planes of a 32 x 24 4:2:0 rung are
    below it, as they were before - so the pass with scale and sync runs on the luma planes of the same frames (layout gray)."""
    from rtvqa_amd import video_processing as vp
    ref, dist = clip[:2]
    rung = SC.half_size(dist, H, W)
    assert rung.shape == (12, 24 * 32 * 3 // 2)
    res = vp.frame_sync(ref, rung, dist_height=24, dist_width=32, **KW)
    assert (res["offset"], res["overlap"], res["frames_off"]) == (3, 12, 0)
    assert (res["dist_sig"] == R.signatures(rung[:, :24 * 32].reshape(12, 24, 32))).all()
    scaled = dict(scale="bicubic", dist_height=24, dist_width=32)
    with pytest.raises(ValueError, match="at least 16 x 16"):
        _run(tmp_path, "chroma", ref, rung, sync=True, sync_apply=True, **scaled)
    luma, rung_luma = ref[:, :H * W].reshape(20, H, W), rung[:, :24 * 32].reshape(12, 24, 32)
    gray = dict(layout="gray", gmsd=True, **scaled)
    plain = _run(tmp_path, "plain", luma[3:15], rung_luma, **gray)
    synced = _run(tmp_path, "sync", luma, rung_luma, sync=True, sync_apply=True, **gray)
    _same_files(plain, synced)
    doc, was = json.load(open(synced[2])), json.load(open(plain[2]))
    assert (doc["SYNC_OFFSET"], doc["SYNC_FRAMES_OFF"], doc["SYNC_APPLIED"]) == (3, 0, 1)
    assert [k for k in doc if not k.startswith("SYNC")] == list(was) and doc["DIST_RES"] == "32x24"
    kept = _run(tmp_path, "kept", luma[3:15], rung_luma, sync=True, **gray)   # sync with scale is allowed, and nothing to cut
    _same_files(plain, kept)
    assert json.load(open(kept[2]))["SYNC_APPLIED"] == 0
