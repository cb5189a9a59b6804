"""run_ffmpeg_metrics(.., fields=True) on the GPU: a telecined distorted clip against its progressive film reference - the nine
keys where the issue puts them, FIELDS_MATCH 0 and the warnings - and the same calls without the flag, whose files the flag must
not change; process_video_and_extract_metrics' row with the config key."""
import json
import logging

import numpy as np
import pytest

from rtvqa_amd import fields as F
from rtvqa_amd import video_processing as vp

pytestmark = pytest.mark.gpu

H, W, FILM = 48, 64, 24


@pytest.fixture(scope="module")
def pair(engine):
    """(30 progressive frames, the 2:3 pulldown of their first 24), planar yuv420p"""
    from rtvqa_amd import synth
    from rtvqa_amd.frames import bgr_to_yuv420p
    bgr = synth.s_natural(4 * 30, H, W, seed=5)[::4]
    ref = bgr_to_yuv420p(bgr)
    top, bottom = F.telecine_plan(FILM)
    dist = vp.frame_weave(bgr_to_yuv420p(synth.distort(bgr)), "yuv420p", top, bottom, H, W, engine=engine, window=7)
    assert dist.shape == ref.shape
    return ref, dist, bgr


def _logs(tmp_path, tag):
    return [str(tmp_path / ("%s_%s.log" % (k, tag))) for k in ("psnr", "ssim", "vmaf")]


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def test_the_nine_keys_the_warning_and_untouched_files(pair, tmp_path, caplog):
    import os
    ref, dist, _ = pair
    kw = dict(layout="yuv420p", height=H, width=W)
    plain, flagged, kind, both = (_logs(tmp_path, t) for t in ("plain", "flagged", "kind", "both"))
    vp.run_ffmpeg_metrics(ref, dist, *plain, **kw)
    assert not os.path.exists(plain[2])                                # nothing asked for a feature log: as ever
    with caplog.at_level(logging.WARNING, logger=vp.__name__):
        vp.run_ffmpeg_metrics(ref, dist, *flagged, fields=True, **kw)
    assert sum("not progressive" in r.getMessage() for r in caplog.records) == 1
    assert sum("differ in field structure" in r.getMessage() for r in caplog.records) == 1
    assert _read(flagged[0]) == _read(plain[0]) and _read(flagged[1]) == _read(plain[1])   # the frames were not changed
    doc = json.load(open(flagged[2]))
    got = {k: doc[k] for k in F.FIELDS_KEYS}
    assert got == dict(FIELDS_REF_TYPE="progressive", FIELDS_REF_COMBED=0, FIELDS_REF_CADENCE="none", FIELDS_REF_REPEATS=0,
                       FIELDS_DIST_TYPE="tff", FIELDS_DIST_COMBED=got["FIELDS_DIST_COMBED"], FIELDS_DIST_CADENCE="3:2",
                       FIELDS_DIST_REPEATS=12, FIELDS_MATCH=0)
    assert got["FIELDS_DIST_COMBED"] >= 12                             # the two mixed frames of each of six periods at least
    # next to a kind and a pre-pass: the log without the flag is what it was, and the flag adds the nine keys before the pre-pass's
    vp.run_ffmpeg_metrics(ref, dist, *kind, vif=True, align=2, **kw)
    vp.run_ffmpeg_metrics(ref, dist, *both, vif=True, align=2, fields=True, **kw)
    without, with_ = json.load(open(kind[2])), json.load(open(both[2]))
    assert not any(k.startswith("FIELDS_") for k in without)
    assert {k: v for k, v in with_.items() if k not in F.FIELDS_KEYS} == without
    keys = list(with_)
    at = keys.index("FIELDS_REF_TYPE")
    assert keys[at:at + 9] == list(F.FIELDS_KEYS) and keys[at + 9:] == [k for k in without if k.startswith("ALIGN_")]
    assert [k for k in keys if k not in F.FIELDS_KEYS] == list(without)
    assert _read(both[0]) == _read(kind[0]) == _read(plain[0])


def test_frame_fields_and_the_inverse_over_the_pair(pair, engine):
    ref, dist, _ = pair
    rec, a = vp.frame_fields(dist, "yuv420p", H, W, engine=engine, window=11)
    assert (a["cadence"], a["phase"], a["order"], a["breaks"]) == ("3:2", 0, "tff", []) and len(rec) == 30
    back = vp.frame_weave(dist, "yuv420p", *F.ivtc_plan(a, 30), H, W, engine=engine, window=5)
    assert back.shape == (FILM, ref.shape[1])
    _, again = vp.frame_fields(back, "yuv420p", H, W, engine=engine)
    assert again["clip_type"] == "progressive" and again["cadence"] == "none"
    with pytest.raises(ValueError, match="name source frames"):
        vp.frame_weave(dist, "yuv420p", [30], [0], H, W, engine=engine)


def test_the_row_gains_the_nine_columns(pair, tmp_path):
    ref, dist, bgr = pair
    cfg = {"crf": 23, "resize_width": 64, "resize_height": 64, "frame_interval": 1, "batch_size": 16, "pixfmt": "yuv420p",
           "height": H, "width": W}
    plain = vp.process_video_and_extract_metrics(ref, dist, cfg, csv_file=str(tmp_path / "a.csv"), column_order="fixed",
                                                 encoded_bgr=bgr)
    row = vp.process_video_and_extract_metrics(ref, dist, dict(cfg, fields=True), csv_file=str(tmp_path / "b.csv"),
                                               column_order="fixed", encoded_bgr=bgr)
    assert list(row)[-9:] == list(F.FIELDS_KEYS) and list(row)[:-9] == list(plain)
    assert {k: row[k] for k in plain} == plain
    assert row["FIELDS_MATCH"] == 0 and row["FIELDS_DIST_CADENCE"] == "3:2" and row["FIELDS_REF_TYPE"] == "progressive"
