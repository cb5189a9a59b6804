"""GPU: spatial registration through the reference-shaped entry points - frame_shift on a clip whose distorted stream is the
reference moved by two samples, run_ffmpeg_metrics and process_video_and_extract_metrics with and without the `shift` key, and
with `align` next to it.  The grid is compared word for word with the restatement (tests/shift_reference.py); SHIFT_PSNR_GAIN is
host arithmetic on exact integers and is held to 4 ulp of the same formula over the restatement's sums."""
import csv
import json
import math
import os

import numpy as np
import pytest

import shift_cases as SC
import shift_reference as R

pytestmark = pytest.mark.gpu

MOVED = (2, -2)


@pytest.fixture(scope="module")
def clip():
    ref, enc = SC.moved_clip(shift=MOVED)
    want = R.grids(ref.astype(np.int64), enc.astype(np.int64), 4)
    total = want.astype(object).sum(axis=0)
    return ref, enc, want, 10.0 * math.log10(int(total[4, 4]) / int(total[4 + MOVED[0], 4 + MOVED[1]]))


def test_frame_shift_finds_the_move(engine, clip):
    from rtvqa_amd import video_processing as vp
    ref, enc, want, gain = clip
    res = vp.frame_shift(ref, enc, "gray", radius=4, engine=engine)
    assert res["sse"].dtype == np.uint64 and (res["sse"] == want).all()
    assert res["shift"] == MOVED and res["per_frame"] == [MOVED] * len(ref) and res["frames_off"] == 0 and res["edge"] is False
    print("psnr_gain %.17g, the restatement's %.17g" % (res["psnr_gain"], gain))
    assert abs(res["psnr_gain"] - gain) <= 4 * math.ulp(gain)
    for window in (1, 4):   # any window size gives the same array
        assert (vp.frame_shift(ref, enc, "gray", radius=4, engine=engine, window=window)["sse"] == want).all(), window
    edge = vp.frame_shift(ref, enc, "gray", radius=2, margin=4, engine=engine)   # the move lies on the border of R = 2
    assert edge["shift"] == MOVED and edge["edge"] is True and (edge["sse"] == want[:, 2:-2, 2:-2]).all()


def _bgr(a):
    return np.ascontiguousarray(np.repeat(a[..., None], 3, axis=3))


def _run(tmp_path, tag, ref, enc, **kw):
    from rtvqa_amd import video_processing as vp
    logs = [str(tmp_path / ("%s_%s.log" % (k, tag))) for k in ("psnr", "ssim", "vmaf")]
    assert vp.run_ffmpeg_metrics(ref, enc, *logs, **kw) is None
    return logs


def test_run_ffmpeg_metrics_writes_the_keys_and_nothing_else_changes(tmp_path, clip):
    from rtvqa_amd import align as A
    from rtvqa_amd import shift as S
    from rtvqa_amd import video_processing as vp
    ref, enc, _want, gain = clip
    ref, enc = _bgr(ref), _bgr(enc)   # plane 0 of bgr24 is the B channel: the same samples
    plain = _run(tmp_path, "plain", ref, enc)
    none = _run(tmp_path, "none", ref, enc, shift=None, shift_margin=None)
    moved = _run(tmp_path, "shift", ref, enc, shift=4)
    for a, b, c in zip(plain[:2], none[:2], moved[:2]):
        assert open(a, "rb").read() == open(b, "rb").read() == open(c, "rb").read()
    assert not os.path.exists(plain[2]) and not os.path.exists(none[2])   # no kind is on: no feature log, as before
    doc = json.load(open(moved[2]))
    assert list(doc)[-5:] == list(S.SHIFT_KEYS)
    assert [doc[k] for k in S.SHIFT_KEYS[:4]] == [4, MOVED[0], MOVED[1], 0] and abs(doc["SHIFT_PSNR_GAIN"] - gain) <= 4 * math.ulp(gain)
    row = vp.extract_metrics_from_logs(*moved, "x", 23, 0, "64x48", 30.0)
    assert list(row)[-5:] == list(S.SHIFT_KEYS) and (row["SHIFT_DY"], row["SHIFT_DX"]) == MOVED
    # next to a kind: the feature log without the key is the log with it minus the five keys, byte for byte
    plain = _run(tmp_path, "plain_g", ref, enc, gmsd=True)
    none = _run(tmp_path, "none_g", ref, enc, gmsd=True, shift=None)
    moved = _run(tmp_path, "shift_g", ref, enc, gmsd=True, shift=4, shift_margin=6)
    for a, b, c in zip(plain, none, moved[:2] + none[2:]):
        assert open(a, "rb").read() == open(b, "rb").read() == open(c, "rb").read()
    doc = json.load(open(moved[2]))
    assert not any(k.startswith("SHIFT") for k in json.load(open(plain[2])))
    assert (doc["SHIFT_DY"], doc["SHIFT_DX"]) == MOVED
    for k in S.SHIFT_KEYS:
        del doc[k]
    assert open(plain[2]).read() == json.dumps(doc, indent=1) + "\n"
    # align and shift together: both groups, ALIGN_* first
    both = _run(tmp_path, "both", ref, enc, align=2, shift=4)
    doc = json.load(open(both[2]))
    assert list(doc)[-10:] == list(A.ALIGN_KEYS) + list(S.SHIFT_KEYS)
    # (what the temporal band says of moved noise is its own matter: in place, no frame of it resembles any other)
    assert [doc[k] for k in S.SHIFT_KEYS[:4]] == [4, MOVED[0], MOVED[1], 0] and doc["ALIGN_RADIUS"] == 2


def test_the_row_of_the_one_pass_entry_point(tmp_path, clip):
    from rtvqa_amd import align as A
    from rtvqa_amd import shift as S
    from rtvqa_amd import video_processing as vp
    ref, enc, _want, gain = clip
    ref, enc = _bgr(ref), _bgr(enc)
    cfg = {"crf": 23, "resize_width": 64, "resize_height": 64, "frame_interval": 1, "batch_size": 16}
    plain = vp.process_video_and_extract_metrics(ref, enc, cfg, csv_file=str(tmp_path / "plain.csv"), column_order="fixed")
    none = vp.process_video_and_extract_metrics(ref, enc, dict(cfg, shift=None), csv_file=str(tmp_path / "none.csv"),
                                                column_order="fixed")
    moved = vp.process_video_and_extract_metrics(ref, enc, dict(cfg, shift=4), csv_file=str(tmp_path / "shift.csv"),
                                                 column_order="fixed")
    assert open(str(tmp_path / "plain.csv"), "rb").read() == open(str(tmp_path / "none.csv"), "rb").read()
    assert list(none) == list(plain) and list(moved)[:-5] == list(plain) and list(moved)[-5:] == list(S.SHIFT_KEYS)
    assert all(repr(moved[k]) == repr(plain[k]) for k in plain)   # (repr: a NaN equals a NaN)
    assert [moved[k] for k in S.SHIFT_KEYS[:4]] == [4, MOVED[0], MOVED[1], 0] and abs(moved["SHIFT_PSNR_GAIN"] - gain) <= 4 * math.ulp(gain)
    rows = list(csv.reader(open(str(tmp_path / "shift.csv"))))
    assert rows[0][-5:] == list(S.SHIFT_KEYS) and rows[1][-5:-1] == ["4", str(MOVED[0]), str(MOVED[1]), "0"]
    assert "SHIFT" not in open(str(tmp_path / "plain.csv")).read().splitlines()[0]
    both = vp.process_video_and_extract_metrics(ref, enc, dict(cfg, align=2, shift=4), csv_file=str(tmp_path / "both.csv"),
                                                column_order="fixed")
    assert list(both)[:-10] == list(plain) and list(both)[-10:] == list(A.ALIGN_KEYS) + list(S.SHIFT_KEYS)
    assert list(csv.reader(open(str(tmp_path / "both.csv"))))[0][-10:] == list(A.ALIGN_KEYS) + list(S.SHIFT_KEYS)
