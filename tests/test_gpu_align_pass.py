"""GPU: temporal alignment through the reference-shaped entry points - frame_align on the clip with a dropped and a repeated
frame, run_ffmpeg_metrics and process_video_and_extract_metrics with and without the `align` key.  The band is compared word for
word with the restatement (tests/align_reference.py); ALIGN_PSNR_GAIN is host arithmetic on exact integers and is held to 4 ulp of
the same formula over the restatement's integers."""
import csv
import json
import math
import os

import numpy as np
import pytest

import align_cases as AC
import align_reference as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def clip():
    ref, enc, index = AC.dropped_and_repeated(h=48, w=64)
    want = R.band(ref.astype(np.int64), enc.astype(np.int64), 4)
    given = sum(int(want[j, 4]) for j in range(40))
    aligned = sum(int(want[j, 4 + index[j] - j]) for j in range(40))
    return ref, enc, index, want, 10.0 * math.log10(given / aligned)


def test_frame_align_finds_the_dropped_and_the_repeated_frame(engine, clip):
    from rtvqa_amd import video_processing as vp
    ref, enc, index, want, gain = clip
    res = vp.frame_align(ref, enc, "gray", radius=4, engine=engine)
    assert res["sse"].dtype == np.uint64 and (res["sse"] == want).all()
    assert res["ref_index"] == index and (res["offset"], res["dropped"], res["repeated"]) == (0, 1, 1)
    print("psnr_gain %.17g, the restatement's %.17g" % (res["psnr_gain"], gain))
    assert abs(res["psnr_gain"] - gain) <= 4 * math.ulp(gain)
    for window in (1, 9, 40):   # any window size gives the same array
        assert (vp.frame_align(ref, enc, "gray", radius=4, engine=engine, window=window)["sse"] == want).all(), window
    # clips of different lengths: the rows past the reference's end name no frame
    short = vp.frame_align(ref[:20], enc, "gray", radius=4, engine=engine, window=16)["sse"]
    assert (short == R.band(ref[:20].astype(np.int64), enc.astype(np.int64), 4)).all() and (short[30:] == R.NONE).all()


def _bgr(a):
    return np.ascontiguousarray(np.repeat(a[..., None], 3, axis=3))


def _run(tmp_path, tag, ref, enc, **kw):
    from rtvqa_amd import video_processing as vp
    logs = [str(tmp_path / ("%s_%s.log" % (k, tag))) for k in ("psnr", "ssim", "vmaf")]
    assert vp.run_ffmpeg_metrics(ref, enc, *logs, **kw) is None
    return logs


def test_run_ffmpeg_metrics_writes_the_keys_and_nothing_else_changes(tmp_path, clip):
    from rtvqa_amd import align as A
    from rtvqa_amd import video_processing as vp
    ref, enc, _index, _want, gain = clip
    ref, enc = _bgr(ref), _bgr(enc)   # plane 0 of bgr24 is the B channel: the same samples
    plain = _run(tmp_path, "plain", ref, enc)
    lined = _run(tmp_path, "align", ref, enc, align=4)
    for a, b in zip(plain[:2], lined[:2]):
        assert open(a, "rb").read() == open(b, "rb").read()
    assert not os.path.exists(plain[2])   # no kind is on: no feature log, as before
    doc = json.load(open(lined[2]))
    assert list(doc)[-5:] == list(A.ALIGN_KEYS)
    assert [doc[k] for k in A.ALIGN_KEYS[:4]] == [4, 0, 1, 1] and abs(doc["ALIGN_PSNR_GAIN"] - gain) <= 4 * math.ulp(gain)
    row = vp.extract_metrics_from_logs(*lined, "x", 23, 0, "64x48", 30.0)
    assert list(row)[-5:] == list(A.ALIGN_KEYS) and row["ALIGN_DROPPED"] == 1 and row["ALIGN_REPEATED"] == 1
    # next to a kind: the feature log without the key is the log with it minus the five keys, byte for byte
    plain = _run(tmp_path, "plain_g", ref, enc, gmsd=True)
    lined = _run(tmp_path, "align_g", ref, enc, gmsd=True, align=4)
    for a, b in zip(plain[:2], lined[:2]):
        assert open(a, "rb").read() == open(b, "rb").read()
    doc = json.load(open(lined[2]))
    assert not any(k.startswith("ALIGN") for k in json.load(open(plain[2])))
    for k in A.ALIGN_KEYS:
        del doc[k]
    assert open(plain[2]).read() == json.dumps(doc, indent=1) + "\n"


def test_the_row_of_the_one_pass_entry_point(tmp_path, clip):
    from rtvqa_amd import align as A
    from rtvqa_amd import video_processing as vp
    ref, enc, _index, _want, gain = clip
    ref, enc = _bgr(ref), _bgr(enc)
    cfg = {"crf": 23, "resize_width": 64, "resize_height": 64, "frame_interval": 1, "batch_size": 16}
    plain = vp.process_video_and_extract_metrics(ref, enc, cfg, csv_file=str(tmp_path / "plain.csv"), column_order="fixed")
    lined = vp.process_video_and_extract_metrics(ref, enc, dict(cfg, align=4), csv_file=str(tmp_path / "align.csv"),
                                                 column_order="fixed")
    assert list(lined)[:-5] == list(plain) and list(lined)[-5:] == list(A.ALIGN_KEYS)
    assert all(repr(lined[k]) == repr(plain[k]) for k in plain)   # (repr: a NaN equals a NaN)
    assert [lined[k] for k in A.ALIGN_KEYS[:4]] == [4, 0, 1, 1] and abs(lined["ALIGN_PSNR_GAIN"] - gain) <= 4 * math.ulp(gain)
    rows = list(csv.reader(open(str(tmp_path / "align.csv"))))
    assert rows[0][-5:] == list(A.ALIGN_KEYS) and rows[1][-5:-1] == ["4", "0", "1", "1"]
    head = open(str(tmp_path / "plain.csv")).read().splitlines()[0]
    assert "ALIGN" not in head
