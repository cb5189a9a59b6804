"""GPU: colour registration through the reference-shaped entry points - frame_colorfit, run_ffmpeg_metrics and
process_video_and_extract_metrics with and without the `colorfit` key.  All cases use yuv420p at 104 x 72: three frames of the
project's synthetic clip and the same frames with the limited-to-full range map applied, rounded and clipped.  Records and tables
are compared for equality with the restatement (tests/colorfit_reference.py); files are compared byte for byte."""
import csv
import json
import logging
import math
import os

import numpy as np
import pytest

import colorfit_reference as CR

pytestmark = pytest.mark.gpu

H, W = 72, 104
KW = dict(layout="yuv420p", height=H, width=W)
PLANES = [(W, H, 0, W, 1), (W // 2, H // 2, W * H, W // 2, 1), (W // 2, H // 2, W * H + (W // 2) * (H // 2), W // 2, 1)]


@pytest.fixture(scope="module")
def clip():
    """(ref, the limited-to-full copy): d_Y = (r_Y - 16) 255 / 219, d_C = (r_C - 128) 255 / 224 + 128, rounded, clipped"""
    from rtvqa_amd import frames, synth
    ref = frames.bgr_to_yuv420p(synth.s_natural(3, H, W))
    x = ref.astype(np.float64)
    hurt = np.concatenate([(x[:, :H * W] - 16.0) * 255.0 / 219.0, (x[:, H * W:] - 128.0) * 255.0 / 224.0 + 128.0], axis=1)
    return ref, np.clip(np.rint(hurt), 0, 255).astype(np.uint8)


def test_frame_colorfit_names_the_mishap_in_any_window(engine, clip):
    from rtvqa_amd import colorfit as CF
    from rtvqa_amd import video_processing as vp
    ref, hurt = clip
    rec, tab, res = vp.frame_colorfit(ref, hurt, engine=engine, **KW)
    want = CR.records(ref, hurt, PLANES)
    for i, r in enumerate(want):
        for k in CR.FIELDS:
            g = rec[i][k]
            assert (g.tolist() if isinstance(g, np.ndarray) else g.item()) == r[k], (i, k)
    assert (tab.astype(np.int64) == CR.tables(ref, hurt, PLANES, 8)).all()
    assert res["match"] == "limited_to_full" and res["per_frame"] == ["limited_to_full"] * 3 and res["frames_off"] == 0
    assert res["match_psnr_gain"] > 10.0 * math.log10(2.0) and res["psnr_gain"] >= res["match_psnr_gain"]
    again = CF.analyse(want, 8, "yuv", CR.tables(ref, hurt, PLANES, 8).tolist())      # the same analysis off the restatement's words
    assert {k: again[k] for k in again if k != "curve"} == {k: res[k] for k in res if k != "curve"}
    for window in (1, 2, 1024):   # any window gives the same records and tables
        r2, t2, res2 = vp.frame_colorfit(ref, hurt, engine=engine, window=window, **KW)
        assert r2.tobytes() == rec.tobytes() and t2.tobytes() == tab.tobytes() and res2["match"] == res["match"], window
    r3, t3, res3 = vp.frame_colorfit(engine.upload(ref), engine.upload(hurt), engine=engine, window=2, **KW)
    assert r3.tobytes() == rec.tobytes() and t3.tobytes() == tab.tobytes()
    r4, t4, res4 = vp.frame_colorfit(ref, hurt, tables=False, engine=engine, **KW)
    assert r4.tobytes() == rec.tobytes() and t4 is None and "tone_psnr_gain" not in res4 and res4["match"] == res["match"]
    with pytest.raises(ValueError, match="window"):
        vp.frame_colorfit(ref, hurt, engine=engine, window=0, **KW)


def _run(tmp_path, tag, ref, enc, **kw):
    from rtvqa_amd import video_processing as vp
    logs = [str(tmp_path / ("%s_%s.log" % (k, tag))) for k in ("psnr", "ssim", "vmaf")]
    assert vp.run_ffmpeg_metrics(ref, enc, *logs, **dict(KW, **kw)) is None
    return logs


def _same_files(a, b, upto=2):
    for x, y in zip(a[:upto], b[:upto]):
        assert open(x, "rb").read() == open(y, "rb").read()


def test_the_keys_of_the_log_and_their_place(engine, tmp_path, clip, caplog):
    from rtvqa_amd import align as A
    from rtvqa_amd import colorfit as CF
    from rtvqa_amd import sync as S
    from rtvqa_amd import video_processing as vp
    ref, hurt = clip
    plain = _run(tmp_path, "plain", ref, hurt)
    off = _run(tmp_path, "off", ref, hurt, colorfit=False)
    _same_files(plain, off)                                         # colorfit=False: the files written without the keyword
    assert not os.path.exists(plain[2]) and not os.path.exists(off[2])
    with caplog.at_level(logging.WARNING):
        fit = _run(tmp_path, "fit", ref, hurt, colorfit=True)
    said = [r.getMessage() for r in caplog.records if "NOT corrected" in r.getMessage()]
    assert len(said) == 1 and "limited_to_full" in said[0]
    _same_files(plain, fit)                                         # nothing is corrected: the stats files are what they were
    doc = json.load(open(fit[2]))
    assert list(doc)[-7:] == list(CF.COLORFIT_KEYS)
    want = CF.log_keys(vp.frame_colorfit(ref, hurt, engine=engine, **KW)[2], 8)
    assert {k: doc[k] for k in CF.COLORFIT_KEYS} == want and doc["COLORFIT_MATCH"] == "limited_to_full"
    assert doc["COLORFIT_FRAMES_OFF"] == 0 and abs(doc["COLORFIT_GAIN_Y"] - 255.0 / 219.0) < 0.02
    # next to a kind, sync and align: after the SYNC_* and before the ALIGN_* keys; the log differs by the seven keys only
    both = dict(gmsd=True, sync=True, align=1)
    was = _run(tmp_path, "was", ref, hurt, **both)
    now = _run(tmp_path, "now", ref, hurt, colorfit=True, **both)
    _same_files(was, now)
    doc = json.load(open(now[2]))
    names = list(doc)
    assert names[-5:] == list(A.ALIGN_KEYS) and names[-12:-5] == list(CF.COLORFIT_KEYS) and names[-18:-12] == list(S.SYNC_KEYS)
    assert {k: doc[k] for k in CF.COLORFIT_KEYS} == want
    for k in CF.COLORFIT_KEYS:
        del doc[k]
    assert open(was[2]).read() == json.dumps(doc, indent=1) + "\n"
    off = _run(tmp_path, "off2", ref, hurt, colorfit=False, **both)
    _same_files(was, off, upto=3)
    # an untouched pair says "none" and warns of nothing
    caplog.clear()
    with caplog.at_level(logging.WARNING):
        same = _run(tmp_path, "same", ref, ref.copy(), colorfit=True)
    assert not [r for r in caplog.records if "NOT corrected" in r.getMessage()]
    doc = json.load(open(same[2]))
    assert doc["COLORFIT_MATCH"] == "none" and doc["COLORFIT_PSNR_GAIN"] == 0.0 and doc["COLORFIT_TONE_PSNR_GAIN"] == 0.0


def test_the_refusals_of_the_entry_point(tmp_path, clip):
    ref, hurt = clip
    with pytest.raises(ValueError, match="colorfit and scale"):
        _run(tmp_path, "scale", ref, hurt, colorfit=True, scale="bicubic", dist_height=H, dist_width=W)
    with pytest.raises(ValueError, match="colorfit must be true or false"):
        _run(tmp_path, "int", ref, hurt, colorfit=1)


def test_the_row_of_the_one_pass_entry_point(tmp_path, clip):
    from rtvqa_amd import colorfit as CF
    from rtvqa_amd import shift as SH
    from rtvqa_amd import synth
    from rtvqa_amd import video_processing as vp
    ref, hurt = clip
    cfg = {"crf": 23, "resize_width": 64, "resize_height": 64, "frame_interval": 1, "batch_size": 16, "pixfmt": "yuv420p",
           "height": H, "width": W}
    bgr = synth.s_natural(3, H, W)
    plain = vp.process_video_and_extract_metrics(ref, hurt, cfg, csv_file=str(tmp_path / "plain.csv"), column_order="fixed",
                                                 encoded_bgr=bgr)
    off = vp.process_video_and_extract_metrics(ref, hurt, dict(cfg, colorfit=False), csv_file=str(tmp_path / "off.csv"),
                                               column_order="fixed", encoded_bgr=bgr)
    assert list(off) == list(plain) and all(repr(off[k]) == repr(plain[k]) for k in plain)
    assert open(str(tmp_path / "plain.csv"), "rb").read() == open(str(tmp_path / "off.csv"), "rb").read()
    fit = vp.process_video_and_extract_metrics(ref, hurt, dict(cfg, colorfit=True, shift=1), csv_file=str(tmp_path / "fit.csv"),
                                               column_order="fixed", encoded_bgr=bgr)
    assert list(fit)[-5:] == list(SH.SHIFT_KEYS) and list(fit)[-12:-5] == list(CF.COLORFIT_KEYS)
    assert [k for k in fit if k not in CF.COLORFIT_KEYS and k not in SH.SHIFT_KEYS] == list(plain)
    assert all(repr(fit[k]) == repr(plain[k]) for k in plain)   # (repr: a NaN equals a NaN)
    assert fit["COLORFIT_MATCH"] == "limited_to_full" and fit["COLORFIT_FRAMES_OFF"] == 0
    rows = list(csv.reader(open(str(tmp_path / "fit.csv"))))
    assert rows[0][-12:-5] == list(CF.COLORFIT_KEYS) and rows[1][-12] == "limited_to_full"
