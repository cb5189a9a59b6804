"""GPU: HDR light levels through the reference-shaped entry points - frame_light on a small 10-bit 4:2:0 clip against the
restatement (tests/light_reference.py) and against Engine.light, run_ffmpeg_metrics and process_video_and_extract_metrics with and
without the `light` key, and with `align` and `shift` next to it for the key order."""
import csv
import json
import os

import numpy as np
import pytest

import itp_reference as IR
import light_cases as LC
import light_reference as LR

pytestmark = pytest.mark.gpu

H, W, DEPTH, LAYOUT, FRAMES = 48, 64, 10, "yuv420p10le", 6


@pytest.fixture(scope="module")
def clip():
    from rtvqa_amd import engine as E
    ref, planes = LC.clip("420", H, W, DEPTH, FRAMES, seed=21)
    ref[:, :H * W] = np.clip(ref[:, :H * W], 64, 940)             # legal luma: something is left unclamped in every frame
    enc = ref.copy()
    enc[:, :H * W] = np.clip(enc[:, :H * W].astype(np.int64) + np.random.default_rng(1).integers(-3, 4, (FRAMES, H * W)), 0, 1023)
    T, m709, mp3 = E.light_table("pq"), E.light_gamut("bt709"), E.light_gamut("p3")
    want = LR.records(ref, planes, DEPTH, IR.YUV2020, False, T, m709, mp3)
    return ref, enc, planes, want


def _summary_of(want):
    from rtvqa_amd import light as L
    return L.summarise([r for r, _ in want])


def test_frame_light_against_the_restatement_and_the_engine(engine, clip):
    from rtvqa_amd import light as L
    from rtvqa_amd import video_processing as vp
    ref, _enc, planes, want = clip
    rec, summary = vp.frame_light(ref, LAYOUT, H, W, engine=engine)
    assert rec.tobytes() == engine.light(ref, planes).tobytes()
    for i, (r, _h) in enumerate(want):
        for k in ("sum_q", "sum_y", "max_y", "max_code_rgb", "min_code_rgb", "out_709", "out_p3", "clamped", "max_nits", "avg_nits",
                  "y_avg"):
            assert rec[i][k].item() == r[k], (i, k)
        assert rec[i]["pct_bin"].tolist() == r["pct_bin"] and rec[i]["max_code"].tolist() == r["max_code"]
    assert summary == _summary_of(want) and list(summary) == list(L.LIGHT_KEYS)
    assert summary["LIGHT_MAXFALL"] <= summary["LIGHT_MAXCLL"] <= 10000.0
    for window in (1, 4):                                          # any window size gives the same records
        assert vp.frame_light(ref, LAYOUT, H, W, engine=engine, window=window)[0].tobytes() == rec.tobytes(), window
    dev = engine.upload(ref)
    assert vp.frame_light(dev, LAYOUT, H, W, engine=engine, window=4)[0].tobytes() == rec.tobytes()
    dev._owner.free()
    rec_h, summary_h, hist = vp.frame_light(ref, LAYOUT, H, W, engine=engine, histogram=True, window=4)
    assert rec_h.tobytes() == rec.tobytes() and summary_h == summary and all((hist[i] == h).all() for i, (_r, h) in enumerate(want))
    full = vp.frame_light(ref, LAYOUT, H, W, full_range=True, engine=engine)[0]
    assert full.tobytes() == engine.light(ref, planes, full_range=True).tobytes() != rec.tobytes()


def _run(tmp_path, tag, ref, enc, **kw):
    from rtvqa_amd import video_processing as vp
    logs = [str(tmp_path / ("%s_%s.log" % (k, tag))) for k in ("psnr", "ssim", "vmaf")]
    assert vp.run_ffmpeg_metrics(ref, enc, *logs, layout=LAYOUT, height=H, width=W, **kw) is None
    return logs


def test_run_ffmpeg_metrics_writes_the_keys_and_nothing_else_changes(tmp_path, clip):
    from rtvqa_amd import align as A
    from rtvqa_amd import light as L
    from rtvqa_amd import shift as S
    from rtvqa_amd import video_processing as vp
    ref, enc, _planes, want = clip
    summary = _summary_of(want)
    plain = _run(tmp_path, "plain", ref, enc)
    off = _run(tmp_path, "off", ref, enc, light=False, light_full_range=True)
    lit = _run(tmp_path, "light", ref, enc, light=True)
    for a, b, c in zip(plain[:2], off[:2], lit[:2]):
        assert open(a, "rb").read() == open(b, "rb").read() == open(c, "rb").read()
    assert not os.path.exists(plain[2]) and not os.path.exists(off[2])     # no kind is on: no feature log, as before
    doc = json.load(open(lit[2]))
    assert list(doc) == ["frames", "pooled_metrics"] + list(L.LIGHT_KEYS)
    assert {k: doc[k] for k in L.LIGHT_KEYS} == summary                    # the REFERENCE stream's figures, those of frame_light
    row = vp.extract_metrics_from_logs(*lit, "x", 23, 0, "64x48", 30.0)
    assert list(row)[-8:] == list(L.LIGHT_KEYS) and row["LIGHT_MAXCLL"] == summary["LIGHT_MAXCLL"]
    # next to a kind: the feature log without the key is the log with it minus the eight keys, byte for byte
    plain = _run(tmp_path, "plain_g", ref, enc, gmsd=True)
    lit = _run(tmp_path, "light_g", ref, enc, gmsd=True, light=True)
    for a, b in zip(plain[:2], lit[:2]):
        assert open(a, "rb").read() == open(b, "rb").read()
    doc = json.load(open(lit[2]))
    assert not any(k.startswith("LIGHT") for k in json.load(open(plain[2])))
    for k in L.LIGHT_KEYS:
        del doc[k]
    assert open(plain[2]).read() == json.dumps(doc, indent=1) + "\n"
    # with align and shift on: the LIGHT_* keys stand before the ALIGN_* and SHIFT_* keys, which stay the last
    both = _run(tmp_path, "all", ref, enc, light=True, align=2, shift=4)
    doc = json.load(open(both[2]))
    assert list(doc)[2:] == list(L.LIGHT_KEYS) + list(A.ALIGN_KEYS) + list(S.SHIFT_KEYS)
    assert {k: doc[k] for k in L.LIGHT_KEYS} == summary
    row = vp.extract_metrics_from_logs(*both, "x", 23, 0, "64x48", 30.0)
    assert list(row)[-18:] == list(L.LIGHT_KEYS) + list(A.ALIGN_KEYS) + list(S.SHIFT_KEYS)
    rng = _run(tmp_path, "full", ref, enc, light=True, light_full_range=True)
    assert json.load(open(rng[2]))["LIGHT_MAXFALL"] != summary["LIGHT_MAXFALL"]
    with pytest.raises(ValueError, match="three planes"):
        vp.run_ffmpeg_metrics(ref[:, :H * W], enc[:, :H * W], *plain, layout="gray10le", height=H, width=W, light=True)


def test_the_row_of_the_one_pass_entry_point(tmp_path, clip):
    from rtvqa_amd import align as A
    from rtvqa_amd import light as L
    from rtvqa_amd import shift as S
    from rtvqa_amd import synth
    from rtvqa_amd import video_processing as vp
    ref, enc, _planes, want = clip
    summary = _summary_of(want)
    bgr = synth.s_natural(FRAMES, H, W, seed=12)
    cfg = {"crf": 23, "resize_width": 32, "resize_height": 32, "frame_interval": 1, "batch_size": 4, "pixfmt": LAYOUT}

    def row(name, **more):
        return vp.process_video_and_extract_metrics(ref, enc, dict(cfg, **more), csv_file=str(tmp_path / (name + ".csv")),
                                                    column_order="fixed", encoded_bgr=bgr, height=H, width=W)

    plain, off, lit = row("plain"), row("off", light=False, light_range="full"), row("light", light=True)
    assert open(str(tmp_path / "plain.csv"), "rb").read() == open(str(tmp_path / "off.csv"), "rb").read()
    assert list(off) == list(plain) and list(lit)[:-8] == list(plain) and list(lit)[-8:] == list(L.LIGHT_KEYS)
    assert all(repr(lit[k]) == repr(plain[k]) for k in plain)              # (repr: a NaN equals a NaN)
    assert {k: lit[k] for k in L.LIGHT_KEYS} == summary
    rows = list(csv.reader(open(str(tmp_path / "light.csv"))))
    assert rows[0][-8:] == list(L.LIGHT_KEYS) and float(rows[1][-8]) == summary["LIGHT_MAXCLL"]
    assert "LIGHT" not in open(str(tmp_path / "plain.csv")).read().splitlines()[0]
    both = row("all", light=True, align=2, shift=4)
    assert list(both)[:-18] == list(plain) and list(both)[-18:] == list(L.LIGHT_KEYS) + list(A.ALIGN_KEYS) + list(S.SHIFT_KEYS)
    assert list(csv.reader(open(str(tmp_path / "all.csv"))))[0][-10:] == list(A.ALIGN_KEYS) + list(S.SHIFT_KEYS)
    full = row("full", light=True, light_range="full")
    assert full["LIGHT_MAXFALL"] != summary["LIGHT_MAXFALL"]
