"""CPU: the signal statistics' NumPy restatement against hand-computed answers, events.signal_events, the additive ABI and the
log / row / config key - no GPU.  The device is held to the same restatement and the same hand cases in test_gpu_sigstats.py."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import sigstats_cases as SC
import sigstats_reference as R
from rtvqa_amd import _native as N
from rtvqa_amd import events, stream
from rtvqa_amd import video_processing as vp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOOD = {"crf": 23, "resize_width": 64, "resize_height": 64, "frame_interval": 1}


def hand_cases():
    """(name, samples [h, w], depth, levels or None, the words that are known by hand) - shared with the device's test"""
    h, w = 20, 26                                   # N = 520: the three ranks are 52, 260 and 468
    n = h * w
    out = []
    for name, k in zip(("low", "median", "high"), R.ranks(n)):
        out.append(("%s: exactly k samples of a" % name, SC.two_level(h, w, k, 50, 180), 8, None, {name: 50}))
        out.append(("%s: one sample fewer" % name, SC.two_level(h, w, k - 1, 50, 180), 8, None, {name: 180}))
    out.append(("flat", np.full((h, w), 93), 8, None,
                dict(min=93, low=93, median=93, high=93, max=93, or_mask=93, and_mask=93, sum=93 * n, sum_sq=93 * 93 * n)))
    x = 4 * np.random.default_rng(3).integers(0, 256, (h, w))
    out.append(("multiples of 4 at 10 bits", x, 10, None, dict(bits_used=8, above_peak=0)))
    out.append(("all zero", np.zeros((h, w), np.int64), 10, None, dict(bits_used=0, or_mask=0, and_mask=0, top=h, bottom=-1)))
    # crop_level 30: row 5 sums to exactly 30 w (dark), row 6 to one more (not dark); the columns likewise
    x = np.full((h, w), 30)
    x[6, 0] = 31
    out.append(("a row one above the limit", x, 8, (None, 30), dict(top=6, bottom=6, left=0, right=0)))
    out.append(("every row at the limit", np.full((h, w), 30), 8, (None, 30), dict(top=h, bottom=-1, left=w, right=-1)))
    x = np.zeros((h, w), np.int64)
    x[::2, ::2] = 65535
    out.append(("0 and 65535 together", x, 16, None,
                dict(min=0, max=65535, or_mask=65535, and_mask=0, bits_used=16, low=0, median=0, high=65535, sum=65535 * 130,
                     sum_sq=65535 * 65535 * 130, over_luma=130, under=390, above_peak=0)))
    x = np.full((h, w), 1023)
    x[3, 4] = 1024
    out.append(("one sample above the 10-bit peak", x, 10, None, dict(above_peak=1, max=1024, bits_used=10)))
    return out


@pytest.mark.parametrize("case", hand_cases(), ids=[c[0] for c in hand_cases()])
def test_the_restatement_against_hand_answers(case):
    _name, x, depth, levels, known = case
    black, crop = levels or (None, None)
    r = R.record(x, depth, None, black, crop)
    assert {k: r[k] for k in known} == known
    assert r["count"] == x.size and r["sad"] == 0 and r["changed"] == 0


def test_the_restatement_counts_sad_and_the_box():
    rng = np.random.default_rng(1)
    a = rng.integers(0, 256, (17, 23))
    b = a.copy()
    b[2, 3] += 5 if b[2, 3] < 250 else -5
    b[9, 9] -= 2 if b[9, 9] > 1 else -2
    r = R.record(b, 8, a)
    assert r["sad"] == 7 and r["changed"] == 2
    x, want = SC.boxed(rng, 30, 40, 8, 24)
    assert R.box(x, 24) == want == (3, 27, 2, 36)
    assert R.box(x, 23)[0] == 0                     # one below the bars' level: nothing is dark
    assert R.doubles(dict(count=4, sum=10, sum_sq=30, sad=6)) == (2.5, np.sqrt(30 / 4 - 6.25), 1.5)


# ---- events ---------------------------------------------------------------------------------------------------------------------
def _records(plane, depth=8):
    from rtvqa_amd.engine import SIGSTATS_DTYPE
    want = R.series(plane, depth)
    rec = np.zeros(len(want), SIGSTATS_DTYPE)
    for i, r in enumerate(want):
        for k in R.INT_FIELDS:
            rec[i][k] = r[k]
        rec[i]["mean"], rec[i]["stdev"], rec[i]["dif"] = R.doubles(r)
    return rec


def test_signal_events_on_the_qc_clip():
    plane, want_box = SC.qc_clip()
    rec = _records(plane)
    ev = events.signal_events(rec, 8)
    assert ev["black"].tolist() == [False, False, True, False, False, False, False]
    assert ev["frozen"].tolist() == [False, False, False, False, True, False, False]
    assert ev["black_runs"] == [(2, 2)] and ev["frozen_runs"] == [(4, 4)]
    assert ev["cuts"] == [2, 5]          # into the black frame, and between the two shots; not out of the black frame
    assert ev["crop"] == want_box
    n = plane[0].size
    assert ev["mafd"][0] == 0.0 and ev["scene_score"][0] == 0.0            # the frame-0 rules
    assert ev["mafd"][1] == 100.0 * 2400 / (n * 256) and ev["mafd"][4] == 0.0
    assert ev["scene_score"][5] == min(ev["mafd"][5], abs(ev["mafd"][5] - ev["mafd"][4])) > 10.0
    assert ev["scene_score"][3] < 1.0 and ev["mafd"][3] > 10.0     # out of the black frame: as far as into it
    # the same from [n, p] records: plane 0's are used
    two = np.stack([rec, rec[::-1]], axis=1)
    again = events.signal_events(two, 8)
    assert again["cuts"] == ev["cuts"] and again["crop"] == ev["crop"]


def test_signal_events_thresholds_runs_and_the_frame_0_rules():
    h, w = 16, 16
    n = h * w
    base = np.full((h, w), 100)
    # freeze_noise chosen so that freeze_noise N (2^d - 1) = 40.8: a sad of 40 is frozen, 41 is not
    rec = _records(np.stack([base, base, base, base]))
    rec["sad"] = [0, 40, 41, 0]
    ev = events.signal_events(rec, 8, freeze_noise=40.8 / (n * 255))
    assert ev["frozen"].tolist() == [False, True, False, True]              # frame 0 has no predecessor: never frozen
    assert events.signal_events(rec, 8, freeze_noise=40.8 / (n * 255), first_has_prev=True)["frozen"][0]
    assert ev["frozen_runs"] == [(1, 1), (3, 3)]
    assert events.signal_events(rec, 8, freeze_noise=40.8 / (n * 255), min_run=2)["frozen_runs"] == []
    rec["sad"] = [0, 0, 0, 900]
    ev = events.signal_events(rec, 8, min_run=2)
    assert ev["frozen_runs"] == [(1, 2)] and events.signal_events(rec, 8, min_run=3)["frozen_runs"] == []
    # black_share: 0.5 N = 128 dark samples is black, 127 is not
    rec["below_black"] = [128, 127, 256, 256]
    ev = events.signal_events(rec, 8, black_share=0.5)
    assert ev["black"].tolist() == [True, False, True, True] and ev["black_runs"] == [(0, 0), (2, 3)]
    assert events.signal_events(rec, 8, black_share=0.5, min_run=2)["black_runs"] == [(2, 3)]
    # a cut between two static shots: mafd = 0, 0, big, 0 -> the score marks the first frame of the new shot alone
    rec["sad"] = [0, 0, n * 64, 0]
    ev = events.signal_events(rec, 8)
    assert ev["mafd"].tolist() == [0.0, 0.0, 25.0, 0.0] and ev["scene_score"].tolist() == [0.0, 0.0, 25.0, 0.0] and ev["cuts"] == [2]
    assert events.signal_events(rec, 8, scene_threshold=25.0)["cuts"] == [2]
    assert events.signal_events(rec, 8, scene_threshold=25.5)["cuts"] == []
    # frame 0's sad (a prev0 the caller gave) counts only when the caller says so, and frame 0 is never a cut
    rec["sad"] = [n * 64, 0, 0, 0]
    assert events.signal_events(rec, 8)["mafd"][0] == 0.0
    ev = events.signal_events(rec, 8, first_has_prev=True)
    assert ev["mafd"][0] == 25.0 and ev["scene_score"][0] == 0.0 and ev["cuts"] == []
    # crop over a clip with black frames: the union of the others; all black: None
    rec["below_black"] = [256, 0, 0, 256]
    rec["top"], rec["bottom"], rec["left"], rec["right"] = [16, 2, 4, 0], [-1, 12, 10, 15], [16, 3, 1, 0], [-1, 9, 13, 15]
    assert events.signal_events(rec, 8)["crop"] == (2, 12, 1, 13)
    rec["below_black"] = 256
    ev = events.signal_events(rec, 8)
    assert ev["crop"] is None and ev["black_runs"] == [(0, 3)]
    empty = events.signal_events(rec[:0], 8)
    assert empty["cuts"] == [] and empty["crop"] is None and empty["black"].shape == (0,)


# ---- ABI -------------------------------------------------------------------------------------------------------------------------
def test_the_additive_abi():
    assert N.VQA_ABI_VERSION == 8
    assert C.sizeof(N.VqaSigstatsMetrics) == R.SIZE == 152
    assert tuple(getattr(N.VqaSigstatsMetrics, f).offset for f in R.FIELDS) == R.OFFSETS
    from rtvqa_amd.engine import SIGSTATS_DTYPE
    assert SIGSTATS_DTYPE.itemsize == 152 and SIGSTATS_DTYPE.names == R.FIELDS
    assert tuple(SIGSTATS_DTYPE.fields[f][1] for f in R.FIELDS) == R.OFFSETS
    assert (N.K_SIGSTATS_ACCUM, N.K_SIGSTATS_SCAN, N.K_FRINGE) == (63, 64, 65) and N.K_HEM == 62
    assert N.K_IDS_COMPLETE == N.K_IDS_ENTIRE + (63, 64) and 62 not in N.K_IDS_COMPLETE and 65 not in N.K_IDS_COMPLETE
    txt = open(os.path.join(REPO, "include", "vqa.h")).read()
    for name, val in (("VQA_K_SIGSTATS_ACCUM", 63), ("VQA_K_SIGSTATS_SCAN", 64), ("VQA_K_FRINGE", 65), ("VQA_K_HEM", 62)):
        assert re.search(r"%s\s*=\s*%d\b" % (name, val), txt), name
    assert re.search(r"#define VQA_ABI_VERSION\s+8", txt)
    part = txt[txt.index("---- Signal statistics"):]
    part = part[:part.index("VQA_API int vqa_sigstats_wait")]
    for word in ("(N + 9) / 10", "(N + 1) / 2", "(9 N + 9) / 10", "32 s", "24 s", "16 s", "235 s", "240 s", "ctz(or_mask)",
                 "top = h, bottom = -1", "2^28", "2^26", "65535", "overflow", "16-bit counter", "256 MiB", "at least 16 x 16",
                 "no floating point", "Not built"):
        assert word in part, word
    lib = N.load()
    assert lib.vqa_abi_version() == 8
    lib.vqa_kernel_name.restype = C.c_char_p
    assert [lib.vqa_kernel_name(i) for i in (63, 64)] == [b"k_sigstats_accum", b"k_sigstats_scan"]
    assert lib.vqa_kernel_name(62) == b"?" and lib.vqa_kernel_name(65) == b"?" and lib.vqa_kernel_name(61) == b"k_fsim_pool"
    assert lib.vqa_profile_read(None, 63, None, None, 0) == N.VQA_ERR_INVALID
    assert lib.vqa_sigstats_submit(None, None, None, 0, 0, 0, None, 0, -1, -1) == N.VQA_ERR_INVALID
    assert lib.vqa_sigstats_wait(None, None, 0, 0, None, 0) == N.VQA_ERR_INVALID
    for path in (N.LIB_PATH, N.LAB_LIB_PATH):
        assert hasattr(C.CDLL(path), "vqa_sigstats_submit") and hasattr(C.CDLL(path), "vqa_sigstats_wait")


def test_the_header_to_the_c_compiler(tmp_path):
    names = ", ".join("offsetof(vqa_sigstats_metrics, %s)" % f for f in R.FIELDS)
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "vqa.h"\n'
           'int (*submit)(vqa_ctx *, const uint8_t *, const uint8_t *, int, int, int64_t, const vqa_plane_desc *, int, int, int) '
           '= vqa_sigstats_submit;\n'
           'int (*wait_)(vqa_ctx *, vqa_sigstats_metrics *, int, int, uint64_t *, int64_t) = vqa_sigstats_wait;\n'
           'int main(void){size_t o[] = {' + names + '}; unsigned i;\n'
           'printf("%zu %d %d %d %d %d %d", sizeof(vqa_sigstats_metrics), VQA_K_SIGSTATS_ACCUM, VQA_K_SIGSTATS_SCAN, VQA_K_FRINGE, '
           'VQA_K_HEM, VQA_ABI_VERSION, vqa_abi_version());\n'
           'for (i = 0; i < sizeof o / sizeof o[0]; i++) printf(" %zu", o[i]);\n'
           'printf("\\n"); return submit == 0 || wait_ == 0;}\n')
    (tmp_path / "s.c").write_text(src)
    lib_dir = os.path.dirname(N.LIB_PATH)
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), "-o", str(tmp_path / "s"), str(tmp_path / "s.c"),
                           "-L", lib_dir, "-l:" + os.path.basename(N.LIB_PATH), "-Wl,-rpath," + lib_dir,
                           "-Wl,--allow-shlib-undefined"])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "s")]).decode().split()]
    assert got == [152, 63, 64, 65, 62, 8, 8] + list(R.OFFSETS)


# ---- the Python layers -----------------------------------------------------------------------------------------------------------
def test_the_json_log_and_what_the_row_takes_from_it(tmp_path):
    from rtvqa_amd.engine import FSIM_DTYPE
    plane, want_box = SC.qc_clip()
    rec = _records(plane)
    fs = np.zeros(len(rec), FSIM_DTYPE)
    fs["fsim"], fs["fsimc"] = 0.5, 0.25
    old, log, only = str(tmp_path / "old.json"), str(tmp_path / "vmaf.json"), str(tmp_path / "sig.json")
    vp.write_vif_log(old, fsim=fs)
    vp.write_vif_log(log, fsim=fs, sigstats=rec)
    doc0, doc = json.load(open(old)), json.load(open(log))
    assert "y_low" not in json.dumps(doc0) and "signal" not in doc0
    names0 = list(doc0["frames"][0]["metrics"])
    assert names0[-1] == "fsimc"
    keys = ["y_min", "y_low", "y_avg", "y_high", "y_max", "y_dif", "out_of_range", "black", "frozen", "scene_score"]
    assert list(doc["frames"][1]["metrics"]) == names0 + keys == list(doc["pooled_metrics"])
    assert list(doc) == ["frames", "pooled_metrics", "signal"]
    ev = events.signal_events(rec, 8)
    for i, f in enumerate(doc["frames"]):
        m = f["metrics"]
        assert [m[k] for k in keys[:6]] == [float(rec[i][k]) for k in ("min", "low", "mean", "high", "max", "dif")]
        assert m["out_of_range"] == (int(rec[i]["under"]) + int(rec[i]["over_luma"])) / plane[0].size
        assert (m["black"], m["frozen"]) == (float(ev["black"][i]), float(ev["frozen"][i])) and m["scene_score"] == ev["scene_score"][i]
    assert doc["signal"] == {"black_frames": 1, "frozen_frames": 1, "scene_cuts": 2, "crop": list(want_box)}
    assert {k: doc["pooled_metrics"][k] for k in names0} == doc0["pooled_metrics"]
    vp.write_vif_log(only, sigstats=rec)
    assert list(json.load(open(only))["frames"][0]["metrics"]) == keys
    pl, sl = tmp_path / "psnr.log", tmp_path / "ssim.log"
    pl.write_text("n:1 mse_avg:1.00 psnr_avg:48.13 \n")
    sl.write_text("n:1 Y:0.990000 All:0.990000 (20.000000)\n")
    m0 = vp.extract_metrics_from_logs(str(pl), str(sl), old, "x", 23, 1000, "64x64", 30.0)
    m = vp.extract_metrics_from_logs(str(pl), str(sl), log, "x", 23, 1000, "64x64", 30.0)
    cols = ["Y_LOW", "Y_HIGH", "OUT_OF_RANGE", "BLACK_FRAMES", "FROZEN_FRAMES", "SCENE_CUTS", "CROP_TOP", "CROP_BOTTOM", "CROP_LEFT",
            "CROP_RIGHT"]
    assert list(m0)[-1] == "FSIMC" and list(m) == list(m0) + cols
    assert {k: m[k] for k in m0} == m0
    assert m["Y_LOW"] == float(rec["low"].min()) == 16.0 and m["Y_HIGH"] == float(rec["high"].max())
    assert m["OUT_OF_RANGE"] == float(np.mean((rec["under"].astype(np.float64) + rec["over_luma"]) / plane[0].size))
    assert [m[k] for k in cols[3:]] == [1, 1, 2] + list(want_box)
    # all frames black: the crop columns are -1
    dark = _records(np.full((3, 16, 16), 16))
    vp.write_vif_log(only, sigstats=dark)
    assert json.load(open(only))["signal"]["crop"] is None
    m = vp.extract_metrics_from_logs(str(pl), str(sl), only, "x", 23, 1000, "64x64", 30.0)
    assert [m[k] for k in cols[3:]] == [3, 2, 0, -1, -1, -1, -1]
    # a 10-bit stream: the events use the depth
    rec10 = _records(plane * 4, 10)
    vp.write_vif_log(only, sigstats=rec10, sigstats_depth=10)
    assert json.load(open(only))["signal"] == doc["signal"]
    # logs without the key are what they were, byte for byte
    again = str(tmp_path / "again.json")
    vp.write_vif_log(again, fsim=fs, sigstats=None)
    assert open(again, "rb").read() == open(old, "rb").read()
    # the pass's tuple -> the log: the last element is the kind's [n, p], FSIM's [n] the one before it
    q = (None, None, fs, np.stack([rec, rec], axis=1))
    vp._write_feature_log(again, q, dict(vif=False, adm=False, fsim=True, sigstats=True))
    assert open(again, "rb").read() == open(log, "rb").read()
    vp._write_feature_log(again, q[:-1], dict(vif=False, adm=False, fsim=True))
    assert open(again, "rb").read() == open(old, "rb").read()


def test_the_config_keys():
    vp.validate_config(dict(GOOD))
    vp.validate_config(dict(GOOD, sigstats=True))
    vp.validate_config(dict(GOOD, sigstats=False, sigstats_black=0, sigstats_crop=65535))
    vp.validate_config(dict(GOOD, sigstats=True, sigstats_black=None, sigstats_crop=None))
    for bad in (1, 0, "true", None, "only"):
        with pytest.raises(ValueError) as e:
            vp.validate_config(dict(GOOD, sigstats=bad))
        assert str(e.value) == "sigstats must be true or false."
    for key in ("sigstats_black", "sigstats_crop"):
        for bad in (-1, 65536, 1.5, "32", True):
            with pytest.raises(ValueError) as e:
                vp.validate_config(dict(GOOD, **{key: bad}))           # (validated whether the kind is on or not)
            assert str(e.value) == "%s must be null or an integer from 0 to 65535." % key


def test_the_stream_request():
    p = [(16, 16, 0, 16, 1), (8, 8, 256, 8, 1), (8, 8, 320, 8, 1)]
    assert stream.PLANE_KINDS[-1].name == "sigstats" and stream.PLANE_KINDS[-1].reads == "ref" and stream.PLANE_KINDS[-1].halo
    assert [k for k, _ in stream.PLANE_KINDS[-1].params] == ["sigstats_black", "sigstats_crop"]
    q = stream.Quality(p)
    assert q.sigstats is False and q.sigstats_black is None and q.sigstats_crop is None
    q = stream.Quality(p, sigstats=True, sigstats_black=40, sigstats_crop=0)
    assert q.sigstats is True and q.ssim is True and (q.sigstats_black, q.sigstats_crop) == (40, 0)
    assert stream.Quality(p[:2], sigstats="only").ssim is False                   # any number of planes
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="sigstats must be False, True or 'only'"):
            stream.Quality(p, sigstats=bad)
    for key in ("sigstats_black", "sigstats_crop"):
        for bad in (-1, 65536, 2.0, "1", True):
            with pytest.raises(ValueError, match=key):
                stream.Quality(p, **{key: bad})                                   # off: still validated
    z = np.zeros((0, 384), np.uint8)
    for kw, length in ((dict(), 2), (dict(vif=True), 3), (dict(fsim=True), 3)):
        q0, _ = stream.run(z, z, quality=stream.Quality(p, **kw))
        q1, _ = stream.run(z, z, quality=stream.Quality(p, sigstats=True, **kw))
        assert len(q0) == length and len(q1) == length + 1, kw
        assert q1[-1].shape == (0, 3) and q1[-1].dtype.names == R.FIELDS
        for a, b in zip(q0, q1):
            assert (a is None and b is None) or (a.dtype == b.dtype and a.shape == b.shape)
