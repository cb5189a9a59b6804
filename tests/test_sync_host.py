"""Host: clip-wide sync without a GPU - the restatement against hand answers, sync.py's rules on the issue's scenarios (through the
restatement's diag and best) and on hand-made words, the key order of the log, the request and config checks, the additive ABI
(header text, kernel ids, exported symbols, NULL ctx) and the header under a C compiler."""
import ctypes as C
import json
import logging
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import sync_cases as SC
import sync_reference as R
from rtvqa_amd import _native as N
from rtvqa_amd import sync as S
from rtvqa_amd import video_processing as vp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def test_the_restatement_against_hand_answers():
    x = np.arange(256, dtype=np.uint8).reshape(1, 16, 16)
    assert R.signatures(x).tolist() == [list(range(256))]                      # one-sample cells: the samples
    x10 = (np.arange(256, dtype=np.uint16) * 4 + 3).reshape(1, 16, 16)
    assert R.signatures(x10, 10).tolist() == [list(range(256))]                # 10 bits: x >> 2
    assert (R.signatures(np.full((1, 16, 16), 65535, np.uint16), 10) == 255).all()   # above the peak: the min clamps
    # 17 rows: cell row 15 is rows 15 and 16 (floor(15 * 17 / 16) = 15 .. floor(16 * 17 / 16) - 1 = 16), the others one row
    y = np.zeros((1, 17, 16), np.uint8)
    y[0, 15], y[0, 16] = 10, 21
    sig = R.signatures(y)[0].reshape(16, 16)
    assert (sig[15] == 15).all() and (sig[:15] == 0).all()                     # floor(31 / 2)
    # 37 x 19: the first cell is rows 0 .. 1 (floor(37 / 16) = 2) and column 0 (floor(19 / 16) = 1)
    z = SC.clip(1, 37, 19, 8, 1)
    assert R.signatures(z)[0, 0] == (int(z[0, 0, 0]) + int(z[0, 1, 0])) // 2
    assert R.signatures(z)[0, 255] == int(z[0, 34:37, 17:19].astype(np.int64).sum()) // 6
    d = np.zeros((2, 256), np.uint8)
    r = np.zeros((3, 256), np.uint8)
    d[0, 0], d[1, 5], r[1, 0], r[2, 5] = 3, 4, 3, 6
    assert R.distances(d, r).tolist() == [[9, 0, 45], [16, 25, 4]]
    diag, best = R.cross(d, r)
    #                        k = -1  k = 0   k = 1  k = 2
    assert diag.tolist() == [16, 9 + 25, 0 + 4, 45]
    assert best.tolist() == [(0 << 32) | 1, (4 << 32) | 2]
    assert [a.tolist() for a in R.cross_fast(d, r)] == [diag.tolist(), best.tolist()]
    zero, full = np.zeros((1, 256), np.uint8), np.full((2, 256), 255, np.uint8)
    diag, best = R.cross(zero, full)
    assert diag.tolist() == [16646400, 16646400] and best.tolist() == [16646400 << 32]   # the tie: the smaller index


# ---- sync.py on the scenarios -------------------------------------------------------------------------------------------------------
def _analyse(ref, dist, **kw):
    rs, ds = R.signatures(ref), R.signatures(dist)
    diag, best = R.cross_fast(ds, rs)
    return S.analyse(diag, best, len(ds), len(rs), **kw), diag


def test_a_start_37_frames_late_in_a_panning_clip():
    ref, dist = SC.late_start()
    assert ref.shape == (300, 270, 480) and dist.shape == (200, 270, 480)
    res, _diag = _analyse(ref, dist)
    assert res["offset"] == 37 and res["frames_off"] == 0 and res["overlap"] == 200 and not res["ambiguous"]
    assert res["per_frame"] == [37] * 200 and res["runs"] == [(0, 200, 37)] and res["trim"] == (37, 0, 200)
    assert res["runner_up"] is not None and abs(res["runner_up"][0] - 37) > 2 and res["runner_up"][1] > 16 * res["mean"]
    keys = S.log_keys(res, True)
    assert keys["SYNC_DISTANCE"] == float(res["mean"] / 256) < 1.0 and keys["SYNC_APPLIED"] == 1


def test_an_excerpt_of_unrelated_frames_under_min_overlap():
    ref, dist = SC.excerpt()
    assert ref.shape == (24, 19, 37) and dist.shape == (12, 19, 37)
    res, _diag = _analyse(ref, dist, min_overlap=6)
    assert res["offset"] == 5 and res["mean"] == 0 and res["frames_off"] == 0 and res["trim"] == (5, 0, 12)
    assert not res["ambiguous"] and res["runner_up"][1] > 0


def test_a_negative_offset():
    ref, dist = SC.excerpt()
    res, _diag = _analyse(dist, ref, min_overlap=6)   # the streams swapped: the long one is the distorted
    assert res["offset"] == -5 and res["overlap"] == 12 and res["trim"] == (0, 5, 12)
    assert res["per_frame"][5:17] == [-5] * 12 and res["frames_off"] == 12   # the 12 frames outside the excerpt pair somewhere


def test_a_static_clip_is_ambiguous_and_offset_0_by_the_tie_rule():
    one = SC.clip(1, 19, 37, 8, 3)
    ref, dist = np.repeat(one, 10, axis=0), np.repeat(one, 6, axis=0)
    res, diag = _analyse(ref, dist)
    assert (diag == 0).all()
    assert res["offset"] == 0 and res["ambiguous"] and res["mean"] == 0 and res["runner_up"] == (-3, 0)   # (|k|, k) beyond the guard
    assert res["per_frame"] == [-j for j in range(6)]   # every frame's best is reference frame 0, the smallest index
    assert S.log_keys(res, False)["SYNC_RUNNER_UP"] == 0.0


# ---- sync.py on hand-made words ------------------------------------------------------------------------------------------------------
def _best(index, dist=0):
    return [(dist << 32) | i for i in index]


def test_overlap_and_trim_at_the_ends():
    assert [S.overlap(k, 3, 5) for k in range(-3, 6)] == [0, 1, 2, 3, 3, 3, 2, 1, 0]
    assert [S.overlap(k, 5, 3) for k in range(-5, 4)] == [0, 1, 2, 3, 3, 3, 2, 1, 0]
    assert S.overlap(0, 1, 1) == 1 and S.overlap(1, 1, 1) == 0 and S.overlap(-10 ** 9, 4, 4) == 0
    # n_dist = 3, n_ref = 5: k = -2 .. 4; the last diagonal is the best and legal under min_overlap = 1
    res = S.analyse([9, 9, 9, 9, 9, 9, 0], _best([4, 4, 4]), 3, 5, min_overlap=1)
    assert res["offset"] == 4 and res["overlap"] == 1 and res["trim"] == (4, 0, 1)
    res = S.analyse([0, 9, 9, 9, 9, 9, 9], _best([0, 0, 0]), 3, 5, min_overlap=1)
    assert res["offset"] == -2 and res["overlap"] == 1 and res["trim"] == (0, 2, 1)
    assert res["per_frame"] == [0, -1, -2] and res["frames_off"] == 2


def test_the_tie_order_is_abs_k_then_k():
    # n_dist = n_ref = 3: k = -2 .. 2, overlaps 1, 2, 3, 2, 1
    assert S.analyse([5, 10, 15, 10, 5], _best([0, 1, 2]), 3, 3, min_overlap=1)["offset"] == 0      # all means 5
    assert S.analyse([5, 8, 15, 8, 5], _best([0, 1, 2]), 3, 3, min_overlap=1)["offset"] == -1       # 4 = 4: the negative
    assert S.analyse([3, 8, 15, 9, 3], _best([0, 1, 2]), 3, 3, min_overlap=1)["offset"] == -2       # 3 = 3 at |k| = 2
    assert S.analyse([3, 8, 15, 6, 3], _best([0, 1, 2]), 3, 3, min_overlap=1)["offset"] == 1        # 3 at |k| = 1 first
    big = 2 ** 60   # exact: 2 (big + 1) / 2 < (3 big + 4) / 3, which no double could tell
    assert S.analyse([0, 2 * big + 2, 3 * big + 4, 9 * big, 0], _best([0, 1, 2]), 3, 3)["offset"] == -1


def test_min_overlap_excludes_a_short_lucky_diagonal():
    diag = [0, 40, 30, 80, 70]   # k = -2 (one pair, distance 0) .. 2
    assert S.analyse(diag, _best([0, 1, 2]), 3, 3, min_overlap=1)["offset"] == -2
    res = S.analyse(diag, _best([0, 1, 2]), 3, 3)                 # the default: (3 + 1) // 2 = 2 pairs at least
    assert res["offset"] == 0 and res["mean"] == 10 and res["runner_up"] is None   # -1 and 1 are within the guard
    assert S.analyse(diag, _best([0, 1, 2]), 3, 3, min_overlap=3)["offset"] == 0
    with pytest.raises(ValueError, match="no offset"):
        S.analyse(diag, _best([0, 1, 2]), 3, 3, min_overlap=4)


def test_runner_up_honours_the_guard():
    # n_dist = n_ref = 6: k = -5 .. 5, overlaps 1 .. 6 .. 1; min_overlap = 3 leaves k = -3 .. 3
    diag = [0, 0, 30, 40, 5, 0, 10, 44, 90, 0, 0]
    res = S.analyse(diag, _best(range(6)), 6, 6)
    assert res["offset"] == 0 and res["mean"] == 0
    assert res["runner_up"] == (-3, Fraction(10)) and not res["ambiguous"]      # -1, 1, -2, 2 are guarded; 30 / 3 < 90 / 3
    assert S.analyse(diag, _best(range(6)), 6, 6, guard=0)["runner_up"] == (-1, Fraction(1))
    assert S.analyse(diag, _best(range(6)), 6, 6, guard=1)["runner_up"] == (-2, Fraction(10))   # 40 / 4 = 10 < 44 / 4
    assert S.analyse(diag, _best(range(6)), 6, 6, guard=3)["runner_up"] is None
    keys = S.log_keys(S.analyse(diag, _best(range(6)), 6, 6, guard=3), False)
    assert keys["SYNC_RUNNER_UP"] == -1.0
    tie = S.analyse([0, 0, 0, 40, 5, 0, 10, 44, 90, 0, 0], _best(range(6)), 6, 6)
    assert tie["offset"] == 0 and tie["runner_up"] == (-3, Fraction(0)) and tie["ambiguous"]


def test_runs_for_an_inserted_segment():
    # frames 0 .. 3 at offset 2, three inserted frames that match elsewhere, frames 7 .. 9 at offset -1 (2 - 3)
    index = [2, 3, 4, 5, 40, 41, 17, 6, 7, 8]
    res = S.analyse([0] * 59, _best(index), 10, 50, min_overlap=10)
    assert res["per_frame"] == [2, 2, 2, 2, 36, 36, 11, -1, -1, -1]
    assert res["runs"] == [(0, 4, 2), (4, 2, 36), (6, 1, 11), (7, 3, -1)]
    assert res["offset"] == 0 and res["frames_off"] == 10
    # the distance half of a word takes no part in the index
    assert S.analyse([0] * 59, _best(index, dist=16646400), 10, 50, min_overlap=10)["per_frame"] == res["per_frame"]


def test_the_value_errors():
    ok = ([0, 0, 0], [0, 0])
    S.analyse(*ok, 2, 2)
    for bad in (([0, 0], [0, 0], 2, 2), ([0, 0, 0], [0], 2, 2), ([0, 0, 0], [0, 0], 0, 2), ([0, 0, 0], [0, 0], 2, True)):
        with pytest.raises(ValueError):
            S.analyse(*bad)
    for kw in (dict(min_overlap=0), dict(min_overlap=True), dict(min_overlap=1.5), dict(guard=-1), dict(min_overlap=3)):
        with pytest.raises(ValueError):
            S.analyse(*ok, 2, 2, **kw)


# ---- the log, the requests and the config ---------------------------------------------------------------------------------------------
HAND = {"offset": 3, "mean": Fraction(512, 1), "overlap": 12, "runner_up": (7, Fraction(25600, 1)), "ambiguous": False,
        "per_frame": [3] * 11 + [4], "frames_off": 1, "runs": [(0, 11, 3), (11, 1, 4)], "trim": (3, 0, 12)}


def test_the_key_order_and_the_log(tmp_path, caplog):
    keys = S.log_keys(HAND, True)
    assert list(keys) == list(S.SYNC_KEYS) == ["SYNC_OFFSET", "SYNC_OVERLAP", "SYNC_DISTANCE", "SYNC_RUNNER_UP", "SYNC_FRAMES_OFF",
                                               "SYNC_APPLIED"]
    assert list(keys.values()) == [3, 12, 2.0, 100.0, 1, 1]
    assert [type(v) for v in keys.values()] == [int, int, float, float, int, int]
    with caplog.at_level(logging.WARNING):
        assert vp.sync_extra(HAND, True) == keys
    assert any("trimmed" in r.getMessage() for r in caplog.records)
    caplog.clear()
    with caplog.at_level(logging.WARNING):
        assert vp.sync_extra(HAND, False)["SYNC_APPLIED"] == 0
    assert any("NOT re-paired" in r.getMessage() for r in caplog.records)
    caplog.clear()
    with caplog.at_level(logging.WARNING):
        vp.sync_extra(dict(HAND, ambiguous=True, runner_up=(7, Fraction(512, 1))), False)
    assert any("ambiguous" in r.getMessage() for r in caplog.records)
    caplog.clear()
    with caplog.at_level(logging.WARNING):
        vp.sync_extra(dict(HAND, offset=0, frames_off=0, trim=(0, 0, 12)), False)
    assert not caplog.records
    # in the log: after the LIGHT_* keys, before the ALIGN_* / SHIFT_* keys; in the row likewise
    from rtvqa_amd.align import ALIGN_KEYS
    from rtvqa_amd.light import LIGHT_KEYS
    from rtvqa_amd.shift import SHIFT_KEYS
    found = {"shift": {k: 1 for k in SHIFT_KEYS}, "align": {k: 1 for k in ALIGN_KEYS}, "sync": keys,
             "light": {k: 1 for k in LIGHT_KEYS}}   # (in no order: the table orders them)
    merged = vp._prepass_keys(found)
    assert list(merged) == list(LIGHT_KEYS) + list(S.SYNC_KEYS) + list(ALIGN_KEYS) + list(SHIFT_KEYS)
    assert list(vp._prepass_keys({"sync": keys})) == list(S.SYNC_KEYS)
    log = str(tmp_path / "v.json")
    vp.write_vif_log(log, extra=merged)
    doc = json.load(open(log))
    assert list(doc) == ["frames", "pooled_metrics"] + list(merged) and doc["SYNC_DISTANCE"] == 2.0
    row = vp.extract_metrics_from_logs("absent", "absent", log, "x", 23, 0, "8x8", 30.0)
    assert list(row)[-len(merged):] == list(merged) and [row[k] for k in S.SYNC_KEYS] == [3, 12, 2.0, 100.0, 1, 1]
    vp.write_vif_log(log)
    assert not any(k.startswith("SYNC") for k in vp.extract_metrics_from_logs("absent", "absent", log, "x", 23, 0, "8x8", 30.0))


BASE = {"crf": 23, "resize_width": 64, "resize_height": 64, "frame_interval": 1}


def test_the_requests_and_the_config_keys():
    vp.validate_config(dict(BASE))
    for ok in (dict(sync=True), dict(sync=False), dict(sync=True, sync_min_overlap=1), dict(sync=True, sync_min_overlap=None),
               dict(sync=True, sync_apply=True), dict(sync=True, sync_apply=True, sync_min_overlap=40),
               dict(sync=True, scale="bicubic", dist_height=32, dist_width=32)):
        vp.validate_config(dict(BASE, **ok))
    for bad in (1, 0, "yes", None, [True]):
        with pytest.raises(ValueError, match="sync must be true or false"):
            vp.validate_config(dict(BASE, sync=bad))
    for bad in (1, "no", None):
        with pytest.raises(ValueError, match="sync_apply must be true or false"):
            vp.validate_config(dict(BASE, sync=True, sync_apply=bad))
    for bad in (0, -3, True, 2.0, "4", [4]):
        with pytest.raises(ValueError, match="sync_min_overlap must be null or an integer >= 1"):
            vp.validate_config(dict(BASE, sync=True, sync_min_overlap=bad))
    with pytest.raises(ValueError, match="sync_apply needs sync"):
        vp.validate_config(dict(BASE, sync_apply=True))
    assert vp._sync_request(False) is None and vp._sync_request(True) == (None, False)
    assert vp._sync_request(True, 7, True) == (7, True)
    # the entry points refuse before any stream is opened or any device touched
    z = np.zeros((2, 32, 32, 3), np.uint8)
    with pytest.raises(ValueError, match="sync_apply needs sync"):
        vp.run_ffmpeg_metrics(z, z, "p", "s", "v", sync_apply=True)
    with pytest.raises(ValueError, match="sync_min_overlap"):
        vp.run_ffmpeg_metrics(z, z, "p", "s", "v", sync=True, sync_min_overlap=0)
    with pytest.raises(ValueError, match="sync must be"):
        vp.process_video_and_extract_metrics(z, z, dict(BASE, sync="on"))
    g = np.zeros((2, 16, 16), np.uint8)
    for bad in (0, N.SIG_MAX_BATCH + 1):
        with pytest.raises(ValueError, match="window"):
            vp.frame_sync(g, g, "gray", window=bad)
    with pytest.raises(ValueError, match="refine"):
        vp.frame_sync(g, g, "gray", refine=33)
    with pytest.raises(ValueError, match="one geometry"):
        vp.frame_sync(g, g, "gray", dist_height=16, dist_width=16, refine=2)


# ---- the additive ABI -----------------------------------------------------------------------------------------------------------------
def test_the_additive_abi():
    assert N.VQA_ABI_VERSION == 8
    assert (N.K_LINTEL, N.K_SIG, N.K_SIG_DIAG, N.K_SIG_BEST, N.K_EAVE) == (74, 75, 76, 77, 78)
    assert N.K_IDS_EXTANT == N.K_IDS_NEWEST + (75, 76, 77) and 74 not in N.K_IDS_EXTANT and 78 not in N.K_IDS_EXTANT
    assert (N.SIG_GRID, N.SIG_BYTES, N.SIG_MAX_BATCH, N.SIG_MAX_FRAMES) == (16, 256, 32768, 262144)
    txt = open(os.path.join(REPO, "include", "vqa.h")).read()
    for name, val in (("VQA_K_LINTEL", 74), ("VQA_K_SIG", 75), ("VQA_K_SIG_DIAG", 76), ("VQA_K_SIG_BEST", 77), ("VQA_K_EAVE", 78)):
        assert re.search(r"%s\s*=\s*%d\b" % (name, val), txt), name
    assert re.search(r"#define VQA_ABI_VERSION\s+8", txt)
    for name, val in (("VQA_SIG_GRID", 16), ("VQA_SIG_BYTES", 256), ("VQA_SIG_MAX_BATCH", 32768), ("VQA_SIG_MAX_FRAMES", 262144)):
        assert re.search(r"#define %s\s+%d\b" % (name, val), txt), name
    assert txt.index("---- Clip-wide sync") > txt.index("VQA_API int vqa_light_gamut")   # a new section after the light kind
    part = txt[txt.index("---- Clip-wide sync"):]
    part = part[:part.index("VQA_API int vqa_sig_cross_wait")]
    for word in ("floor(a h / 16) .. floor((a + 1) h / 16) - 1", "min(255, floor(S / (c << (depth - 8))))", "unsigned 64-bit integer division",
                 "9 .. 16", "pixel_step = 3", "THE SLOW PATH", "No byte beyond", "at least 16 x 16", "n <= 32768", "VQA_ERR_UNSUPPORTED",
                 "sum_k (dist_sig[j][k] - ref_sig[i][k])^2", "256 * 255^2 < 2^24", "diag[k + n_dist - 1]", "n_dist + n_ref - 1 words",
                 "((D[j][i] << 32) | i)", "ties to the smallest i", "E_d[j] + E_r[i] - 2 C[j][i]", "int8 matrix cores", "k_sig_diag",
                 "k_sig_best", "VQA_ERR_STATE", "contribute to neither", "Not built", "any place of any batch"):
        assert word in part, word
    lib = N.load()
    lib.vqa_kernel_name.restype = C.c_char_p
    assert [lib.vqa_kernel_name(k) for k in (75, 76, 77)] == [b"k_sig", b"k_sig_diag", b"k_sig_best"]
    assert lib.vqa_kernel_name(74) == b"?" and lib.vqa_kernel_name(78) == b"?" and lib.vqa_kernel_name(73) == b"k_light_scan"
    assert lib.vqa_sig_submit(None, None, 0, 0, 0, None) == N.VQA_ERR_INVALID
    assert lib.vqa_sig_wait(None, None, 0) == N.VQA_ERR_INVALID
    assert lib.vqa_sig_cross_submit(None, None, 0, None, 0) == N.VQA_ERR_INVALID
    assert lib.vqa_sig_cross_wait(None, None, 0, None, 0) == N.VQA_ERR_INVALID
    for k in (74, 78):
        assert lib.vqa_profile_read(None, k, None, None, 0) == N.VQA_ERR_INVALID
    for path in (N.LIB_PATH, N.LAB_LIB_PATH):
        assert all(hasattr(C.CDLL(path), f) for f in ("vqa_sig_submit", "vqa_sig_wait", "vqa_sig_cross_submit", "vqa_sig_cross_wait"))


def test_the_header_to_the_c_compiler(tmp_path):
    src = ('#include <stdio.h>\n#include "vqa.h"\n'
           'int (*submit)(vqa_ctx *, const uint8_t *, int, int, int64_t, const vqa_plane_desc *) = vqa_sig_submit;\n'
           'int (*wait_)(vqa_ctx *, uint8_t *, int) = vqa_sig_wait;\n'
           'int (*xsubmit)(vqa_ctx *, const uint8_t *, int, const uint8_t *, int) = vqa_sig_cross_submit;\n'
           'int (*xwait)(vqa_ctx *, uint64_t *, int64_t, uint64_t *, int64_t) = vqa_sig_cross_wait;\n'
           'int main(void){int rc = vqa_sig_submit(0, 0, VQA_MEM_HOST, 1, 0, 0), rx = vqa_sig_cross_submit(0, 0, 1, 0, 1);\n'
           'printf("%d %d %d %d %d %d %d %d %d %d\\n", VQA_K_LINTEL, VQA_K_SIG, VQA_K_SIG_DIAG, VQA_K_SIG_BEST, VQA_K_EAVE, VQA_SIG_GRID,'
           ' VQA_SIG_BYTES, VQA_SIG_MAX_FRAMES, rc, rx);'
           ' return submit == 0 || wait_ == 0 || xsubmit == 0 || xwait == 0;}\n')
    (tmp_path / "a.c").write_text(src)
    lib_dir = os.path.dirname(N.LIB_PATH)
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), "-o", str(tmp_path / "a"), str(tmp_path / "a.c"),
                           "-L", lib_dir, "-l:" + os.path.basename(N.LIB_PATH), "-Wl,-rpath," + lib_dir,
                           "-Wl,--allow-shlib-undefined"])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "a")]).decode().split()]
    assert got == [74, 75, 76, 77, 78, 16, 256, 262144, N.VQA_ERR_INVALID, N.VQA_ERR_INVALID]
