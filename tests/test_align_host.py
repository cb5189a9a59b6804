"""Host: temporal alignment without a GPU - the restatement against hand answers, align.py's rules on the issue's three scenarios
and on hand-made bands, the additive ABI (header text, kernel ids, exported symbols, NULL ctx), the header under a C compiler,
the config checks, and the log and row writers fed a hand-made analyse dict."""
import ctypes as C
import json
import logging
import math
import os
import re
import subprocess

import numpy as np
import pytest

import align_cases as AC
import align_reference as R
from rtvqa_amd import _native as N
from rtvqa_amd import align as A
from rtvqa_amd import video_processing as vp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X = A.NONE


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def test_the_restatement_against_hand_answers():
    r = np.array([[[1, 2], [3, 4]], [[0, 0], [0, 10]]], np.uint8)
    d = np.array([[[2, 2], [1, 4]]], np.uint8)
    rp, dp = R.plane_series(r, AC.mono(2, 2)[0]), R.plane_series(d, AC.mono(2, 2)[0])
    assert rp.tolist() == r.tolist() and rp.dtype == np.int64
    #                 k = -1   k = 0: 1 + 0 + 4 + 0   k = 1: 4 + 4 + 1 + 36
    assert R.band(rp, dp, 1).tolist() == [[X, 5, 45]]
    assert R.band(rp, dp, 1, offset=1).tolist() == [[5, 45, X]]
    z, f = np.zeros((1, 3, 5), np.uint8), np.full((1, 3, 5), 255, np.uint8)
    assert R.band(R.plane_series(z, AC.mono(5, 3)[0]), R.plane_series(f, AC.mono(5, 3)[0]), 0).tolist() == [[15 * 255 * 255]]
    z, f = np.zeros((1, 3, 5), np.uint16), np.full((1, 3, 5), 65535, np.uint16)
    p = AC.mono(5, 3, 16)[0]
    assert R.band(R.plane_series(z, p), R.plane_series(f, p), 0).tolist() == [[15 * 65535 * 65535]]
    # a plane at pixel step 3 inside padded rows: the G channel
    bgr = np.arange(2 * 2 * 3 * 3, dtype=np.uint8).reshape(2, 2, 3, 3)
    assert R.plane_series(bgr, (3, 2, 1, 9, 3)).tolist() == bgr[..., 1].tolist()
    assert R.NONE == A.NONE == N.ALIGN_NONE == 2 ** 64 - 1


# ---- align.py: the three scenarios ------------------------------------------------------------------------------------------------
def _band(ref, enc, radius):
    return R.band(ref.astype(np.int64), enc.astype(np.int64), radius)


def test_a_dropped_and_a_repeated_frame_are_found():
    ref, enc, index = AC.dropped_and_repeated()
    assert len(index) == 40 and 10 not in index and index.count(25) == 2
    sse = _band(ref, enc, 4)
    res = A.analyse(sse)
    assert res["ref_index"] == index and res["offset"] == 0
    assert (res["dropped"], res["repeated"], res["mismatched"]) == (1, 1, 15)
    assert res["match"] == [i - j for j, i in enumerate(index)]
    given = sum(int(sse[j, 4]) for j in range(40) if int(sse[j, 4]) != X)
    aligned = sum(int(sse[j, 4 + res["match"][j]]) for j in range(40) if int(sse[j, 4]) != X)
    assert (res["sse_given"], res["sse_aligned"]) == (given, aligned) and aligned < given
    want = 10.0 * math.log10(given / aligned)
    assert abs(res["psnr_gain"] - want) <= 4 * math.ulp(want) and want > 20


def test_a_static_clip_is_the_constant_zero_path():
    ref, enc = AC.static_clip()
    res = A.analyse(_band(ref, enc, 4))
    assert res["offset"] == 0 and res["match"] == [0] * 12 and res["psnr_gain"] == 0.0
    assert (res["dropped"], res["repeated"], res["mismatched"], res["sse_given"], res["sse_aligned"]) == (0, 0, 0, 0, 0)


def test_a_late_start_is_a_constant_offset():
    ref, enc = AC.late_start()
    res = A.analyse(_band(ref, enc, 4))
    assert res["offset"] == 3 and res["match"] == [3] * 30 and res["ref_index"] == list(range(3, 33))
    assert (res["dropped"], res["repeated"], res["mismatched"], res["sse_aligned"]) == (0, 0, 30, 0)
    assert res["psnr_gain"] == A.PSNR_GAIN_CAP == 100.0


# ---- align.py: the tie rules on hand-made bands -------------------------------------------------------------------------------------
def test_offset_of_compares_exact_means_and_breaks_ties_towards_zero_then_negative():
    assert A.offset_of([[5, 5, 5], [5, 5, 5]]) == 0
    assert A.offset_of([[4, 5, 4], [4, 5, 4]]) == -1                      # -1 and +1 tie: the negative one
    assert A.offset_of([[4, 5, 3], [4, 5, 4]]) == 1
    assert A.offset_of([[X, 5, 3], [3, 5, X]]) == -1                      # means over the VALID entries: 3 = 3, the negative one
    assert A.offset_of([[X, 9, 1], [X, 9, X], [X, 9, 2]]) == 1            # 3 / 2 < 9
    big = 2 ** 60
    assert A.offset_of([[big + 1, big + 2, big], [big + 1, big + 2, big + 3]]) == -1   # 2 big + 2 < 2 big + 3: no double could tell
    assert A.offset_of([[X, X, X]]) == 0
    assert A.offset_of([[7, 1, 7, 1, 7]]) == -1


def test_match_path_is_monotone_and_breaks_ties_as_stated():
    assert A.match_path([[0, 0, 0]] * 4) == [0, 0, 0, 0]
    assert A.match_path([[0, 0, 0]] * 4, offset=1) == [1, 1, 1, 1]        # equally good ends: the nearest to the offset
    assert A.match_path([[0, 9, 0]] * 3, offset=0) == [-1, -1, -1]        # ... then the smaller
    # j + m[j] may not decrease: m = [1, -1] would cost 0 but steps back
    assert A.match_path([[9, 9, 0], [0, 9, 9]]) == [1, 0]                 # every path costs 9: the end nearest to the offset
    assert A.match_path([[9, 5, 0], [0, 5, 9]]) == [1, 0]                 # 0 + 5 = 5 + 0: likewise
    assert A.match_path([[9, 5, 0], [0, 7, 9]]) == [0, -1] and A.match_path([[9, 5, 0], [0, 3, 9]]) == [1, 0]
    assert A.match_path([[9, 1, 0], [0, 20, 30]]) == [0, -1]              # 1 + 0 beats 0 + 20
    # rows with invalid entries: the path uses valid columns only
    assert A.match_path([[X, 0, 5], [X, 5, 0], [5, 0, X]]) == [0, 1, 0]
    assert A.match_path([[X, X, X], [X, 2, 1]]) == [0, 1]                 # a row with nothing valid takes no part
    # equally good predecessors: k itself first (the path stays), so the step comes as LATE as the cost allows
    assert A.match_path([[0, 0, 9], [0, 0, 9], [9, 0, 9]]) == [0, 0, 0]
    assert A.match_path([[1, 1, 9], [1, 1, 9], [9, 9, 1]], offset=1) == [0, 0, 1]
    res = A.analyse([[X, 0, 5], [X, 5, 0], [5, 0, X]])
    assert res["ref_index"] == [0, 2, 2] and (res["dropped"], res["repeated"], res["mismatched"]) == (1, 1, 1)
    assert (res["sse_given"], res["sse_aligned"]) == (5, 0) and res["psnr_gain"] == 100.0
    with pytest.raises(ValueError):
        A.analyse([[1, 2]])
    with pytest.raises(ValueError):
        A.analyse([])


def test_psnr_gain():
    assert A.psnr_gain(0, 0) == 0.0 and A.psnr_gain(7, 7) == 0.0 and A.psnr_gain(7, 0) == 100.0
    assert A.psnr_gain(1000, 10) == 20.0 and A.psnr_gain(10 ** 30, 1) == 100.0


# ---- the additive ABI -----------------------------------------------------------------------------------------------------------------
def test_the_additive_abi():
    assert N.VQA_ABI_VERSION == 8
    assert (N.K_MARGIN, N.K_ALIGN_CROSS, N.K_LEDGE) == (67, 68, 69)
    assert N.K_IDS_CURRENT == N.K_IDS_PRESENT + (68,) and 67 not in N.K_IDS_CURRENT and 69 not in N.K_IDS_CURRENT
    assert (N.ALIGN_MAX_RADIUS, N.ALIGN_MAX_DIST, N.ALIGN_MAX_REF) == (32, 32768, 32768 + 64)
    txt = open(os.path.join(REPO, "include", "vqa.h")).read()
    for name, val in (("VQA_K_MARGIN", 67), ("VQA_K_ALIGN_CROSS", 68), ("VQA_K_LEDGE", 69)):
        assert re.search(r"%s\s*=\s*%d\b" % (name, val), txt), name
    assert re.search(r"#define VQA_ABI_VERSION\s+8", txt)
    assert re.search(r"#define VQA_ALIGN_NONE\s+UINT64_MAX", txt) and re.search(r"#define VQA_ALIGN_MAX_RADIUS\s+32", txt)
    part = txt[txt.index("---- Temporal alignment"):]
    part = part[:part.index("VQA_API int vqa_align_wait")]
    for word in ("j + offset + k", "sum over the plane of (d_j - r_i)^2", "VQA_ALIGN_NONE otherwise", "row-major", "9 .. 16",
                 "pixel_step = 3", "THE SLOW PATH", "exactly 0", "E_d[j] + E_r[i] - 2 C[j][i]", "int8 matrix cores", "at least 1 x 1",
                 "n_dist <= 32768", "32768 + 64", "VQA_ERR_UNSUPPORTED", "0 .. 32 is VQA_ERR_INVALID", "VQA_ERR_STATE",
                 "k_align_cross", "are not read", "Not built", "No byte beyond"):
        assert word in part, word
    lib = N.load()
    lib.vqa_kernel_name.restype = C.c_char_p
    assert lib.vqa_kernel_name(68) == b"k_align_cross" and lib.vqa_kernel_name(67) == b"?" and lib.vqa_kernel_name(69) == b"?"
    assert lib.vqa_kernel_name(66) == b"k_scale"
    assert lib.vqa_align_submit(None, None, 0, None, 0, 0, 0, 0, None, 0, 8) == N.VQA_ERR_INVALID
    assert lib.vqa_align_wait(None, None, 0) == N.VQA_ERR_INVALID
    for k in (67, 69):
        assert lib.vqa_profile_read(None, k, None, None, 0) == N.VQA_ERR_INVALID
    for path in (N.LIB_PATH, N.LAB_LIB_PATH):
        assert all(hasattr(C.CDLL(path), f) for f in ("vqa_align_submit", "vqa_align_wait"))


def test_the_header_to_the_c_compiler(tmp_path):
    src = ('#include <stdio.h>\n#include "vqa.h"\n'
           'int (*submit)(vqa_ctx *, const uint8_t *, int, const uint8_t *, int, int, int64_t, int64_t, const vqa_plane_desc *, int, '
           'int) = vqa_align_submit;\n'
           'int (*wait_)(vqa_ctx *, uint64_t *, int64_t) = vqa_align_wait;\n'
           'int main(void){uint64_t none = VQA_ALIGN_NONE; int rc = vqa_align_submit(0, 0, 1, 0, 1, VQA_MEM_HOST, 0, 0, 0, 0, 8);\n'
           'printf("%d %d %d %d %d %d\\n", VQA_K_MARGIN, VQA_K_ALIGN_CROSS, VQA_K_LEDGE, VQA_ALIGN_MAX_RADIUS, none + 1 == 0, rc);'
           ' return submit == 0 || wait_ == 0;}\n')
    (tmp_path / "a.c").write_text(src)
    lib_dir = os.path.dirname(N.LIB_PATH)
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), "-o", str(tmp_path / "a"), str(tmp_path / "a.c"),
                           "-L", lib_dir, "-l:" + os.path.basename(N.LIB_PATH), "-Wl,-rpath," + lib_dir,
                           "-Wl,--allow-shlib-undefined"])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "a")]).decode().split()]
    assert got == [67, 68, 69, 32, 1, N.VQA_ERR_INVALID]


# ---- the Python layers ----------------------------------------------------------------------------------------------------------------
BASE = {"crf": 23, "resize_width": 64, "resize_height": 64, "frame_interval": 1}


def test_the_config_key():
    for ok in (None, 1, 8, 32):
        vp.validate_config(dict(BASE, align=ok))
    vp.validate_config(dict(BASE))
    for bad in (0, 33, -1, True, False, 2.0, "8", [4]):
        with pytest.raises(ValueError, match="align must be null or an integer radius from 1 to 32"):
            vp.validate_config(dict(BASE, align=bad))
    with pytest.raises(ValueError, match="align and scale"):
        vp.validate_config(dict(BASE, align=4, scale="bicubic", dist_height=32, dist_width=32))
    with pytest.raises(ValueError, match="align and scale"):
        vp.run_ffmpeg_metrics(np.zeros((2, 32, 32, 3), np.uint8), np.zeros((2, 16, 16, 3), np.uint8), "p", "s", "v", scale="bicubic",
                              align=4)
    with pytest.raises(ValueError, match="align must be"):
        vp.run_ffmpeg_metrics(np.zeros((2, 32, 32, 3), np.uint8), np.zeros((2, 32, 32, 3), np.uint8), "p", "s", "v", align=40)
    for bad in (-1, 33):
        with pytest.raises(ValueError, match="radius"):
            vp.frame_align(np.zeros((2, 8, 8), np.uint8), np.zeros((2, 8, 8), np.uint8), "gray", radius=bad)


HAND = {"offset": 0, "match": [0, 1, 1], "ref_index": [0, 2, 3], "dropped": 1, "repeated": 0, "mismatched": 2,
        "sse_given": 3000, "sse_aligned": 30, "psnr_gain": 20.0}


def test_the_log_and_the_row_from_a_hand_made_result(tmp_path, caplog):
    with caplog.at_level(logging.WARNING):
        extra = vp.align_extra(HAND, 4)
    assert list(extra) == list(A.ALIGN_KEYS) == ["ALIGN_RADIUS", "ALIGN_OFFSET", "ALIGN_DROPPED", "ALIGN_REPEATED", "ALIGN_PSNR_GAIN"]
    assert list(extra.values()) == [4, 0, 1, 0, 20.0]
    assert any("not aligned" in r.getMessage() and "NOT re-paired" in r.getMessage() for r in caplog.records)
    caplog.clear()
    with caplog.at_level(logging.WARNING):
        quiet = vp.align_extra(dict(HAND, dropped=0, match=[0, 0, 0], psnr_gain=0.0), 4)
    assert not caplog.records and list(quiet.values()) == [4, 0, 0, 0, 0.0]
    log = str(tmp_path / "v.json")
    vp.write_vif_log(log, extra=extra)
    doc = json.load(open(log))
    assert list(doc) == ["frames", "pooled_metrics"] + list(A.ALIGN_KEYS) and doc["ALIGN_PSNR_GAIN"] == 20.0
    row = vp.extract_metrics_from_logs("absent", "absent", log, "x", 23, 0, "8x8", 30.0)
    assert list(row)[-5:] == list(A.ALIGN_KEYS) and [row[k] for k in A.ALIGN_KEYS] == [4, 0, 1, 0, 20.0]
    # a log without the keys gives the row it gave
    vp.write_vif_log(log)
    assert not any(k.startswith("ALIGN") for k in vp.extract_metrics_from_logs("absent", "absent", log, "x", 23, 0, "8x8", 30.0))
