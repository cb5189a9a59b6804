"""Host: the restatement of spatial registration (tests/shift_reference.py) against grids computed by hand, the cases' own
guarantees (tests/shift_cases.py), the pure-host reader rtvqa_amd.shift on hand-made grids, the additive ABI, and the argument
errors of the Python entry points.  No GPU."""
import ctypes as C
import logging
import math
import json
import os
import re
import subprocess

import numpy as np
import pytest

import shift_cases as SC
import shift_reference as R
from rtvqa_amd import _native as N
from rtvqa_amd import shift as S
from rtvqa_amd import video_processing as vp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement, by hand -----------------------------------------------------------------------------------------------------------
def _both(ref, dist, radius, margin=None):
    a = R.grid(np.array(ref, np.int64), np.array(dist, np.int64), radius, margin)
    assert a.dtype == np.uint64 and a.tolist() == R.loops(ref, dist, radius, margin)
    return a.tolist()


def test_a_single_impulse():
    """5 x 5, R = M = 1: the core is rows and columns 1 .. 3.  A reference impulse of 5 at (2, 3) lies inside the moved core
    for every dy and for dx = 0, 1 (column 3 - dx must be 1 .. 3); a distorted impulse of 7 at (2, 2) is in every sum; the two
    meet at (dy, dx) = (0, 1), where (7 - 5)^2 = 4 replaces 49 + 25."""
    zero = [[0] * 5 for _ in range(5)]
    ref = [row[:] for row in zero]
    ref[2][3] = 5
    assert _both(ref, zero, 1) == [[0, 25, 25]] * 3
    dist = [row[:] for row in zero]
    dist[2][2] = 7
    assert _both(zero, dist, 1) == [[49] * 3] * 3
    assert _both(ref, dist, 1) == [[49, 74, 74], [49, 74, 4], [49, 74, 74]]


def test_a_5x5_plane_written_out():
    """ref(y, x) = 5 y + x + 1; the distorted core is the reference's plus e = +1 at its first and -1 at its last sample, so
    d(y, x) - r(y + dy, x + dx) = e - k with k = 5 dy + dx, and the nine samples sum to 9 k^2 - 2 k sum(e) + sum(e^2) = 9 k^2 + 2."""
    ref = [[5 * y + x + 1 for x in range(5)] for y in range(5)]
    dist = [[0] * 5 for _ in range(5)]
    for y in range(1, 4):
        for x in range(1, 4):
            dist[y][x] = ref[y][x]
    dist[1][1] += 1
    dist[3][3] -= 1
    assert _both(ref, dist, 1) == [[326, 227, 146], [11, 2, 11], [146, 227, 326]]


def test_a_ramp_and_a_margin_above_the_radius():
    """ref = dist = 3 y + 2 x on 9 x 11 (h x w), R = 2, M = 3: a core of 3 x 5 samples, each off by 3 dy + 2 dx"""
    ramp = [[3 * y + 2 * x for x in range(11)] for y in range(9)]
    assert _both(ramp, ramp, 2, 3) == [[15 * (3 * dy + 2 * dx) ** 2 for dx in range(-2, 3)] for dy in range(-2, 3)]
    # the margin is part of the definition: M = 2 sums 5 x 7 samples
    assert _both(ramp, ramp, 2, 2)[0][0] == 35 * 100
    # the sign: the distorted picture shows at (y, x) what the reference shows at (y + 1, x - 2)
    ref = np.arange(9 * 11).reshape(9, 11) ** 2 % 251
    dist = np.zeros_like(ref)
    dist[0:8, 2:11] = ref[1:9, 0:9]
    g = R.grid(ref, dist, 2)
    assert g[1 + 2, -2 + 2] == 0 and SC.smallest(g) == ((1, -2), 1)


def test_the_cases_have_one_smallest_word_and_the_translated_cases_one_zero():
    for case in SC.GEOMETRY + SC.DEPTHS:
        ref, dist = SC.pair(case)
        for g in R.grids(ref.astype(np.int64), dist.astype(np.int64), case[2], case[3]):
            assert SC.smallest(g)[1] == 1 and g.min() > 0, case
    for case in SC.TRANSLATED:
        ref, dist = SC.translated_pair(case)
        for g in R.grids(ref.astype(np.int64), dist.astype(np.int64), case[2], case[3]):
            assert SC.smallest(g) == (case[4], 1) and g.min() == 0 and (g == 0).sum() == 1, case
    ref, dist = SC.moved_clip()
    for g in R.grids(ref.astype(np.int64), dist.astype(np.int64), 4):
        assert SC.smallest(g) == ((2, -2), 1)
    w, h, _r, _m = SC.RANGE_PLANE
    assert SC.ROWS * ((w - 2) // 64) >= 2 * SC.FLUSH and h - 2 + 2 >= SC.ROWS   # two flushes before the visit's last
    assert 2 * 64 * SC.FLUSH * 128 * 128 == 1 << 30
    assert (SC.ROWS, SC.FLUSH) == (N.SHIFT_ROWS, N.SHIFT_FLUSH)


# ---- shift.py on hand-made grids --------------------------------------------------------------------------------------------------------
def test_best_of_and_its_ties():
    assert S.best_of([[5] * 3] * 3) == (0, 0)                                  # all equal: the centre
    assert S.best_of([[9, 1, 9], [1, 9, 9], [9, 9, 9]]) == (-1, 0)              # (-1, 0) and (0, -1): the smaller dy
    assert S.best_of([[9, 9, 9], [1, 9, 1], [9, 9, 9]]) == (0, -1)              # (0, -1) and (0, 1): the smaller dx
    assert S.best_of([[1, 9, 9], [9, 9, 1], [9, 9, 9]]) == (0, 1)               # a corner and an edge: the nearer
    assert S.best_of([[9, 9, 9], [9, 9, 9], [9, 9, 0]]) == (1, 1)               # a strict improvement wins wherever it lies
    g = [[50] * 5 for _ in range(5)]
    g[0][4] = g[4][0] = 3
    assert S.best_of(g) == (-2, 2)                                             # equal distance: the smaller dy
    for bad in ([], [[1]], [[1, 2], [3, 4]], [[1, 2, 3], [4, 5, 6]], [[1, 2, 3], [4, 5], [6, 7, 8]]):
        with pytest.raises(ValueError):
            S.best_of(bad)


def _quad(R, y0, x0, scale=1):
    """an exact quadratic with integer words: (4 dy - 4 y0)^2 + (4 dx - 4 x0)^2, y0 and x0 multiples of 1/4"""
    return [[scale * (int(4 * dy - 4 * y0) ** 2 + int(4 * dx - 4 * x0) ** 2) for dx in range(-R, R + 1)] for dy in range(-R, R + 1)]


def test_analyse():
    a, b = _quad(2, 1, -1), _quad(2, 0, 0)
    b[2][2] = 1
    res = S.analyse([a, a, b])
    assert res["shift"] == (1, -1) and res["per_frame"] == [(1, -1), (1, -1), (0, 0)] and res["frames_off"] == 1
    assert res["edge"] is False and res["sse_given"] == 32 + 32 + 1 and res["sse_shifted"] == 0 + 0 + 32
    assert res["psnr_gain"] == 10.0 * math.log10(65 / 32) and res["subpixel"] != (0.0, 0.0)
    # the border of the band
    assert S.analyse([_quad(2, 2, 0)])["edge"] is True and S.analyse([_quad(2, 0, -2)])["edge"] is True
    assert S.analyse([_quad(2, 2, 0)])["subpixel"] == (0.0, 0.0)
    # psnr_gain: the cap and the zero
    assert S.analyse([_quad(1, 1, 0)])["psnr_gain"] == 100.0                   # sse_shifted == 0 away from (0, 0)
    assert S.analyse([_quad(1, 0, 0)])["psnr_gain"] == 0.0 and S.analyse([[[7] * 3] * 3])["psnr_gain"] == 0.0
    big = [[10 ** 30] * 3 for _ in range(3)]
    big[0][0] = 1
    assert S.analyse([big])["psnr_gain"] == 100.0                              # 300 dB, capped
    assert S.psnr_gain(1000, 10, (0, 1)) == 20.0 and S.psnr_gain(1000, 10, (0, 0)) == 0.0
    # the parabola on an exact quadratic: the vertex itself
    res = S.analyse([_quad(2, 0.25, -0.25, 3), _quad(2, 0.25, -0.25, 5)])
    assert res["shift"] == (0, 0) and res["subpixel"] == (0.25, -0.25)
    flat = [[4, 4, 4], [4, 4, 4], [4, 4, 4]]
    assert S.analyse([flat])["subpixel"] == (0.0, 0.0)                         # the second difference is not positive
    # sums are exact: two frames whose words need more than 53 bits
    h1, h2 = [[(1 << 60) + 5] * 3 for _ in range(3)], [[(1 << 60) + 5] * 3 for _ in range(3)]
    h1[1][2] = 1 << 60
    h2[1][2] = (1 << 60) + 11
    h2[2][1] = (1 << 60) + 4
    assert S.analyse(np.array([h1, h2], np.uint64))["shift"] == (1, 0)        # 2^61 + 9 against 2^61 + 10 and 2^61 + 11
    for bad in ([], [[[1, 2, 3]] * 3, [[1] * 5] * 5]):
        with pytest.raises(ValueError):
            S.analyse(bad)


# ---- the additive ABI -------------------------------------------------------------------------------------------------------------------
def test_the_additive_abi():
    assert N.VQA_ABI_VERSION == 8
    assert (N.K_LEDGE, N.K_SHIFT, N.K_SILL) == (69, 70, 71)
    assert N.K_IDS_LATEST == N.K_IDS_CURRENT + (70,) and 69 not in N.K_IDS_LATEST and 71 not in N.K_IDS_LATEST
    assert (N.SHIFT_MAX_RADIUS, N.SHIFT_MAX_FRAMES) == (16, 32768)
    txt = open(os.path.join(REPO, "include", "vqa.h")).read()
    for name, val in (("VQA_K_LEDGE", 69), ("VQA_K_SHIFT", 70), ("VQA_K_SILL", 71)):
        assert re.search(r"%s\s*=\s*%d\b" % (name, val), txt), name
    assert re.search(r"#define VQA_ABI_VERSION\s+8", txt) and re.search(r"#define VQA_SHIFT_MAX_RADIUS\s+16", txt)
    part = txt[txt.index("---- Spatial registration"):]
    part = part[:part.index("VQA_API int vqa_shift_wait")]
    for word in ("(d_j(y, x) - r_j(y + dy, x + dx))^2", "M <= y < h - M", "row-major", "9 .. 16", "pixel_step = 3", "THE SLOW PATH",
                 "exactly 0", "E_d + E_r(dy, dx) - 2 C(dy, dx)", "matrix cores", "SAME core", "what the reference shows at (y + dy, x + dx)",
                 "1 <= n <= 32768", "VQA_ERR_UNSUPPORTED", "1 .. 16 or M < R is", "VQA_ERR_STATE", "k_shift", "are not read",
                 "Not built", "No byte beyond", "2^14"):
        assert word in part, word
    kern = open(os.path.join(os.path.dirname(N.LIB_PATH), "k_shift.hip")).read()
    assert re.search(r"SHIFT_FLUSH = %d;" % N.SHIFT_FLUSH, kern) and "Range:" in kern
    hpp = open(os.path.join(os.path.dirname(N.LIB_PATH), "vqa_kernels.hpp")).read()
    assert re.search(r"SHIFT_ROWS = %d;" % N.SHIFT_ROWS, hpp)
    lib = N.load()
    lib.vqa_kernel_name.restype = C.c_char_p
    assert lib.vqa_kernel_name(70) == b"k_shift" and lib.vqa_kernel_name(69) == b"?" and lib.vqa_kernel_name(71) == b"?"
    assert lib.vqa_kernel_name(68) == b"k_align_cross"
    assert lib.vqa_shift_submit(None, None, None, 0, 0, 0, 0, None, 4, 4) == N.VQA_ERR_INVALID
    assert lib.vqa_shift_wait(None, None, 0) == N.VQA_ERR_INVALID
    for k in (69, 71):
        assert lib.vqa_profile_read(None, k, None, None, 0) == N.VQA_ERR_INVALID
    for path in (N.LIB_PATH, N.LAB_LIB_PATH):
        assert all(hasattr(C.CDLL(path), f) for f in ("vqa_shift_submit", "vqa_shift_wait"))


def test_the_header_to_the_c_compiler(tmp_path):
    src = ('#include <stdio.h>\n#include "vqa.h"\n'
           'int (*submit)(vqa_ctx *, const uint8_t *, const uint8_t *, int, int, int64_t, int64_t, const vqa_plane_desc *, int, int) '
           '= vqa_shift_submit;\n'
           'int (*wait_)(vqa_ctx *, uint64_t *, int64_t) = vqa_shift_wait;\n'
           'int main(void){int rc = vqa_shift_submit(0, 0, 0, 1, VQA_MEM_HOST, 0, 0, 0, 4, 4);\n'
           'printf("%d %d %d %d %d\\n", VQA_K_LEDGE, VQA_K_SHIFT, VQA_K_SILL, VQA_SHIFT_MAX_RADIUS, rc);'
           ' return submit == 0 || wait_ == 0;}\n')
    (tmp_path / "a.c").write_text(src)
    lib_dir = os.path.dirname(N.LIB_PATH)
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), "-o", str(tmp_path / "a"), str(tmp_path / "a.c"),
                           "-L", lib_dir, "-l:" + os.path.basename(N.LIB_PATH), "-Wl,-rpath," + lib_dir,
                           "-Wl,--allow-shlib-undefined"])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "a")]).decode().split()]
    assert got == [69, 70, 71, 16, N.VQA_ERR_INVALID]


# ---- the Python layers ------------------------------------------------------------------------------------------------------------------
BASE = {"crf": 23, "resize_width": 64, "resize_height": 64, "frame_interval": 1}


def test_the_request_and_the_config_keys():
    assert vp._shift_request(None) is None and vp._shift_request(4) == (4, 4) and vp._shift_request(4, 6) == (4, 6)
    assert vp._shift_request(np.int64(16), np.int32(16)) == (16, 16)
    for ok in (None, 1, 4, 16):
        vp.validate_config(dict(BASE, shift=ok))
    vp.validate_config(dict(BASE, shift=4, shift_margin=9))
    vp.validate_config(dict(BASE, shift=4, align=8))
    vp.validate_config(dict(BASE))
    for bad in (0, 17, -1, True, False, 2.0, "4", [4]):
        with pytest.raises(ValueError, match="shift must be null or an integer radius from 1 to 16"):
            vp.validate_config(dict(BASE, shift=bad))
    for bad in (3, 0, -1, True, 4.0, "4"):
        with pytest.raises(ValueError, match="shift_margin must be null or an integer not below shift"):
            vp.validate_config(dict(BASE, shift=4, shift_margin=bad))
    with pytest.raises(ValueError, match="shift_margin needs shift"):
        vp.validate_config(dict(BASE, shift_margin=4))
    with pytest.raises(ValueError, match="shift and scale"):
        vp.validate_config(dict(BASE, shift=4, scale="bicubic", dist_height=32, dist_width=32))
    with pytest.raises(ValueError, match="shift and scale"):
        vp.run_ffmpeg_metrics(np.zeros((2, 32, 32, 3), np.uint8), np.zeros((2, 16, 16, 3), np.uint8), "p", "s", "v", scale="bicubic",
                              shift=4)
    with pytest.raises(ValueError, match="shift must be"):
        vp.run_ffmpeg_metrics(np.zeros((2, 32, 32, 3), np.uint8), np.zeros((2, 32, 32, 3), np.uint8), "p", "s", "v", shift=17)
    with pytest.raises(ValueError, match="shift_margin must be"):
        vp.run_ffmpeg_metrics(np.zeros((2, 32, 32, 3), np.uint8), np.zeros((2, 32, 32, 3), np.uint8), "p", "s", "v", shift=4,
                              shift_margin=2)
    for bad in (0, 17):
        with pytest.raises(ValueError, match="radius"):
            vp.frame_shift(np.zeros((2, 40, 40), np.uint8), np.zeros((2, 40, 40), np.uint8), "gray", radius=bad)
    with pytest.raises(ValueError, match="window"):
        vp.frame_shift(np.zeros((2, 40, 40), np.uint8), np.zeros((2, 40, 40), np.uint8), "gray", window=0)


HAND = {"shift": (2, -1), "per_frame": [(2, -1), (2, -1), (0, 0)], "frames_off": 1, "edge": False, "sse_given": 3000,
        "sse_shifted": 30, "psnr_gain": 20.0, "subpixel": (0.0, 0.0)}


def test_the_log_and_the_row_from_a_hand_made_result(tmp_path, caplog):
    from rtvqa_amd import align as A
    with caplog.at_level(logging.WARNING):
        extra = vp.shift_extra(HAND, 4)
    assert list(extra) == list(S.SHIFT_KEYS) == ["SHIFT_RADIUS", "SHIFT_DY", "SHIFT_DX", "SHIFT_FRAMES_OFF", "SHIFT_PSNR_GAIN"]
    assert list(extra.values()) == [4, 2, -1, 1, 20.0]
    assert any("not in place" in r.getMessage() and "NOT moved" in r.getMessage() for r in caplog.records)
    caplog.clear()
    with caplog.at_level(logging.WARNING):
        quiet = vp.shift_extra(dict(HAND, shift=(0, 0), frames_off=0, psnr_gain=0.0), 4)
    assert not caplog.records and list(quiet.values()) == [4, 0, 0, 0, 0.0]
    with caplog.at_level(logging.WARNING):
        vp.shift_extra(dict(HAND, shift=(0, 4), edge=True), 4)
    assert any("border" in r.getMessage() for r in caplog.records)
    log = str(tmp_path / "v.json")
    vp.write_vif_log(log, extra=extra)
    doc = json.load(open(log))
    assert list(doc) == ["frames", "pooled_metrics"] + list(S.SHIFT_KEYS) and doc["SHIFT_PSNR_GAIN"] == 20.0
    row = vp.extract_metrics_from_logs("absent", "absent", log, "x", 23, 0, "8x8", 30.0)
    assert list(row)[-5:] == list(S.SHIFT_KEYS) and [row[k] for k in S.SHIFT_KEYS] == [4, 2, -1, 1, 20.0]
    # both pre-passes: the ALIGN_* group, then the SHIFT_* group
    both = dict(A.log_keys({"offset": 0, "dropped": 1, "repeated": 0, "psnr_gain": 3.0}, 8), **extra)
    vp.write_vif_log(log, extra=both)
    row = vp.extract_metrics_from_logs("absent", "absent", log, "x", 23, 0, "8x8", 30.0)
    assert list(row)[-10:] == list(A.ALIGN_KEYS) + list(S.SHIFT_KEYS)
    # a log without the keys gives the row it gave
    vp.write_vif_log(log)
    assert not any(k.startswith("SHIFT") for k in vp.extract_metrics_from_logs("absent", "absent", log, "x", 23, 0, "8x8", 30.0))
