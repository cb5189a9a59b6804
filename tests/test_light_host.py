"""Host: the library's PQ table and gamut matrices (no ctx, no GPU) against the restatement of tests/light_reference.py and the
pinned entries of the header; the restatement on frames worked out by hand; the false-positive condition the two gamut constants
were chosen by; the pure-host reader rtvqa_amd.light on hand-made records; the key order of the log and the row; the config keys;
the additive ABI.  No GPU."""
import ctypes as C
import json
import logging
import os
import re
import subprocess

import numpy as np
import pytest

import itp_reference as IR
import light_cases as LC
import light_reference as LR
from rtvqa_amd import _native as N
from rtvqa_amd import engine as E
from rtvqa_amd import light as L
from rtvqa_amd import video_processing as vp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tables():
    return E.light_table("pq"), E.light_gamut("bt709"), E.light_gamut("p3")


# ---- the table and the matrices -----------------------------------------------------------------------------------------------------------
def test_the_pq_table(tables):
    T = tables[0]
    assert T.dtype == np.uint64 and T.shape == (65536,)
    ref = LR.table_pq()
    assert np.abs(T.astype(np.int64) - ref.astype(np.int64)).max() <= 1          # libm's pow against NumPy's
    assert (T[1:] >= T[:-1]).all()
    assert T[0] == 0 and T[65535] == 10485760000 == 10000 << 20 and int(np.nonzero(T)[0][0]) == 6
    assert int(T[65535]) < N.LIGHT_TABLE_LIMIT == LR.TABLE_LIMIT
    assert E.light_table(N.ITP_PQ).tobytes() == T.tobytes()
    with pytest.raises(ValueError, match="not a per-channel function"):
        E.light_table("hlg")
    for bad in ("sdr", 2, None, True):
        with pytest.raises(ValueError, match="transfer must be 'pq'"):
            E.light_table(bad)
    lib = N.load()
    buf = (C.c_uint64 * 65536)()
    assert lib.vqa_light_table(N.ITP_HLG, buf) == N.VQA_ERR_UNSUPPORTED
    assert lib.vqa_light_table(2, buf) == N.VQA_ERR_INVALID and lib.vqa_light_table(N.ITP_PQ, None) == N.VQA_ERR_INVALID


def test_the_gamut_matrices(tables):
    _, m709, mp3 = tables
    assert m709.dtype == np.int64 and m709.tolist() == LR.INT_709 and mp3.tolist() == LR.INT_P3
    assert LR.gamut_int("bt709").tolist() == LR.INT_709 and LR.gamut_int("p3").tolist() == LR.INT_P3
    assert np.abs(LR.gamut_double("bt709") - np.array(LR.BT2087)).max() <= 5e-5      # BT.2087's four decimals
    assert np.abs(LR.gamut_double("p3") - np.array(LR.P3_4DEC)).max() <= 5e-5
    assert np.abs(m709 / 65536.0 - LR.gamut_double("bt709")).max() <= 2.0 ** -17
    assert np.abs(m709).max() < 1 << 17 and np.abs(mp3).max() < 1 << 17            # the header's overflow bound
    for a in (LR.gamut_double("bt709"), LR.gamut_double("p3")):
        assert np.abs(a.sum(axis=1) - 1.0).max() < 1e-12                           # white stays white
    for bad in ("bt2020", "709", 0, None):
        with pytest.raises(ValueError, match="gamut must be"):
            E.light_gamut(bad)
    lib = N.load()
    m = (C.c_int64 * 9)()
    assert lib.vqa_light_gamut(2, m) == N.VQA_ERR_INVALID and lib.vqa_light_gamut(0, None) == N.VQA_ERR_INVALID


def test_a_bad_table_is_refused(tables):
    T = tables[0]
    assert E.check_light_table(T).tobytes() == T.tobytes()
    dec = T.copy()
    dec[30000] = dec[29999] - 1
    big = T.copy()
    big[65535] = 1 << 34
    for bad in (dec, big, T[::-1].copy(), T[:-1], T.astype(np.int64), T.astype(np.float64)):
        with pytest.raises(ValueError, match="table must"):
            E.check_light_table(bad)
    ok = np.minimum(np.arange(65536, dtype=np.uint64) << 18, np.uint64((1 << 34) - 1))   # flat runs are monotone
    assert E.check_light_table(ok) is not None


# ---- the restatement, by hand -------------------------------------------------------------------------------------------------------------
def test_the_restatement_on_a_flat_frame_by_hand():
    """T[c] = c; 8-bit full-range BGR flat (10, 200, 30): the codes are 257 times the samples"""
    toy = np.arange(65536, dtype=np.uint64)
    n = 16 * 16
    planes = [np.full((16, 16), v) for v in (10, 200, 30)]
    rec, hist = LR.record(planes, 8, IR.BGR, True, toy, LR.INT_709, LR.INT_P3)
    assert rec["max_code"] == [7710, 51400, 2570] and rec["sum_q"] == 51400 * n and rec["pct_bin"] == [51400 >> 4] * 10
    assert rec["sum_y"] == n * ((2627 * 7710 + 6780 * 51400 + 593 * 2570 + 5000) // 10000) and hist[51400 >> 4] == n
    # S = M (7710, 51400, 2570): the red row of BT.709 is 108822 * 7710 - 38512 * 51400 - 4774 * 2570 = -1152768360, negative and
    # beyond 2^-6 of the largest component - but in this table's tiny units it is still above the floor of -2^32: inside
    s_red = 108822 * 7710 - 38512 * 51400 - 4774 * 2570
    assert s_red == -1152768360 and s_red < -((51400 << 16) >> 6) and not s_red < -((51400 << 16) >> 6) - (1 << 32)
    assert rec["out_709"] == 0 and rec["out_p3"] == 0 and rec["clamped"] == 0
    # T[c] = c 2^18 scales S by 2^18 and leaves the floor where it was: now outside both (P3's red row: -281993250 2^18)
    big = np.arange(65536, dtype=np.uint64) << np.uint64(18)
    assert (s_red << 18) < -(((51400 << 18) << 16) >> 6) - (1 << 32)
    assert (88053 * 7710 - 18493 * 51400 - 4024 * 2570) == -281993250
    rec, _ = LR.record(planes, 8, IR.BGR, True, big, LR.INT_709, LR.INT_P3)
    assert rec["out_709"] == n and rec["out_p3"] == n and rec["sum_q"] == (51400 << 18) * n


def test_the_restatement_on_a_two_level_frame_and_the_rank_rule():
    """10-bit limited 4:4:4, neutral chroma: Y = 64 is black (code 0), Y = 940 is peak white (code 65535)"""
    T = LR.table_pq()
    y = np.full((16, 16), 64)
    y[0, :3] = 940                                    # 3 of 256 pixels
    c = np.full((16, 16), 512)
    rec, hist = LR.record([y, c, c], 10, IR.YUV2020, False, T, LR.INT_709, LR.INT_P3)
    assert rec["max_code_rgb"] == 65535 and rec["min_code_rgb"] == 0 and rec["max_nits"] == 10000.0 and rec["min_nits"] == 0.0
    assert rec["sum_q"] == 3 * 10485760000 and rec["avg_nits"] == 30000.0 / 256 and hist[0] == 253 and hist[4095] == 3
    # ranks per ten thousand of 256: 99 % is k = 254 (the first white pixel), 95 % is k = 244 (black)
    assert [(p * 256 + 9999) // 10000 for p in (9500, 9900, 9998)] == [244, 254, 256]
    assert rec["pct_bin"] == [0] * 8 + [4095, 4095] and rec["out_709"] == 0 and rec["out_p3"] == 0
    # Y below black is clamped and counted; chroma far off neutral on black too
    y2 = np.full((16, 16), 64)
    y2[5, 5] = 0
    assert LR.record([y2, c, c], 10, IR.YUV2020, False, T, LR.INT_709, LR.INT_P3)[0]["clamped"] == 1


def test_the_two_gamut_constants_flag_no_in_gamut_colour_from_ten_bits_on(tables):
    """the condition the constants were chosen by: in-gamut BT.709 and P3 colours, saturated primaries included, at 1e-4 .. 1 of
    1000 cd/m2, through 10- and 12-bit limited-range Y'CbCr, are never outside their gamut; pure BT.2020 primaries at 5 cd/m2
    and more are outside both; red at 0.5 cd/m2 is hidden by the floor"""
    T, m709, mp3 = tables
    for name, field in (("bt709", ("out_709", "out_p3")), ("p3", ("out_p3",))):
        lin = LC.in_gamut_colours(name, 200 * 200, seed=4)
        for depth in (10, 12):
            planes = [p.reshape(200, 200) for p in LR.encode_2020(lin, depth)]
            rec, _ = LR.record(planes, depth, IR.YUV2020, False, T, m709, mp3)
            for f in field:
                assert rec[f] == 0, (name, depth, f, rec[f])
        planes = [p.reshape(200, 200) for p in LR.encode_2020(lin, 8)]
        assert LR.record(planes, 8, IR.YUV2020, False, T, m709, mp3)[0][field[0]] > 0     # at 8 bits quantisation alone crosses it
    n = 16 * 16
    for nits in (5.0, 100.0, 1000.0):
        for ch in (0, 1):
            v = np.zeros((16, 16, 3))
            v[..., ch] = nits
            rec, _ = LR.record(LR.encode_2020(v, 10), 10, IR.YUV2020, False, T, m709, mp3)
            assert rec["out_709"] == n and rec["out_p3"] == n, (nits, ch)
    v = np.zeros((16, 16, 3))
    v[..., 0] = 0.5
    rec, _ = LR.record(LR.encode_2020(v, 10), 10, IR.YUV2020, False, T, m709, mp3)
    assert rec["out_709"] == 0 and rec["out_p3"] == 0


# ---- light.py on hand-made records --------------------------------------------------------------------------------------------------------
def _rec(max_nits, avg_nits, p9998, y_avg, count=100, out_709=0, out_p3=0, clamped=0):
    return {"max_nits": max_nits, "avg_nits": avg_nits, "pct_nits": [0.0] * 9 + [p9998], "y_avg": y_avg, "count": count,
            "out_709": out_709, "out_p3": out_p3, "clamped": clamped}


def test_summarise():
    recs = [_rec(400.0, 50.0, 390.0, 40.0, out_709=10), _rec(1000.0, 30.0, 700.0, 20.0, count=300, out_p3=3),
            _rec(1000.0, 80.0, 650.0, 60.0, clamped=5)]
    s = L.summarise(recs)
    assert list(s) == list(L.LIGHT_KEYS) == ["LIGHT_MAXCLL", "LIGHT_MAXFALL", "LIGHT_MAXCLL_FRAME", "LIGHT_P9998", "LIGHT_Y_AVG",
                                            "LIGHT_OUT_709", "LIGHT_OUT_P3", "LIGHT_CLAMPED"]
    assert s == {"LIGHT_MAXCLL": 1000.0, "LIGHT_MAXFALL": 80.0, "LIGHT_MAXCLL_FRAME": 1, "LIGHT_P9998": 700.0, "LIGHT_Y_AVG": 40.0,
                 "LIGHT_OUT_709": 10 / 500, "LIGHT_OUT_P3": 3 / 500, "LIGHT_CLAMPED": 5 / 500}
    assert L.check(s) is s
    arr = np.zeros(2, E.LIGHT_DTYPE)                       # the engine's records work the same
    arr["count"] = 64
    arr["max_nits"] = [5.0, 7.0]
    arr["avg_nits"] = [1.0, 0.5]
    arr["pct_nits"][:, 9] = [4.0, 6.0]
    arr["out_709"] = [64, 0]
    assert L.summarise(arr) == {"LIGHT_MAXCLL": 7.0, "LIGHT_MAXFALL": 1.0, "LIGHT_MAXCLL_FRAME": 1, "LIGHT_P9998": 6.0,
                                "LIGHT_Y_AVG": 0.0, "LIGHT_OUT_709": 0.5, "LIGHT_OUT_P3": 0.0, "LIGHT_CLAMPED": 0.0}
    with pytest.raises(ValueError):
        L.summarise([])
    with pytest.raises(ValueError, match="above 10000"):                 # MaxCLL above 10000 is impossible
        L.check(dict(s, LIGHT_MAXCLL=10000.5))
    with pytest.raises(ValueError, match="MaxFALL"):                     # a MaxFALL above MaxCLL is a bug
        L.check(dict(s, LIGHT_MAXFALL=1000.5))


# ---- the log and the row ------------------------------------------------------------------------------------------------------------------
SUMMARY = {"LIGHT_MAXCLL": 1000.0, "LIGHT_MAXFALL": 80.5, "LIGHT_MAXCLL_FRAME": 1, "LIGHT_P9998": 700.0, "LIGHT_Y_AVG": 40.25,
           "LIGHT_OUT_709": 0.02, "LIGHT_OUT_P3": 0.0, "LIGHT_CLAMPED": 0.0}


def test_the_log_and_the_row_from_a_hand_made_summary(tmp_path, caplog):
    from rtvqa_amd import align as A
    from rtvqa_amd import shift as S
    with caplog.at_level(logging.WARNING):
        extra = vp.light_extra(SUMMARY)
    assert list(extra) == list(L.LIGHT_KEYS) and extra == SUMMARY and not caplog.records
    assert isinstance(extra["LIGHT_MAXCLL_FRAME"], int) and isinstance(extra["LIGHT_OUT_P3"], float)
    with caplog.at_level(logging.WARNING):
        vp.light_extra(dict(SUMMARY, LIGHT_CLAMPED=0.25))
    assert any("clamped" in r.getMessage() for r in caplog.records)
    with pytest.raises(ValueError, match="MaxFALL"):
        vp.light_extra(dict(SUMMARY, LIGHT_MAXFALL=2000.0))
    log = str(tmp_path / "v.json")
    vp.write_vif_log(log, extra=extra)
    doc = json.load(open(log))
    assert list(doc) == ["frames", "pooled_metrics"] + list(L.LIGHT_KEYS) and doc["LIGHT_MAXFALL"] == 80.5
    row = vp.extract_metrics_from_logs("absent", "absent", log, "x", 23, 0, "8x8", 30.0)
    assert list(row)[-8:] == list(L.LIGHT_KEYS) and [row[k] for k in L.LIGHT_KEYS] == list(SUMMARY.values())
    # with both other pre-passes: LIGHT_*, then ALIGN_*, then SHIFT_* - those stay the last columns
    al = A.log_keys({"offset": 0, "dropped": 1, "repeated": 0, "psnr_gain": 3.0}, 8)
    sh = S.log_keys({"shift": (2, -1), "frames_off": 1, "psnr_gain": 20.0}, 4)
    vp.write_vif_log(log, extra=dict(dict(extra, **al), **sh))
    assert list(json.load(open(log)))[2:] == list(L.LIGHT_KEYS) + list(A.ALIGN_KEYS) + list(S.SHIFT_KEYS)
    row = vp.extract_metrics_from_logs("absent", "absent", log, "x", 23, 0, "8x8", 30.0)
    assert list(row)[-18:] == list(L.LIGHT_KEYS) + list(A.ALIGN_KEYS) + list(S.SHIFT_KEYS)
    assert list(row)[-10:] == list(A.ALIGN_KEYS) + list(S.SHIFT_KEYS)
    # the order in the log does not decide the row's: the light group goes first wherever the keys stand
    vp.write_vif_log(log, extra=dict(dict(sh, **al), **extra))
    row = vp.extract_metrics_from_logs("absent", "absent", log, "x", 23, 0, "8x8", 30.0)
    assert list(row)[-18:] == list(L.LIGHT_KEYS) + list(A.ALIGN_KEYS) + list(S.SHIFT_KEYS)
    # a log without the keys gives the row and the file it gave
    vp.write_vif_log(log)
    plain = open(log, "rb").read()
    assert not any(k.startswith("LIGHT") for k in vp.extract_metrics_from_logs("absent", "absent", log, "x", 23, 0, "8x8", 30.0))
    vp.write_vif_log(log, extra=None)
    assert open(log, "rb").read() == plain and b"LIGHT" not in plain
    vp.write_vif_log(log, extra=al)
    assert list(json.load(open(log)))[2:] == list(A.ALIGN_KEYS)


# ---- the request and the config keys ------------------------------------------------------------------------------------------------------
BASE = {"crf": 23, "resize_width": 64, "resize_height": 64, "frame_interval": 1}


def test_the_request_and_the_config_keys():
    assert vp._light_request(False) is None and vp._light_request(True) == ("pq", False)
    assert vp._light_request(True, "pq", True) == ("pq", True) and vp._light_request(np.bool_(True), "pq", np.bool_(False)) == ("pq", False)
    assert vp._light_config(dict(BASE)) is None and vp._light_config(dict(BASE, light=True, light_range="full")) == ("pq", True)
    for ok in (dict(light=True), dict(light=False), dict(light=True, light_transfer="pq", light_range="limited"),
               dict(light=True, align=8, shift=4), dict(light_range="full"), dict(light=True, scale="bicubic", dist_height=32,
                                                                               dist_width=32)):
        vp.validate_config(dict(BASE, **ok))
    for bad in (1, 0, "true", None, [True]):
        with pytest.raises(ValueError, match="light must be true or false"):
            vp.validate_config(dict(BASE, light=bad))
    for on in (True, False):                                   # the parameters are validated whether light is on or not
        with pytest.raises(ValueError, match="not a per-channel function"):
            vp.validate_config(dict(BASE, light=on, light_transfer="hlg"))
        for bad in ("sdr", 0, None, True):
            with pytest.raises(ValueError, match="light_transfer must be 'pq'"):
                vp.validate_config(dict(BASE, light=on, light_transfer=bad))
        for bad in ("tv", 0, None, True, "Full"):
            with pytest.raises(ValueError, match='light_range must be "limited" or "full"'):
                vp.validate_config(dict(BASE, light=on, light_range=bad))
    z = np.zeros((2, 32, 32, 3), np.uint8)
    with pytest.raises(ValueError, match="not a per-channel function"):
        vp.run_ffmpeg_metrics(z, z, "p", "s", "v", light=True, light_transfer="hlg")
    with pytest.raises(ValueError, match="light_full_range must be true or false"):
        vp.run_ffmpeg_metrics(z, z, "p", "s", "v", light=True, light_full_range="full")
    with pytest.raises(ValueError, match="light must be true or false"):
        vp.run_ffmpeg_metrics(z, z, "p", "s", "v", light=1)
    with pytest.raises(ValueError, match="three planes"):                          # one-plane layouts
        vp.frame_light(np.zeros((2, 32 * 32), np.uint8), "gray", 32, 32)
    with pytest.raises(ValueError, match="not a per-channel function"):
        vp.frame_light(np.zeros((2, 32 * 32 * 3 // 2), np.uint8), "yuv420p", 32, 32, transfer="hlg")
    with pytest.raises(ValueError, match="window"):
        vp.frame_light(np.zeros((2, 32 * 32 * 3 // 2), np.uint8), "yuv420p", 32, 32, window=0)
    import inspect
    args = inspect.signature(vp.run_ffmpeg_metrics).parameters
    assert (args["light"].default, args["light_transfer"].default, args["light_full_range"].default) == (False, "pq", False)
    from rtvqa_amd import stream
    assert "light" not in [k.name for k in stream.PLANE_KINDS]                    # a pre-pass, not a row of the table


# ---- the additive ABI ---------------------------------------------------------------------------------------------------------------------
def test_the_additive_abi():
    assert N.VQA_ABI_VERSION == 8
    assert (N.K_SILL, N.K_LIGHT_ACCUM, N.K_LIGHT_SCAN, N.K_LINTEL) == (71, 72, 73, 74)
    assert N.K_IDS_NEWEST == N.K_IDS_LATEST + (72, 73) and 71 not in N.K_IDS_NEWEST and 74 not in N.K_IDS_NEWEST
    assert C.sizeof(N.VqaLightMetrics) == 280 == E.LIGHT_DTYPE.itemsize
    assert E.LIGHT_DTYPE.names == tuple(f[0] for f in N.VqaLightMetrics._fields_)
    assert N.LIGHT_PERCENTILES == LR.PERCENTILES and N.LIGHT_BINS == LR.BINS == 4096
    assert (N.LIGHT_GAMUT_REL_SHIFT, N.LIGHT_GAMUT_FLOOR) == (LR.REL_SHIFT, LR.FLOOR) == (6, 1 << 32)
    txt = open(os.path.join(REPO, "include", "vqa.h")).read()
    for name, val in (("VQA_K_SILL", 71), ("VQA_K_LIGHT_ACCUM", 72), ("VQA_K_LIGHT_SCAN", 73), ("VQA_K_LINTEL", 74)):
        assert re.search(r"%s\s*=\s*%d\b" % (name, val), txt), name
    assert re.search(r"#define VQA_ABI_VERSION\s+8", txt) and re.search(r"#define VQA_LIGHT_GAMUT_REL_SHIFT\s+6", txt)
    assert re.search(r"#define VQA_LIGHT_GAMUT_FLOOR\s+4294967296LL", txt) and re.search(r"#define VQA_LIGHT_BINS\s+4096", txt)
    part = txt[txt.index("---- HDR light levels and gamut QC"):]
    part = part[:part.index("VQA_API int vqa_light_gamut")]
    for word in ("MaxCLL", "MaxFALL", "CTA-861.3", "not compared with any tool", "ONE stream", "rint(min(max(E', 0), 1) 65535)",
                 "THE ONLY ROUNDING", "clamped", "TRAVELS WITH THE CALL", "non-decreasing", "T[65535] < 2^34", "10485760000",
                 "code 6", "VQA_ERR_UNSUPPORTED", "(2627 qR + 6780 qG + 593 qB + 5000) / 10000", "(0.3127, 0.3290)", "(0.708, 0.292)",
                 "(0.680,", "BT.2087", "VQA_LIGHT_GAMUT_REL_SHIFT) - VQA_LIGHT_GAMUT_FLOOR", "2^-4 cd/m2", "FROM 10 BITS ON",
                 "half a cd/m2", "|S_k| < 3 2^51", "2^62", "(p N + 9999) / 10000", "9998", "LOWER EDGE", "256 MiB", "16384 frames",
                 "k_light_accum", "k_light_scan", "VQA_ERR_STATE", "Not built", "HLG", "ST 2094-40", "letterbox"):
        assert word in part, word
    lib = N.load()
    lib.vqa_kernel_name.restype = C.c_char_p
    assert lib.vqa_kernel_name(72) == b"k_light_accum" and lib.vqa_kernel_name(73) == b"k_light_scan"
    assert lib.vqa_kernel_name(71) == b"?" and lib.vqa_kernel_name(74) == b"?" and lib.vqa_kernel_name(70) == b"k_shift"
    assert lib.vqa_light_submit(None, None, 0, 0, 0, None, 0, 0, 0, None, 0) == N.VQA_ERR_INVALID
    assert lib.vqa_light_wait(None, None, 0, None) == N.VQA_ERR_INVALID
    for k in (71, 74):
        assert lib.vqa_profile_read(None, k, None, None, 0) == N.VQA_ERR_INVALID
    for path in (N.LIB_PATH, N.LAB_LIB_PATH):
        assert all(hasattr(C.CDLL(path), f) for f in ("vqa_light_submit", "vqa_light_wait", "vqa_light_table", "vqa_light_gamut"))
    kern = open(os.path.join(os.path.dirname(N.LIB_PATH), "k_light.hip")).read()
    hpp = open(os.path.join(os.path.dirname(N.LIB_PATH), "vqa_kernels.hpp")).read()
    assert re.search(r"LIGHT_WALK = %d;" % N.LIGHT_WALK, hpp) and re.search(r"LIGHT_SUB_FRAMES = %d;" % N.LIGHT_SUB_FRAMES, hpp)
    assert "Range" in kern and "pow(" not in kern[:kern.index("light_table_host")]   # no transcendental in the kernels
    mk = open(os.path.join(os.path.dirname(N.LIB_PATH), "Makefile")).read()
    assert re.search(r"FP_k_light := -ffp-contract=off", mk)                        # equality needs every operation rounded once


def test_the_header_to_the_c_compiler(tmp_path, tables):
    src = ('#include <stdio.h>\n#include <stdlib.h>\n#include "vqa.h"\n'
           'int (*submit)(vqa_ctx *, const uint8_t *, int, int, int64_t, const vqa_plane_desc *, int, int, int, const uint64_t *, int) '
           '= vqa_light_submit;\n'
           'int (*wait_)(vqa_ctx *, vqa_light_metrics *, int, uint32_t *) = vqa_light_wait;\n'
           'int main(void){uint64_t *t = malloc(65536 * sizeof *t); int64_t m[9]; int a = vqa_light_table(VQA_ITP_PQ, t);\n'
           'int b = vqa_light_gamut(VQA_LIGHT_GAMUT_709, m), c = vqa_light_table(VQA_ITP_HLG, t);\n'
           'printf("%zu %d %d %d %d %d %d %d %d %llu %lld %lld\\n", sizeof(vqa_light_metrics), VQA_K_LIGHT_ACCUM, VQA_K_LIGHT_SCAN, '
           'VQA_K_LINTEL, VQA_LIGHT_PERCENTILES, VQA_LIGHT_BINS, a, b, c, (unsigned long long)t[65535], (long long)m[0], '
           '(long long)VQA_LIGHT_GAMUT_FLOOR); return submit == 0 || wait_ == 0;}\n')
    (tmp_path / "a.c").write_text(src)
    lib_dir = os.path.dirname(N.LIB_PATH)
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), "-o", str(tmp_path / "a"), str(tmp_path / "a.c"),
                           "-L", lib_dir, "-l:" + os.path.basename(N.LIB_PATH), "-Wl,-rpath," + lib_dir,
                           "-Wl,--allow-shlib-undefined"])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "a")]).decode().split()]
    assert got == [280, 72, 73, 74, 10, 4096, 0, 0, N.VQA_ERR_UNSUPPORTED, 10485760000, 108822, 1 << 32]
