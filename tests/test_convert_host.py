"""Convert on the host: the restatement's taps against torch (bilinear interpolation, average pooling) by equality times 16,
hand-computed answers for left siting, odd sizes and the clamped edges, the four consequences include/vqa.h states, the
refusals of check_convert_planes and of the request parser, and the additive ABI."""
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

import convert_cases as CC
import convert_reference as R
from rtvqa_amd import _native as N
from rtvqa_amd import stream
from rtvqa_amd import video_processing as vp
from rtvqa_amd.engine import (CONVERT_CHROMA, CONVERT_RANGE, CONVERT_SITING, check_convert_planes, convert_options, mono_planes,
                              yuv_planes)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEPTHS = tuple(range(8, 17))


def v16(s, dh, dw, chroma="linear", siting="center"):
    """the exact value with denominator 16, before the depth step"""
    s = np.asarray(s, np.int64)
    return R.taps(R.taps(s, dw, chroma, siting == "left", 1), dh, chroma, False, 0)


# ---- the taps against torch ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", ((8, 8), (9, 13), (16, 24), (21, 10)))
def test_centre_sited_linear_up_is_torch_bilinear_times_16(hw):
    import torch
    import torch.nn.functional as F
    s = np.random.default_rng(hw[0]).integers(0, 65536, hw)
    want = F.interpolate(torch.tensor(s, dtype=torch.float64)[None, None], scale_factor=2, mode="bilinear", align_corners=False)[0, 0]
    got = v16(s, 2 * hw[0], 2 * hw[1])
    assert (torch.tensor(got, dtype=torch.float64) == want * 16).all()
    # n_d = 2 n_s - 1 is the same picture without its last row and column
    assert (v16(s, 2 * hw[0] - 1, 2 * hw[1] - 1) == got[:-1, :-1]).all()
    # one axis alone: the other is `same`, whose weight is 4
    assert (v16(s, hw[0], 2 * hw[1])[:, ::1] == R.taps(s.astype(np.int64), 2 * hw[1], "linear", False, 1) * 4).all()


@pytest.mark.parametrize("hw", ((8, 8), (10, 14), (16, 24)))
@pytest.mark.parametrize("chroma", CC.FILTERS[:2])
def test_down_on_even_sizes_is_torch_avg_pool_times_16(hw, chroma):
    import torch
    import torch.nn.functional as F
    s = np.random.default_rng(hw[1]).integers(0, 65536, hw)
    want = F.avg_pool2d(torch.tensor(s, dtype=torch.float64)[None, None], 2)[0, 0]
    got = v16(s, hw[0] // 2, hw[1] // 2, *chroma)
    assert (torch.tensor(got, dtype=torch.float64) == want * 16).all()


def test_box_up_replicates_and_box_is_siting_blind():
    s = np.arange(12).reshape(3, 4) * 7 + 1
    assert (v16(s, 6, 8, "box") == 16 * np.repeat(np.repeat(s, 2, 0), 2, 1)).all()
    assert (v16(s, 5, 7, "box", "left") == 16 * np.repeat(np.repeat(s, 2, 0), 2, 1)[:5, :7]).all()


# ---- by hand ---------------------------------------------------------------------------------------------------------------
def test_hand_answers_per_axis():
    s = np.array([[10, 20, 40, 80]], np.int64)
    one = lambda n_d, chroma, left: R.taps(s, n_d, chroma, left, 1)[0].tolist()
    # up, centre-sited: even x leans on the left neighbour, odd x on the right one; both ends replicate
    assert one(8, "linear", False) == [3 * 10 + 10, 3 * 10 + 20, 3 * 20 + 10, 3 * 20 + 40, 3 * 40 + 20, 3 * 40 + 80, 3 * 80 + 40, 3 * 80 + 80]
    assert one(7, "linear", False) == one(8, "linear", False)[:7]                      # n_d = 2 n_s - 1
    # up, left-sited: even x sits on the sample, odd x halfway to the next; the last one replicates
    assert one(8, "linear", True) == [40, 2 * 10 + 2 * 20, 80, 2 * 20 + 2 * 40, 160, 2 * 40 + 2 * 80, 320, 2 * 80 + 2 * 80]
    assert one(7, "linear", True) == one(8, "linear", True)[:7]
    # down
    assert one(2, "linear", False) == one(2, "box", False) == one(2, "box", True) == [2 * 10 + 2 * 20, 2 * 40 + 2 * 80]
    assert one(2, "linear", True) == [10 + 2 * 10 + 20, 20 + 2 * 40 + 80]              # s[c(-1)] is s[0]
    # down from an odd n_s: the last cell has one sample, read twice
    t = np.array([[10, 20, 40, 80, 7]], np.int64)
    assert R.taps(t, 3, "box", False, 1)[0].tolist() == [60, 240, 2 * 7 + 2 * 7]
    assert R.taps(t, 3, "linear", True, 1)[0].tolist() == [10 + 2 * 10 + 20, 20 + 2 * 40 + 80, 80 + 2 * 7 + 7]
    # same
    assert one(4, "linear", True) == [40, 80, 160, 320]
    with pytest.raises(ValueError):
        R.relation(4, 6)
    assert [R.relation(*p) for p in ((5, 5), (5, 10), (5, 9), (9, 5), (10, 5))] == ["same", "up", "up", "down", "down"]


def test_hand_answers_two_axes_and_the_one_rounding():
    # vertical is centre-sited whatever the siting: 4:2:0 -> 4:4:4 of a 2 x 2 chroma plane, left-sited
    s = np.array([[0, 16], [32, 64]], np.int64)
    hz = np.array([[0, 32, 64, 64], [128, 192, 256, 256]])                               # left-sited rows, times 4
    want = np.stack([3 * hz[0] + hz[0], 3 * hz[0] + hz[1], 3 * hz[1] + hz[0], 3 * hz[1] + hz[1]])
    assert (v16(s, 4, 4, "linear", "left") == want).all()
    # ONE rounding: v = 3 * 4 * 1 + 4 * 0 ... take v = 8 (half) and v = 7
    assert R.round_v([7, 8, 23, 24], 8, 8, "limited").tolist() == [0, 1, 1, 2]
    assert R.round_v([16 * 16, 16 * 235], 8, 10, "limited").tolist() == [64, 940]
    assert R.round_v([16 * 64 + 16 * 2, 16 * 64 + 16 * 2 - 1, 16 * 940], 10, 8, "limited").tolist() == [17, 16, 235]
    assert R.round_v([0, 16 * 255, 16 * 128], 8, 10, "full").tolist() == [0, 1023, (2 * 16 * 128 * 1023 + 16 * 255) // (32 * 255)]
    assert R.round_v([16 * 65535], 10, 8, "limited").tolist() == [255]                     # above Ps on the way in: only the output is clipped
    assert R.round_v([16 * 65535], 16, 8, "full").tolist() == [255]


# ---- the header's consequences, exhaustively ---------------------------------------------------------------------------------
@pytest.mark.parametrize("range", CONVERT_RANGE)
def test_equal_formats_are_the_identity_and_round_trips_return_every_code(range):
    for ds in DEPTHS:
        codes = np.arange(1 << ds, dtype=np.int64)
        assert (R.round_v(16 * codes, ds, ds, range) == codes).all()
        for dd in DEPTHS:
            if dd < ds:
                continue
            up = R.round_v(16 * codes, ds, dd, range)
            assert up.max() <= (1 << dd) - 1
            assert (R.round_v(16 * up, dd, ds, range) == codes).all(), (ds, dd)
    # through the whole function, at an unchanged layout
    s = np.random.default_rng(1).integers(0, 1 << 10, (9, 11))
    for chroma, siting in CC.FILTERS:
        assert (R.convert_plane(s, 9, 11, 10, 10, chroma, siting, range) == s).all()


@pytest.mark.parametrize("range", CONVERT_RANGE)
def test_flat_stays_flat_and_full_maps_the_range_ends(range):
    for ds in DEPTHS:
        ps = (1 << ds) - 1
        for dd in DEPTHS:
            pd = (1 << dd) - 1
            levels = np.unique(np.concatenate([np.arange(min(ps + 1, 300)), np.arange(max(ps - 300, 0), ps + 1)]))
            want = R.round_v(16 * levels, ds, dd, range)
            if range == "full":
                assert want[0] == 0 and want[-1] == pd
            for level, out in zip(levels[[0, 1, len(levels) // 2, -2, -1]], want[[0, 1, len(levels) // 2, -2, -1]]):
                flat = np.full((9, 10), level)
                for (dh, dw), (chroma, siting) in ((hw, f) for hw in ((9, 10), (18, 20), (17, 19), (5, 5), (9, 20), (5, 10)) for f in CC.FILTERS):
                    got = R.convert_plane(flat, dh, dw, ds, dd, chroma, siting, range)
                    assert (got == out).all(), (ds, dd, level, dh, dw, chroma, siting)


def test_the_thinned_cases_hold_every_combination_at_an_odd_and_an_even_size():
    seen = {}
    for hw, cs, cd, ds, dd, chroma, siting, _range, _pads in CC.CASES:
        key = (CC.relations(cs, cd), (chroma, siting), (ds > 8, dd > 8))
        seen.setdefault(key, set()).add((hw[0] % 2, hw[1] % 2) != (0, 0))
    # the nine ordered pairs of 4:2:0 / 4:2:2 / 4:4:4 give seven pairs of relations; (up, down) and (down, up) need planes that
    # no layout has: CC.MIXED builds them by hand
    for c in CC.MIXED:
        key = (c[1], (c[4], c[5]), (c[2] > 8, c[3] > 8))
        seen.setdefault(key, set()).add((c[0][0] % 2, c[0][1] % 2) != (0, 0))
    rel = ("same", "up", "down")
    for rx in rel:
        for ry in rel:
            for f in CC.FILTERS:
                for t in ((False, False), (False, True), (True, False), (True, True)):
                    assert seen.get(((rx, ry), f, t)) == {False, True}, (rx, ry, f, t)
    assert {c[0] for c in CC.CASES} == set(CC.SIZES) and {c[7] for c in CC.CASES} == set(CC.RANGES)
    assert {(c[3], c[4]) for c in CC.CASES} == set(CC.DEPTH_PAIRS)
    assert len(CC.CASES) == 10 * 8 * 3 * 2


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_check_convert_planes_and_options():
    check_convert_planes(yuv_planes(48, 64, "422", 10), yuv_planes(48, 64, "420", 8))
    check_convert_planes(yuv_planes(17, 33, "420", 8), yuv_planes(17, 33, "444", 16))
    check_convert_planes(mono_planes(16, 16), mono_planes(16, 16, 12))
    assert (CONVERT_CHROMA, CONVERT_SITING, CONVERT_RANGE) == (("box", "linear"), ("center", "left"), ("limited", "full"))
    assert convert_options() == (N.CHROMA_LINEAR, N.SITING_CENTER, N.RANGE_LIMITED) == (1, 0, 0)
    assert convert_options("box", "left", "full") == (0, 1, 1)
    for bad, message in ((dict(chroma="bicubic"), "convert chroma must be one of"), (dict(siting="top"), "convert siting must be one of"),
                         (dict(range="pc"), "convert range must be one of"), (dict(chroma=1), "convert chroma must be one of")):
        with pytest.raises(ValueError, match=message):
            convert_options(**bad)
    p = yuv_planes(48, 64, "420", 8)
    for a, b, message in ((p, mono_planes(48, 64), "one to four planes and as many on both sides"),
                          (p + p[:2], p + p[:2], "one to four planes and as many on both sides"),
                          (mono_planes(15, 64), mono_planes(15, 64, 10), "at least 16 x 16"),
                          ([(16, 16, 0, 16, 1), (7, 8, 256, 7, 1)], [(16, 16, 0, 16, 1), (7, 8, 256, 7, 1)], "at least 8 x 8"),
                          (mono_planes(64, 64), mono_planes(64, 33, 10), "the same size, twice or half of it per axis"),
                          (mono_planes(64, 64), mono_planes(16, 64, 10), "chroma ratios other than 1 and 2 are not built"),
                          ([p[0], p[1], p[2][:5] + (10,)], p, "share a sample depth")):
        with pytest.raises(ValueError, match=message):
            check_convert_planes(a, b)


BASE = {"crf": 23, "resize_width": 64, "resize_height": 64}
REFUSED = (
    (dict(dist_pixfmt="yuv420p"), "dist_pixfmt needs convert: nothing is converted without being named"),
    (dict(convert="bicubic", dist_pixfmt="yuv420p"), "convert must be \"box\" or \"linear\""),
    (dict(convert="linear", convert_siting="top"), "convert_siting must be \"center\" or \"left\""),
    (dict(convert="linear", convert_range="tv"), "convert_range must be \"limited\" or \"full\""),
    (dict(convert="linear", dist_pixfmt="nv12"), "dist_pixfmt must be null or one of the pixel layouts"),
    (dict(convert="linear", sync=True), "sync and convert do not go together"),
    (dict(convert="linear", align=2), "align and convert do not go together"),
    (dict(convert="linear", shift=2), "shift and convert do not go together"),
    (dict(convert="box", colorfit=True), "colorfit and convert do not go together"),
    (dict(convert="box", conform=True, conform_color="none", shift=2), "shift and convert do not go together"),
    (dict(convert="box", conform=True, colorfit=True), "colorfit and convert do not go together"),
)


@pytest.mark.parametrize("keys,message", REFUSED, ids=[",".join(sorted(k)) + str(i) for i, (k, _m) in enumerate(REFUSED)])
def test_the_request_parser_refuses(keys, message):
    with pytest.raises(ValueError, match=re.escape(message)):
        vp.validate_config(dict(BASE, **keys))
    kw = dict(dict(light=False, light_transfer="pq", light_full_range=False, colorfit=False, scale=None), **keys)
    with pytest.raises(ValueError, match=re.escape(message)):
        vp._requests(kw)


def test_the_request_parser_accepts_and_stays_the_tuple_it_was():
    off = vp._requests({}, config=True)
    assert off == (False, None, None, None, None, False, None) and off.convert is None
    req = vp._requests(dict(BASE, convert="linear", dist_pixfmt="yuv420p", light=True), config=True)
    assert req.convert == ("linear", "center", "limited") and req.lit is not None          # light reads the reference only
    req = vp._requests(dict(BASE, convert="box", convert_siting="left", convert_range="full", scale="bicubic", dist_height=24,
                            dist_width=32), config=True)
    assert req.convert == ("box", "left", "full") and req.scaling
    vp.validate_config(dict(BASE, convert=None, dist_pixfmt=None, convert_siting="left", convert_range="full"))


def _clip(layout, n=2, h=48, w=64, seed=0):
    from rtvqa_amd.frames import frame_samples
    depth = vp.layout_depth(layout)
    rng = np.random.default_rng(seed)
    return rng.integers(0, 1 << depth, (n, frame_samples(h, w, layout))).astype(np.uint16 if depth > 8 else np.uint8)


def test_the_entry_points_refuse_layouts_that_do_not_fit(tmp_path):
    logs = [str(tmp_path / k) for k in ("p.log", "s.log", "v.json")]
    run = lambda ref, dist, **kw: vp.run_ffmpeg_metrics(ref, dist, *logs, height=48, width=64, **kw)
    with pytest.raises(ValueError, match="convert needs streams of different pixel layouts"):
        run(_clip("yuv420p"), _clip("yuv420p"), layout="yuv420p", convert="linear")
    with pytest.raises(ValueError, match="convert needs streams of different pixel layouts"):
        run(_clip("yuv420p"), _clip("yuv420p"), layout="yuv420p", convert="linear", dist_pixfmt="yuv420p")
    with pytest.raises(ValueError, match="mono to or from three planes is not built"):
        run(_clip("gray10le"), _clip("yuv420p"), layout="gray10le", convert="linear", dist_pixfmt="yuv420p")
    with pytest.raises(ValueError, match="mono to or from three planes is not built"):
        run(_clip("yuv420p"), _clip("gray"), layout="yuv420p", convert="box", dist_pixfmt="gray")
    bgr = np.zeros((2, 48, 64, 3), np.uint8)
    with pytest.raises(ValueError, match="packed bgr24 and planar YUV is a colour-matrix question"):
        run(bgr, _clip("yuv420p"), layout="bgr24", convert="linear", dist_pixfmt="yuv420p")
    with pytest.raises(ValueError, match="packed bgr24 and planar YUV is a colour-matrix question"):
        run(_clip("yuv420p"), bgr, layout="yuv420p", convert="linear", dist_pixfmt="bgr24")
    # differing layouts without convert stay the error they were (.y4m files bring their own)
    from rtvqa_amd.frames import write_y4m
    paths = [str(tmp_path / "a.y4m"), str(tmp_path / "b.y4m")]
    write_y4m(paths[0], _clip("yuv422p10le"), 48, 64, pixfmt="yuv422p10le")
    write_y4m(paths[1], _clip("yuv420p"), 48, 64, pixfmt="yuv420p")
    with pytest.raises(ValueError, match="reference and distorted streams must share a pixel layout"):
        vp.run_ffmpeg_metrics(paths[0], paths[1], *logs)
    cfg = dict(BASE, frame_interval=1, batch_size=2, pixfmt="yuv422p10le")
    with pytest.raises(ValueError, match="reference and distorted streams must share a pixel layout"):
        vp.process_video_and_extract_metrics(paths[0], paths[1], cfg, csv_file=str(tmp_path / "r.csv"), encoded_bgr=bgr)
    with pytest.raises(ValueError, match="convert needs streams of different pixel layouts"):
        vp.process_video_and_extract_metrics(paths[1], paths[1], dict(cfg, convert="linear"), csv_file=str(tmp_path / "r.csv"),
                                             encoded_bgr=bgr)


def test_quality_takes_convert_with_dist_planes_alone_or_with_scale():
    ref, dist = yuv_planes(48, 64, "422", 10), yuv_planes(48, 64, "420", 8)
    q = stream.Quality(ref, dist_planes=dist, convert=("linear", "center", "limited"))
    assert q.convert == ("linear", "center", "limited") and q.scale is None and q.mid_planes is ref
    rung = yuv_planes(24, 32, "420", 8)
    q = stream.Quality(ref, dist_planes=rung, scale="bicubic", convert=("box", "left", "full"))
    assert [tuple(p[:2]) for p in q.mid_planes] == [(32, 24), (16, 24), (16, 24)]
    assert {int(p[5]) for p in q.mid_planes} == {10} and q.mid_planes[1][2] == 32 * 24 * 2
    assert "convert" not in vars(stream.Quality(ref))                                       # off: the object it was
    for kw, message in ((dict(convert=("linear", "center", "limited")), "convert needs dist_planes"),
                        (dict(dist_planes=dist), "dist_planes and scale go together"),
                        (dict(dist_planes=dist, convert=("linear", "top", "limited")), "convert siting must be one of"),
                        (dict(dist_planes=dist, convert=("linear", "center")), "convert is a \\(chroma, siting, range\\) tuple"),
                        (dict(dist_planes=yuv_planes(24, 32, "420", 8), convert=("linear", "center", "limited")),
                         "the same size, twice or half of it per axis"),
                        (dict(dist_planes=mono_planes(48, 64), convert=("linear", "center", "limited")), "as many on both sides")):
        with pytest.raises(ValueError, match=message):
            stream.Quality(ref, **kw)
    from rtvqa_amd import conform as CO
    plan = CO.plan(lambda h, w: yuv_planes(h, w, "420", 8), 48, 64, 8, "yuv", shift=(-1, 2))
    with pytest.raises(ValueError, match="convert and conform do not go together"):
        stream.Quality(plan["out_planes"], conform=plan, dist_planes=dist, convert=("linear", "center", "limited"))


# ---- the ABI ---------------------------------------------------------------------------------------------------------------
def test_the_additive_abi():
    assert N.VQA_ABI_VERSION == 8
    txt = open(os.path.join(REPO, "include", "vqa.h")).read()
    assert re.search(r"#define VQA_ABI_VERSION 8\b", txt)
    for name, value in (("VQA_CHROMA_BOX", 0), ("VQA_CHROMA_LINEAR", 1), ("VQA_SITING_CENTER", 0), ("VQA_SITING_LEFT", 1),
                        ("VQA_RANGE_LIMITED", 0), ("VQA_RANGE_FULL", 1)):
        assert re.search(r"%s\s*=\s*%d" % (name, value), txt), name
    assert (N.CHROMA_BOX, N.CHROMA_LINEAR, N.SITING_CENTER, N.SITING_LEFT, N.RANGE_LIMITED, N.RANGE_FULL) == (0, 1, 0, 1, 0, 1)
    assert N.CONVERT_MIN_DIM == 16 and N.CONVERT_MAX_FRAMES == 32768
    # the kernel-id table is what it was: the kind takes no id
    enum = re.search(r"enum vqa_kernel_id \{(.*?)\}", txt, flags=re.S).group(1)
    ids = re.findall(r"VQA_(K_\w+)\s*=\s*(\d+)", enum)
    assert "CONVERT" not in enum and len(ids) == 79 and zlib.crc32(repr(ids).encode()) == 1164667588
    part = txt[txt.index("---- Convert:"):]
    part = part[:part.index("VQA_API int vqa_convert_wait")]
    for word in ("this text is what is built", "3 s[x>>1] + s[c((x>>1) - 1)]", "2 s[x>>1] + 2 s[c((x>>1) + 1)]",
                 "s[c(2x - 1)] + 2 s[2x] + s[c(2x + 1)]", "((v << (dd - ds)) + 8) >> 4", "(v + (1 << (3 + ds - dd))) >> (4 + ds - dd)",
                 "(2 v Pd + 16 Ps) / (32 Ps)", "NOT pinned", "swscale", "never written", "VQA_ABI_VERSION stays", "Not built"):
        assert word in part, word
    for section in ("The resampler:", "---- Conform:"):
        sec = txt[txt.index(section):]
        assert "vqa_convert_submit" in sec[:sec.index("VQA_API")], section               # their Not built lines point here
    lib = N.load()
    assert hasattr(lib, "vqa_convert_submit") and hasattr(lib, "vqa_convert_wait")        # both symbols are exported and bound
    assert lib.vqa_convert_submit.argtypes is not None and len(lib.vqa_convert_submit.argtypes) == 13
    assert lib.vqa_convert_submit(None, None, 0, 0, 0, None, None, 0, None, 0, 0, 0, 0) == N.VQA_ERR_INVALID
    assert lib.vqa_convert_wait(None) == N.VQA_ERR_INVALID


def test_the_header_compiles_under_a_c_compiler(tmp_path):
    src = ('#include <stdio.h>\n#include "vqa.h"\n'
           'int (*submit)(vqa_ctx *, const uint8_t *, int, int, int64_t, const vqa_plane_desc *, uint8_t *, int64_t, '
           'const vqa_plane_desc *, int, int, int, int) = vqa_convert_submit;\n'
           'int (*wait_)(vqa_ctx *) = vqa_convert_wait;\n'
           'int main(void){printf("%d %d %d %d %d %d %d %d\\n", VQA_CHROMA_BOX, VQA_CHROMA_LINEAR, VQA_SITING_CENTER, VQA_SITING_LEFT, '
           'VQA_RANGE_LIMITED, VQA_RANGE_FULL, VQA_ABI_VERSION, wait_(0));return submit == 0 || wait_ == 0;}\n')
    (tmp_path / "s.c").write_text(src)
    lib_dir = os.path.dirname(N.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), "-o", str(tmp_path / "s"),
                           str(tmp_path / "s.c"), "-L", lib_dir, "-l:" + os.path.basename(N.LIB_PATH), "-Wl,-rpath," + lib_dir,
                           "-Wl,--allow-shlib-undefined"])
    assert subprocess.check_output([str(tmp_path / "s")]).decode().split() == ["0", "1", "0", "1", "0", "1", "8", str(N.VQA_ERR_INVALID)]
