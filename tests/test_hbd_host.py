"""9..16-bit and 4:2:2 / 4:4:4 / mono planar frames on the host side (no GPU): Y4M tags, raw streams, plane tuples,
FFmpeg's psnr peak, and the float64 reference of tests/hbd_reference.py checked against the C oracle at 8 bits."""
import ctypes as C

import numpy as np
import pytest

import hbd_reference as ref
from rtvqa_amd import _native as N
from rtvqa_amd import frames
from rtvqa_amd import video_processing as vp
from rtvqa_amd.engine import (gray_planes, mono_planes, plane_descs, planes_depth, yuv420p_planes, yuv_planes)

TAGS = {  # C tag -> (pix_fmt, chroma, depth)
    "420jpeg": ("yuv420p", "420", 8), "422": ("yuv422p", "422", 8), "444": ("yuv444p", "444", 8), "mono": ("gray", "mono", 8),
    "420p10": ("yuv420p10le", "420", 10), "422p10": ("yuv422p10le", "422", 10), "444p10": ("yuv444p10le", "444", 10),
    "420p12": ("yuv420p12le", "420", 12), "422p12": ("yuv422p12le", "422", 12), "444p12": ("yuv444p12le", "444", 12),
    "420p16": ("yuv420p16le", "420", 16), "444p16": ("yuv444p16le", "444", 16),
    "mono10": ("gray10le", "mono", 10), "mono12": ("gray12le", "mono", 12), "mono16": ("gray16le", "mono", 16),
}


def _memmap_base(a):
    b = a
    while b is not None and not isinstance(b, np.memmap):
        b = b.base
    return b


@pytest.mark.parametrize("tag", sorted(TAGS))
def test_y4m_round_trip_every_tag_odd_geometry(tmp_path, tag):
    pixfmt, chroma, depth = TAGS[tag]
    h, w = 13, 21
    ns = frames.frame_samples(h, w, pixfmt)
    assert ns == sum(pw * ph for pw, ph, *_ in yuv_planes(h, w, chroma, depth))
    dt = np.uint16 if depth > 8 else np.uint8
    x = np.random.default_rng(1).integers(0, 1 << depth, (3, ns)).astype(dt)
    p = str(tmp_path / ("c_%s.y4m" % tag))
    frames.write_y4m(p, x, h, w, pixfmt=pixfmt)
    with open(p, "rb") as f:
        assert (b" C%s\n" % tag.encode()) in f.readline()
    assert frames.y4m_pixfmt(p) == pixfmt
    arr, hh, ww, _fps = frames.open_y4m(p)
    assert (hh, ww) == (h, w) and arr.shape == (3, ns) and arr.dtype == dt
    assert isinstance(_memmap_base(arr), np.memmap) and not arr.flags.writeable   # mapped, not read
    assert (arr == x).all()
    # the layout: planes back to back, Y then U then V, little-endian samples
    raw = np.fromfile(p, np.uint8)
    first = raw[raw.tobytes().index(b"FRAME\n") + 6:][:ns * np.dtype(dt).itemsize]
    assert (first.view("<u2" if depth > 8 else np.uint8) == x[0]).all()
    eager = frames.read_y4m(p)[0]
    assert eager.dtype == dt and (eager == x).all()
    # the quality layout the entry point picks from the header, and its planes
    got, layout, gh, gw = vp._open_quality_stream(p, "bgr24", None, None)
    assert layout == pixfmt and (gh, gw) == (h, w) and (got == x).all()
    pl = vp.LAYOUTS[layout][0](h, w)
    assert planes_depth(pl) == depth and sum(q[0] * q[1] for q in pl) == ns


def test_unsupported_y4m_tags_raise(tmp_path):
    for header in (b"YUV4MPEG2 W8 H8 F25:1 Ip C411\n", b"YUV4MPEG2 W8 H8 F25:1 Ip C420p14\n",
                   b"YUV4MPEG2 W8 H8 F25:1 Ip C444alpha\n", b"YUV4MPEG2 W8 H8 F25:1 It C420jpeg\n"):
        p = tmp_path / "bad.y4m"
        p.write_bytes(header + b"FRAME\n" + bytes(200))
        with pytest.raises(ValueError, match="unsupported Y4M colour space|interlaced"):
            frames.open_y4m(str(p))
        with pytest.raises(ValueError):
            frames.read_y4m(str(p))
    with pytest.raises(ValueError, match="unsupported pixfmt"):
        frames.write_y4m(str(tmp_path / "x.y4m"), np.zeros((1, 96), np.uint8), 8, 8, pixfmt="nv12")


def test_raw_yuv_takes_its_format_from_pixfmt(tmp_path):
    h, w = 9, 15
    x = np.random.default_rng(2).integers(0, 1024, (4, frames.frame_samples(h, w, "yuv422p10le"))).astype(np.uint16)
    q = str(tmp_path / "clip.yuv")
    x.tofile(q)
    arr, layout, hh, ww = vp._open_quality_stream(q, "yuv422p10le", h, w)
    assert layout == "yuv422p10le" and (hh, ww) == (h, w) and isinstance(arr, np.memmap) and arr.dtype == np.uint16
    assert (arr == x).all()
    vp.validate_config({"crf": 23, "resize_width": 64, "resize_height": 64, "frame_interval": 10, "pixfmt": "gray16le"})


def test_psnr_peak_follows_the_depth():
    sizes, comps = [(4, 2)], "y"
    assert "psnr_y:60.20" in vp.psnr_stats_lines(1, [[8]], sizes, comps, peak=1023)   # MSE 1 at 10 bits
    for sse in ([[8]], [[0]], [[123457]]):   # peak 255: today's text, byte for byte
        assert vp.psnr_stats_lines(1, sse, sizes, comps, peak=255) == vp.psnr_stats_lines(1, sse, sizes, comps)
    assert "psnr_y:48.13" in vp.psnr_stats_lines(1, [[8]], sizes, comps)
    assert vp.layout_depth("yuv420p10le") == 10 and vp.layout_depth("yuv420p") == 8 and vp.layout_depth("bgr24") == 8


def test_ffmpeg_restatement_matches_the_c_oracle_at_8_bits(oracle):
    """hbd_reference.ssim_ffmpeg at max = 255 (double end formula, unrounded constants) against the C oracle's 8-bit
    vf_ssim (float end formula, constants rounded to integers): the same filter, to 1e-6"""
    rng = np.random.default_rng(3)
    for h, w in ((24, 40), (67, 259), (37, 53)):
        a = rng.integers(0, 256, (h, w), dtype=np.uint8)
        b = np.clip(a.astype(int) + rng.integers(-20, 21, (h, w)), 0, 255).astype(np.uint8)
        for x, y in ((a, b), (a, a), (a, 255 - a)):
            got = ref.ssim_ffmpeg(x.astype(np.int64), y.astype(np.int64), 255)
            want = oracle.ssim_ffmpeg(x, y)
            assert abs(got - want) <= 1e-6 * max(abs(want), 1e-3), (h, w, got, want)
            assert ref.sse(x.astype(np.int64), y.astype(np.int64)) == oracle.sse_plane(x, y)


def test_gauss_restatement_matches_the_c_oracle_at_8_bits(oracle):
    rng = np.random.default_rng(4)
    a = rng.integers(0, 256, (40, 52), dtype=np.uint8)
    b = np.clip(a.astype(int) + rng.integers(-9, 10, a.shape), 0, 255).astype(np.uint8)
    got = ref.ssim_gauss(a.astype(np.int64), b.astype(np.int64), 255)
    assert abs(got - oracle.ssim_gauss(a, b)) <= 1e-6 * abs(got)


def test_plane_tuples_carry_the_depth_into_the_descs():
    # 5-tuples (every builder of ABI 7) -> bit_depth 0
    for pl in (yuv420p_planes(7, 9), gray_planes(7, 9), yuv_planes(7, 9)):
        d = plane_descs(pl)
        assert all(len(p) == 5 for p in pl) and [x.bit_depth for x in d] == [0] * len(pl)
        assert planes_depth(pl) == 8
    assert yuv_planes(7, 9) == yuv420p_planes(7, 9) and mono_planes(7, 9) == gray_planes(7, 9)
    # 6-tuples -> bit_depth, offsets / strides / steps in bytes
    pl = yuv_planes(67, 259, "420", 10)
    assert pl == [(259, 67, 0, 518, 2, 10), (130, 34, 259 * 67 * 2, 260, 2, 10),
                  (130, 34, 259 * 67 * 2 + 130 * 34 * 2, 260, 2, 10)]
    d = plane_descs(pl)
    assert C.sizeof(d) == 3 * C.sizeof(N.VqaPlaneDesc) == 3 * 32
    assert [(x.width, x.height, x.offset, x.row_stride, x.pixel_step, x.bit_depth) for x in d] == pl
    assert [p[:2] for p in yuv_planes(5, 7, "422", 12)] == [(7, 5), (4, 5), (4, 5)]
    assert [p[:2] for p in yuv_planes(5, 7, "444", 16)] == [(7, 5), (7, 5), (7, 5)]
    assert mono_planes(5, 7, 16) == [(7, 5, 0, 14, 2, 16)]
    assert N.VqaPlaneDesc.bit_depth.offset == 28 and N.VQA_ABI_VERSION == 8
    with pytest.raises(ValueError, match="share a sample depth"):
        planes_depth(yuv_planes(8, 8, "420", 10)[:1] + yuv420p_planes(8, 8)[1:])
    with pytest.raises(ValueError):
        yuv_planes(8, 8, "411")
    with pytest.raises(ValueError):
        yuv_planes(8, 8, "420", 17)


def test_quality_submit_refuses_a_dtype_that_does_not_match_the_depth():
    """no silent uint8 truncation of uint16 frames (and no reinterpretation the other way): a ValueError before the library
    is called, so no engine is needed"""
    from rtvqa_amd.engine import Engine
    eng = Engine.__new__(Engine)   # (no vqa_create: the check comes first)
    x16 = np.zeros((2, frames.frame_samples(16, 16, "yuv420p10le")), np.uint16)
    x8 = np.zeros((2, frames.frame_samples(16, 16, "yuv420p")), np.uint8)
    with pytest.raises(ValueError, match="uint8"):
        eng.quality_submit(x16, x16, yuv420p_planes(16, 16))
    with pytest.raises(ValueError, match="uint16"):
        eng.quality_submit(x8, x8, yuv_planes(16, 16, "420", 10))
