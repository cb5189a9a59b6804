"""vqa_weave_submit on the GPU against a NumPy weave: every byte of the destination, pad bytes included - the destination is
prefilled with a pattern that must survive where no sample lies - over the five layouts at 8 and 10 bits, widths around a
16-byte granule, byte phases that differ between source and destination; pulldown and its inverse on the device; the woven
frames handed on without a wait."""
import numpy as np
import pytest

import convert_cases as CC
import convert_reference as CR
import fields_reference as R
from rtvqa_amd import _native as N
from rtvqa_amd import fields as F

pytestmark = pytest.mark.gpu

FILL = 0xA5
LAYOUTS = ("420", "422", "444", "mono", "bgr")
SIZES = ((16, 16), (17, 33), (18, 47), (34, 65), (21, 130))   # luma (h, w): around a 16-byte granule, odd and even


def _planes(h, w, layout, depth, row_pad=0, lead=0, plane_pad=0):
    """-> (plane tuples, frame bytes); pads in samples, as convert_cases.planes_of; "bgr": three interleaved planes"""
    if layout != "bgr":
        return CC.planes_of(h, w, layout, depth, row_pad, lead, plane_pad)
    bps = 2 if depth > 8 else 1
    rs = (3 * w + row_pad) * bps
    return [(w, h, (lead + c) * bps, rs, 3 * bps, depth) for c in range(3)], lead * bps + h * rs + plane_pad * bps


def _expected(frames, planes, top, bottom, ofb):
    out = np.full((len(top), ofb), FILL, np.uint8)
    for p in planes:
        woven = R.weave(np.stack([CR.read_plane(f, p) for f in frames]), top, bottom)
        for j in range(len(top)):
            CR.write_plane(out[j], p, woven[j])
    return out


def _run(engine, frames, planes, fb, top, bottom, depth, shift=0, mem="host"):
    """the weave into a destination prefilled with FILL that starts `shift` bytes into its allocation -> [n_out, fb] uint8"""
    from rtvqa_amd.engine import DeviceFrames
    isz, n_out = 2 if depth > 8 else 1, len(top)
    canvas = engine.upload(CC.as_samples(np.full((1, n_out * fb + 32), FILL, np.uint8), depth))
    dst = DeviceFrames(canvas.ptr + shift, n_out, 1, fb // isz, frame_stride=fb, owner=canvas, channels=1, itemsize=isz)
    src = CC.as_samples(frames, depth)
    if mem == "device":
        src = engine.upload(src)
    res = engine.weave(src, planes, top, bottom, out=dst, frame_bytes=fb)
    got = engine.download(res, np.uint8)
    whole = engine.download(canvas, np.uint8).reshape(-1)
    assert (whole[:shift] == FILL).all() and (whole[shift + n_out * fb:] == FILL).all()
    canvas._owner.free()
    return got


def _check(engine, hw, layout, depth, pads=(0, 0, 0), shift=0, mem="host", seed=1):
    planes, fb = _planes(hw[0], hw[1], layout, depth, *pads)
    frames = CC.content(4, fb, depth, seed)
    top, bottom = [0, 1, 3, 2, 0], [1, 1, 0, 3, 0]
    got = _run(engine, frames, planes, fb, top, bottom, depth, shift, mem)
    want = _expected(frames, planes, top, bottom, fb)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (hw, layout, depth, pads, shift, mem, len(bad), bad[:4].tolist())


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_layout_at_sizes_around_a_granule(engine, layout, depth):
    for k, hw in enumerate(SIZES):
        _check(engine, hw, layout, depth, seed=k)
        _check(engine, hw, layout, depth, pads=((3, 1, 5), (5, 3, 1), (16, 0, 0))[k % 3], mem=("host", "device")[k % 2], seed=k + 10)


@pytest.mark.parametrize("depth", [8, 10])
def test_byte_phases_that_differ_between_the_two_sides(engine, depth):
    """the destination starts 1 .. 15 bytes (16 bits: 2 .. 14) into a granule while the source keeps its phase"""
    for shift in (range(1, 16, 3) if depth == 8 else range(2, 16, 4)):
        _check(engine, (17, 33), "420", depth, pads=(1, 1, 0), shift=shift, seed=shift)
        _check(engine, (16, 21), "bgr", depth, pads=(2, 0, 0), shift=shift, seed=shift)


def test_a_pixel_step_of_two_takes_the_gather(engine):
    for depth in (8, 10):
        planes, fb = CC.planes_of(17, 33, "420", depth, 1, 1, 0, step=2)
        frames = CC.content(3, fb, depth, 6)
        top, bottom = [2, 0], [1, 0]
        got = _run(engine, frames, planes, fb, top, bottom, depth)
        assert (got == _expected(frames, planes, top, bottom, fb)).all()


def _film(n, distorted=False):
    from rtvqa_amd import synth
    from rtvqa_amd.frames import bgr_to_yuv420p
    fr = synth.s_natural(4 * n, 48, 64, seed=5)[::4]
    return bgr_to_yuv420p(synth.distort(fr) if distorted else fr)


def test_pulldown_and_its_inverse_on_the_device(engine):
    from rtvqa_amd.engine import yuv420p_planes
    planes, film = yuv420p_planes(48, 64), _film(12)
    for phase, order in ((0, "tff"), (3, "bff")):
        top, bottom = F.telecine_plan(12, phase, order)
        tc = engine.weave_submit(film, planes, top, bottom)
        a = F.analyse(engine.fields(tc, planes))                     # (no wait in between: the stream orders them)
        engine.weave_wait()
        assert (a["cadence"], a["phase"], a["order"], a["breaks"]) == ("3:2", phase, order, [])
        it, ib = F.ivtc_plan(a, len(top))
        back = engine.download(engine.weave(tc, planes, it, ib))
        kept = np.array(top)[it]
        assert (kept == np.array(bottom)[ib]).all() and (np.diff(kept) == 1).all() and kept[-1] == 11
        assert (back == film[kept]).all()
        assert (engine.download(tc).reshape(len(top), -1) == _expected(film, planes, top, bottom, film.shape[1])).all()


def test_woven_frames_go_straight_into_fields_and_quality(engine):
    from rtvqa_amd.engine import yuv420p_planes
    planes, film, enc = yuv420p_planes(48, 64), _film(8), _film(8, distorted=True)
    top, bottom = F.telecine_plan(8)
    ref = engine.weave(film, planes, top, bottom)
    dist = engine.weave_submit(enc, planes, top, bottom)
    rec = engine.fields(dist, planes)                                 # no weave_wait: the submits follow it on the stream
    q = engine.quality(ref, dist, planes)
    engine.weave_wait()
    ref_h, dist_h = engine.download(ref), engine.download(dist)
    assert (dist_h == _expected(enc, planes, top, bottom, enc.shape[1])).all()
    assert rec.tobytes() == engine.fields(dist_h, planes).tobytes()
    assert q.tobytes() == engine.quality(ref_h, dist_h, planes).tobytes()
    rec0 = R.records(np.stack([CR.read_plane(f, planes[0]) for f in dist_h]))
    assert all(R.same(g, w) for g, w in zip(rec, rec0))


def test_the_refusals_come_before_anything_is_launched(engine):
    planes, fb = CC.planes_of(16, 16, "420", 8)
    frames = CC.content(3, fb, 8, 1)
    for top, bottom in (([0, 3], [0, 1]), ([0, 1], [-1, 1]), ([0], [0, 1]), ([], [])):
        with pytest.raises(ValueError, match="top_index and bottom_index"):
            engine.weave(frames, planes, top, bottom)
    with pytest.raises(ValueError, match="at least 16 x 16"):
        engine.weave(frames, [(16, 15, 0, 16, 1)], [0], [0])
    with pytest.raises(ValueError, match="uint8"):
        engine.weave(frames.astype(np.uint16), planes, [0], [0])
    dev = engine.upload(frames)
    with pytest.raises(N.VqaError):                                   # out overlaps in
        engine.weave(dev, planes, [0, 1, 2], [1, 2, 0], out=dev)
    assert (engine.download(dev, np.uint8).reshape(3, -1) == frames).all()
    # the C entry point checks the indices itself
    idx = (np.array([0, 3], np.int32), np.array([0, 1], np.int32))
    from rtvqa_amd.engine import DeviceBuffer, plane_descs
    import ctypes as C
    buf = DeviceBuffer(engine, 2 * fb)
    i32 = C.POINTER(C.c_int32)
    st = engine.lib.vqa_weave_submit(engine.ctx, frames.ctypes.data, N.VQA_MEM_HOST, 3, fb, plane_descs(planes), buf.ptr, fb,
                                     plane_descs(planes), 3, idx[0].ctypes.data_as(i32), idx[1].ctypes.data_as(i32), 2)
    assert st == N.VQA_ERR_INVALID and engine.lib.vqa_weave_wait(engine.ctx) == N.VQA_ERR_STATE
    buf.free()
    _check(engine, (16, 16), "420", 8)
