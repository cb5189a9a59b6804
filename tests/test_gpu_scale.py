"""GPU: the resampler (vqa_scale_submit, k_scale) against tests/scale_reference.py fed the library's own tables, byte for byte,
pad bytes of the destination included.  k_scale's workgroup owns a 64 x 32 tile of the destination and walks its source footprint
in chunks of 16 rows: tests/scale_cases.GEOMETRIES says which seam each size hits.  Three frames of different content per case
(noise, 0 / peak runs, flat)."""
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path[:0] = [REPO, os.path.dirname(os.path.abspath(__file__))]

import scale_cases as SC

pytestmark = pytest.mark.gpu


def _check(engine, layout, depth, h, w, oh, ow, filt, seed, src_pad=(0, 0, 0), dst_pad=(0, 0, 0), above_peak=False, mem="host", n=3):
    planes, fb = SC.padded(SC.planes_of(layout, h, w, depth), *src_pad)
    out_planes, ofb = SC.padded(SC.planes_of(layout, oh, ow, depth), *dst_pad)
    frames = SC.content(n, planes, fb, depth, seed, above_peak)
    want = SC.expected(frames, planes, out_planes, ofb, filt, depth)
    got = SC.run(engine, frames, planes, out_planes, ofb, filt, depth, mem)
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, (layout, depth, (h, w), (oh, ow), filt, len(bad), bad[:4].tolist())
    return got


@pytest.mark.parametrize("filt", SC.FILTERS)
@pytest.mark.parametrize("geo", SC.GEOMETRIES, ids=["%dx%d-%dx%d" % (g[1], g[0], g[3], g[2]) for g in SC.GEOMETRIES])
def test_every_geometry_and_filter_on_one_plane(engine, geo, filt):
    h, w, oh, ow, _why = geo
    _check(engine, "mono", 8, h, w, oh, ow, filt, seed=h * 1000 + w)


@pytest.mark.parametrize("filt", SC.FILTERS)
@pytest.mark.parametrize("depth", (8, 10))
def test_420_with_odd_luma_sizes(engine, depth, filt):
    """luma 47 x 33 -> 95 x 67, chroma 24 x 17 -> 48 x 34: two launches (Y; U and V as one group), both across the seams"""
    _check(engine, "420", depth, 33, 47, 67, 95, filt, seed=420 + depth)
    _check(engine, "420", depth, 67, 95, 33, 47, filt, seed=421 + depth)


@pytest.mark.parametrize("filt", ("bicubic", "lanczos"))
def test_444_at_16_bits_with_samples_at_the_peak(engine, filt):
    _check(engine, "444", 16, 27, 48, 41, 72, filt, seed=444)
    _check(engine, "444", 16, 132, 260, 33, 65, filt, seed=445)


@pytest.mark.parametrize("depth", (9, 10, 15))
def test_444_samples_above_the_peak_are_clipped_on_the_way_out(engine, depth):
    got = _check(engine, "444", depth, 27, 48, 41, 72, "bicubic", seed=depth, above_peak=True)
    assert int(got.view("<u2").max()) == (1 << depth) - 1
    got = _check(engine, "444", depth, 31, 40, 45, 40, "lanczos", seed=depth, above_peak=True)   # one axis copied
    assert int(got.view("<u2").max()) == (1 << depth) - 1


@pytest.mark.parametrize("filt", SC.FILTERS)
def test_mono_at_12_bits(engine, filt):
    _check(engine, "mono", 12, 22, 43, 33, 65, filt, seed=12)
    _check(engine, "mono", 12, 81, 144, 54, 96, filt, seed=13)


@pytest.mark.parametrize("filt", SC.FILTERS)
def test_packed_bgr24_on_both_sides(engine, filt):
    _check(engine, "bgr24", 8, 27, 48, 41, 72, filt, seed=24)
    _check(engine, "bgr24", 8, 41, 72, 27, 48, filt, seed=25, src_pad=(3, 0, 5), dst_pad=(2, 0, 7))


@pytest.mark.parametrize("layout,depth", (("420", 8), ("420", 10), ("mono", 8)))
def test_padded_rows_and_a_frame_pad_stay_untouched(engine, layout, depth):
    """_check compares the whole destination, so the lead, the bytes behind every row and the frame pad must still hold FILL"""
    got = _check(engine, layout, depth, 33, 47, 67, 95, "bicubic", seed=7, src_pad=(5, 6, 10), dst_pad=(3, 4, 18))
    assert (got[:, :4] == SC.FILL).all() and (got[:, -18:] == SC.FILL).all()


def test_flat_planes_stay_flat_at_every_level(engine):
    for depth, layout in ((8, "mono"), (10, "mono"), (16, "mono")):
        peak = (1 << depth) - 1
        for level in (0, 1, peak // 2, peak - 1, peak):
            for filt in SC.FILTERS:
                planes, fb = SC.padded(SC.planes_of(layout, 31, 57, depth))
                out_planes, ofb = SC.padded(SC.planes_of(layout, 70, 130, depth))
                fr = np.zeros((1, fb), np.uint8)
                SC._view(fr[0], planes[0], 2 if depth > 8 else 1)[...] = level
                got = SC.run(engine, fr, planes, out_planes, ofb, filt, depth)
                vals = SC.as_samples(got, depth)
                assert (vals == level).all(), (depth, level, filt)


def test_the_same_frame_gives_the_same_bytes_anywhere_from_any_memory(engine):
    planes, fb = SC.padded(SC.planes_of("420", 33, 47, 8))
    out_planes, ofb = SC.padded(SC.planes_of("420", 67, 95, 8))
    pool = SC.content(3, planes, fb, 8, seed=99)
    batch = np.stack([pool[0], pool[0], pool[1], pool[2], pool[0]])
    want = SC.expected(pool[:1], planes, out_planes, ofb, "lanczos", 8)[0]
    for mem in ("host", "pinned", "device"):
        got = SC.run(engine, batch, planes, out_planes, ofb, "lanczos", 8, mem)
        for place in (0, 1, 4):
            assert (got[place] == want).all(), (mem, place)


# ---- the slice seam: VQA_QSLICE=3 on the lab library, in a child process ------------------------------------------------
SLICE_CASES = (("420", 8, 33, 47, 67, 95, "bicubic"), ("mono", 10, 41, 72, 27, 48, "lanczos"))


def _slice_inputs(case):
    layout, depth, h, w, oh, ow, filt = case
    planes, fb = SC.padded(SC.planes_of(layout, h, w, depth))
    out_planes, ofb = SC.padded(SC.planes_of(layout, oh, ow, depth))
    return planes, out_planes, ofb, SC.content(7, planes, fb, depth, seed=h + w), filt, depth


def _child(out_path):
    import rtvqa_amd
    os.environ["VQA_QSLICE"] = "3"               # read once, in vqa_create
    eng = rtvqa_amd.Engine(0)
    os.environ.pop("VQA_QSLICE")
    assert eng.lib.vqa_build_flavour() == 3
    got = {}
    for i, case in enumerate(SLICE_CASES):
        planes, out_planes, ofb, frames, filt, depth = _slice_inputs(case)
        for mem in ("host", "device"):
            got["%d|%s" % (i, mem)] = SC.run(eng, frames, planes, out_planes, ofb, filt, depth, mem)
    eng.close()
    np.savez(out_path, **got)
    print("SCALE-SLICES-OK", len(got))


def test_seven_frames_in_slices_of_three_equal_the_shipped_library(engine, tmp_path):
    from rtvqa_amd import _native as N
    assert engine.lib.vqa_build_flavour() == 0
    out = str(tmp_path / "slices.npz")
    env = dict(os.environ, VQA_LIB_PATH=N.LAB_LIB_PATH)
    env.pop("VQA_QSLICE", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True, timeout=300, cwd=REPO)
    assert r.returncode == 0 and "SCALE-SLICES-OK" in r.stdout, (r.stdout[-300:], r.stderr[-2000:])
    with np.load(out) as z:
        for i, case in enumerate(SLICE_CASES):
            planes, out_planes, ofb, frames, filt, depth = _slice_inputs(case)
            whole = SC.run(engine, frames, planes, out_planes, ofb, filt, depth)
            assert (whole == SC.expected(frames, planes, out_planes, ofb, filt, depth)).all()
            for mem in ("host", "device"):
                assert (z["%d|%s" % (i, mem)] == whole).all(), (case, mem)


# ---- chaining: what follows on the same engine reads the scaled frames, with no wait in between ----------------------------
def _chain_inputs(depth=8):
    from rtvqa_amd import synth
    from rtvqa_amd.frames import bgr_to_yuv420p
    h, w, oh, ow = 48, 64, 96, 128
    ref = bgr_to_yuv420p(synth.s_natural(3, oh, ow, seed=5))
    rung = bgr_to_yuv420p(synth.distort(synth.s_natural(3, h, w, seed=5)))
    planes, out_planes = SC.planes_of("420", h, w), SC.planes_of("420", oh, ow)
    want = SC.expected(rung, planes, out_planes, SC.frame_bytes(out_planes), "bicubic", 8)
    return ref, rung, planes, out_planes, want


def test_quality_and_gmsd_follow_the_scale_without_a_wait(engine):
    ref, rung, planes, out_planes, want = _chain_inputs()
    dref = engine.upload(ref)
    q_want, g_want = engine.quality(ref, want, out_planes), engine.gmsd(ref, want, out_planes)
    scaled = engine.scale_submit(rung, planes, out_planes, "bicubic")
    q = engine.quality(dref, scaled, out_planes)          # (no scale_wait)
    g = engine.gmsd(dref, scaled, out_planes)
    engine.scale_wait()
    assert q.tobytes() == q_want.tobytes() and g.tobytes() == g_want.tobytes()
    assert (engine.download(scaled) == want).all()
    assert float(q["sse"].sum()) > 0


def test_the_scale_batch_pends_next_to_another_kinds_batch(engine):
    ref, rung, planes, out_planes, want = _chain_inputs()
    dref = engine.upload(ref)
    s_want, g_want = engine.siti(ref, out_planes), engine.gmsd(ref, want, out_planes)
    engine.siti_submit(dref, out_planes)
    scaled = engine.scale_submit(engine.upload(rung), planes, out_planes, "bicubic")
    engine.gmsd_submit(dref, scaled, out_planes)
    s = engine.siti_wait()
    g = engine.gmsd_wait()
    engine.scale_wait()
    assert s.tobytes() == s_want.tobytes() and g.tobytes() == g_want.tobytes()


# ---- errors ---------------------------------------------------------------------------------------------------------------
def _raw_submit(engine, src, planes, dst_ptr, out_planes, filt=1, mem=None, n=None, fs=None, ofs=None):
    from rtvqa_amd import _native as N
    from rtvqa_amd.engine import DeviceFrames, plane_descs, planes_span
    dev = isinstance(src, DeviceFrames)
    ptr = src.ptr if dev else src.ctypes.data
    n = n if n is not None else (src.n if dev else src.shape[0])
    fs = fs if fs is not None else (src.frame_stride if dev else src.strides[0])
    return engine.lib.vqa_scale_submit(engine.ctx, ptr, (N.VQA_MEM_DEVICE if dev else N.VQA_MEM_HOST) if mem is None else mem, n, fs,
                                       plane_descs(planes), dst_ptr, ofs if ofs is not None else planes_span(out_planes),
                                       plane_descs(out_planes), len(planes), filt)


def test_limits_and_invalid_arguments_leave_nothing_in_flight(engine):
    from rtvqa_amd import _native as N
    from rtvqa_amd.engine import DeviceBuffer, mono_planes, yuv_planes
    src = np.zeros((2, 64 * 64), np.uint8)
    p64 = mono_planes(64, 64)
    buf = DeviceBuffer(engine, 2 * 512 * 512)
    sub = lambda planes, out_planes, **kw: _raw_submit(engine, kw.pop("src", src), planes, kw.pop("dst", buf.ptr), out_planes, **kw)
    U, I = N.VQA_ERR_UNSUPPORTED, N.VQA_ERR_INVALID
    assert sub(p64, mono_planes(15, 64)) == U                      # a side below 16
    assert sub(mono_planes(15, 64), p64) == U
    assert sub(p64, mono_planes(64, 513)) == U                     # more than 8x up
    assert sub(p64, mono_planes(16, 16)) == N.VQA_OK and engine.lib.vqa_scale_wait(engine.ctx) == N.VQA_OK   # exactly 1/4
    assert sub(mono_planes(65, 64), mono_planes(16, 64), src=np.zeros((2, 65 * 64), np.uint8)) == U      # below 1/4
    assert sub(p64, mono_planes(32, 32, 10)) == U                  # another depth
    assert sub(p64, mono_planes(32, 32), filt=3) == I and sub(p64, mono_planes(32, 32), filt=-1) == I
    assert sub(p64, mono_planes(32, 32), dst=None) == I
    assert sub(p64, mono_planes(32, 32), n=0) == I
    assert sub(p64, mono_planes(32, 32), ofs=32 * 32 - 1) == I     # frames of the destination overlap each other
    host_dst = np.zeros(2 * 32 * 32, np.uint8)
    assert sub(p64, mono_planes(32, 32), dst=host_dst.ctypes.data) == I          # pageable host memory
    pinned = engine.alloc_pinned((2 * 32 * 32,))
    assert sub(p64, mono_planes(32, 32), dst=pinned.ctypes.data) == I            # pinned host memory
    engine.free_pinned(pinned)
    dsrc = engine.upload(np.zeros((4, 64 * 64), np.uint8))                       # two source frames, then room for a destination
    assert sub(p64, mono_planes(32, 32), src=dsrc, n=2, dst=dsrc.ptr) == I       # the destination IS the source
    assert sub(p64, mono_planes(32, 32), src=dsrc, n=2, dst=dsrc.ptr + 2 * 64 * 64 - 1) == I   # ... or shares its last byte
    assert sub(p64, mono_planes(32, 32), src=dsrc, n=2, dst=dsrc.ptr + 2 * 64 * 64) == N.VQA_OK   # ... but may follow it
    assert engine.lib.vqa_scale_wait(engine.ctx) == N.VQA_OK
    five = yuv_planes(64, 64, "444") + yuv_planes(64, 64, "444")[:2]
    assert _raw_submit(engine, np.zeros((1, 5 * 64 * 64), np.uint8), five, buf.ptr, five) == I    # five planes
    assert engine.lib.vqa_scale_wait(engine.ctx) == N.VQA_ERR_STATE              # nothing was left in flight
    assert engine.lib.vqa_scale_wait(None) == I
    # a pending scale batch refuses the next one and survives the refusal
    assert sub(p64, mono_planes(32, 32)) == N.VQA_OK
    assert sub(p64, mono_planes(32, 32)) == N.VQA_ERR_STATE
    assert engine.lib.vqa_scale_wait(engine.ctx) == N.VQA_OK
    assert engine.lib.vqa_scale_wait(engine.ctx) == N.VQA_ERR_STATE
    assert engine.lib.vqa_trim(engine.ctx) == N.VQA_OK
    got = engine.scale(src, p64, mono_planes(32, 32))            # usable afterwards
    assert (engine.download(got) == 0).all()
    buf.free()


def test_python_refuses_the_wrong_sample_type_and_a_small_out(engine):
    from rtvqa_amd.engine import mono_planes
    with pytest.raises(ValueError):
        engine.scale(np.zeros((1, 64 * 64), np.uint16), mono_planes(64, 64), mono_planes(32, 32))
    with pytest.raises(ValueError):
        engine.scale(np.zeros((1, 64 * 64), np.uint8), mono_planes(64, 64, 10), mono_planes(32, 32, 10))
    small = engine.upload(np.zeros((1, 100), np.uint8))
    with pytest.raises(ValueError):
        engine.scale(np.zeros((1, 64 * 64), np.uint8), mono_planes(64, 64), mono_planes(32, 32), out=small)
    with pytest.raises(ValueError):
        engine.scale(np.zeros((1, 64 * 64), np.uint8), mono_planes(64, 64), mono_planes(32, 32), out=engine.upload(np.zeros((1, 4096), np.uint16)))
    assert not getattr(engine, "_pending_k", None)


def test_profile_names_the_kernel(engine):
    from rtvqa_amd.engine import mono_planes
    engine.profile(True)
    try:
        engine.profile_read(reset=True)
        engine.scale(np.zeros((2, 64 * 64), np.uint8), mono_planes(64, 64), mono_planes(96, 96))
        prof = engine.profile_read(reset=True)
    finally:
        engine.profile(False)
    assert prof["k_scale"][1] == 1 and prof["k_scale"][0] > 0


if __name__ == "__main__":
    _child(sys.argv[1])
