"""vqa_convert_submit on the GPU against the NumPy restatement of include/vqa.h (convert_reference): every byte of the
destination, pad bytes included - the destination is prefilled with a pattern that must survive where no sample lies."""
import itertools

import numpy as np
import pytest

import convert_cases as CC
import convert_reference as R

pytestmark = pytest.mark.gpu

PAIRS = list(itertools.product(CC.CHROMAS, repeat=2)) + [("mono", "mono")]


@pytest.mark.parametrize("cs,cd", PAIRS, ids=["%s-%s" % p for p in PAIRS])
def test_every_layout_pair_depth_pair_and_option(engine, cs, cd):
    """the thinned list (convert_cases.CASES): every depth pair x (filter, siting) at an even and an odd size, ranges, sizes and
    pad patterns walking along; above 8 bits the noise holds samples above the source's peak"""
    mine = [c for c in CC.CASES if (c[1], c[2]) == (cs, cd)]
    assert len(mine) == 48
    for k, (hw, _cs, _cd, ds, dd, chroma, siting, rng, (src_pad, dst_pad)) in enumerate(mine):
        CC.check(engine, hw, cs, cd, ds, dd, chroma, siting, rng, src_pad, dst_pad, n=1 + k % 3, seed=k, above=8 < ds < 16 and k % 2 == 1)


def test_relations_that_no_layout_pair_has(engine):
    """(up, down) and (down, up) on one plane: the rule is per plane and per axis"""
    for k, (hw, (rx, ry), ds, dd, chroma, siting, rng) in enumerate(CC.MIXED):
        planes, fb = CC.mixed_planes(hw, rx, ry, ds, "src")
        out_planes, ofb = CC.mixed_planes(hw, rx, ry, dd, "dst")
        frames = CC.content(2, fb, ds, k)
        want = CC.expected(frames, planes, out_planes, ofb, chroma, siting, rng)
        got = CC.run(engine, frames, planes, out_planes, ofb, chroma, siting, rng)
        assert (got == want).all(), (hw, rx, ry, ds, dd, chroma, siting, rng)


@pytest.mark.parametrize("ds,dd", ((8, 8), (8, 10), (10, 8), (10, 12)))
def test_row_pairs_where_the_destination_rows_share_a_phase(engine, ds, dd):
    """vertical up with a destination row stride that is a multiple of 16: a lane takes its granule in both rows that the same
    two source rows feed - at odd and even heights, with 2 n and 2 n - 1 rows, next to the single-row path on the same samples"""
    for hw, cd in (((17, 33), "444"), ((34, 65), "422"), ((16, 16), "444"), ((50, 130), "444")):
        for chroma, siting in CC.FILTERS:
            planes, fb = CC.planes_of(hw[0], hw[1], "420", ds, lead=1)
            frames = CC.content(2, fb, ds, hw[1])
            got = {}
            for row_pad in (16 - hw[1] % 16, 16 - hw[1] % 16 + 1):     # the luma's stride a multiple of 16 samples, and not
                out_planes, ofb = CC.planes_of(hw[0], hw[1], cd, dd, row_pad=row_pad)
                want = CC.expected(frames, planes, out_planes, ofb, chroma, siting, "limited")
                res = CC.run(engine, frames, planes, out_planes, ofb, chroma, siting, "limited")
                assert (res == want).all(), (hw, cd, chroma, siting, row_pad)
                got[row_pad] = [R.read_plane(res[0], q) for q in out_planes]
            a, b = got.values()
            assert all((x == y).all() for x, y in zip(a, b))


@pytest.mark.parametrize("ds,dd", ((8, 10), (10, 8), (8, 8), (12, 12)))
def test_a_pixel_step_of_two_takes_the_gather_and_gives_the_rows_bytes(engine, ds, dd):
    for hw, cs, cd in (((17, 33), "420", "444"), ((18, 47), "444", "420"), ((16, 16), "422", "422")):
        for (chroma, siting), rng in zip(CC.FILTERS, ("limited", "full", "limited")):
            packed_s, fb = CC.planes_of(hw[0], hw[1], cs, ds)
            packed_d, ofb = CC.planes_of(hw[0], hw[1], cd, dd)
            frames = CC.content(2, fb, ds, 5)
            rows = CC.run(engine, frames, packed_s, packed_d, ofb, chroma, siting, rng)
            assert (rows == CC.expected(frames, packed_s, packed_d, ofb, chroma, siting, rng)).all()
            samples = [R.read_plane(rows[1], q) for q in packed_d]
            # the same samples behind a step of two on the source side ...
            step_s, fb2 = CC.planes_of(hw[0], hw[1], cs, ds, step=2)
            wide = np.full((2, fb2), 0x5A, np.uint8)
            for j in range(2):
                for a, b in zip(packed_s, step_s):
                    R.write_plane(wide[j], b, R.read_plane(frames[j], a))
            got = CC.run(engine, wide, step_s, packed_d, ofb, chroma, siting, rng)
            assert (got == rows).all(), (hw, cs, cd, chroma, "source step")
            # ... and written behind a step of two on the destination side: the bytes between the samples keep the pattern
            step_d, ofb2 = CC.planes_of(hw[0], hw[1], cd, dd, step=2)
            got = CC.run(engine, frames, packed_s, step_d, ofb2, chroma, siting, rng)
            assert (got == CC.expected(frames, packed_s, step_d, ofb2, chroma, siting, rng)).all()
            assert all((R.read_plane(got[1], q) == s).all() for q, s in zip(step_d, samples))


def test_more_rows_than_one_band(engine):
    """a workgroup owns 64 KB of destination rows: 1030 samples a row is 63 rows a band at 8 bits and 31 at 16"""
    CC.check(engine, (140, 1030), "420", "444", 8, 8, "linear", "left", "full", n=1)
    CC.check(engine, (139, 1030), "444", "420", 8, 10, "linear", "center", "limited", n=1)
    CC.check(engine, (70, 1031), "mono", "mono", 10, 8, n=2)


def test_the_same_bytes_from_any_memory_in_any_batch(engine):
    planes, fb = CC.planes_of(34, 65, "422", 10, 3, 1, 5)
    out_planes, ofb = CC.planes_of(34, 65, "420", 8, 0, 0, 0)
    pool = CC.content(3, fb, 10, 99, above=True)
    want = CC.expected(pool[:1], planes, out_planes, ofb, "linear", "center", "limited")[0]
    batch = np.stack([pool[0], pool[0], pool[1], pool[2], pool[0]])
    for mem in ("host", "pinned", "device"):
        got = CC.run(engine, batch, planes, out_planes, ofb, "linear", "center", "limited", mem=mem)
        for place in (0, 1, 4):
            assert (got[place] == want).all(), (mem, place)
    assert (CC.run(engine, pool[:1], planes, out_planes, ofb, "linear", "center", "limited")[0] == want).all()


# ---- chaining --------------------------------------------------------------------------------------------------------------
def _chain_inputs():
    from rtvqa_amd import synth
    from rtvqa_amd.frames import bgr_to_yuv420p
    h, w = 48, 64
    ref = bgr_to_yuv420p(synth.s_natural(3, h, w, seed=5))
    dist = bgr_to_yuv420p(synth.distort(synth.s_natural(3, h, w, seed=5)))
    p8, _ = CC.planes_of(h, w, "420", 8)
    p10, _ = CC.planes_of(h, w, "422", 10)
    ref10 = R.convert_packed(ref, p8, p10, "linear", "center", "limited")          # the 10-bit 4:2:2 source of an 8-bit 4:2:0 encode
    want = R.convert_packed(dist, p8, p10, "linear", "left", "full")
    return ref10, dist, p8, p10, want


def test_gmsd_follows_a_convert_without_a_wait(engine):
    ref10, dist, p8, p10, want = _chain_inputs()
    g_want = engine.gmsd(ref10, want, p10)
    cd = engine.convert_submit(dist, p8, p10, "linear", "left", "full")
    g = engine.gmsd(engine.upload(ref10), cd, p10)          # (no convert_wait)
    engine.convert_wait()
    assert g.tobytes() == g_want.tobytes() and float(g["gmsd"].sum()) > 0
    assert (engine.download(cd) == want).all()


def test_a_convert_batch_pends_next_to_a_gmsd_batch(engine):
    ref10, dist, p8, p10, want = _chain_inputs()
    g_alone = engine.gmsd(ref10, want, p10)
    c_alone = engine.download(engine.convert(dist, p8, p10, "box", "center", "limited"))
    engine.gmsd_submit(ref10, want, p10)
    cd = engine.convert_submit(dist, p8, p10, "box", "center", "limited")
    with pytest.raises(Exception):
        engine.convert_submit(dist, p8, p10)                 # VQA_ERR_STATE while one is pending
    g = engine.gmsd_wait()
    engine.convert_wait()
    assert g.tobytes() == g_alone.tobytes() and (engine.download(cd) == c_alone).all()
    assert (c_alone == R.convert_packed(dist, p8, p10, "box", "center", "limited")).all()


# ---- errors ----------------------------------------------------------------------------------------------------------------
def _raw(engine, src, planes, dst_ptr, out_planes, n=None, ofs=None, opts=(1, 0, 0)):
    from rtvqa_amd import _native as N
    from rtvqa_amd.engine import DeviceFrames, plane_descs, planes_span
    dev = isinstance(src, DeviceFrames)
    ptr = src.ptr if dev else src.ctypes.data
    n = n if n is not None else (src.n if dev else src.shape[0])
    fs = src.frame_stride if dev else src.strides[0]
    return engine.lib.vqa_convert_submit(engine.ctx, ptr, N.VQA_MEM_DEVICE if dev else N.VQA_MEM_HOST, n, fs, plane_descs(planes),
                                         dst_ptr, ofs if ofs is not None else planes_span(out_planes), plane_descs(out_planes),
                                         len(planes), *opts)


def test_limits_and_invalid_arguments_leave_nothing_in_flight(engine):
    from rtvqa_amd import _native as N
    from rtvqa_amd.engine import DeviceBuffer
    p8, fb = CC.planes_of(32, 32, "420", 8)
    p10, ofb = CC.planes_of(32, 32, "444", 10)
    src = CC.content(2, fb, 8, 1)
    buf = DeviceBuffer(engine, 2 * ofb)
    try:
        mono = lambda w, h, d: [(w, h, 0, w * (2 if d > 8 else 1), 2 if d > 8 else 1, d)]
        for planes, out_planes, opts, n, status in (
                (p8, p10, (2, 0, 0), None, N.VQA_ERR_INVALID), (p8, p10, (1, 2, 0), None, N.VQA_ERR_INVALID),
                (p8, p10, (1, 0, -1), None, N.VQA_ERR_INVALID), (p8, p10, (1, 0, 0), 32769, N.VQA_ERR_UNSUPPORTED),
                (mono(32, 32, 8), mono(32, 17, 10), (1, 0, 0), None, N.VQA_ERR_UNSUPPORTED),
                (mono(32, 32, 8), mono(15, 16, 10), (1, 0, 0), None, N.VQA_ERR_UNSUPPORTED),
                (mono(32, 15, 8), mono(32, 15, 10), (1, 0, 0), None, N.VQA_ERR_UNSUPPORTED),
                (p8[:2], [p10[0], (7, 32) + tuple(p10[1][2:])], (1, 0, 0), None, N.VQA_ERR_UNSUPPORTED)):
            assert _raw(engine, src, planes, buf.ptr, out_planes, n=n, opts=opts) == status, (planes, out_planes, opts, n)
            assert engine.lib.vqa_convert_wait(engine.ctx) == N.VQA_ERR_STATE          # nothing is in flight
        assert _raw(engine, src, p8, src.ctypes.data, p10) == N.VQA_ERR_INVALID        # dst is host memory
        dsrc = engine.upload(src)
        assert _raw(engine, dsrc, p8, dsrc.ptr + 16, p8) == N.VQA_ERR_INVALID          # dst overlaps the source
        assert _raw(engine, src, p8, buf.ptr, p10, ofs=ofb - 2) == N.VQA_ERR_INVALID   # frames of dst overlap each other
        assert engine.lib.vqa_convert_wait(engine.ctx) == N.VQA_ERR_STATE
        assert _raw(engine, src, p8, buf.ptr, p10) == N.VQA_OK
        assert _raw(engine, src, p8, buf.ptr, p10) == N.VQA_ERR_STATE                  # one is pending
        assert engine.lib.vqa_convert_wait(engine.ctx) == N.VQA_OK
        engine.trim()                                                                  # the staging buffer goes with the slot
        assert _raw(engine, src, p8, buf.ptr, p10) == N.VQA_OK and engine.lib.vqa_convert_wait(engine.ctx) == N.VQA_OK
        dsrc._owner.free()
    finally:
        buf.free()


def test_python_refuses_before_anything_is_uploaded(engine):
    p8, fb = CC.planes_of(32, 32, "420", 8)
    p10, _ = CC.planes_of(32, 32, "420", 10)
    src = CC.content(1, fb, 8, 1)
    with pytest.raises(ValueError):
        engine.convert_submit(src.view(np.uint16), p8, p10)          # a sample type that does not match the depth: never a cast
    with pytest.raises(ValueError):
        engine.convert_submit(src, p10, p8)
    with pytest.raises(ValueError):
        engine.convert_submit(src, p8, p10, chroma="lanczos")
    with pytest.raises(ValueError):
        engine.convert_submit(src, p8, p10, out=engine.upload(src))  # an out of the wrong sample type
    with pytest.raises(TypeError):
        engine.convert_submit(src, p8, p10, out=src)
    assert (engine.download(engine.convert(src, p8, p10)) == R.convert_packed(src, p8, p10)).all()


def test_frame_convert_walks_a_clip_in_chunks(engine):
    from rtvqa_amd import video_processing as vp
    from rtvqa_amd.frames import frame_samples
    h, w = 34, 66
    clip = np.random.default_rng(2).integers(0, 1024, (5, frame_samples(h, w, "yuv422p10le"))).astype(np.uint16)
    got = vp.frame_convert(clip, "yuv422p10le", "yuv420p", h, w, engine=engine, batch_size=2)
    p10, p8 = vp.LAYOUTS["yuv422p10le"][0](h, w), vp.LAYOUTS["yuv420p"][0](h, w)
    assert got.dtype == np.uint8 and (got == R.convert_packed(clip, p10, p8)).all()
    back = vp.frame_convert(got, "yuv420p", "yuv444p12le", h, w, chroma="box", range="full", engine=engine)
    assert back.dtype == np.uint16 and (back == R.convert_packed(got, p8, vp.LAYOUTS["yuv444p12le"][0](h, w), "box", "center", "full")).all()
    with pytest.raises(ValueError):
        vp.frame_convert(got, "yuv420p", "gray", h, w, engine=engine)
