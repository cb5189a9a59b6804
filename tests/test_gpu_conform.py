"""GPU: vqa_conform_submit (k_conform.hip) against tests/conform_reference.py, byte for byte, pad bytes of the destination
included: the destination is prefilled with a pattern and compared whole.  tests/conform_cases.py says which seam each size,
window corner and index list is there for.  Three source frames of different content per case (noise, 0 / peak runs, flat)."""
import numpy as np
import pytest

import conform_cases as CC
import scale_cases as SC

pytestmark = pytest.mark.gpu

LD = CC.layout_depths()


@pytest.mark.parametrize("layout,depth", LD, ids=["%s-%d" % ld for ld in LD])
def test_every_size_window_and_index_is_a_copy_of_the_window(engine, layout, depth):
    """no table, no matrix: the copy kernel's realign path at every byte phase, the ends of the rows, the frame gather"""
    k = 0
    for size in CC.SIZES:
        for origin in CC.ORIGINS:
            CC.check(engine, layout, depth, size, origin, CC.INDICES[k % len(CC.INDICES)], seed=1000 * depth + k)
            k += 1


@pytest.mark.parametrize("depth", CC.DEPTHS)
def test_the_table_alone(engine, depth):
    """in LDS up to 12 bits, through L2 at 16; three tables that differ, bgr24's picked by sample % 3"""
    for k, layout in enumerate(CC.LAYOUTS):
        if layout == "bgr24" and depth != 8:
            continue
        n_planes = 1 if layout == "mono" else 3
        lut = CC.random_lut(n_planes, depth, seed=depth + k)
        CC.check(engine, layout, depth, (33, 47), CC.ORIGINS[(k + 1) % 6], CC.INDICES[k % 4], lut=lut, seed=50 + k)
        CC.check(engine, layout, depth, (18, 130), CC.ORIGINS[(k + 3) % 6], lut=lut, seed=60 + k)


def test_a_sample_above_the_peak_reads_the_peaks_entry(engine):
    sh, sw = 20, 37
    planes, fb = SC.padded(SC.planes_of("444", sh, sw, 10))
    out_planes, ofb = SC.padded(SC.planes_of("444", 16, 33, 10))
    frames = SC.content(3, planes, fb, 10, seed=5, above_peak=True)
    assert int(SC.as_samples(frames, 10).max()) > 1023
    lut = CC.random_lut(3, 10, seed=9)
    origins = [(2, 3)] * 3
    want = CC.expected(frames, planes, out_planes, ofb, 10, origins, None, lut)
    assert (CC.run(engine, frames, planes, out_planes, ofb, 10, origins, None, lut) == want).all()
    # and without a table the copy carries it as it is
    want = CC.expected(frames, planes, out_planes, ofb, 10, origins)
    assert int(SC.as_samples(want, 10).max()) > 1023
    assert (CC.run(engine, frames, planes, out_planes, ofb, 10, origins) == want).all()


MATRIX_CASES = [(l, d) for l in ("420", "422", "444", "bgr24") for d in (8, 10, 16) if l != "bgr24" or d == 8]


@pytest.mark.parametrize("layout,depth", MATRIX_CASES, ids=["%s-%d" % ld for ld in MATRIX_CASES])
def test_the_matrix_alone_clips_at_both_ends(engine, layout, depth):
    m = CC.clipping_matrix(depth)
    assert (m[:, 3] < 0).any()
    peak = (1 << depth) - 1
    for k, (size, origin) in enumerate((((33, 47), (1, 3)), ((16, 16), (0, 0)), ((18, 130), (3, 5)), ((64, 80), (2, 2)))):
        got = CC.check(engine, layout, depth, size, origin, CC.INDICES[k % 4], matrix=m, seed=70 + k)
        vals = SC.as_samples(got, depth)
        assert (vals == 0).any() and (vals == peak).any()
    # the whole of an odd-sized source: the last cells hold one and two luma samples
    CC.check(engine, layout, depth, (33, 47), (0, 0), matrix=m, seed=75, extra=(0, 0))


def test_the_matrix_with_windows_of_their_own_per_plane(engine):
    """the definition is stated in SOURCE coordinates: a chroma window that is not the luma's, halved, and planes 1 and 2 apart;
    the source's odd size gives cells of one, two and four luma samples"""
    m = CC.clipping_matrix(8)
    for layout in ("420", "422"):
        CC.check(engine, layout, 8, (32, 46), (3, 5), matrix=m, seed=81, origins=[(3, 5), (0, 1), (2, 0)])
        CC.check(engine, layout, 10, (33, 47), (1, 0), matrix=CC.clipping_matrix(10), seed=82, origins=[(1, 0), (1, 1), (0, 1)])
        CC.check(engine, layout, 8, (31, 45), (2, 2), matrix=m, seed=83, origins=[(2, 2), (0, 0), (1, 1)], extra=(0, 0))


@pytest.mark.parametrize("layout,depth", (("420", 8), ("420", 10), ("444", 12), ("422", 16), ("bgr24", 8)))
def test_table_then_matrix(engine, layout, depth):
    lut = CC.random_lut(3, depth, seed=depth)
    CC.check(engine, layout, depth, (33, 47), (1, 3), (2, 0, 0), lut=lut, matrix=CC.clipping_matrix(depth), seed=90)


@pytest.mark.parametrize("layout,depth", (("420", 8), ("420", 10), ("mono", 8), ("bgr24", 8), ("444", 16)))
def test_padded_rows_and_frame_pads_on_both_sides(engine, layout, depth):
    """check compares the whole destination, so the lead, the bytes behind every row and the frame pad must still hold FILL"""
    for origin in ((1, 3), (0, 0), (2, 5)):
        got = CC.check(engine, layout, depth, (33, 47), origin, src_pad=(5, 6, 10), dst_pad=(3, 4, 18), seed=11)
        assert (got[:, :4] == CC.FILL).all() and (got[:, -18:] == CC.FILL).all()
    lut = CC.random_lut(1 if layout == "mono" else 3, depth, seed=3)
    odd = 1 if depth == 8 else 2   # (16-bit frames keep an even size)
    CC.check(engine, layout, depth, (18, 130), (1, 1), lut=lut, src_pad=(1, 2, 3 * odd), dst_pad=(7, 10, odd), seed=12)
    if layout != "mono":
        CC.check(engine, layout, depth, (18, 130), (1, 1), matrix=CC.clipping_matrix(depth), src_pad=(1, 2, 3 * odd),
                 dst_pad=(7, 10, odd), seed=13)


@pytest.mark.parametrize("depth", (8, 10))
def test_a_pixel_step_of_two(engine, depth):
    """one plane with a step of two samples takes the gather; two that interleave alike go as one plane of twice the samples;
    a step on one side only takes the gather again"""
    isz = 2 if depth > 8 else 1
    lut2 = CC.random_lut(2, depth, seed=21)
    for count, src_step2, dst_step2 in ((1, True, True), (2, True, True), (1, True, False), (1, False, True), (2, True, False)):
        sh, sw, oh, ow = 21, 40, 17, 33
        planes = CC.step2_planes(sh, sw, depth, count) if src_step2 else SC.padded(SC.planes_of("444", sh, sw, depth))[0][:count]
        out_planes = CC.step2_planes(oh, ow, depth, count) if dst_step2 else SC.padded(SC.planes_of("444", oh, ow, depth), 2, 6, 4)[0][:count]
        fb, ofb = SC.frame_bytes(planes) + 6, SC.frame_bytes(out_planes) + 4
        frames = SC.content(3, planes, fb, depth, seed=count)
        for origins, lut in (([(2, 5)] * count, None), ([(3, 2)] * count, lut2[:count]), ([(1, 1), (2, 3)][:count], lut2[:count])):
            want = CC.expected(frames, planes, out_planes, ofb, depth, origins, (1, 2, 2, 0), lut)
            got = CC.run(engine, frames, planes, out_planes, ofb, depth, origins, (1, 2, 2, 0), lut)
            assert (got == want).all(), (count, src_step2, dst_step2, origins, isz)


def test_more_rows_than_one_band(engine):
    """a workgroup owns 64 KB of destination rows: 1030 x 70 at 8 bits is 63 rows a band, 600 x 60 at 10 bits is 54"""
    CC.check(engine, "mono", 8, (70, 1030), (1, 3), seed=31, n=2)
    CC.check(engine, "mono", 10, (60, 600), (2, 1), lut=CC.random_lut(1, 10, 4), seed=32, n=2)
    CC.check(engine, "420", 8, (140, 1030), (1, 3), (1, 0), seed=33, n=2)


def test_the_same_bytes_from_any_memory_in_any_batch(engine):
    planes, fb = SC.padded(SC.planes_of("420", 37, 52, 8))
    out_planes, ofb = SC.padded(SC.planes_of("420", 33, 47, 8))
    pool = SC.content(3, planes, fb, 8, seed=99)
    origins = CC.plane_origins("420", (1, 3))
    lut = CC.random_lut(3, 8, seed=1)
    want = CC.expected(pool[:1], planes, out_planes, ofb, 8, origins, None, lut)[0]
    batch = np.stack([pool[0], pool[0], pool[1], pool[2], pool[0]])
    for mem in ("host", "pinned", "device"):
        got = CC.run(engine, batch, planes, out_planes, ofb, 8, origins, None, lut, mem=mem)
        for place in (0, 1, 4):
            assert (got[place] == want).all(), (mem, place)
    # two batch sizes: one frame alone, and the five through an index that names every place
    assert (CC.run(engine, pool[:1], planes, out_planes, ofb, 8, origins, None, lut)[0] == want).all()
    got = CC.run(engine, batch, planes, out_planes, ofb, 8, origins, (4, 3, 0, 0, 1, 2, 4), lut, mem="device")
    for place in (0, 2, 3, 4, 6):
        assert (got[place] == want).all(), place


# ---- chaining: what follows on the same engine reads the conformed frames, with no wait in between -------------------------
def _chain_inputs():
    from rtvqa_amd import synth
    from rtvqa_amd.frames import bgr_to_yuv420p
    h, w, oh, ow = 52, 70, 48, 64
    ref = bgr_to_yuv420p(synth.s_natural(3, h, w, seed=5))
    dist = bgr_to_yuv420p(synth.distort(synth.s_natural(3, h, w, seed=5)))
    planes, out_planes = SC.planes_of("420", h, w), SC.planes_of("420", oh, ow)
    ofb = SC.frame_bytes(out_planes)
    kw_r = dict(origin=CC.plane_origins("420", (2, 4)), index=(0, 1, 1))
    kw_d = dict(origin=CC.plane_origins("420", (0, 2)), index=(2, 1, 0), lut=CC.random_lut(3, 8, seed=2) // 2 + 60)
    want_r = CC.expected(ref, planes, out_planes, ofb, 8, kw_r["origin"], kw_r["index"])
    want_d = CC.expected(dist, planes, out_planes, ofb, 8, kw_d["origin"], kw_d["index"], kw_d["lut"])
    return ref, dist, planes, out_planes, kw_r, kw_d, want_r, want_d


def test_quality_follows_two_conforms_without_a_wait(engine):
    ref, dist, planes, out_planes, kw_r, kw_d, want_r, want_d = _chain_inputs()
    q_want = engine.quality(want_r, want_d, out_planes)
    cr = engine.conform_submit(ref, planes, out_planes, **kw_r)
    engine.conform_wait()
    dd = engine.upload(dist)
    cd = engine.conform_submit(dd, planes, out_planes, **kw_d)
    q = engine.quality(cr, cd, out_planes)          # (no conform_wait)
    engine.conform_wait()
    assert q.tobytes() == q_want.tobytes()
    assert (engine.download(cd) == want_d).all() and (engine.download(cr) == want_r).all()
    assert float(q["sse"].sum()) > 0


def test_a_conform_batch_pends_next_to_another_kinds_batch(engine):
    ref, dist, planes, out_planes, kw_r, kw_d, want_r, want_d = _chain_inputs()
    dref = engine.upload(want_r)
    s_want, g_want = engine.siti(want_r, out_planes), engine.gmsd(want_r, want_d, out_planes)
    engine.siti_submit(dref, out_planes)
    cd = engine.conform_submit(engine.upload(dist), planes, out_planes, **kw_d)
    engine.gmsd_submit(dref, cd, out_planes)
    s = engine.siti_wait()
    g = engine.gmsd_wait()
    engine.conform_wait()
    assert s.tobytes() == s_want.tobytes() and g.tobytes() == g_want.tobytes()


# ---- errors ---------------------------------------------------------------------------------------------------------------
def _raw(engine, src, planes, dst_ptr, out_planes, origin=None, index=None, n_out=0, lut=None, matrix=None, n=None, ofs=None):
    import ctypes as C
    from rtvqa_amd import _native as N
    from rtvqa_amd.engine import DeviceFrames, plane_descs, planes_span
    dev = isinstance(src, DeviceFrames)
    ptr = src.ptr if dev else src.ctypes.data
    n = n if n is not None else (src.n if dev else src.shape[0])
    fs = src.frame_stride if dev else src.strides[0]
    i32 = C.POINTER(C.c_int32)
    o = np.ascontiguousarray(origin, np.int32) if origin is not None else None
    ix = np.ascontiguousarray(index, np.int32) if index is not None else None
    m = np.ascontiguousarray(matrix, np.int64) if matrix is not None else None
    return engine.lib.vqa_conform_submit(engine.ctx, ptr, N.VQA_MEM_DEVICE if dev else N.VQA_MEM_HOST, n, fs, plane_descs(planes),
                                         dst_ptr, ofs if ofs is not None else planes_span(out_planes), plane_descs(out_planes),
                                         len(planes), o.ctypes.data_as(i32) if o is not None else None,
                                         ix.ctypes.data_as(i32) if ix is not None else None, len(ix) if ix is not None else n_out,
                                         lut.ctypes.data if lut is not None else None,
                                         m.ctypes.data_as(C.POINTER(C.c_int64)) if m is not None else None)


def test_limits_and_invalid_arguments_leave_nothing_in_flight(engine):
    from rtvqa_amd import _native as N
    from rtvqa_amd.engine import DeviceBuffer, mono_planes, yuv_planes
    src = np.zeros((2, 64 * 64), np.uint8)
    p64, p32 = mono_planes(64, 64), mono_planes(32, 32)
    buf = DeviceBuffer(engine, 4 * 64 * 64 * 3)
    sub = lambda planes, out_planes, **kw: _raw(engine, kw.pop("src", src), planes, kw.pop("dst", buf.ptr), out_planes, **kw)
    U, I, OK = N.VQA_ERR_UNSUPPORTED, N.VQA_ERR_INVALID, N.VQA_OK
    wait = lambda: engine.lib.vqa_conform_wait(engine.ctx)
    assert sub(p64, mono_planes(15, 64)) == U                           # a side below 16
    assert sub(p64, mono_planes(32, 32, 10)) == U                       # another depth
    assert sub(p64, mono_planes(65, 32)) == I                           # the window leaves the plane
    assert sub(p64, p32, origin=[(33, 0)]) == I and sub(p64, p32, origin=[(0, 33)]) == I and sub(p64, p32, origin=[(-1, 0)]) == I
    assert sub(p64, p32, origin=[(32, 32)]) == OK and wait() == OK      # ... exactly inside
    assert sub(p64, p32, index=[0, 2]) == I and sub(p64, p32, index=[-1]) == I
    assert sub(p64, p32, index=[1, 1, 0, 1]) == OK and wait() == OK
    bad_lut = np.full((1, 1024), 1024, np.uint16)
    assert sub(mono_planes(64, 64, 10), mono_planes(32, 32, 10), src=np.zeros((2, 64 * 64), np.uint16), lut=bad_lut) == I
    ident = [[65536, 0, 0, 0], [0, 65536, 0, 0], [0, 0, 65536, 0]]
    assert sub(p64, p32, matrix=ident) == I                             # a matrix needs three planes
    p444, o444 = yuv_planes(64, 64, "444"), yuv_planes(32, 32, "444")
    src3 = np.zeros((2, 3 * 64 * 64), np.uint8)
    assert sub(p444, o444, src=src3, matrix=ident) == OK and wait() == OK
    for k, i, v in ((0, 0, (1 << 20) + 1), (2, 1, -(1 << 20) - 1), (1, 3, (1 << 33) + 1), (0, 3, -(1 << 33) - 1)):
        m = [row[:] for row in ident]
        m[k][i] = v
        assert sub(p444, o444, src=src3, matrix=m) == I
    m = [row[:] for row in ident]
    m[0][0], m[1][3] = 1 << 20, -(1 << 33)                              # the bounds themselves
    assert sub(p444, o444, src=src3, matrix=m) == OK and wait() == OK
    apart = [p444[0], p444[1], (32, 64) + tuple(p444[2][2:])]           # planes 1 and 2 differ: no joint grid
    assert sub(apart, o444, src=src3, matrix=ident) == I
    assert sub(p64, p32, dst=None) == I and sub(p64, p32, n=0) == I
    assert sub(p64, p32, ofs=32 * 32 - 1) == I                          # frames of the destination overlap each other
    host_dst = np.zeros(2 * 32 * 32, np.uint8)
    assert sub(p64, p32, dst=host_dst.ctypes.data) == I                 # pageable host memory
    dsrc = engine.upload(np.zeros((4, 64 * 64), np.uint8))
    assert sub(p64, p32, src=dsrc, n=2, dst=dsrc.ptr) == I              # the destination IS the source
    assert sub(p64, p32, src=dsrc, n=2, dst=dsrc.ptr + 2 * 64 * 64 - 1) == I
    assert sub(p64, p32, src=dsrc, n=2, dst=dsrc.ptr + 2 * 64 * 64) == OK and wait() == OK
    assert wait() == N.VQA_ERR_STATE                                    # nothing was left in flight
    assert engine.lib.vqa_conform_wait(None) == I
    assert sub(p64, p32) == OK and sub(p64, p32) == N.VQA_ERR_STATE     # a pending batch refuses the next and survives it
    assert wait() == OK and wait() == N.VQA_ERR_STATE
    assert engine.lib.vqa_trim(engine.ctx) == OK
    got = engine.conform(src, p64, p32)                                 # usable afterwards
    assert (engine.download(got) == 0).all()
    buf.free()


def test_python_refuses_before_anything_is_uploaded(engine):
    from rtvqa_amd.engine import mono_planes, yuv_planes
    z8, p64, p32 = np.zeros((2, 64 * 64), np.uint8), mono_planes(64, 64), mono_planes(32, 32)
    with pytest.raises(ValueError):
        engine.conform(np.zeros((1, 64 * 64), np.uint16), p64, p32)                 # the wrong sample type is no cast
    with pytest.raises(ValueError):
        engine.conform(z8, mono_planes(64, 64, 10), mono_planes(32, 32, 10))
    with pytest.raises(ValueError):
        engine.conform(z8, p64, p32, origin=[(40, 0)])
    with pytest.raises(ValueError):
        engine.conform(z8, p64, p32, index=[2])
    with pytest.raises(ValueError):
        engine.conform(z8, p64, p32, lut=np.zeros((1, 255), np.uint8))
    with pytest.raises(ValueError):
        engine.conform(z8, p64, p32, matrix=np.eye(3, 4, dtype=np.int64))
    with pytest.raises(ValueError):
        engine.conform(np.zeros((1, 3 * 64 * 64), np.uint8), yuv_planes(64, 64, "444"), yuv_planes(32, 32, "444"),
                       matrix=np.full((3, 4), 1 << 21, np.int64))
    with pytest.raises(ValueError):
        engine.conform(z8, p64, p32, out=engine.upload(np.zeros((1, 100), np.uint8)))
    with pytest.raises(ValueError):
        engine.conform(z8, p64, p32, out=engine.upload(np.zeros((2, 4096), np.uint16)))
    assert not getattr(engine, "_pending_cm", None)
