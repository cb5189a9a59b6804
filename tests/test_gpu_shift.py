"""GPU: spatial registration (vqa_shift_submit / vqa_shift_wait) through the C ABI and the engine, against the NumPy restatement
of tests/shift_reference.py, which forms (d - r)^2 directly in int64, shift by shift.  EVERY word is compared for equality: the
kernel does integer arithmetic only, so there is no bar to set.  The streams are unrelated random frames (shift_cases.pair): a
transposed tile, swapped operands, a grid read backwards or dy taken for dx change words.  tests/test_shift_host.py shows on the
CPU where the smallest word of every case lies and that it is the only one."""
import ctypes as C

import numpy as np
import pytest

import shift_cases as SC
import shift_reference as R

pytestmark = pytest.mark.gpu


def _want(ref, dist, plane, radius, margin=None, ref_fs=None, dist_fs=None):
    return R.grids(R.plane_series(ref, plane, ref_fs), R.plane_series(dist, plane, dist_fs), radius, margin)


def _same(got, want, tag):
    assert got.dtype == np.uint64 and got.shape == want.shape, tag
    bad = np.argwhere(got != want)
    print(tag, "words", got.size, "differing", len(bad))
    assert len(bad) == 0, (tag, bad[:8].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


_ids = ["%dx%d-R%d-M%d-%dbit" % c for c in SC.GEOMETRY]


@pytest.mark.parametrize("case", SC.GEOMETRY, ids=_ids)
def test_geometry(engine, case):
    """a core of one sample; the widths about one matrix step; the heights about SHIFT_ROWS; one, four and nine tiles; M > R"""
    w, h, radius, margin, depth = case
    ref, dist = SC.pair(case)
    planes = SC.mono(w, h, depth)
    _same(engine.shift(ref, dist, planes, radius, margin), _want(ref, dist, planes[0], radius, margin), str(case))


@pytest.mark.parametrize("case", SC.DEPTHS, ids=["%dx%d-R%d-M%d-%dbit" % c for c in SC.DEPTHS])
def test_depths(engine, case):
    w, h, radius, margin, depth = case
    ref, dist = SC.pair(case, n=3)
    planes = SC.mono(w, h, depth)
    _same(engine.shift(ref, dist, planes, radius, margin), _want(ref, dist, planes[0], radius, margin), str(case))
    if depth == 10:   # samples above 2^depth - 1 are read as they are
        ref, dist = SC.clip(2, h, w, depth, 5, full_range=True), SC.clip(2, h, w, depth, 6, full_range=True)
        _same(engine.shift(ref, dist, planes, radius, margin), _want(ref, dist, planes[0], radius, margin), "above peak")


@pytest.mark.parametrize("depth", [8, 12])
def test_padded_rows_that_start_at_odd_addresses(engine, depth):
    """130 x 11 at a row stride of 131 samples, the plane one sample into the frame: at 8 bits every row starts at another
    alignment and every second one at an odd address"""
    bps = 2 if depth > 8 else 1
    w, h, rs = 130, 11, 131 * bps
    plane = (w, h, bps, rs, bps) + ((depth,) if depth > 8 else ())
    fs = bps + h * rs
    rng = np.random.default_rng(5)
    ref, dist = (rng.integers(0, 256, (3, fs)).astype(np.uint8) for _ in range(2))
    if depth > 8:
        ref, dist = ref.view(np.uint16), dist.view(np.uint16)
    _same(engine.shift(ref, dist, [plane], 3, 4), _want(ref, dist, plane, 3, 4), "130x11 stride 131 lead 1, %d bits" % depth)


def test_a_frame_whose_last_row_ends_its_allocation(engine):
    """device frames in allocations of exactly (n - 1) frame_stride + 1 + (h - 1) row_stride + w bytes: the last row of the last
    frame has no padding behind it, and no byte past it may be read (the widest shift reads up to its last sample)"""
    from rtvqa_amd.engine import DeviceBuffer, DeviceFrames
    w, h, rs, n = 130, 9, 131, 3
    plane = (w, h, 1, rs, 1)
    fs = 1 + h * rs
    rng = np.random.default_rng(6)
    streams, host = [], []
    for _ in range(2):
        nbytes = (n - 1) * fs + 1 + (h - 1) * rs + w
        a = rng.integers(0, 256, nbytes).astype(np.uint8)
        buf = DeviceBuffer(engine, nbytes)
        engine.h2d_async(buf.ptr, a.ctypes.data, nbytes)
        engine.sync()
        streams.append(DeviceFrames(buf.ptr, n, h, rs, frame_stride=fs, row_stride=rs, owner=buf, channels=1))
        host.append(a)
    got = engine.shift(streams[0], streams[1], [plane], radius=2)
    _same(got, _want(host[0], host[1], plane, 2, None, fs, fs), "last row ends the allocation")
    for s in streams:
        s._owner.free()


def test_one_channel_of_packed_bgr_host_and_device(engine):
    """the G channel of packed BGR, pixel_step = 3 (the gather path), from host arrays and from device frames"""
    from rtvqa_amd.engine import bgr_planes
    h, w = 13, 75
    rng = np.random.default_rng(9)
    ref, dist = (rng.integers(0, 256, (3, h, w, 3)).astype(np.uint8) for _ in range(2))
    planes = bgr_planes(h, w)
    want = _want(ref, dist, planes[1], 2)
    assert (want == R.grids(ref[..., 1].astype(np.int64), dist[..., 1].astype(np.int64), 2)).all()
    _same(engine.shift(ref, dist, planes, radius=2, plane=1), want, "bgr G host")
    _same(engine.shift(engine.upload(ref), engine.upload(dist), planes, radius=2, plane=1), want, "bgr G device")


def test_two_frame_strides(engine):
    h, w = 9, 40
    planes = SC.mono(w, h)
    rng = np.random.default_rng(10)
    ref, dist = rng.integers(0, 256, (4, h * w + 13)).astype(np.uint8), rng.integers(0, 256, (4, h * w + 50)).astype(np.uint8)
    got = engine.shift(ref, dist, planes, radius=1, frame_bytes=h * w + 13, dist_frame_bytes=h * w + 50)
    _same(got, _want(ref, dist, planes[0], 1), "strides 373 and 410")


@pytest.mark.parametrize("case", SC.TRANSLATED, ids=["%dx%d-R%d-M%d-%s" % c for c in SC.TRANSLATED])
def test_a_translated_reference_gives_zero_there_and_nowhere_else(engine, case):
    w, h, radius, margin, (dy, dx) = case
    ref, dist = SC.translated_pair(case)
    got = engine.shift(ref, dist, SC.mono(w, h), radius, margin)
    _same(got, R.grids(ref.astype(np.int64), dist.astype(np.int64), radius, margin), str(case))
    for g in got:
        assert g[dy + radius, dx + radius] == 0 and (g == 0).sum() == 1


def test_identical_frames(engine):
    w, h = 45, 19
    for depth in (8, 16):
        ref = SC.clip(3, h, w, depth, 21)
        got = engine.shift(ref, ref.copy(), SC.mono(w, h, depth), 3)
        _same(got, R.grids(ref.astype(np.int64), ref.astype(np.int64), 3), "identical, %d bits" % depth)
        assert (got[:, 3, 3] == 0).all() and ((got == 0).sum(axis=(1, 2)) == 1).all()


@pytest.mark.parametrize("d_level,r_level", SC.RANGE_LEVELS + [(0, 0)], ids=lambda v: str(v))
def test_accumulator_range(engine, d_level, r_level):
    """flat 16-bit planes at the ends of the range on shift_cases.RANGE_PLANE: the largest products, all of one sign, on a
    plane whose first visit of SHIFT_ROWS = 8 rows is at least 8 * 130 = 1040 matrix steps - every 32-bit accumulator of that wave is
    flushed at step 512 and at step 1024 before the visit ends.  (0, 0) is X = -32896 on both sides: bytes of -128, the largest
    product of all, 2 * 64 * 512 * 2^14 = 2^30 in the accumulator HL and LH share.)  Every word is (d - r)^2 times the core."""
    w, h, radius, margin = SC.RANGE_PLANE
    ref = np.full((1, h, w), r_level, np.uint16)
    dist = np.full((1, h, w), d_level, np.uint16)
    got = engine.shift(ref, dist, SC.mono(w, h, 16), radius, margin)
    want = (d_level - r_level) ** 2 * (w - 2 * margin) * (h - 2 * margin)
    print(d_level, r_level, "want", want, "got", sorted(set(int(v) for v in got.reshape(-1))))
    assert got.shape == (1, 3, 3) and all(int(v) == want for v in got.reshape(-1))


def test_batch_independence(engine):
    """n = 1, 16, 17: frame j alone gives the words it has in every batch, at any position"""
    w, h, radius = 45, 19, 3
    planes = SC.mono(w, h)
    ref, dist = SC.clip(17, h, w, 8, 41), SC.clip(17, h, w, 8, 42)
    want = R.grids(ref.astype(np.int64), dist.astype(np.int64), radius)
    whole = engine.shift(ref, dist, planes, radius)
    _same(whole, want, "n = 17")
    _same(engine.shift(ref[:16], dist[:16], planes, radius), want[:16], "n = 16")
    for j in (0, 15, 16):
        _same(engine.shift(ref[j:j + 1], dist[j:j + 1], planes, radius), want[j:j + 1], "frame %d alone" % j)
    back = engine.shift(ref[::-1], dist[::-1], planes, radius)
    _same(back, want[::-1], "the batch reversed")


def test_a_radius_inside_a_larger_one(engine):
    """R = 4 is the centre of R = 8 at the same M (one tile against four), and R = 15 the centre of R = 16 (four against nine)"""
    for small, large, w, h in ((4, 8, 40, 30), (15, 16, 50, 41)):
        ref, dist = SC.clip(2, h, w, 8, 51 + small), SC.clip(2, h, w, 8, 52 + small)
        planes = SC.mono(w, h)
        a, b = engine.shift(ref, dist, planes, small, large), engine.shift(ref, dist, planes, large, large)
        k = large - small
        assert (a == b[:, k:-k, k:-k]).all()
        _same(b, R.grids(ref.astype(np.int64), dist.astype(np.int64), large), "R = %d" % large)


def test_host_pinned_and_device_memory_and_a_roi_view(engine):
    h, w = 30, 50
    ref, dist = SC.clip(3, h, w, 8, 61), SC.clip(3, h, w, 8, 62)
    planes = SC.mono(w, h)
    want = R.grids(ref.astype(np.int64), dist.astype(np.int64), 2, 3)
    _same(engine.shift(ref, dist, planes, 2, 3), want, "host")
    pr, pd = engine.alloc_pinned(ref.shape), engine.alloc_pinned(dist.shape)
    pr[...], pd[...] = ref, dist
    assert engine.is_pinned(pr) and engine.is_pinned(pd)
    _same(engine.shift(pr, pd, planes, 2, 3), want, "pinned")
    engine.free_pinned(pr)
    engine.free_pinned(pd)
    dr, dd = engine.upload(ref), engine.upload(dist)
    _same(engine.shift(dr, dd, planes, 2, 3), want, "device")
    plane = (37, 21, 0, w, 1)
    want = R.grids(ref[:, 3:24, 7:44].astype(np.int64), dist[:, 3:24, 7:44].astype(np.int64), 2)
    _same(engine.shift(dr.roi(3, 24, 7, 44), dd.roi(3, 24, 7, 44), [plane], 2), want, "roi")


def test_windows_give_the_array_of_one_submit(engine):
    from rtvqa_amd import video_processing as vp
    h, w = 19, 37
    ref, dist = SC.clip(11, h, w, 8, 71), SC.clip(11, h, w, 8, 72)
    whole = engine.shift(ref, dist, SC.mono(w, h), 2)
    for window in (1, 4, 11):
        res = vp.frame_shift(ref, dist, "gray", radius=2, engine=engine, window=window)
        assert res["sse"].dtype == np.uint64 and (res["sse"] == whole).all(), window


def test_next_to_a_gmsd_and_an_align_batch(engine):
    h, w = 19, 37
    ref, dist = SC.clip(6, h, w, 8, 81), SC.clip(6, h, w, 8, 82)
    planes = SC.mono(w, h)
    alone = engine.shift(ref, dist, planes, 2)
    _same(alone, R.grids(ref.astype(np.int64), dist.astype(np.int64), 2), "alone")
    g_alone = engine.gmsd(ref.reshape(6, -1), dist.reshape(6, -1), planes)
    a_alone = engine.align(ref, dist, planes, radius=2)
    engine.gmsd_submit(ref.reshape(6, -1), dist.reshape(6, -1), planes)
    engine.shift_submit(ref, dist, planes, 2)
    engine.align_submit(ref, dist, planes, radius=2)
    g = engine.gmsd_wait()
    got = engine.shift_wait()
    a = engine.align_wait()
    assert (got == alone).all() and g.tobytes() == g_alone.tobytes() and (a == a_alone).all()


def test_state_and_argument_errors(engine):
    from rtvqa_amd import _native as N
    ref, dist = SC.clip(2, 9, 9, 8, 1), SC.clip(2, 9, 9, 8, 2)
    planes = SC.mono(9, 9)

    def status(call):
        with pytest.raises(N.VqaError) as e:
            call()
        return e.value.status

    assert status(engine.shift_wait) == N.VQA_ERR_STATE
    engine.shift_submit(ref, dist, planes, radius=1)
    assert status(lambda: engine.shift_submit(ref, dist, planes, radius=1)) == N.VQA_ERR_STATE
    one = np.zeros(1, np.uint64)
    assert engine.lib.vqa_shift_wait(engine.ctx, one.ctypes.data_as(C.POINTER(C.c_uint64)), 1) == N.VQA_ERR_STATE   # 18 words pend
    assert engine.shift_wait().shape == (2, 3, 3)
    for radius, margin in ((0, None), (-1, None), (17, None), (2, 1), (4, 3)):
        assert status(lambda: engine.shift(ref, dist, planes, radius, margin)) == N.VQA_ERR_INVALID, (radius, margin)
    assert engine.shift(ref, dist, planes, 4).shape == (2, 9, 9)                       # h = w = 2M + 1: a core of one sample
    for radius, margin in ((5, None), (1, 5), (16, None), (1, 1 << 30), (1, (1 << 31) - 1)):   # h, w < 2M + 1
        assert status(lambda: engine.shift(ref, dist, planes, radius, margin)) == N.VQA_ERR_UNSUPPORTED, (radius, margin)
    wide = np.zeros((1, 3, (1 << 28) // 3 + 1), np.uint8)                               # h w > 2^28
    assert status(lambda: engine.shift(wide, wide, SC.mono(wide.shape[2], 3), 1)) == N.VQA_ERR_UNSUPPORTED
    many = np.zeros((N.SHIFT_MAX_FRAMES + 1, 9), np.uint8)
    assert status(lambda: engine.shift(many, many, SC.mono(3, 3), 1)) == N.VQA_ERR_UNSUPPORTED
    assert status(lambda: engine.shift(ref, dist, planes, 1, frame_bytes=80)) == N.VQA_ERR_INVALID   # a stride below the span
    with pytest.raises(ValueError):
        engine.shift(ref.astype(np.uint16), dist, planes)
    with pytest.raises(ValueError):
        engine.shift(ref, dist[:1], planes)
    with pytest.raises(TypeError):
        engine.shift(engine.upload(ref), dist, planes)
    assert (engine.shift(ref, dist, planes, 1) == R.grids(ref.astype(np.int64), dist.astype(np.int64), 1)).all()   # usable after every refusal
