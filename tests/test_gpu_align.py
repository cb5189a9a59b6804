"""GPU: temporal alignment (vqa_align_submit / vqa_align_wait) through the C ABI and the engine, against the NumPy restatement
of tests/align_reference.py, which forms (d - r)^2 directly in int64, pair by pair.  EVERY word is compared for equality: the
kernel does integer arithmetic only, so there is no bar to set.  The streams are unrelated random frames (align_cases.clip): a
transposed tile, swapped operands or a band read backwards change words."""
import ctypes as C

import numpy as np
import pytest

import align_cases as AC
import align_reference as R

pytestmark = pytest.mark.gpu


def _want(ref, dist, plane, radius, offset=0, ref_fs=None, dist_fs=None):
    return R.band(R.plane_series(ref, plane, ref_fs), R.plane_series(dist, plane, dist_fs), radius, offset)


def _same(got, want, tag):
    assert got.dtype == np.uint64 and got.shape == want.shape, tag
    bad = np.argwhere(got != want)
    print(tag, "words", got.size, "differing", len(bad))
    assert len(bad) == 0, (tag, bad[:8].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def _pair(n_dist, n_ref, h, w, depth=8, seed=0, full_range=False):
    return AC.clip(n_ref, h, w, depth, 2 * seed + 11, full_range), AC.clip(n_dist, h, w, depth, 2 * seed + 12, full_range)


@pytest.mark.parametrize("w,h", AC.GEOMETRY, ids=["%dx%d" % g for g in AC.GEOMETRY])
def test_geometry(engine, w, h):
    ref, dist = _pair(5, 6, h, w, seed=w)
    planes = AC.mono(w, h)
    _same(engine.align(ref, dist, planes, radius=2), _want(ref, dist, planes[0], 2), "%dx%d" % (w, h))


def test_padded_rows_with_a_one_byte_lead(engine):
    """130 x 5 at row_stride 131, the plane one byte into the frame: every row starts at another alignment"""
    w, h, rs = 130, 5, 131
    plane = (w, h, 1, rs, 1)
    fs = 1 + h * rs
    rng = np.random.default_rng(5)
    ref, dist = rng.integers(0, 256, (7, fs)).astype(np.uint8), rng.integers(0, 256, (6, fs)).astype(np.uint8)
    _same(engine.align(ref, dist, [plane], radius=3, offset=1), _want(ref, dist, plane, 3, 1), "130x5 stride 131 lead 1")


def test_a_frame_whose_last_row_ends_its_allocation(engine):
    """device frames in allocations of exactly (n - 1) frame_stride + 1 + (h - 1) row_stride + w bytes: the last row of the last
    frame has no padding behind it, and no byte past it may be read"""
    from rtvqa_amd.engine import DeviceBuffer, DeviceFrames
    w, h, rs = 130, 5, 131
    plane = (w, h, 1, rs, 1)
    fs = 1 + h * rs
    rng = np.random.default_rng(6)
    streams, host = [], []
    for n in (4, 3):
        nbytes = (n - 1) * fs + 1 + (h - 1) * rs + w
        a = rng.integers(0, 256, nbytes).astype(np.uint8)
        buf = DeviceBuffer(engine, nbytes)
        engine.h2d_async(buf.ptr, a.ctypes.data, nbytes)
        engine.sync()
        streams.append(DeviceFrames(buf.ptr, n, h, rs, frame_stride=fs, row_stride=rs, owner=buf, channels=1))
        host.append(a)
    got = engine.align(streams[0], streams[1], [plane], radius=2)
    _same(got, _want(host[0], host[1], plane, 2, 0, fs, fs), "last row ends the allocation")
    for s in streams:
        s._owner.free()


@pytest.mark.parametrize("n_dist,n_ref,offset,radius", AC.COUNTS + [AC.OUT_OF_RANGE], ids=lambda v: str(v))
def test_frame_counts_and_band(engine, n_dist, n_ref, offset, radius):
    h, w = 19, 37
    ref, dist = _pair(n_dist, n_ref, h, w, seed=n_dist + radius)
    planes = AC.mono(w, h)
    got = engine.align(ref, dist, planes, radius=radius, offset=offset)
    _same(got, _want(ref, dist, planes[0], radius, offset), str((n_dist, n_ref, offset, radius)))
    if (n_dist, n_ref, offset, radius) == AC.OUT_OF_RANGE:
        assert (got == R.NONE).all()


@pytest.mark.parametrize("w,h", AC.RANGE_PLANES, ids=["%dx%d" % g for g in AC.RANGE_PLANES])
@pytest.mark.parametrize("depth", sorted(AC.RANGE_LEVELS))
def test_accumulator_range(engine, w, h, depth):
    """flat planes at the ends of the range (align_cases.RANGE_PLANES says which sizes of the kernel they span): the largest
    products, all of one sign, as many as a wave sees between two flushes and more"""
    planes = AC.mono(w, h, depth)
    for d_level, r_level in AC.RANGE_LEVELS[depth]:
        ref = np.full((1, h, w), r_level, AC.dtype_of(depth))
        dist = np.full((1, h, w), d_level, AC.dtype_of(depth))
        got = engine.align(ref, dist, planes, radius=0)
        assert int(got[0, 0]) == (d_level - r_level) ** 2 * w * h, (w, h, depth, d_level, r_level, int(got[0, 0]))


@pytest.mark.parametrize("depth,full_range", [(d, False) for d in AC.DEPTHS] + [(10, True)],
                         ids=["%d" % d for d in AC.DEPTHS] + ["10-above-peak"])
def test_depths(engine, depth, full_range):
    h, w = 19, 37
    ref, dist = _pair(6, 7, h, w, depth, seed=depth, full_range=full_range)
    planes = AC.mono(w, h, depth)
    _same(engine.align(ref, dist, planes, radius=3, offset=-1), _want(ref, dist, planes[0], 3, -1), "depth %d" % depth)


def test_one_channel_of_packed_bgr_host_and_device(engine):
    """the G channel of packed BGR, pixel_step = 3 (the gather path), from host arrays and from device frames"""
    from rtvqa_amd.engine import bgr_planes
    h, w = 9, 21
    rng = np.random.default_rng(9)
    ref, dist = rng.integers(0, 256, (5, h, w, 3)).astype(np.uint8), rng.integers(0, 256, (4, h, w, 3)).astype(np.uint8)
    planes = bgr_planes(h, w)
    want = _want(ref, dist, planes[1], 2)
    _same(engine.align(ref, dist, planes, radius=2, plane=1), want, "bgr G host")
    _same(engine.align(engine.upload(ref), engine.upload(dist), planes, radius=2, plane=1), want, "bgr G device")


def test_a_frame_stride_larger_than_the_frame_and_two_strides(engine):
    h, w = 7, 40
    planes = AC.mono(w, h)
    rng = np.random.default_rng(10)
    ref, dist = rng.integers(0, 256, (5, h * w + 13)).astype(np.uint8), rng.integers(0, 256, (6, h * w + 50)).astype(np.uint8)
    got = engine.align(ref, dist, planes, radius=1, frame_bytes=h * w + 13, dist_frame_bytes=h * w + 50)
    _same(got, _want(ref, dist, planes[0], 1), "strides 293 and 330")


def test_a_roi_view(engine):
    h, w = 24, 50
    ref, dist = _pair(4, 5, h, w, seed=77)
    dr, dd = engine.upload(ref).roi(3, 20, 7, 44), engine.upload(dist).roi(3, 20, 7, 44)
    plane = (37, 17, 0, w, 1)
    want = R.band(ref[:, 3:20, 7:44].astype(np.int64), dist[:, 3:20, 7:44].astype(np.int64), 2)
    _same(engine.align(dr, dd, [plane], radius=2), want, "roi")


def test_windows_give_the_array_of_one_submit(engine):
    """one submit of 48 x 48 frames against frame_align's windows of 7 and of 16"""
    from rtvqa_amd import video_processing as vp
    h, w = 19, 37
    ref, dist = _pair(48, 48, h, w, seed=48)
    whole = engine.align(ref, dist, AC.mono(w, h), radius=8)
    _same(whole, _want(ref, dist, AC.mono(w, h)[0], 8), "48 x 48")
    for window in (7, 16):
        got = vp.frame_align(ref, dist, "gray", radius=8, engine=engine, window=window)["sse"]
        assert (got == whole).all(), window


def test_next_to_a_gmsd_batch_and_identical_streams(engine):
    h, w = 19, 37
    ref, dist = _pair(6, 6, h, w, seed=3)
    planes = AC.mono(w, h)
    alone = engine.align(ref, dist, planes, radius=2)
    g_alone = engine.gmsd(ref.reshape(6, -1), dist.reshape(6, -1), planes)
    engine.gmsd_submit(ref.reshape(6, -1), dist.reshape(6, -1), planes)
    engine.align_submit(ref, dist, planes, radius=2)
    g = engine.gmsd_wait()
    got = engine.align_wait()
    assert (got == alone).all() and g.tobytes() == g_alone.tobytes()
    same = engine.align(ref, ref, planes, radius=2)
    assert (same[:, 2] == 0).all() and (same[:, 1][1:] != 0).all()


def test_state_and_argument_errors(engine):
    from rtvqa_amd import _native as N
    ref, dist = _pair(2, 2, 4, 4, seed=1)
    planes = AC.mono(4, 4)
    with pytest.raises(N.VqaError) as e:
        engine.align_wait()
    assert e.value.status == N.VQA_ERR_STATE
    engine.align_submit(ref, dist, planes, radius=1)
    with pytest.raises(N.VqaError) as e:
        engine.align_submit(ref, dist, planes, radius=1)
    assert e.value.status == N.VQA_ERR_STATE
    one = np.zeros(1, np.uint64)
    assert engine.lib.vqa_align_wait(engine.ctx, one.ctypes.data_as(C.POINTER(C.c_uint64)), 1) == N.VQA_ERR_STATE   # 6 words pend
    assert engine.align_wait().shape == (2, 3)
    for radius in (-1, 33):
        with pytest.raises(N.VqaError) as e:
            engine.align(ref, dist, planes, radius=radius)
        assert e.value.status == N.VQA_ERR_INVALID
    many = np.zeros((N.ALIGN_MAX_DIST + 1, 1), np.uint8)
    with pytest.raises(N.VqaError) as e:
        engine.align(ref[:, :1, :1].reshape(2, 1), many, AC.mono(1, 1), radius=0)
    assert e.value.status == N.VQA_ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        engine.align(ref.astype(np.uint16), dist, planes)
    assert engine.align(ref, dist, planes, radius=0).shape == (2, 1)   # the engine is usable after every refusal
