"""GPU: clip-wide sync (vqa_sig_submit / vqa_sig_wait, vqa_sig_cross_submit / vqa_sig_cross_wait) through the C ABI and the
engine, against the NumPy restatement of tests/sync_reference.py: cells by slicing and `//` in uint64, D as the direct squared
difference in int64.  EVERY byte and EVERY word is compared for equality: the kernels do integer arithmetic only, so there is no
bar to set.  The clips are unrelated random frames (sync_cases): a transposed tile or swapped operands change words."""
import ctypes as C

import numpy as np
import pytest

import sync_cases as SC
import sync_reference as R

pytestmark = pytest.mark.gpu


def _same(got, want, tag):
    assert got.dtype == want.dtype and got.shape == want.shape, (tag, got.dtype, got.shape, want.shape)
    bad = np.argwhere(got != want)
    print(tag, "values", got.size, "differing", len(bad))
    assert len(bad) == 0, (tag, bad[:8].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


# ---- signatures: geometry and depths -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", SC.GEOMETRY, ids=["%dx%d" % (w, h) for h, w in SC.GEOMETRY])
def test_geometry(engine, h, w):
    frames = SC.clip(3, h, w, 8, seed=h + w)
    got = engine.signature(frames, SC.mono(w, h))
    _same(got, R.signatures(frames), "%dx%d" % (w, h))
    if (h, w) == (16, 16):
        assert (got == frames.reshape(3, 256)).all()


def test_padded_rows_with_a_one_byte_lead(engine):
    """130 x 21 at row_stride 131, the plane one byte into the frame: every row starts at another alignment"""
    h, w, rs, lead = SC.PADDED
    plane = (w, h, lead, rs, 1)
    frames = np.random.default_rng(5).integers(0, 256, (4, lead + h * rs)).astype(np.uint8)
    _same(engine.signature(frames, [plane]), R.signatures(R.plane_series(frames, plane)), "130x21 stride 131 lead 1")


def test_wide_rows_at_odd_addresses(engine):
    """300 x 18 at row_stride 301 with a one-byte lead: the 16-byte loads of the wide path start at every alignment"""
    h, w, rs = 18, 300, 301
    plane = (w, h, 1, rs, 1)
    frames = np.random.default_rng(6).integers(0, 256, (3, 1 + h * rs)).astype(np.uint8)
    _same(engine.signature(frames, [plane]), R.signatures(R.plane_series(frames, plane)), "300x18 stride 301 lead 1")


@pytest.mark.parametrize("depth", SC.DEPTHS)
@pytest.mark.parametrize("h,w", [(19, 37), (20, 1030)], ids=["37x19", "1030x20"])
def test_depths_with_samples_above_the_peak(engine, depth, h, w):
    frames = SC.clip(3, h, w, depth, seed=depth, full_range=True)   # over all of uint16: the min clamps
    got = engine.signature(frames, SC.mono(w, h, depth))
    _same(got, R.signatures(frames, depth), "depth %d %dx%d" % (depth, w, h))
    assert depth == 16 or (got == 255).any()
    inside = SC.clip(2, h, w, depth, seed=depth + 100)
    _same(engine.signature(inside, SC.mono(w, h, depth)), R.signatures(inside, depth), "depth %d in range" % depth)


def test_ten_bits_on_one_sample_cells(engine):
    x = SC.clip(2, 16, 16, 10, seed=10)
    assert (engine.signature(x, SC.mono(16, 16, 10)) == (x >> 2).reshape(2, 256)).all()


# ---- signatures: memory and batching ---------------------------------------------------------------------------------------------------
def test_one_channel_of_packed_bgr_host_and_device(engine):
    """the G channel of packed BGR, pixel_step = 3 (the gather path), from host arrays and from device frames"""
    from rtvqa_amd.engine import bgr_planes
    h, w = 21, 300
    frames = np.random.default_rng(9).integers(0, 256, (4, h, w, 3)).astype(np.uint8)
    planes = bgr_planes(h, w)
    want = R.signatures(frames[..., 1])
    _same(engine.signature(frames, planes, plane=1), want, "bgr G host")
    _same(engine.signature(engine.upload(frames), planes, plane=1), want, "bgr G device")
    _same(engine.signature(frames, planes), R.signatures(frames[..., 0]), "bgr B host")


def test_a_frame_whose_last_row_ends_its_allocation(engine):
    """device frames in an allocation of exactly (n - 1) frame_stride + 1 + (h - 1) row_stride + w bytes: the last row of the
    last frame has no padding behind it, and no byte past it may be read; 130 is the narrow path, 300 the wide one"""
    from rtvqa_amd.engine import DeviceBuffer, DeviceFrames
    for w in (130, 300):
        h, rs, n = 21, w + 1, 3
        plane = (w, h, 1, rs, 1)
        fs = 1 + h * rs
        nbytes = (n - 1) * fs + 1 + (h - 1) * rs + w
        a = np.random.default_rng(w).integers(0, 256, nbytes).astype(np.uint8)
        buf = DeviceBuffer(engine, nbytes)
        engine.h2d_async(buf.ptr, a.ctypes.data, nbytes)
        engine.sync()
        dev = DeviceFrames(buf.ptr, n, h, rs, frame_stride=fs, row_stride=rs, owner=buf, channels=1)
        _same(engine.signature(dev, [plane]), R.signatures(R.plane_series(a, plane, fs)), "last row ends the allocation, w %d" % w)
        buf.free()


def test_two_frame_strides(engine):
    h, w = 19, 37
    planes = SC.mono(w, h)
    rng = np.random.default_rng(10)
    for pad in (13, 50):
        frames = rng.integers(0, 256, (5, h * w + pad)).astype(np.uint8)
        got = engine.signature(frames, planes, frame_bytes=h * w + pad)
        _same(got, R.signatures(frames[:, :h * w].reshape(5, h, w)), "frame stride %d" % (h * w + pad))


def test_a_roi_view(engine):
    h, w = 40, 60
    frames = SC.clip(4, h, w, 8, seed=77)
    dev = engine.upload(frames).roi(3, 36, 7, 54)
    _same(engine.signature(dev, [(47, 33, 0, w, 1)]), R.signatures(frames[:, 3:36, 7:54]), "roi")


def test_windows_of_seven_frames_give_the_bytes_of_one_submit(engine):
    from rtvqa_amd import video_processing as vp
    frames = SC.clip(30, 19, 37, 8, seed=30)
    whole = engine.signature(frames, SC.mono(37, 19))
    _same(whole, R.signatures(frames), "30 frames")
    parts = np.concatenate([engine.signature(frames[a:a + 7], SC.mono(37, 19)) for a in range(0, 30, 7)])
    assert (parts == whole).all()
    res = vp.frame_sync(frames, frames[4:20], "gray", engine=engine, window=7)
    assert (res["ref_sig"] == whole).all() and (res["dist_sig"] == whole[4:20]).all() and res["offset"] == 4


def test_cell_sums_beyond_32_bits(engine):
    """one flat uint16 frame of 4112 x 4100 at 65535: a cell of 257 x 256 = 65792 samples sums to 65792 * 65535 > 2^32"""
    h, w = 4112, 4100
    assert (h // 16) * (w // 16) * 65535 > 2 ** 32
    frame = np.full((1, h, w), 65535, np.uint16)
    assert (engine.signature(frame, SC.mono(w, h, 16)) == 255).all()
    frame[0, :, :] = 40000   # below the clamp: 40000 >> 8 = 156 from every cell, 256 or 257 samples wide
    assert (engine.signature(frame, SC.mono(w, h, 16)) == 156).all()


def test_flat_planes_at_zero(engine):
    for depth, h, w in ((8, 16, 16), (8, 20, 1030), (12, 37, 19), (16, 20, 1030)):
        z = np.zeros((2, h, w), SC.dtype_of(depth))
        assert (engine.signature(z, SC.mono(w, h, depth)) == 0).all()


def test_pending_next_to_a_gmsd_batch(engine):
    h, w = 19, 37
    ref, dist = SC.clip(6, h, w, 8, 3), SC.clip(6, h, w, 8, 4)
    planes = SC.mono(w, h)
    alone = engine.signature(dist, planes)
    x_alone = engine.sig_cross(alone, engine.signature(ref, planes))
    g_alone = engine.gmsd(ref.reshape(6, -1), dist.reshape(6, -1), planes)
    engine.gmsd_submit(ref.reshape(6, -1), dist.reshape(6, -1), planes)
    engine.signature_submit(dist, planes)
    engine.sig_cross_submit(alone, R.signatures(ref))
    g = engine.gmsd_wait()
    x = engine.sig_cross_wait()
    got = engine.signature_wait()
    assert (got == alone).all() and g.tobytes() == g_alone.tobytes()
    assert (x[0] == x_alone[0]).all() and (x[1] == x_alone[1]).all()


def test_state_errors_and_small_planes(engine):
    from rtvqa_amd import _native as N
    frames = SC.clip(2, 16, 16, 8, seed=1)
    planes = SC.mono(16, 16)
    with pytest.raises(N.VqaError) as e:
        engine.signature_wait()
    assert e.value.status == N.VQA_ERR_STATE
    engine.signature_submit(frames, planes)
    with pytest.raises(N.VqaError) as e:
        engine.signature_submit(frames, planes)
    assert e.value.status == N.VQA_ERR_STATE
    one = np.zeros(256, np.uint8)
    assert engine.lib.vqa_sig_wait(engine.ctx, one.ctypes.data, 1) == N.VQA_ERR_STATE   # two frames pend
    assert engine.signature_wait().shape == (2, 256)
    for h, w in ((15, 16), (16, 15), (1, 1), (8, 300)):
        with pytest.raises(N.VqaError) as e:
            engine.signature(np.zeros((1, h, w), np.uint8), SC.mono(w, h))
        assert e.value.status == N.VQA_ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        engine.signature(frames.astype(np.uint16), planes)
    with pytest.raises(ValueError):
        engine.signature(frames, SC.mono(16, 16, 10))
    # more frames than one submit takes: the count is refused before anything is read (the array holds 2 frames)
    assert engine.lib.vqa_sig_submit(engine.ctx, frames.ctypes.data, N.VQA_MEM_HOST, N.SIG_MAX_BATCH + 1, 256,
                                     _descs(planes)) == N.VQA_ERR_UNSUPPORTED
    assert engine.signature(frames, planes).shape == (2, 256)   # the engine is usable after every refusal


def _descs(planes):
    from rtvqa_amd.engine import plane_descs
    return plane_descs(planes)


# ---- the cross ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_dist,n_ref", SC.COUNTS, ids=lambda v: str(v))
def test_counts(engine, n_dist, n_ref):
    d, r = SC.random_sigs(n_dist, 2 * n_dist + 1), SC.random_sigs(n_ref, 2 * n_ref + 2)
    diag, best = engine.sig_cross(d, r)
    want = (R.cross_fast if max(n_dist, n_ref) >= SC.BIG else R.cross)(d, r)
    _same(diag, want[0], "diag %d x %d" % (n_dist, n_ref))
    _same(best, want[1], "best %d x %d" % (n_dist, n_ref))


def test_the_largest_distance(engine):
    """all-0 against all-255 rows: every D is 256 * 255^2 = 16646400, the largest; 20 x 37 rows pad tiles on both sides"""
    d, r = np.zeros((20, 256), np.uint8), np.full((37, 256), 255, np.uint8)
    for a, b in ((d, r), (r, d)):
        diag, best = engine.sig_cross(a, b)
        want = R.cross(a, b)
        _same(diag, want[0], "diag")
        _same(best, want[1], "best")
        assert (best == np.uint64(16646400 << 32)).all() and int(diag.max()) == 20 * 16646400


def test_identical_arrays_and_the_mirror(engine):
    a, b = SC.random_sigs(40, 40), SC.random_sigs(25, 41)
    diag, best = engine.sig_cross(a, a)
    assert int(diag[39]) == 0 and (diag[:39] != 0).all() and (diag[40:] != 0).all()
    assert (best == np.arange(40, dtype=np.uint64)).all()
    assert (diag == diag[::-1]).all()
    d1, _ = engine.sig_cross(a, b)
    d2, _ = engine.sig_cross(b, a)
    assert (d1 == d2[::-1]).all() and (d1 == R.cross(a, b)[0]).all()


def test_duplicated_reference_rows_tie_to_the_smaller_index(engine):
    """every reference row appears three times: 16 apart (the same lane of two tiles), and 5 further (another lane)"""
    base = SC.random_sigs(16, 7)
    r = np.concatenate([base, base, np.roll(base, 5, axis=0)])
    d = base[::-1].copy()
    diag, best = engine.sig_cross(d, r)
    assert (best == np.arange(15, -1, -1, dtype=np.uint64)).all()
    want = R.cross(d, r)
    _same(diag, want[0], "diag")
    _same(best, want[1], "best")
    # a tie inside one tile between lanes, at a non-zero distance
    d2 = SC.random_sigs(3, 8)
    r2 = np.concatenate([SC.random_sigs(4, 9), d2[1:2] ^ 1, SC.random_sigs(6, 10), d2[1:2] ^ 1])
    _same(engine.sig_cross(d2, r2)[1], R.cross(d2, r2)[1], "best, a tie at distance 256")


def test_cross_state_errors_and_counts_beyond_the_limit(engine):
    from rtvqa_amd import _native as N
    a = SC.random_sigs(3, 1)
    with pytest.raises(N.VqaError) as e:
        engine.sig_cross_wait()
    assert e.value.status == N.VQA_ERR_STATE
    engine.sig_cross_submit(a, a[:2])
    with pytest.raises(N.VqaError) as e:
        engine.sig_cross_submit(a, a)
    assert e.value.status == N.VQA_ERR_STATE
    w = np.zeros(8, np.uint64)
    p = w.ctypes.data_as(C.POINTER(C.c_uint64))
    assert engine.lib.vqa_sig_cross_wait(engine.ctx, p, 5, p, 3) == N.VQA_ERR_STATE   # diag is 3 + 2 - 1 = 4 words
    assert engine.lib.vqa_sig_cross_wait(engine.ctx, p, 4, p, 2) == N.VQA_ERR_STATE   # best is 3 words
    diag, best = engine.sig_cross_wait()
    assert diag.shape == (4,) and best.shape == (3,)
    # beyond the limit: the status only - the arrays hold 3 rows and are not read
    big = N.SIG_MAX_FRAMES + 1
    assert engine.lib.vqa_sig_cross_submit(engine.ctx, a.ctypes.data, big, a.ctypes.data, 3) == N.VQA_ERR_UNSUPPORTED
    assert engine.lib.vqa_sig_cross_submit(engine.ctx, a.ctypes.data, 3, a.ctypes.data, big) == N.VQA_ERR_UNSUPPORTED
    assert engine.lib.vqa_sig_cross_submit(engine.ctx, a.ctypes.data, 0, a.ctypes.data, 3) == N.VQA_ERR_INVALID
    with pytest.raises(ValueError):
        engine.sig_cross(a[:, :255], a)
    with pytest.raises(ValueError):
        engine.sig_cross(a.astype(np.uint16), a)
    assert engine.sig_cross(a, a)[1].tolist() == [0, 1, 2]   # the engine is usable after every refusal
