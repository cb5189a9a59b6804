"""GPU: HDR light levels and gamut QC (vqa_light_submit / vqa_light_wait) through the C ABI and the engine, against the NumPy
restatement of tests/light_reference.py (written from the definition in include/vqa.h), fed the LIBRARY's table and matrices.

The bar is EQUALITY of every field of the record, the doubles included, and of every bin of the histogram: the decode uses only
correctly rounded double operations with contraction off, there is one rounding, and everything after it is integer.  If a case
ever differs, an operation was contracted or reordered: find it, do not loosen the bar."""
import ctypes as C

import numpy as np
import pytest

import itp_reference as IR
import light_cases as LC
import light_reference as LR

pytestmark = pytest.mark.gpu

INT_FIELDS = ("count", "max_code", "max_code_rgb", "min_code_rgb", "reserved", "sum_q", "sum_y", "max_y", "out_709", "out_p3",
              "clamped", "pct_bin")
DBL_FIELDS = ("max_nits", "min_nits", "avg_nits", "y_avg", "y_max", "maxscl", "pct_nits", "share_709", "share_p3")


@pytest.fixture(scope="module")
def lib_tables():
    from rtvqa_amd import engine as E
    return E.light_table("pq"), E.light_gamut("bt709"), E.light_gamut("p3")


def _check(got, want, tag, hist=None):
    """every field of every record equals the restatement's; with hist, every bin too"""
    assert got.shape == (len(want),) and got.dtype.names == INT_FIELDS + DBL_FIELDS
    for i, (ref, ref_hist) in enumerate(want):
        for k in INT_FIELDS + DBL_FIELDS:
            g = got[i][k]
            g = g.tolist() if isinstance(g, np.ndarray) else g.item()
            assert g == ref[k], (tag, i, k, g, ref[k])
        if hist is not None:
            assert (hist[i] == ref_hist).all(), (tag, i)


@pytest.mark.parametrize("shape,chroma,depth,full", LC.matrix(), ids=LC.matrix_ids())
def test_every_word_on_every_shape_layout_depth_and_range(engine, lib_tables, shape, chroma, depth, full):
    h, w = shape
    T, M709, MP3 = lib_tables
    frames, planes = LC.clip(chroma, h, w, depth, max(LC.COUNTS))
    model = LC.model_of(chroma)
    assert engine.itp_model(planes) == model
    want = LC.reference(frames, planes, depth, model, full, T, M709, MP3, key=(shape, chroma, depth, full))
    got, hist = engine.light(frames, planes, full_range=full, histogram=True)
    tag = "%dx%d %s %d %s" % (w, h, chroma, depth, "full" if full else "limited")
    _check(got, want, tag, hist)
    assert (hist.sum(axis=1) == h * w).all()
    for m in LC.COUNTS:                                        # n = 1 and n = 3: the same bytes
        assert engine.light(frames[:m], planes, full_range=full).tobytes() == got[:m].tobytes(), m
    assert engine.light(frames, planes, table=T, full_range=full).tobytes() == got.tobytes()   # the table travels with the call
    if chroma == "bgr":                                        # the range does not reach B, G, R
        assert engine.light(frames, planes, full_range=True).tobytes() == got.tobytes()
    # device-resident frames with a lead and a row pad: plane offsets 2 samples off, rows 3 samples longer - the unvectorised path
    bps = 2 if depth > 8 else 1
    if chroma != "bgr":
        lead, at, padded = 2, 2, []
        for (pw, ph, _off, _rs, step, *rest) in planes:
            padded.append((pw, ph, at * bps, (pw + 3) * bps, step) + tuple(rest))
            at += (pw + 3) * ph
        buf = np.zeros((len(frames), at + lead), frames.dtype)
        for f in range(len(frames)):
            for (pw, ph, off, rs, _s, *_r), (_w, _h, poff, prs, _ps, *_pr) in zip(planes, padded):
                src = frames[f, off // bps: off // bps + pw * ph].reshape(ph, pw)
                for y in range(ph):
                    buf[f, poff // bps + y * (prs // bps): poff // bps + y * (prs // bps) + pw] = src[y]
        dev = engine.upload(buf)
        assert engine.light(dev, padded, full_range=full).tobytes() == got.tobytes()
        assert engine.light(buf, padded, full_range=full).tobytes() == got.tobytes()
        dev._owner.free()
    dev = engine.upload(frames)
    assert engine.light(dev, planes, full_range=full).tobytes() == got.tobytes()
    dev._owner.free()


def test_a_toy_table_by_hand(engine):
    """T[c] = c: an 8-bit full-range BGR frame that is flat (10, 200, 30) has codes 257 times the samples"""
    h, w = 18, 20
    N = h * w
    frame = np.tile(np.array([10, 200, 30], np.uint8), N)[None, :]
    planes = LC.planes_of("bgr", h, w, 8)
    toy = np.arange(65536, dtype=np.uint64)
    rec, hist = engine.light(frame, planes, full_range=True, table=toy, histogram=True)
    r = rec[0]
    assert r["max_code"].tolist() == [7710, 51400, 2570]     # R = 30, G = 200, B = 10
    assert r["max_code_rgb"] == 51400 == r["min_code_rgb"] and r["sum_q"] == 51400 * N and r["count"] == N
    assert r["pct_bin"].tolist() == [51400 >> 4] * 10 and r["clamped"] == 0
    assert r["sum_y"] == N * ((2627 * 7710 + 6780 * 51400 + 593 * 2570 + 5000) // 10000) and r["max_y"] * N == r["sum_y"]
    assert hist[0, 51400 >> 4] == N and hist[0].sum() == N
    assert r["max_nits"] == 51400 * LR.UNIT == r["min_nits"] == r["avg_nits"] and r["pct_nits"][9] == ((51400 >> 4) << 4) * LR.UNIT


def test_hostile_content(engine, lib_tables):
    T, M709, MP3 = lib_tables
    h, w, depth = 66, 130, 10
    planes = LC.planes_of("420", h, w, depth)
    total = LC.samples_of(planes)
    s = 1 << (depth - 8)
    zero = np.zeros(total, np.uint16)
    peak = np.concatenate([np.full(h * w, 235 * s), np.full(total - h * w, 128 * s)]).astype(np.uint16)   # flat at peak white
    above = np.random.default_rng(5).integers(1 << depth, 65536, total).astype(np.uint16)                  # above 2^d - 1
    lone = np.concatenate([np.full(h * w, 16 * s), np.full(total - h * w, 128 * s)]).astype(np.uint16)     # black ...
    lone[(h - 1) * w + (w - 1)] = 235 * s                        # ... but the last pixel, in the last partial patch
    noise = LC.clip("420", h, w, depth, 1, seed=9)[0][0]
    frames = np.stack([zero, peak, above, lone, noise])
    want = LC.reference(frames, planes, depth, IR.YUV2020, False, T, M709, MP3)
    got, hist = engine.light(frames, planes, histogram=True)
    _check(got, want, "hostile", hist)
    N = h * w
    # all zero: Y below black and Cb = Cr far below neutral, an illegal combination: R' and B' are negative (code 0), G' is
    # ((y - Kr R') - Kb B') / Kg = 0.3475, code 22771 - every pixel is clamped and counted
    assert got["clamped"][0] == N and got["max_code"][0].tolist() == [0, 22771, 0] and got["min_code_rgb"][0] == 22771
    assert got["max_nits"][1] == 10000.0 == got["avg_nits"][1] and (hist[1] > 0).sum() == 1 and got["pct_bin"][1].tolist() == [4095] * 10
    assert got["clamped"][2] == N and got["max_nits"][2] == 10000.0
    # one bright pixel of 8580: the maximum sees it, the 99.98 % rank (k = 8579) does not
    assert got["max_nits"][3] == 10000.0 and got["pct_bin"][3][9] == 0 and got["min_code_rgb"][3] == 0 and hist[3, 4095] == 1
    # two frames of one batch with different content: no leakage between their histograms
    for order in ([3, 1], [1, 3], [4, 0, 2]):
        g, hh = engine.light(frames[order], planes, histogram=True)
        assert g.tobytes() == got[order].tobytes() and (hh == hist[order]).all(), order
    with pytest.raises(Exception):
        engine.light(frames, planes, table=np.arange(65536, dtype=np.uint64)[::-1].copy())   # a decreasing table is refused


def test_batch_splits_and_a_pending_itp_batch_give_the_same_bytes(engine):
    h, w, depth = 66, 130, 10
    frames, planes = LC.clip("420", h, w, depth, 5, seed=3)
    whole = engine.light(frames, planes)
    assert engine.light(frames, planes).tobytes() == whole.tobytes()                                  # run to run
    assert np.concatenate([engine.light(frames[:2], planes), engine.light(frames[2:], planes)]).tobytes() == whole.tobytes()
    assert np.concatenate([engine.light(frames[i:i + 1], planes) for i in range(5)]).tobytes() == whole.tobytes()
    itp = engine.itp(frames, frames[::-1].copy(), planes)
    for src in (frames, engine.upload(frames)):
        engine.itp_submit(frames, frames[::-1].copy(), planes)
        engine.light_submit(src, planes)
        assert engine.light_wait().tobytes() == whole.tobytes()
        assert engine.itp_wait().tobytes() == itp.tobytes()
    engine.trim()                                                                                      # the table is uploaded again
    assert engine.light(frames, planes).tobytes() == whole.tobytes()


def test_the_state_machine_and_the_refusals(engine, lib_tables):
    from rtvqa_amd import _native as N
    from rtvqa_amd.engine import plane_descs
    T = lib_tables[0]
    f, planes = LC.clip("420", 16, 16, 8, 2, seed=8)
    want = engine.light(f, planes)
    lib, ctx = engine.lib, engine.ctx
    out = (N.VqaLightMetrics * 2)()
    hist = np.zeros((2, 4096), np.uint32)
    u64, u32 = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)

    def submit(pl=planes, n=2, model=0, full=0, table=T, want_hist=0):
        return lib.vqa_light_submit(ctx, f.ctypes.data, N.VQA_MEM_HOST, n, f.shape[1], plane_descs(pl), len(pl), model, full,
                                    None if table is None else table.ctypes.data_as(u64), want_hist)

    assert lib.vqa_light_wait(ctx, out, 2, None) == N.VQA_ERR_STATE                  # wait without submit
    assert submit() == N.VQA_OK and submit() == N.VQA_ERR_STATE                      # submit while pending
    assert lib.vqa_trim(ctx) == N.VQA_ERR_STATE
    assert lib.vqa_light_wait(ctx, out, 3, None) == N.VQA_ERR_STATE                  # a wrong entry count
    assert lib.vqa_light_wait(ctx, out, 2, hist.ctypes.data_as(u32)) == N.VQA_ERR_INVALID   # histograms were not asked for
    assert lib.vqa_light_wait(ctx, out, 2, None) == N.VQA_OK and bytes(out) == want.tobytes()
    assert submit(want_hist=1) == N.VQA_OK
    assert lib.vqa_light_wait(ctx, out, 2, hist.ctypes.data_as(u32)) == N.VQA_OK and bytes(out) == want.tobytes()
    assert (hist.sum(axis=1) == 256).all()
    bad_dec, bad_big = T.copy(), T.copy()
    bad_dec[1000] = bad_dec[999] - 1
    bad_big[65535] = 1 << 34
    Y, U, V = planes
    for k, (kw, status) in enumerate([
            (dict(table=bad_dec), N.VQA_ERR_INVALID), (dict(table=bad_big), N.VQA_ERR_INVALID), (dict(table=None), N.VQA_ERR_INVALID),
            (dict(pl=planes[:1]), N.VQA_ERR_INVALID), (dict(pl=planes[:2]), N.VQA_ERR_INVALID), (dict(model=2), N.VQA_ERR_INVALID),
            (dict(model=N.ITP_BGR), N.VQA_ERR_INVALID), (dict(full=2), N.VQA_ERR_INVALID),
            (dict(pl=[Y, U, (V[0] - 1,) + V[1:]]), N.VQA_ERR_INVALID),
            (dict(pl=[(16, 15, 0, 16, 1), (8, 8, 240, 8, 1), (8, 8, 304, 8, 1)], n=1), N.VQA_ERR_UNSUPPORTED)]):
        assert submit(**kw) == status, k
        assert lib.vqa_light_wait(ctx, out, 2, None) == N.VQA_ERR_STATE, k           # nothing in flight
    with pytest.raises(ValueError, match="hlg"):
        engine.light(f, planes, transfer="hlg")
    assert engine.light(f, planes).tobytes() == want.tobytes()


def test_the_slice_and_sub_slice_seams_of_the_shipped_library(engine, lib_tables):
    """32771 frames of 16 x 16 from a pool of 7: sub-slices end at 16384 and 32768, the slice at 32768; record i is the pool's
    record i % 7, as bytes, and so is its histogram"""
    T, M709, MP3 = lib_tables
    pool, planes = LC.seam_pool()
    want = LC.reference(pool, planes, 8, IR.YUV2020, False, T, M709, MP3, key="seam")
    idx = np.arange(LC.SEAM_FRAMES) % LC.SEAM_POOL
    got, hist = engine.light(pool[idx], planes, histogram=True)
    _check(got[:LC.SEAM_POOL], want, "seam pool", hist[:LC.SEAM_POOL])
    assert got.tobytes() == got[:LC.SEAM_POOL][idx].tobytes()
    assert (hist == hist[:LC.SEAM_POOL][idx]).all()
    dev = engine.upload(pool[idx])
    assert engine.light(dev, planes).tobytes() == got.tobytes()
    dev._owner.free()


def test_profile_names_and_counts():
    import rtvqa_amd
    from rtvqa_amd import _native as N
    f, planes = LC.clip("420", 16, 16, 8, 3, seed=2)
    with rtvqa_amd.Engine(0) as eng:
        eng.profile(True)
        eng.light(f, planes)
        prof = eng.profile_read(reset=True)
        assert prof["k_light_accum"][1] == 1 and prof["k_light_scan"][1] == 1 and "k_itp" not in prof, prof
        ms, cnt = C.c_double(0), C.c_int64(0)
        for bad in (N.K_SILL, N.K_LINTEL):
            assert eng.lib.vqa_profile_read(eng.ctx, bad, C.byref(ms), C.byref(cnt), 0) == N.VQA_ERR_INVALID
