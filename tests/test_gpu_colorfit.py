"""GPU: colour registration (vqa_colorfit_submit / vqa_colorfit_wait) through the C ABI and the engine, against the NumPy
restatement of tests/colorfit_reference.py (written from the definition in include/vqa.h).

The bar is EQUALITY of every word of every record and of every table word: the device forms integer sums only, so neither the
tiling nor the order in which workgroups retire can change a bit.  If a case ever differs, a sample was read twice, skipped or
weighted wrongly, or an accumulator overflowed: find it, do not loosen the bar."""
import ctypes as C

import numpy as np
import pytest

import colorfit_cases as CC
import colorfit_reference as CR

pytestmark = pytest.mark.gpu


def _check_records(got, want, tag):
    assert got.shape == (len(want),) and got.dtype.names == CR.FIELDS
    for i, ref in enumerate(want):
        for k in CR.FIELDS:
            g = got[i][k]
            g = g.tolist() if isinstance(g, np.ndarray) else g.item()
            assert g == ref[k], (tag, i, k, g, ref[k])


def _check_tables(got, want, tag):
    assert got.dtype == np.uint64 and got.shape == want.shape, (tag, got.shape, want.shape)
    assert (got.astype(np.int64) == want).all(), (tag, np.argwhere(got.astype(np.int64) != want)[:4])


@pytest.mark.parametrize("shape,layout,depth", CC.matrix(), ids=CC.matrix_ids())
def test_every_word_on_every_shape_layout_and_depth(engine, shape, layout, depth):
    h, w = shape
    ref, dist, planes = CC.clip(layout, h, w, depth, max(CC.COUNTS))
    want, want_tab = CC.reference(ref, dist, planes, depth, key=(shape, layout, depth))
    tag = "%dx%d %s %d" % (w, h, layout, depth)
    for m in CC.COUNTS:
        got, tab = engine.colorfit(ref[:m], dist[:m], planes, tables=True)
        _check_records(got, want[:m], (tag, m))
        _check_tables(tab, want_tab[m], (tag, m))
        assert int(tab[:, :, 0].sum()) == m * h * w * len(planes)
        bare, none = engine.colorfit(ref[:m], dist[:m], planes)          # without tables: the same records, no table
        assert none is None and bare.tobytes() == got.tobytes(), (tag, m)
    # identical streams (frame 3): no error, and every moment of the pair is the reference's own
    r = got[3]
    n_pl = len(planes)
    assert r["sse"].tolist() == [0, 0, 0]
    for k, q in zip(range(n_pl), (0, 3, 5)):
        assert r["rd"][4 * k] == r["rr"][q] == r["dd"][k] and r["sum_r"][k] == r["sum_d"][k]
    one, tab = engine.colorfit(ref[3:4], ref[3:4], planes, tables=True)
    for p, plane in enumerate(planes):
        g = CR.grid(ref[3], plane, h, w).ravel()
        at = np.minimum(g >> max(depth - 10, 0), CR.bins_of(depth) - 1)
        assert (tab[p, :, 1].astype(np.int64) == np.bincount(at, weights=g.astype(np.float64), minlength=CR.bins_of(depth))).all()
    # the flat pair (frame 1): every position in one bin per plane
    one, tab = engine.colorfit(ref[1:2], dist[1:2], planes, tables=True)
    assert ((tab[:, :, 0] > 0).sum(axis=1) == 1).all() and (tab[:, -1, 0] == h * w).all()
    # device-resident frames give the same words
    dr, dd = engine.upload(ref), engine.upload(dist)
    got_d, tab_d = engine.colorfit(dr, dd, planes, tables=True)
    assert got_d.tobytes() == got.tobytes()
    _check_tables(tab_d, want_tab[max(CC.COUNTS)], (tag, "device"))
    dr._owner.free()
    dd._owner.free()


@pytest.mark.parametrize("layout,depth", [("420", 8), ("422", 10), ("444", 8), ("444", 16), ("bgr", 8), ("gray", 12)])
def test_sse_is_the_quality_kinds_sse(engine, layout, depth):
    """sse[0] is vqa_plane_metrics.sse of plane 0 of the same pair; where every plane is full size (4:4:4, bgr24) all three are"""
    from rtvqa_amd import _native as N
    h, w = 67, 259
    ref, dist, planes = CC.clip(layout, h, w, depth, 5, seed=4)
    got, _ = engine.colorfit(ref, dist, planes)
    q = engine.quality(ref, dist, planes, N.SSIM_FFMPEG)
    full = range(len(planes)) if layout in ("444", "bgr", "gray") else (0,)
    for p in full:
        assert got["sse"][:, p].tolist() == q[:, p]["sse"].tolist(), (layout, depth, p)
    assert int(got["sse"][0, 0]) > 0 and got["sse"][3].tolist() == [0, 0, 0]


def test_a_frame_is_the_same_anywhere_and_tables_add_up(engine):
    h, w, depth = 67, 259, 10
    ref, dist, planes = CC.clip("420", h, w, depth, 5, seed=7)
    whole, tab = engine.colorfit(ref, dist, planes, tables=True)
    singles = [engine.colorfit(ref[i:i + 1], dist[i:i + 1], planes, tables=True) for i in range(5)]
    assert np.concatenate([s[0] for s in singles]).tobytes() == whole.tobytes()
    assert (sum(s[1].astype(object) for s in singles) == tab.astype(object)).all()        # a batch's tables: the sum of its frames'
    probe = 2                                                                               # alone, first, in the middle, last
    alone = singles[probe][0].tobytes()
    for order, at in (([2, 0, 1], 0), ([0, 2, 4], 1), ([3, 4, 2], 2)):
        got, _ = engine.colorfit(ref[order], dist[order], planes)
        assert got[at:at + 1].tobytes() == alone, order
    assert engine.colorfit(ref, dist, planes, tables=True)[1].tobytes() == tab.tobytes()    # run to run


@pytest.mark.parametrize("layout,depth", [("420", 8), ("444", 10), ("gray", 16)])
def test_padded_rows_a_frame_pad_and_a_leading_offset_give_the_same_words(engine, layout, depth):
    h, w = 33, 70
    ref, dist, planes = CC.clip(layout, h, w, depth, 3, seed=5)
    want, want_tab = engine.colorfit(ref, dist, planes, tables=True)
    bps = 2 if depth > 8 else 1
    lead, at, padded = 3, 3, []                           # plane offsets 3 samples off, rows 5 samples longer: never one load per row
    for (pw, ph, _off, _rs, step, *rest) in planes:
        padded.append((pw, ph, at * bps, (pw + 5) * bps, step) + tuple(rest))
        at += (pw + 5) * ph
    frame_pad = 11

    def repack(clip):
        buf = np.full((len(clip), at + frame_pad), 77, clip.dtype)
        for f in range(len(clip)):
            for (pw, ph, off, _rs, _s, *_r), (_w, _h, poff, prs, _ps, *_pr) in zip(planes, padded):
                src = clip[f, off // bps: off // bps + pw * ph].reshape(ph, pw)
                for y in range(ph):
                    buf[f, poff // bps + y * (prs // bps): poff // bps + y * (prs // bps) + pw] = src[y]
        return buf

    br, bd = repack(ref), repack(dist)
    got, tab = engine.colorfit(br, bd, padded, tables=True)
    assert got.tobytes() == want.tobytes() and tab.tobytes() == want_tab.tobytes()
    dr, dd = engine.upload(br), engine.upload(bd)
    got, tab = engine.colorfit(dr, dd, padded, tables=True)
    assert got.tobytes() == want.tobytes() and tab.tobytes() == want_tab.tobytes()
    dr._owner.free()
    dd._owner.free()


def test_a_quality_batch_and_a_colorfit_batch_pending_together(engine):
    from rtvqa_amd import _native as N
    h, w, depth = 67, 259, 8
    ref, dist, planes = CC.clip("420", h, w, depth, 3, seed=6)
    q = engine.quality(ref, dist, planes, N.SSIM_FFMPEG)
    cf, tab = engine.colorfit(ref, dist, planes, tables=True)
    for first in ("quality", "colorfit"):
        if first == "quality":
            engine.quality_submit(ref, dist, planes, N.SSIM_FFMPEG)
            engine.colorfit_submit(ref, dist, planes, tables=True)
        else:
            engine.colorfit_submit(ref, dist, planes, tables=True)
            engine.quality_submit(ref, dist, planes, N.SSIM_FFMPEG)
        got, got_tab = engine.colorfit_wait()
        assert engine.quality_wait().tobytes() == q.tobytes(), first
        assert got.tobytes() == cf.tobytes() and got_tab.tobytes() == tab.tobytes(), first
    engine.trim()                                                                           # scratch is re-grown
    assert engine.colorfit(ref, dist, planes, tables=True)[0].tobytes() == cf.tobytes()


def test_the_state_machine_and_the_refusals(engine):
    from rtvqa_amd import _native as N
    from rtvqa_amd.engine import plane_descs
    ref, dist, planes = CC.clip("420", 16, 16, 8, 2, seed=8)
    want, want_tab = engine.colorfit(ref, dist, planes, tables=True)
    lib, ctx = engine.lib, engine.ctx
    out = (N.VqaColorfitMetrics * 2)()
    words = 3 * 256 * 3
    tab = np.zeros(words, np.uint64)
    u64 = C.POINTER(C.c_uint64)

    def submit(pl=planes, n=2, tables=0, fs=None):
        fs = ref.shape[1] if fs is None else fs
        return lib.vqa_colorfit_submit(ctx, ref.ctypes.data, dist.ctypes.data, N.VQA_MEM_HOST, n, fs, fs, plane_descs(pl), len(pl),
                                       tables)

    def idle(tag):
        assert lib.vqa_colorfit_wait(ctx, out, 2, None, 0) == N.VQA_ERR_STATE, tag

    idle("wait without submit")
    assert submit() == N.VQA_OK and submit() == N.VQA_ERR_STATE                      # submit while pending
    assert lib.vqa_trim(ctx) == N.VQA_ERR_STATE
    assert lib.vqa_colorfit_wait(ctx, out, 3, None, 0) == N.VQA_ERR_STATE            # a wrong entry count
    assert lib.vqa_colorfit_wait(ctx, out, 2, tab.ctypes.data_as(u64), words) == N.VQA_ERR_INVALID   # tables were not asked for
    assert lib.vqa_colorfit_wait(ctx, out, 2, None, 0) == N.VQA_OK and bytes(out) == want.tobytes()
    assert submit(tables=1) == N.VQA_OK
    assert lib.vqa_colorfit_wait(ctx, out, 2, tab.ctypes.data_as(u64), words - 1) == N.VQA_ERR_STATE   # a wrong word count ...
    assert lib.vqa_colorfit_wait(ctx, out, 2, tab.ctypes.data_as(u64), words) == N.VQA_OK              # ... left the batch pending
    assert bytes(out) == want.tobytes() and tab.tobytes() == want_tab.tobytes()
    idle("collected")
    Y, U, V = planes
    ten = [tuple(p) + (10,) for p in planes]
    for k, (kw, status) in enumerate([
            (dict(pl=planes[:2]), N.VQA_ERR_INVALID),                                 # n_planes = 2
            (dict(pl=[Y, U, tuple(V) + (10,)]), N.VQA_ERR_INVALID),                   # mixed depths
            (dict(pl=[Y, U, (V[0] - 1,) + tuple(V[1:])]), N.VQA_ERR_INVALID),         # chroma geometries that differ
            (dict(tables=2), N.VQA_ERR_INVALID),
            (dict(pl=ten), N.VQA_ERR_INVALID),                                        # a pixel step of one byte under 16-bit samples
            (dict(pl=[(16, 15, 0, 16, 1), (8, 8, 240, 8, 1), (8, 8, 304, 8, 1)], n=1), N.VQA_ERR_UNSUPPORTED),   # 15 rows
            (dict(n=32769), N.VQA_ERR_UNSUPPORTED),                                   # refused before a byte is read
            (dict(pl=[(256, 257, 0, 256, 1)], n=32768, tables=1, fs=256 * 257), N.VQA_ERR_UNSUPPORTED)]):   # n h w = 2^31 + h w
        assert submit(**kw) == status, k
        idle(k)
    assert engine.colorfit(ref, dist, planes, tables=True)[0].tobytes() == want.tobytes()


def test_exactly_two_to_the_31_positions_with_tables(engine):
    """n = 32768 frames of 256 x 256, one plane: n h w = 2^31 passes; the same buffer on both sides, so the streams are identical"""
    from rtvqa_amd.engine import DeviceBuffer, DeviceFrames, gray_planes
    n, h, w = 32768, 256, 256
    buf = DeviceBuffer(engine, n * h * w)
    probe = np.random.default_rng(3).integers(0, 256, (2, h, w)).astype(np.uint8)
    frames = DeviceFrames(buf.ptr, n, h, w, owner=buf, channels=1)
    # (the allocation is not initialised: whatever it holds, both sides read the same bytes; two known frames at the ends)
    from rtvqa_amd import _native as N
    N.check(engine.lib.vqa_copy_h2d(engine.ctx, buf.ptr, probe[0].ctypes.data, h * w), "vqa_copy_h2d", engine.ctx)
    N.check(engine.lib.vqa_copy_h2d(engine.ctx, buf.ptr + (n - 1) * h * w, probe[1].ctypes.data, h * w), "vqa_copy_h2d", engine.ctx)
    engine.sync()
    rec, tab = engine.colorfit(frames, frames, gray_planes(h, w), tables=True)
    assert int(tab[0, :, 0].sum()) == 1 << 31 and tab.shape == (1, 256, 3)
    assert not rec["sse"].any() and (rec["count"] == h * w).all()
    assert (rec["rd"][:, 0] == rec["dd"][:, 0]).all() and (rec["rr"][:, 0] == rec["dd"][:, 0]).all()
    for i, f in ((0, probe[0]), (n - 1, probe[1])):
        want = CR.record(f.ravel(), f.ravel(), gray_planes(h, w))
        assert rec[i]["sum_r"][0] == want["sum_r"][0] and rec[i]["dd"][0] == want["dd"][0]
    # per bin: sum_d is the bin's code times its count, sum_dd the code squared times its count (bins are codes at 8 bits)
    code = np.arange(256, dtype=np.uint64)
    assert (tab[0, :, 1] == code * tab[0, :, 0]).all() and (tab[0, :, 2] == code * code * tab[0, :, 0]).all()
    buf.free()
