"""GPU: the frame-slice seam of every plane-batch metric.  The C ABI puts the frames of a batch into gridDim.y and cuts a batch
into slices of 32768 frames (for_each_slice, csrc/vqa_capi.hip); every submit body owns its slice arithmetic - the offsets into
its accumulators and records, scratch sized for one slice and reused by the next, the previous frame carried across the seam.

(a) Small slices through the lab library: one child process creates an engine with VQA_QSLICE unset and one with VQA_QSLICE=3
    (the lab build reads it in vqa_create) and runs all ten kinds - Gaussian, vf_ssim and MS-SSIM quality, VIF, ADM, the motion
    feature and SI/TI with and without prev0, PSNR-HVS, CIEDE2000 (YUV and packed BGR), GMSD, CAMBI - at n = 3, 4 and 8 (one
    slice, one frame over, 3 + 3 + 2), from host and from device-resident frames, on 8- and 10-bit 4:2:0 of 67 x 99 (two geometry
    groups a slice, 34 x 50 chroma, wider than a tile); MS-SSIM on 170 x 161 mono and 322 x 324 4:2:0.  The sliced engine's
    records equal the unsliced engine's byte for byte; the unsliced records of pool entries 0 .. 6 meet each metric's reference
    at the bar and through the _check helper of that metric's own GPU test file; and several kinds queued on the sliced engine
    before any is waited for give the same bytes again.
(b) The shipped library at the shipped constant: n = 32771 on 8-bit 4:2:0 of 32 x 32 and 10-bit mono 16 x 16 (CIEDE2000 also on
    10-bit 4:4:4 16 x 16), on the session engine; every record of the batch against the periodicity maps of
    tests/slice_cases.py, as bytes, and records 0 .. 7 against the references.  CAMBI runs mono 16 x 16 on an engine of its own,
    closed afterwards: its scratch for a full slice is gigabytes ("slice seam").  MS-SSIM is not run at the
    shipped constant - 32769 planes of 161 x 161 are about 0.85 GB a stream plus about 2.3 GB of pyramid; (a) covers its
    slice arithmetic (qms_dev + a0 * n_planes, the pyramid and the partials sized for one slice).

tests/test_slices_host.py checks on the CPU that every entry compared with a reference here is a fair test."""
import contextlib
import os
import subprocess
import sys
import time

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path[:0] = [REPO, os.path.dirname(os.path.abspath(__file__))]

import slice_cases as SC

pytestmark = pytest.mark.gpu

PAIR_KINDS = ("gauss", "ffmpeg", "vif", "adm", "psnr_hvs", "ciede", "gmsd")
TEMPORAL_KINDS = ("motion", "motion_p", "siti", "siti_p")
SMALL_KINDS = PAIR_KINDS + TEMPORAL_KINDS + ("cambi",)
QUEUE_DEVICE = ("gauss", "vif", "adm", "motion_p", "siti_p")
QUEUE_HOST = ("psnr_hvs", "ciede", "gmsd", "cambi")          # they share qstage_*
PREV0_ENTRY = 6                # prev0 of the *_p kinds: pool entry 6, so that record 7 equals record 0
OTHER_PREV0 = 2


def _dtype_of(kind):
    from rtvqa_amd import engine as E
    return {"gauss": E.PLANE_DTYPE, "ffmpeg": E.PLANE_DTYPE, "ms": E.PLANE_DTYPE, "vif": E.VIF_DTYPE, "adm": E.ADM_DTYPE,
            "motion": E.MOTION_DTYPE, "siti": E.SITI_DTYPE, "psnr_hvs": E.PSNR_HVS_DTYPE, "ciede": E.CIEDE_DTYPE,
            "gmsd": E.GMSD_DTYPE, "cambi": E.CAMBI_DTYPE}[kind.split("_p")[0] if kind.endswith("_p") else kind]


def _submit(eng, kind, r, d, planes, prev0=None):
    """enqueue one batch of `kind` (r, d: host arrays or DeviceFrames; prev0 lives where r lives)"""
    from rtvqa_amd import _native as N
    if kind in ("gauss", "ffmpeg", "ms"):
        eng.quality_submit(r, d, planes, {"gauss": N.SSIM_GAUSS, "ffmpeg": N.SSIM_FFMPEG, "ms": N.SSIM_MS}[kind])
    elif kind in ("vif", "adm", "psnr_hvs", "gmsd"):
        getattr(eng, kind + "_submit")(r, d, planes)
    elif kind == "ciede":
        eng.ciede_submit(r, d, planes, weights=(1.0, 1.0, 1.0))
    elif kind in TEMPORAL_KINDS:
        getattr(eng, kind[:-2] + "_submit" if kind.endswith("_p") else kind + "_submit")(r, planes, prev0=prev0 if kind.endswith("_p") else None)
    elif kind == "cambi":
        eng.cambi_submit(d, planes)
    else:
        raise KeyError(kind)


def _wait(eng, kind):
    """-> the batch's records as bytes (MS-SSIM: the records, then the per-scale cs and ssim means)"""
    if kind == "ms":
        res, cs, ssim = eng.quality_wait(scales=True)
        return res.tobytes() + cs.tobytes() + ssim.tobytes()
    if kind in ("gauss", "ffmpeg"):
        return eng.quality_wait().tobytes()
    name = kind[:-2] if kind.endswith("_p") else kind
    return getattr(eng, name + "_wait")().tobytes()


def _decode(kind, raw, n, n_planes):
    """the bytes of _wait -> [n, n_planes] records (CIEDE2000: [n]; MS-SSIM: (records, cs, ssim))"""
    raw = bytes(raw)
    if kind == "ms":
        from rtvqa_amd import engine as E
        a = n * n_planes * E.PLANE_DTYPE.itemsize
        b = a + n * n_planes * 5 * 8
        return (np.frombuffer(raw[:a], E.PLANE_DTYPE).reshape(n, n_planes), np.frombuffer(raw[a:b], np.float64).reshape(n, n_planes, 5),
                np.frombuffer(raw[b:], np.float64).reshape(n, n_planes, 5))
    rec = np.frombuffer(raw, _dtype_of(kind))
    return rec if kind == "ciede" else rec.reshape(n, n_planes)


# ---- (a) the child: two engines on the lab library ------------------------------------------------------------------------------
def _child(out_path):
    import rtvqa_amd
    os.environ.pop("VQA_QSLICE", None)
    engines = {"plain": rtvqa_amd.Engine(0)}
    os.environ["VQA_QSLICE"] = "3"               # read once, in vqa_create
    engines["sliced"] = rtvqa_amd.Engine(0)
    os.environ.pop("VQA_QSLICE")
    assert engines["plain"].lib.vqa_build_flavour() == 3
    got = {}
    jobs = [(lay, SMALL_KINDS) for lay in SC.SMALL] + [(SC.SMALL_BGR, ("ciede",))] + [(lay, ("ms",)) for lay in SC.SMALL_MS]
    for li, (lay, kinds) in enumerate(jobs):
        r, d, planes = SC.pool(*lay)
        for n in SC.SMALL_NS:
            br, bd = SC.batch(r, n), SC.batch(d, n)
            for name, eng in engines.items():
                dr, dd, dp = eng.upload(br), eng.upload(bd), eng.upload(r[PREV0_ENTRY:PREV0_ENTRY + 1])
                for kind in kinds:
                    _submit(eng, kind, br, bd, planes, r[PREV0_ENTRY])
                    got["%s|%s|%d|%d|host" % (name, kind, li, n)] = _wait(eng, kind)
                    _submit(eng, kind, dr, dd, planes, dp)
                    got["%s|%s|%d|%d|device" % (name, kind, li, n)] = _wait(eng, kind)
                if n == 8 and kinds is SMALL_KINDS:
                    # several kinds in flight at once: five from device frames, then four from host frames (one staging pair)
                    for kind in QUEUE_DEVICE:
                        _submit(eng, kind, dr, dd, planes, dp)
                    for kind in QUEUE_HOST:
                        _submit(eng, kind, br, bd, planes)
                    for kind in QUEUE_DEVICE + QUEUE_HOST:
                        got["%s|%s|%d|%d|queue" % (name, kind, li, n)] = _wait(eng, kind)
                for buf in (dr, dd, dp):
                    buf._owner.free()
    for eng in engines.values():
        eng.close()
    np.savez(out_path, **{k: np.frombuffer(v, np.uint8) for k, v in got.items()})
    print("SLICES-OK", len(got))


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    """every record of the child, once for the module: {"engine|kind|job|n|memory": bytes}"""
    from rtvqa_amd import _native as N
    out = str(tmp_path_factory.mktemp("slices") / "small.npz")
    env = dict(os.environ, VQA_LIB_PATH=N.LAB_LIB_PATH)
    env.pop("VQA_QSLICE", None)
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True, timeout=600, cwd=REPO)
    print("the child took %.1f s" % (time.time() - t0))
    assert r.returncode == 0 and "SLICES-OK" in r.stdout, (r.stdout[-300:], r.stderr[-2000:])
    with np.load(out) as z:
        return {k: z[k].tobytes() for k in z.files}


def _jobs_of(kind):
    """(job index, layout) of the child's jobs that ran `kind`"""
    jobs = list(SC.SMALL) + [SC.SMALL_BGR] + list(SC.SMALL_MS)
    if kind == "ms":
        return [(i, lay) for i, lay in enumerate(jobs) if lay in SC.SMALL_MS]
    return [(i, lay) for i, lay in enumerate(jobs) if lay in SC.SMALL or (kind == "ciede" and lay == SC.SMALL_BGR)]


@pytest.mark.parametrize("kind", SMALL_KINDS + ("ms",))
def test_small_slices_give_the_bytes_of_one_slice(small, kind):
    """VQA_QSLICE=3 against the shipped slice length, n = 3, 4, 8, host and device frames: byte for byte, and so do host against
    device frames and the records the batches share (record i of n = 8 is record i of n = 3 where no prev0 differs)"""
    seen = 0
    for li, lay in _jobs_of(kind):
        npl = 1 if kind == "ciede" else len(SC.layout_planes(*lay))
        for n in SC.SMALL_NS:
            plain = small["plain|%s|%d|%d|host" % (kind, li, n)]
            assert len(plain) > 0 and len(plain) % n == 0
            for mem in ("host", "device"):
                assert small["sliced|%s|%d|%d|%s" % (kind, li, n, mem)] == plain, (kind, lay, n, mem)
                assert small["plain|%s|%d|%d|%s" % (kind, li, n, mem)] == plain, (kind, lay, n, mem)
                seen += 1
            if kind != "ms":
                rec = _decode(kind, plain, n, npl)
                first = _decode(kind, small["plain|%s|%d|%d|host" % (kind, li, 3)], 3, npl)
                assert rec[:3].tobytes() == first.tobytes(), (kind, lay, n)
    assert seen == len(_jobs_of(kind)) * 6


@pytest.mark.parametrize("kind", QUEUE_DEVICE + QUEUE_HOST)
def test_small_slices_with_several_kinds_in_flight(small, kind):
    """quality, VIF, ADM, motion and SI/TI from device frames, then PSNR-HVS, CIEDE2000, GMSD and CAMBI from host frames (one
    staging pair, reused by each of the four while the earlier ones are still on the stream), all queued on the sliced engine
    before the first wait: the bytes of the unsliced engine, one kind at a time"""
    for li, lay in enumerate(SC.SMALL):
        want = small["plain|%s|%d|8|host" % (kind, li)]
        assert small["sliced|%s|%d|8|queue" % (kind, li)] == want, (kind, lay)
        assert small["plain|%s|%d|8|queue" % (kind, li)] == want, (kind, lay)


# ---- the references, through each metric's own GPU test file ----------------------------------------------------------------------
@contextlib.contextmanager
def _fresh(worst, label):
    """a module's running worst-gap record, set aside while this file's content passes through its _check"""
    keep = dict(worst)
    for k, v in keep.items():
        worst[k] = type(v)()
    try:
        yield
        print("slice seam, worst gap:", label, {k: v for k, v in worst.items()})
    finally:
        worst.clear()
        worst.update(keep)


def _check_ms(got, r, d, planes, depth, tag):
    """tests/test_gpu_hostile.py::test_msssim's assertions: every per-level mean within 1e-4 absolute, sse exact, the value the
    product of the record's own means and within the propagated bar"""
    import msssim_reference as MS
    res, cs, ssim = got
    worst = 0.0
    for i in range(res.shape[0]):
        sse_w, cs_w, ssim_w, ms_w = MS.frame_msssim(r[i], d[i], planes, depth)
        for p in range(len(planes)):
            ec, es = np.abs(cs[i, p] - cs_w[p]).max(), np.abs(ssim[i, p] - ssim_w[p]).max()
            val = float(res[i, p]["ssim"])
            print(tag, "frame", i, "plane", p, "cs err %.2e ssim err %.2e" % (ec, es), "ms %.9f ref %.9f" % (val, ms_w[p]))
            worst = max(worst, ec, es)
            assert int(res[i, p]["sse"]) == sse_w[p]
            assert ec <= 1e-4 and es <= 1e-4, (tag, i, p, cs[i, p], cs_w[p], ssim[i, p], ssim_w[p])
            own = MS.combine(cs[i, p], ssim[i, p])
            assert abs(val - own) <= 1e-12 * own, (tag, i, p, val, own)
            bound = MS.value_bound(cs_w[p], ssim_w[p], 1e-4)
            if bound is not None:
                assert abs(val - ms_w[p]) <= bound, (tag, i, p, val, ms_w[p], bound)
            if min(list(cs_w[p][:4]) + [ssim_w[p][4]]) < -1e-3:
                assert val == 0.0, (tag, i, p, val)
    print("slice seam, worst gap: msssim per-level mean %.2e (%s)" % (worst, tag))


def _check_kind(kind, got, r, d, planes, chroma, depth, tag, prev0=None):
    """records `got` of frames (r, d) against the reference of `kind`, at the bar and through the helper of the metric's own file"""
    if kind in ("gauss", "ffmpeg"):
        import test_gpu_hostile as TH
        keep = dict(TH.WORST)
        try:
            TH._check_quality(got, r, d, planes, kind, depth, tag)
            print("slice seam, worst gap:", kind, {k: v for k, v in TH.WORST.items() if k in ("ssim_gauss", "vf_ssim")})
        finally:
            TH.WORST.clear()
            TH.WORST.update(keep)
    elif kind == "ms":
        _check_ms(got, r, d, planes, depth, tag)
    elif kind == "vif":
        import test_gpu_vif as TV
        TV._check(got, r, d, planes, depth, tag)
    elif kind == "adm":
        import test_gpu_adm as TA
        TA._check(got, r, d, planes, depth, tag, count=False)        # the plain bar
    elif kind in ("motion", "motion_p"):
        import test_gpu_motion as TM
        with _fresh(TM.WORST, "motion"):
            TM._check(got, TM._reference(r, planes, depth, prev0), planes, tag)
        if prev0 is None:
            assert (got[0]["motion"] == 0.0).all() and (got[0]["sad"] == 0.0).all()       # no predecessor
    elif kind in ("siti", "siti_p"):
        import test_gpu_siti as TS
        with _fresh(TS.WORST, "si / ti"):
            TS._check(got, r, planes, depth, tag, prev0)
        if prev0 is None:
            assert (got[0]["ti"] == 0.0).all()
    elif kind == "psnr_hvs":
        import test_gpu_psnr_hvs as TP
        with _fresh(TP.WORST, "psnr_hvs"):
            TP._check(got, r, d, planes, depth, tag)
    elif kind == "ciede":
        import ciede_reference as CR
        import test_gpu_ciede as TC
        with _fresh(TC.WORST, "ciede"):
            TC._check(got, r, d, planes, depth, CR.BGR if chroma == "bgr" else CR.YUV709, (1.0, 1.0, 1.0), tag)
    elif kind == "gmsd":
        import test_gpu_gmsd as TG
        with _fresh(TG.WORST, "gmsd"):
            TG._check(got, r, d, planes, depth, tag)
    elif kind == "cambi":
        import test_gpu_cambi as TB
        TB._check(got, d, planes, depth, tag)
    else:
        raise KeyError(kind)


def _metric_of(kind):
    return kind[:-2] if kind.endswith("_p") else kind


def _check_pool_records(kind, got, r, d, planes, chroma, depth, tag, count=SC.PERIOD + 1, prev0=None):
    """records 0 .. count - 1 of a batch whose frame i is pool entry i % 7, against the reference; a pair metric leaves out what
    slice_cases.EXCLUDED names"""
    br, bd = SC.batch(r, count), SC.batch(d, count)
    if kind in TEMPORAL_KINDS:
        _check_kind(kind, got[:count], br, bd, planes, chroma, depth, tag, prev0)
        return
    keep = [i for i in range(count) if i % SC.PERIOD in SC.ref_entries(_metric_of(kind), depth)]
    assert len(keep) >= count - SC.MAX_EXCLUDED - 1
    sub = tuple(g[keep] for g in got) if kind == "ms" else got[keep]
    _check_kind(kind, sub, br[keep], bd[keep], planes, chroma, depth, tag)


@pytest.mark.parametrize("kind", SMALL_KINDS + ("ms",))
def test_small_unsliced_records_meet_the_reference(small, kind):
    """pool entries 0 .. 6 (n = 8: records 0 .. 7) of the unsliced lab engine against each metric's reference"""
    for li, lay in _jobs_of(kind):
        chroma, h, w, depth = lay
        r, d, planes = SC.pool(*lay)
        got = _decode(kind, small["plain|%s|%d|8|host" % (kind, li)], 8, len(planes))
        prev0 = r[PREV0_ENTRY] if kind.endswith("_p") else None
        _check_pool_records(kind, got, r, d, planes, chroma, depth, "%s %s %dx%d %d bits" % (kind, chroma, h, w, depth), prev0=prev0)


# ---- (b) the shipped library at the shipped constant ------------------------------------------------------------------------------
_BIG = {}


def _big(lay):
    """the pool and the batch of 32771 frames of a layout, built once: -> (r, d, planes, batch of r, batch of d)"""
    if lay not in _BIG:
        r, d, planes = SC.pool(*lay)
        _BIG[lay] = (r, d, planes, SC.batch(r, SC.BIG_N), SC.batch(d, SC.BIG_N))
    return _BIG[lay]


def _rows(got):
    """one row of bytes per frame"""
    return np.frombuffer(got.tobytes(), np.uint8).reshape(SC.BIG_N, -1)


def _run_big(eng, kind, lay, prev0_entry=None):
    from rtvqa_amd import _native as N
    r, d, planes, br, bd = _big(lay)
    assert eng.lib.vqa_build_flavour() == 0 or os.environ.get("VQA_LIB_PATH")
    prev0 = None if prev0_entry is None else r[prev0_entry]
    t0 = time.time()
    _submit(eng, kind if prev0 is None else kind + "_p", br, bd, planes, prev0)
    got = _decode(kind, _wait(eng, kind), SC.BIG_N, len(planes))
    print("%s %s: %d frames in %.2f s" % (kind, lay, SC.BIG_N, time.time() - t0))
    return got, prev0


# quality on the 4:2:0 layout alone (tests/test_gpu_parity.py::test_more_than_65535_frames_in_one_submit has the mono seam);
# CIEDE2000 on the two layouts of three planes
BIG_PAIR_CASES = ([(k, SC.BIG[0]) for k in ("gauss", "ffmpeg")] + [(k, lay) for k in ("vif", "adm", "psnr_hvs", "gmsd") for lay in SC.BIG]
                  + [("ciede", SC.BIG[0]), ("ciede", SC.BIG_CIEDE)])


@pytest.mark.parametrize("kind,lay", BIG_PAIR_CASES, ids=["%s-%s-%dx%d-%d" % ((k,) + lay) for k, lay in BIG_PAIR_CASES])
def test_every_record_of_32771_frames_follows_the_pool(engine, kind, lay):
    """a pair metric at the shipped slice length: record i is record i % 7, for every i, as bytes; records 0 .. 7 at the bar"""
    got, _ = _run_big(engine, kind, lay)
    rows = _rows(got)
    wrong = np.nonzero((rows != rows[SC.pair_map(SC.BIG_N)]).any(axis=1))[0]
    assert wrong.size == 0, (kind, lay, wrong[:8], wrong.size)
    # the seven contents do give seven records - but for CIEDE2000 at 4:4:4, where the checkerboard against its inverse and all L
    # against all 0 are the same pixel pair (L, L, L) | (0, 0, 0) on every sample, one way round or the other, and dE00 is symmetric
    same = 1 if kind == "ciede" and lay[0] == "444" else 0
    assert len({rows[e].tobytes() for e in range(SC.PERIOD)}) == SC.PERIOD - same
    assert len({rows[e].tobytes() for e in range(SC.PERIOD - 1)}) == SC.PERIOD - 1
    chroma, h, w, depth = lay
    r, d, planes = _big(lay)[:3]
    _check_pool_records(kind, got, r, d, planes, chroma, depth, "%s %s %dx%d %d bits n=%d" % (kind, chroma, h, w, depth, SC.BIG_N))


@pytest.mark.parametrize("lay", SC.BIG, ids=lambda lay: "%s-%dx%d-%d" % lay)
@pytest.mark.parametrize("prev0_entry", [None, PREV0_ENTRY, OTHER_PREV0], ids=["no_prev0", "prev0_entry6", "prev0_entry2"])
@pytest.mark.parametrize("kind", ["motion", "siti"])
def test_the_previous_frame_is_carried_across_the_seam(engine, kind, prev0_entry, lay):
    """the motion feature and SI/TI at the shipped slice length: record i is record i - 7 for every i >= 8 (frame 32768, the first
    of the second slice, against frame 32767 and not against prev0), as bytes; record 7 equals record 0 only when prev0 is pool
    entry 6; records 0 .. 7 at the bar"""
    got, prev0 = _run_big(engine, kind, lay, prev0_entry)
    rows = _rows(got)
    wrong = np.nonzero((rows != rows[SC.temporal_map(SC.BIG_N)]).any(axis=1))[0]
    assert wrong.size == 0, (kind, lay, wrong[:8], wrong.size)
    assert len({rows[i].tobytes() for i in range(1, SC.PERIOD + 1)}) == SC.PERIOD
    assert (rows[7].tobytes() == rows[0].tobytes()) == (prev0_entry == PREV0_ENTRY), (kind, lay, prev0_entry)
    chroma, h, w, depth = lay
    r, d, planes = _big(lay)[:3]
    _check_pool_records(kind if prev0 is None else kind + "_p", got, r, d, planes, chroma, depth,
                        "%s %s %dx%d %d bits n=%d" % (kind, chroma, h, w, depth, SC.BIG_N), prev0=prev0)


def test_cambi_at_the_seam_on_an_engine_of_its_own():
    """CAMBI, mono 16 x 16 at 10 bits, n = 32771: its grow-only scratch holds a full slice (the reservation is printed: DESIGN.md
    section 3), so the engine is this test's own and is closed before the next test; the second slice reuses the scratch"""
    import rtvqa_amd
    import torch
    lay = SC.BIG[1]
    free0 = torch.cuda.mem_get_info(0)[0]
    with rtvqa_amd.Engine(0) as eng:
        got, _ = _run_big(eng, "cambi", lay)
        held = free0 - torch.cuda.mem_get_info(0)[0]
        print("CAMBI %s n=%d: the engine holds %.3f GB (%.1f KB a frame of the slice)" % (lay, SC.BIG_N, held / 1e9, held / 32768 / 1e3))
    rows = _rows(got)
    wrong = np.nonzero((rows != rows[SC.pair_map(SC.BIG_N)]).any(axis=1))[0]
    assert wrong.size == 0, (wrong[:8], wrong.size)
    chroma, h, w, depth = lay
    r, d, planes = _big(lay)[:3]
    _check_pool_records("cambi", got, r, d, planes, chroma, depth, "cambi mono 16x16 10 bits n=%d" % SC.BIG_N)
    assert torch.cuda.mem_get_info(0)[0] >= free0 - (64 << 20)            # the engine's scratch is back


if __name__ == "__main__":
    _child(sys.argv[1])
