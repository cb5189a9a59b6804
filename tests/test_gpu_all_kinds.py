"""GPU: all seventeen kinds of batch pending on ONE context at once, every kind with frames of its own.

A vqa_ctx has one stream.  Ten pair kinds stage pageable host frames into the same two device buffers (qstage_ref, qstage_dist,
through stage_pair of csrc/vqa_capi.hip), CAMBI, the artefact measures and BRISQUE into qstage_dist, VCA into SI/TI's siti_stage
and siti_prev; what keeps a pending kind's frames from being overwritten is the stream's order, and ensure(), which drains every
stream before a staging buffer is freed to grow.  The other files queue several kinds from ONE upload: there an overwritten, a
skipped or a misordered copy replaces bytes by equal bytes.  Here every kind has its own content (a pool seeded by the kind's
index) and its own frame count n_k in {2, 3, 4, 5} (neighbours in KINDS differ), so a kind that read another kind's staging, or
its own before the copy landed, cannot produce its own records.

Expected records: each kind submitted and waited for alone on the same engine, from host frames, before anything is queued.  At
the 8-bit geometry those alone-records pass through each metric's own checker against its CPU reference (the helpers and bars
of tests/test_gpu_slices.py and of the metric files; no tolerance is introduced here).  Every comparison of a queue with the
alone-records is of bytes (the complexity records field by field without hyst_steps, as tests/test_gpu_parity.py compares them).

Geometry: the smallest every kind takes - yuv420p at 66 x 98 (chroma 33 x 49: odd, no multiple of 8, 16 or 32; VCA wants 32)
and yuv420p10le at 70 x 74 (chroma 35 x 37); the complexity batch reads BGR frames of its own at the same size.  Only one
quality batch can be pending, so vf_ssim's mode and MS-SSIM (gray, 177 x 263: planes of at least 161) ride in a second, shorter
round.

Queues (all submits before the first wait):
  ascending   pageable host arrays, kinds ordered by ascending staged bytes after vqa_trim: every size step grows a shared staging
              buffer while earlier kinds are pending (ensure -> sync_all -> free -> malloc)
  descending  pageable host arrays, descending staged bytes: no growth, pure reuse of a buffer a pending kind still has to read
  device      every kind's own frames uploaded before (Engine.upload): read in place
  mixed       even kinds from host, odd kinds from device
(seventeen kinds and four frame counts: kinds of one n_k stage equal byte counts and sit next to each other in the two sorted
queues; their contents still differ.)  The waits are collected in submission order, in reverse and in a shuffled order (seed
SHUFFLE_SEED).  After every queue the context is idle: an option can be set, and a fresh single-kind submit gives its alone-record."""
import random

import numpy as np
import pytest

import hostile_cases as HK
import mdsi_cases as MC
import motion_cases as K

pytestmark = pytest.mark.gpu

KINDS = ("complexity", "gauss", "vif", "adm", "motion", "siti", "psnr_hvs", "ciede", "gmsd", "cambi", "xpsnr", "haarpsi", "vca",
         "artifacts", "brisque", "mdsi", "itp")
FRAMES = (2, 3, 4, 5)                            # n_k = FRAMES[k % 4]
GEOMETRIES = {"yuv420p": (66, 98, 8), "yuv420p10le": (70, 74, 10)}
MS_GEOMETRY = (177, 263, 8)                      # gray
SECOND_ROUND = (("ffmpeg", "yuv420p"), ("gmsd", "yuv420p"), ("cambi", "yuv420p"), ("vca", "yuv420p"), ("ms", "gray"), ("vif", "gray"),
                ("haarpsi", "gray"), ("motion", "gray"))
QUEUES = ("ascending", "descending", "device", "mixed")
SHUFFLE_SEED = 20261019
PAIRS = ("vif", "adm", "psnr_hvs", "gmsd", "haarpsi", "mdsi")
WITH_PREV0 = ("motion", "siti", "vca")
ONE_STREAM = ("cambi", "artifacts", "brisque")
MDSI_NAMES = ("natural", "noise", "noise", "noise", "noise")      # (the natural reference takes no seed: one frame of it)


def _modes():
    from rtvqa_amd import _native as N
    return {"gauss": N.SSIM_GAUSS, "ffmpeg": N.SSIM_FFMPEG, "ms": N.SSIM_MS}


class Job:
    """one kind's batch: its own frames (host arrays; `dev` once uploaded), frame count and planes"""

    def __init__(self, index, kind, n, layout, h, w, depth):
        from rtvqa_amd import synth
        from rtvqa_amd.engine import mono_planes, yuv_planes
        self.index, self.kind, self.n, self.layout, self.h, self.w, self.depth = index, kind, n, layout, h, w, depth
        self.planes = mono_planes(h, w, depth) if layout == "gray" else yuv_planes(h, w, "420", depth)
        self.dev = None
        seed = 100 * (index + 1)
        if kind == "complexity":                 # BGR frames of its own; frame 0 is prev0
            fr = synth.s_natural(n + 1, h, w, seed=seed)
            self.host = (np.ascontiguousarray(fr[1:]), None, np.ascontiguousarray(fr[0]))
            self.staged = fr[1:].nbytes
            return
        dt = np.uint16 if depth > 8 else np.uint8
        if kind == "mdsi":                       # mdsi_cases' contents (tests/test_gpu_mdsi.py::_clip): the checker admits them
            pairs = [MC.pair(MDSI_NAMES[i], "yuv420p", h, w, depth, seed=seed + i) for i in range(n)]   # (its name for 4:2:0 at any depth)
            self.lists = ([p[0] for p in pairs], [p[1] for p in pairs])
            self.host = (MC.pack(self.lists[0], "yuv420p", depth), MC.pack(self.lists[1], "yuv420p", depth), None)
        else:                                    # the suite's ordinary content, every plane of every frame seeded by itself
            out = [[], []]
            for i in range(n + 1):               # (frame n is prev0, the frame before frame 0)
                parts = [HK.natural_pair(p[1], p[0], depth, seed + 10 * i + j) for j, p in enumerate(self.planes)]
                for o, side in zip(out, (0, 1)):
                    o.append(np.concatenate([pt[side].reshape(-1) for pt in parts]))
            r, d = np.stack(out[0]).astype(dt), np.stack(out[1]).astype(dt)
            self.host = (np.ascontiguousarray(r[:n]), np.ascontiguousarray(d[:n]), np.ascontiguousarray(r[n]))
        self.staged = self.host[0].nbytes        # what one stage() call of this kind copies into a shared buffer

    def upload(self, eng):
        r, d, p0 = self.host
        self.dev = (eng.upload(r), eng.upload(d) if d is not None else None, eng.upload(p0[None]) if p0 is not None else None)

    def free(self):
        for b in self.dev or ():
            if b is not None:
                b._owner.free()
        self.dev = None


def _submit(eng, j, mem="host"):
    """j.frame_bytes and j.model, where a job has them (tests/test_gpu_layouts.py: a host layout's frame stride; the colour model
    of the tight clip, which a layout's pixel step must not change): passed on; otherwise the engine's defaults"""
    from rtvqa_amd import _native as N
    r, d, p0 = j.dev if mem == "device" else j.host
    k = j.kind
    fb = {"frame_bytes": j.frame_bytes} if mem == "host" and getattr(j, "frame_bytes", None) else {}
    model = getattr(j, "model", None)
    if k == "complexity":
        j.params = eng.make_params(dct_mode=N.DCT_BLOCK8)
        eng.complexity_submit(r, p0, N.M_ALL, j.params)
    elif k in ("gauss", "ffmpeg", "ms"):
        eng.quality_submit(r, d, j.planes, _modes()[k], **fb)
    elif k in ("mdsi", "itp"):
        getattr(eng, k + "_submit")(r, d, j.planes, model=model, **fb)
    elif k in PAIRS:
        getattr(eng, k + "_submit")(r, d, j.planes, **fb)
    elif k == "ciede":
        eng.ciede_submit(r, d, j.planes, model=model, weights=(1.0, 1.0, 1.0), **fb)
    elif k == "xpsnr":
        eng.xpsnr_submit(r, d, j.planes, prev0=p0, **fb)
    elif k in WITH_PREV0:
        getattr(eng, k + "_submit")(r, j.planes, prev0=p0, **fb)
    elif k in ONE_STREAM:
        getattr(eng, k + "_submit")(d, j.planes, **fb)
    else:
        raise KeyError(k)


def _wait(eng, j):
    """-> (the batch's result as a tuple of bytes: the records, then XPSNR's and VCA's block maps, MS-SSIM's scales; the raw result)"""
    k = j.kind
    if k == "complexity":
        import test_gpu_parity as TPAR
        rec = eng.complexity_wait()
        return TPAR._stable(rec), rec
    if k == "ms":
        raw = eng.quality_wait(scales=True)
        return tuple(a.tobytes() for a in raw), raw
    if k in ("gauss", "ffmpeg"):
        raw = eng.quality_wait()
    elif k == "xpsnr":
        raw = eng.xpsnr_wait(blocks=True)
        return (raw[0].tobytes(),) + tuple(raw[1][key].tobytes() for key in ("sa", "ta", "n", "sse")), raw
    elif k == "vca":
        raw = eng.vca_wait(blocks=True)
        return (raw[0].tobytes(),) + tuple(m[key].tobytes() for m in raw[1] for key in ("qh", "s")), raw
    else:
        raw = getattr(eng, k + "_wait")()
    return (raw.tobytes(),), raw


class Round:
    """the jobs of one geometry with their alone-records"""

    def __init__(self, eng, jobs):
        self.jobs, self.want, self.raw = jobs, {}, {}
        for j in jobs:
            _submit(eng, j)
            self.want[j.kind], self.raw[j.kind] = _wait(eng, j)
        for j in jobs:
            j.upload(eng)

    def free(self):
        for j in self.jobs:
            j.free()


@pytest.fixture(scope="module")
def rounds(engine):
    """every job and its alone-record, collected before anything is queued: {"yuv420p", "yuv420p10le", "second": Round}"""
    out = {}
    for layout, (h, w, depth) in GEOMETRIES.items():
        out[layout] = Round(engine, [Job(k, kind, FRAMES[k % 4], layout, h, w, depth) for k, kind in enumerate(KINDS)])
    jobs = []
    for k, (kind, layout) in enumerate(SECOND_ROUND):
        h, w, depth = MS_GEOMETRY if layout == "gray" else GEOMETRIES[layout]
        jobs.append(Job(len(KINDS) + k, kind, FRAMES[(k + 1) % 4], layout, h, w, depth))
    out["second"] = Round(engine, jobs)
    yield out
    for r in out.values():
        r.free()


def test_the_jobs_are_what_the_queues_need():
    """(host) neighbouring kinds differ in their frame count, every count is used, and no two kinds share a frame"""
    ns = [FRAMES[k % 4] for k in range(len(KINDS))]
    assert len(KINDS) == 17 and all(a != b for a, b in zip(ns, ns[1:])) and set(ns) == set(FRAMES)
    h, w, depth = GEOMETRIES["yuv420p"]
    seen = set()
    for k, kind in enumerate(KINDS):
        j = Job(k, kind, ns[k], "yuv420p", h, w, depth)
        for a in j.host:
            if a is not None:
                rows = a.reshape(j.n if a is not j.host[2] else 1, -1)
                for row in rows:
                    assert row.tobytes() not in seen, kind
                    seen.add(row.tobytes())


# ---- the alone-records against the references -------------------------------------------------------------------------------------
def _lists(a, planes):
    """[n, samples] -> n lists of int64 planes"""
    series = [K.plane_series(a, p) for p in planes]
    return [[s[i] for s in series] for i in range(a.shape[0])]


def _anchor(j, raw, oracle):
    import test_gpu_slices as TSL
    r, d, p0 = j.host
    k, planes, depth = j.kind, j.planes, j.depth
    tag = "all kinds, alone: %s %s %dx%d n=%d" % (k, j.layout, j.h, j.w, j.n)
    chroma = "mono" if j.layout == "gray" else "420"
    if k == "complexity":
        import test_gpu_parity as TPAR
        co, fr = oracle, np.concatenate([p0[None], r])
        for i in range(j.n):
            g, gp = co.bgr2gray(fr[i + 1]), co.bgr2gray(fr[i])
            assert (raw[i]["hist_gray"] == co.hist_u8(g)).all(), (tag, i)
            for c in range(3):
                assert (raw[i]["hist_bgr"][c] == co.hist_u8(fr[i + 1], offset=c, step=3)).all(), (tag, i, c)
            e, l1, _ = co.dct8x8(gp, g)
            assert TPAR._rel(raw[i]["dct_energy"], e) < TPAR.RTOL and TPAR._rel(raw[i]["temporal_dct_l1"], l1) < TPAR.RTOL, (tag, i)
            cnt, strong, weak = co.canny(g, 100, 200)
            assert (int(raw[i]["edge_strong"]), int(raw[i]["edge_weak"]), int(raw[i]["edge_count"])) == (strong, weak, cnt), (tag, i)
            _nb, sad, hist = co.block_sad(gp, g, 7)
            assert int(raw[i]["sad_sum"]) == sad and (raw[i]["mv_d2_hist"] == hist).all(), (tag, i)
    elif k in ("gauss", "ffmpeg", "ms", "vif", "adm", "psnr_hvs", "ciede", "gmsd", "cambi"):
        TSL._check_kind(k, raw, r, d, planes, chroma, depth, tag)
    elif k in ("motion", "siti"):
        TSL._check_kind(k + "_p", raw, r, d, planes, chroma, depth, tag, prev0=p0)
    elif k == "xpsnr":
        import test_gpu_xpsnr as TX
        TX._check(raw[0], raw[1], _lists(r, planes), _lists(d, planes), _lists(p0[None], planes)[0], depth, tag)
    elif k == "haarpsi":
        import test_gpu_haarpsi as THP
        with TSL._fresh(THP.WORST, "haarpsi"):
            THP.check(raw, r, d, planes, depth, tag)
    elif k == "vca":
        import test_gpu_vca as TVC
        with TSL._fresh(TVC.WORST, "vca"):
            TVC._check(raw[0], raw[1], _lists(r, planes), _lists(p0[None], planes)[0], depth, tag)
    elif k == "artifacts":
        import test_gpu_artifacts as TAR
        TAR._check(raw, d, planes, depth, tag)
    elif k == "brisque":
        import brisque_reference as BR
        import test_gpu_brisque as TBQ
        for jx, p in enumerate(planes):
            series = K.plane_series(d, p)
            for i in range(j.n):
                x = series[i]
                ft, flags, ks = BR.float_features(x, depth)
                want = dict(x=x, moments=BR.float_moments(x, depth), features=ft, flags=flags, ks=ks, spans=BR.alpha_spans(x, depth))
                TBQ._check_record(raw[i, jx], want, ("all kinds", j.h, j.w, j.layout, i, jx))
    elif k == "mdsi":
        import test_gpu_mdsi as TMD
        with TSL._fresh(TMD.WORST, "mdsi"):
            for i in range(j.n):
                TMD._check_one(raw[i], j.lists[0][i], j.lists[1][i], "yuv420p", depth, "%s frame %d" % (tag, i))
    elif k == "itp":
        import itp_cases as IC
        import itp_reference as IR
        import test_gpu_itp as TI
        with TSL._fresh(TI.WORST, "itp"):
            TI._check(raw, IC.reference(r, d, planes, depth, IR.YUV2020, IR.PQ, False), j.h, j.w, tag)
    else:
        raise KeyError(k)


@pytest.mark.parametrize("kind", KINDS)
def test_the_alone_records_meet_their_references(rounds, oracle, kind):
    """the 8-bit geometry: what every queue is compared with is itself what the metric's CPU reference says of these frames"""
    rd = rounds["yuv420p"]
    j = rd.jobs[KINDS.index(kind)]
    assert j.kind == kind and j.n == FRAMES[KINDS.index(kind) % 4]
    _anchor(j, rd.raw[kind], oracle)


@pytest.mark.parametrize("at", range(len(SECOND_ROUND)), ids=["%s-%s" % s for s in SECOND_ROUND])
def test_the_alone_records_of_the_second_round_meet_their_references(rounds, oracle, at):
    rd = rounds["second"]
    _anchor(rd.jobs[at], rd.raw[rd.jobs[at].kind], oracle)


# ---- the queues --------------------------------------------------------------------------------------------------------------
def _queue_of(jobs, queue):
    """-> [(job, "host" | "device")] in submission order"""
    jobs = list(jobs)
    if queue == "ascending":
        return [(j, "host") for j in sorted(jobs, key=lambda j: (j.staged, j.index))]
    if queue == "descending":
        return [(j, "host") for j in sorted(jobs, key=lambda j: (-j.staged, j.index))]
    if queue == "device":
        return [(j, "device") for j in jobs]
    return [(j, "device" if at % 2 else "host") for at, j in enumerate(jobs)]


def _orders(count):
    plain, rng = list(range(count)), random.Random(SHUFFLE_SEED)
    shuffled = list(plain)
    while shuffled in (plain, plain[::-1]):      # (a short queue may draw one of the other two orders: draw again)
        rng.shuffle(shuffled)
    return {"in order": plain, "reversed": plain[::-1], "shuffled": shuffled}


def _idle(eng, want, j):
    """nothing is pending (an option is refused while anything is), and a fresh submit of one kind gives its alone-record"""
    from rtvqa_amd import _native as N
    eng.set_option(N.OPT_OVERLAP, eng.get_option(N.OPT_OVERLAP))
    _submit(eng, j)
    assert _wait(eng, j)[0] == want[j.kind], ("alone again", j.kind)


def _run_queue(eng, jobs, want, queue, order, trim_first=False):
    """all of `jobs` submitted before the first wait, waited for in `order` (indices into the queue): the alone-records"""
    q = _queue_of(jobs, queue)
    if trim_first:
        eng.trim()                               # the staging buffers start empty: the ascending queue has to grow them
    for j, mem in q:
        _submit(eng, j, mem)
    got = {}
    for at in order:
        got[q[at][0].kind] = _wait(eng, q[at][0])[0]
    bad = [k for k in got if got[k] != want[k]]
    assert not bad, (queue, "kinds whose records are not their alone-records", bad)
    assert len(got) == len(jobs)


@pytest.mark.parametrize("queue", QUEUES)
@pytest.mark.parametrize("layout", list(GEOMETRIES))
def test_sixteen_kinds_in_flight_each_with_frames_of_its_own(engine, rounds, layout, queue):
    """(named when KINDS held sixteen: every kind of KINDS, seventeen since dE_ITP joined)"""
    rd = rounds[layout]
    assert [j.kind for j in rd.jobs] == list(KINDS)
    if queue in ("ascending", "descending"):
        sizes = [j.staged for j, _mem in _queue_of(rd.jobs, queue)]
        assert sizes == sorted(sizes, reverse=queue == "descending") and len(set(sizes)) >= len(FRAMES)
    for at, (name, order) in enumerate(_orders(len(rd.jobs)).items()):
        _run_queue(engine, rd.jobs, rd.want, queue, order, trim_first=queue == "ascending")
        _idle(engine, rd.want, rd.jobs[(5 * QUEUES.index(queue) + 3 * at) % len(rd.jobs)])


@pytest.mark.parametrize("layout", list(GEOMETRIES))
def test_trim_changes_nothing_in_a_repeat_of_the_descending_queue(engine, rounds, layout):
    rd = rounds[layout]
    order = _orders(len(rd.jobs))["shuffled"]
    _run_queue(engine, rd.jobs, rd.want, "descending", order)
    engine.trim()
    _run_queue(engine, rd.jobs, rd.want, "descending", order)
    _idle(engine, rd.want, rd.jobs[KINDS.index("xpsnr")])


@pytest.mark.parametrize("queue", QUEUES)
def test_the_second_round_with_vf_ssim_and_ms_ssim_in_flight(engine, rounds, queue):
    """vf_ssim's mode on 4:2:0 and MS-SSIM on gray 177 x 263 (with its per-scale means), each beside kinds of its own geometry;
    two quality batches cannot be pending together, so the round is queued in two halves"""
    rd = rounds["second"]
    for half in (rd.jobs[:4], rd.jobs[4:]):
        for order in _orders(len(half)).values():
            _run_queue(engine, half, rd.want, queue, order, trim_first=queue == "ascending")
        _idle(engine, rd.want, half[0])
