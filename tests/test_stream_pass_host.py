"""The one-pass pipeline (stream.run) against a stand-in engine: which engine calls a chunk makes, in what order, on which
frames, and the positional tuple the pass builds from what they return.  No GPU and no shared library: the clips are
DeviceFrames over made-up pointers, which the pass only slices, and the stand-in records every call and returns zero records.

Seven frames of yuv420p at 64 x 64 (VCA needs 32 x 32 chroma) with batch_size 3: chunks of 3 + 3 + 1 frames, so the halo frame
before the chunk exists from chunk 1 on.

The expected sequences are restated here (KINDS below), not taken from the code under test: per kind the stream it reads, whether
it gets the frame before the chunk, one record per plane or per frame, and its extra submit arguments."""
import numpy as np
import pytest

from rtvqa_amd import _native as N
from rtvqa_amd import engine as E
from rtvqa_amd import stream

H = W = 64
N_FRAMES, BATCH = 7, 3
FB = H * W * 3 // 2                       # bytes of a yuv420p frame
REF_PTR, DIST_PTR = 0x10000000, 0x20000000
PLANES = E.yuv420p_planes(H, W)
CHUNKS = ((0, 3), (3, 3), (6, 1))         # (first frame, frames)
WEIGHTS = (1.0, 2.0, 0.5)
# kind: (stream it reads, halo, record dtype, one record per frame instead of per plane, extra submit arguments), in the order of
# the submits and of the tuple's elements
KINDS = {
    "vif": ("pair", False, E.VIF_DTYPE, False, ()),
    "adm": ("pair", False, E.ADM_DTYPE, False, ()),
    "motion": ("ref", True, E.MOTION_DTYPE, False, ()),
    "siti": ("ref", True, E.SITI_DTYPE, False, ()),
    "psnr_hvs": ("pair", False, E.PSNR_HVS_DTYPE, False, ()),
    "ciede": ("pair", False, E.CIEDE_DTYPE, True, (None, WEIGHTS)),
    "gmsd": ("pair", False, E.GMSD_DTYPE, False, ()),
    "cambi": ("dist", False, E.CAMBI_DTYPE, False, ()),
    "xpsnr": ("pair", True, E.XPSNR_DTYPE, False, ()),
    "haarpsi": ("pair", False, E.HAARPSI_DTYPE, False, ()),
    "vca": ("ref", True, E.VCA_DTYPE, False, ()),
    "artifacts": ("dist", False, E.ARTIFACTS_DTYPE, False, ()),
    "brisque": ("dist", False, E.BRISQUE_DTYPE, False, ()),
    "mdsi": ("pair", False, E.MDSI_DTYPE, True, ()),
    "itp": ("pair", False, E.ITP_DTYPE, True, (None, "hlg", True)),
    "pu21": ("pair", False, E.PU21_DTYPE, True, (None, "pq", True)),
    "fsim": ("pair", False, E.FSIM_DTYPE, True, ()),
}
ORDER = list(KINDS)
PARAMS = dict(ciede_weights=WEIGHTS, itp_transfer="hlg", itp_full_range=True, pu21_transfer="pq", pu21_full_range=True)
ALL_ON = dict({k: True for k in ORDER}, vca_blocks=True, **PARAMS)


def _clips():
    return tuple(E.DeviceFrames(ptr, N_FRAMES, 1, FB, channels=1) for ptr in (REF_PTR, DIST_PTR))


def _at(frames):
    return None if frames is None else (frames.ptr, frames.n)


class StandIn:
    """an Engine as the pass sees it: device, drain() and a submit / wait pair per kind.  Every call is appended to `log` (shared
    between the lanes of a pass) as (lane, method, streams [(ptr, n)], prev0 (ptr, n) or None, extra arguments)"""
    device = 0

    def __init__(self, log=None, lane=0, fail=None):
        self.log, self.lane, self.fail = [] if log is None else log, lane, fail
        self.drained = 0
        self.pending = {}

    def drain(self):
        self.drained += 1

    def _submit(self, kind, streams, planes, prev0=None, extra=()):
        assert planes is PLANES and kind not in self.pending
        self.log.append((self.lane, kind + "_submit", [_at(s) for s in streams], _at(prev0), tuple(extra)))
        if kind == self.fail:
            raise RuntimeError("%s_submit failed" % kind)
        self.pending[kind] = streams[0].n

    def _wait(self, kind, dtype, per_frame=False, extra=()):
        n = self.pending.pop(kind)
        self.log.append((self.lane, kind + "_wait", [], None, tuple(extra)))
        return np.zeros(n if per_frame else (n, len(PLANES)), dtype)

    def quality_submit(self, ref, dist, planes, ssim_mode=N.SSIM_GAUSS):
        self._submit("quality", (ref, dist), planes, extra=(ssim_mode,))

    def quality_wait(self, scales=False):
        rec = self._wait("quality", E.PLANE_DTYPE, extra=(scales,))
        sc = np.zeros(rec.shape + (N.MS_LEVELS,))
        return (rec, sc, sc.copy()) if scales else rec

    def vca_wait(self, blocks=False):
        rec = self._wait("vca", E.VCA_DTYPE, extra=(blocks,))
        grids = [E.vca_grid(p[0], p[1])[::-1] for p in PLANES]
        return (rec, [dict(qh=np.zeros((len(rec),) + g, np.uint64), s=np.zeros((len(rec),) + g, np.uint64)) for g in grids]) if blocks else rec


def _add_kind(name, reads, halo, dtype, per_frame):
    if reads == "pair" and halo:       # xpsnr: the halo follows the planes
        def submit(self, ref, dist, planes, prev0=None):
            self._submit(name, (ref, dist), planes, prev0)
    elif reads == "pair":
        def submit(self, ref, dist, planes, *extra):
            self._submit(name, (ref, dist), planes, extra=extra)
    elif halo:
        def submit(self, ref, planes, prev0=None):
            self._submit(name, (ref,), planes, prev0)
    else:
        def submit(self, frames, planes):
            self._submit(name, (frames,), planes)
    setattr(StandIn, name + "_submit", submit)
    if name != "vca":
        setattr(StandIn, name + "_wait", lambda self: self._wait(name, dtype, per_frame))


for _name, (_reads, _halo, _dtype, _per_frame, _extra) in KINDS.items():
    _add_kind(_name, _reads, _halo, _dtype, _per_frame)


def _run(eng=None, **switches):
    ref, dist = _clips()
    q, series = stream.run(dist, ref, quality=stream.Quality(PLANES, **switches), batch_size=BATCH, engine=eng)
    assert series is None
    return q


def _streams(reads, ref, dist):
    """the (ptr, n) a submit of a kind that reads `reads` receives, ref / dist being the chunk's frames of either clip"""
    return {"pair": [ref, dist], "ref": [ref], "dist": [dist]}[reads]


def _expected_dtype(name):
    return stream.MOTION_PASS_DTYPE if name == "motion" else KINDS[name][2]


def _check_element(got, name, blocks=False):
    if name == "vca" and blocks:
        rec, maps = got
        assert rec.dtype == E.VCA_DTYPE and rec.shape == (N_FRAMES, len(PLANES)) and len(maps) == len(PLANES)
        for p, m in zip(PLANES, maps):
            gx, gy = E.vca_grid(p[0], p[1])
            assert sorted(m) == ["qh", "s"] and m["qh"].shape == m["s"].shape == (N_FRAMES, gy, gx) and m["qh"].dtype == np.uint64
        return
    assert got.dtype == _expected_dtype(name), name
    assert got.shape == ((N_FRAMES,) if KINDS[name][3] else (N_FRAMES, len(PLANES))), name


def test_every_switch_on_calls_in_table_order_on_the_right_frames():
    eng = StandIn()
    q = _run(eng, **ALL_ON)
    assert eng.drained == 0 and not eng.pending
    per_chunk = 2 * (1 + len(ORDER))
    assert len(eng.log) == len(CHUNKS) * per_chunk
    for c, (q0, qn) in enumerate(CHUNKS):        # one lane: submit c, wait c, submit c + 1 ...
        calls = eng.log[c * per_chunk:(c + 1) * per_chunk]
        ref, dist = (REF_PTR + q0 * FB, qn), (DIST_PTR + q0 * FB, qn)
        halo = (REF_PTR + (q0 - 1) * FB, 1) if q0 else None
        assert [m for _l, m, *_ in calls] == ["quality_submit"] + [k + "_submit" for k in ORDER] + ["quality_wait"] + [k + "_wait" for k in ORDER]
        assert calls[0] == (0, "quality_submit", [ref, dist], None, (N.SSIM_GAUSS,))
        for call, name in zip(calls[1:], ORDER):
            reads, has_halo, _dt, _pf, extra = KINDS[name]
            assert call == (0, name + "_submit", _streams(reads, ref, dist), halo if has_halo else None, extra), (c, name)
        waits = dict((m, x) for _l, m, _s, _p, x in calls[1 + len(ORDER):])
        assert waits["quality_wait"] == (False,) and waits["vca_wait"] == (True,)
        assert all(x == () for m, x in waits.items() if m not in ("quality_wait", "vca_wait"))
    assert isinstance(q, tuple) and len(q) == 2 + len(ORDER) == 19
    assert q[0].dtype == np.uint64 and q[1].dtype == np.float64 and q[0].shape == q[1].shape == (N_FRAMES, len(PLANES))
    for at, name in enumerate(ORDER, start=2):
        _check_element(q[at], name, blocks=True)


def _want_layout(name, value):
    """the tuple of a pass with one kind on: [None or "sse" / "ssim" ..., placeholders, the kind's element]"""
    head = [None, None] if value == "only" else ["sse", "ssim"]
    return head + {"vif": [], "adm": [None], "motion": [None, None]}.get(name, []) + [name]


@pytest.mark.parametrize("value", [True, "only"])
@pytest.mark.parametrize("name", ORDER)
def test_one_kind_alone(name, value):
    eng = StandIn()
    q = _run(eng, **{name: value})
    want = _want_layout(name, value)
    assert isinstance(q, tuple) and len(q) == len(want)
    for got, w in zip(q, want):
        if w is None:
            assert got is None
        elif w in ("sse", "ssim"):
            assert got.shape == (N_FRAMES, len(PLANES)) and got.dtype == (np.uint64 if w == "sse" else np.float64)
        else:
            _check_element(got, w)
    methods = [m for _l, m, *_ in eng.log]
    per_chunk = (["quality_submit"] if value is True else []) + [name + "_submit"] + (["quality_wait"] if value is True else []) + [name + "_wait"]
    assert methods == per_chunk * len(CHUNKS)
    # a kind that reads one stream, alone and as "only": the pass reads `ref` and nothing else - the distorted clip is never handed
    # to the engine, and CAMBI, the artefact measures and BRISQUE measure the reference clip's frames
    reads = KINDS[name][0]
    submits = [call for call in eng.log if call[1] == name + "_submit"]
    for (q0, qn), call in zip(CHUNKS, submits):
        ref, dist = (REF_PTR + q0 * FB, qn), (DIST_PTR + q0 * FB, qn)
        if value == "only" and reads != "pair":
            assert call[2] == [ref]
        else:
            assert call[2] == _streams(reads, ref, dist)
        assert call[3] == ((REF_PTR + (q0 - 1) * FB, 1) if KINDS[name][1] and q0 else None)
    if value == "only" and reads != "pair":
        assert all(ptr < DIST_PTR for call in eng.log for ptr, _n in call[2])


def test_cambi_only_beside_motion_reads_the_reference_clip():
    eng = StandIn()
    q = _run(eng, cambi="only", motion=True)
    assert len(q) == 6 and all(x is None for x in q[:4])
    _check_element(q[4], "motion")
    _check_element(q[5], "cambi")
    assert [m for _l, m, *_ in eng.log] == ["motion_submit", "cambi_submit", "motion_wait", "cambi_wait"] * len(CHUNKS)
    for (q0, qn), c in zip(CHUNKS, range(len(CHUNKS))):
        motion, cambi = eng.log[4 * c], eng.log[4 * c + 1]
        assert motion[2] == cambi[2] == [(REF_PTR + q0 * FB, qn)]
        assert motion[3] == ((REF_PTR + (q0 - 1) * FB, 1) if q0 else None) and cambi[3] is None


@pytest.mark.parametrize("name", ["cambi", "artifacts", "brisque"])
def test_a_dist_reading_kind_as_true_beside_an_only_reads_the_distorted_clip(name):
    """siti="only" drops SSE / SSIM, but <kind>=True still asks for the distorted stream: the pass reads both"""
    eng = StandIn()
    q = _run(eng, siti="only", **{name: True})
    assert len(q) == 4 and q[0] is None and q[1] is None
    for (q0, qn), call in zip(CHUNKS, [c for c in eng.log if c[1] == name + "_submit"]):
        assert call[2] == [(DIST_PTR + q0 * FB, qn)]


def test_two_lanes_alternate_the_chunks(monkeypatch):
    log = []
    lanes = (StandIn(log, 0), StandIn(log, 1))
    monkeypatch.setattr(stream, "get_engine", lambda device=None: lanes[0])
    monkeypatch.setattr(stream, "get_engine_lanes", lambda device=None, count=2: lanes[:count])
    q = _run(None, gmsd=True, motion=True)
    assert len(q) == 6 and q[2] is None and q[3] is None
    steps = []                                  # (lane, "submit" / "wait") per chunk, from the SSE / SSIM batch's calls
    for lane, m, *_ in log:
        if m.startswith("quality_"):
            steps.append((lane, m[len("quality_"):]))
    assert steps == [(0, "submit"), (1, "submit"), (0, "wait"), (0, "submit"), (1, "wait"), (0, "wait")]
    submits = [c for c in log if c[1] == "gmsd_submit"]
    assert [(c[0], c[2][0]) for c in submits] == [(k % 2, (REF_PTR + q0 * FB, qn)) for k, (q0, qn) in enumerate(CHUNKS)]
    assert lanes[0].drained == lanes[1].drained == 0 and not lanes[0].pending and not lanes[1].pending


def test_a_failing_submit_propagates_and_drains_the_lane():
    eng = StandIn(fail="gmsd")
    with pytest.raises(RuntimeError, match="gmsd_submit failed"):
        _run(eng, **ALL_ON)
    assert eng.drained == 1
    # the first chunk got as far as GMSD: what was submitted before it is still pending for drain() to find, nothing came after
    assert [m for _l, m, *_ in eng.log] == ["quality_submit"] + [k + "_submit" for k in ORDER[:ORDER.index("gmsd") + 1]]
    assert sorted(eng.pending) == sorted(["quality"] + ORDER[:ORDER.index("gmsd")])


@pytest.mark.parametrize("switches", [ALL_ON, dict(ALL_ON, vca_blocks=False, vif=False), dict(cambi="only", motion=True), dict(fsim=True),
                                      dict(adm="only"), dict(vif=True, siti=True, itp=True)])
def test_the_tuple_by_kind_name(switches):
    quality = stream.Quality(PLANES, **switches)
    ref, dist = _clips()
    q, _ = stream.run(dist, ref, quality=quality, batch_size=BATCH, engine=StandIn())
    named = stream.records_by_kind(q, quality)
    assert named["sse"] is q[0] and named["ssim"] is q[1]
    on = [k for k in ORDER if switches.get(k)]
    placeholders = [k for k in ("vif", "adm") if not switches.get(k) and any(switches.get(j) for j in ORDER[ORDER.index(k) + 1:3])]
    assert sorted(named) == sorted(["sse", "ssim"] + on + placeholders)
    for k in placeholders:
        assert named[k] is None
    tail = [k for k in ORDER if k in on or k in placeholders]
    for at, k in enumerate(tail, start=len(q) - len(tail)):
        assert named[k] is q[at], k
    # the same from a plain mapping of the switches, as _write_feature_log has them
    again = stream.records_by_kind(q, {k: bool(switches.get(k)) for k in ORDER})
    assert list(again) == list(named) and all(again[k] is named[k] for k in named)
