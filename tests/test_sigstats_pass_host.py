"""The one-pass pipeline (stream.run) with the signal statistics on, against the stand-in engine of test_stream_pass_host.py: the new
kind's call shape - the first kind of the table with both a halo and parameters -, its halo from chunk 1 on, its place at the end of
the submits and of the tuple, its parameters validated whether it is on or off; and with it off, the tuple and every call are what
they were.  No GPU and no shared library."""
import numpy as np
import pytest

import test_stream_pass_host as P
from rtvqa_amd import engine as E
from rtvqa_amd import stream


class StandIn(P.StandIn):
    """the stand-in with the new kind: submit(frames, planes, prev0, black_level, crop_level) - all five positional"""

    def sigstats_submit(self, frames, planes, prev0, black_level, crop_level):
        self._submit("sigstats", (frames,), planes, prev0, extra=(black_level, crop_level))

    def sigstats_wait(self):
        return self._wait("sigstats", E.SIGSTATS_DTYPE)


def _run(eng, **switches):
    ref, dist = P._clips()
    q, series = stream.run(dist, ref, quality=stream.Quality(P.PLANES, **switches), batch_size=P.BATCH, engine=eng)
    assert series is None
    return q


def _halo(q0):
    return (P.REF_PTR + (q0 - 1) * P.FB, 1) if q0 else None


def test_the_table_entry():
    kind = stream.PLANE_KINDS[-1]
    assert [k.name for k in stream.PLANE_KINDS] == P.ORDER + ["sigstats"]
    assert (kind.reads, kind.halo, kind.per_frame, kind.dtype) == ("ref", True, False, E.SIGSTATS_DTYPE)
    assert kind.check is None and kind.wait == () and kind.whole is None
    assert [(k.name, k.halo, bool(k.params)) for k in stream.PLANE_KINDS if k.halo and k.params] == [("sigstats", True, True)]


@pytest.mark.parametrize("levels", [(None, None), (40, 0), (0, 65535)])
def test_the_call_shape_and_the_halo(levels):
    eng = StandIn()
    q = _run(eng, sigstats=True, sigstats_black=levels[0], sigstats_crop=levels[1])
    assert len(q) == 3 and q[2].dtype == E.SIGSTATS_DTYPE and q[2].shape == (P.N_FRAMES, len(P.PLANES))
    assert [m for _l, m, *_ in eng.log] == ["quality_submit", "sigstats_submit", "quality_wait", "sigstats_wait"] * len(P.CHUNKS)
    for (q0, qn), call in zip(P.CHUNKS, [c for c in eng.log if c[1] == "sigstats_submit"]):
        assert call == (0, "sigstats_submit", [(P.REF_PTR + q0 * P.FB, qn)], _halo(q0), levels)     # the REFERENCE frames
    assert all(c[4] == () for c in eng.log if c[1] == "sigstats_wait")


def test_alone_it_reads_one_stream():
    eng = StandIn()
    q = _run(eng, sigstats="only", sigstats_crop=7)
    assert len(q) == 3 and q[0] is None and q[1] is None and q[2].shape == (P.N_FRAMES, len(P.PLANES))
    assert [m for _l, m, *_ in eng.log] == ["sigstats_submit", "sigstats_wait"] * len(P.CHUNKS)
    assert all(ptr < P.DIST_PTR for call in eng.log for ptr, _n in call[2])
    assert [c[3] for c in eng.log if c[1] == "sigstats_submit"] == [_halo(q0) for q0, _qn in P.CHUNKS]
    assert all(c[4] == (None, 7) for c in eng.log if c[1] == "sigstats_submit")


def test_every_switch_on_it_comes_last():
    eng = StandIn()
    q = _run(eng, sigstats=True, sigstats_black=33, **P.ALL_ON)
    order = P.ORDER + ["sigstats"]
    per_chunk = 2 * (1 + len(order))
    assert len(eng.log) == len(P.CHUNKS) * per_chunk and not eng.pending
    for c, (q0, qn) in enumerate(P.CHUNKS):
        calls = eng.log[c * per_chunk:(c + 1) * per_chunk]
        assert [m for _l, m, *_ in calls] == (["quality_submit"] + [k + "_submit" for k in order] + ["quality_wait"]
                                              + [k + "_wait" for k in order])
        ref, dist = (P.REF_PTR + q0 * P.FB, qn), (P.DIST_PTR + q0 * P.FB, qn)
        for call, name in zip(calls[1:], P.ORDER):          # every existing kind keeps its call shape
            reads, has_halo, _dt, _pf, extra = P.KINDS[name]
            assert call == (0, name + "_submit", P._streams(reads, ref, dist), _halo(q0) if has_halo else None, extra), (c, name)
        assert calls[1 + len(P.ORDER)] == (0, "sigstats_submit", [ref], _halo(q0), (33, None))
    assert len(q) == 2 + len(order) == 20 and q[-1].dtype == E.SIGSTATS_DTYPE
    for at, name in enumerate(P.ORDER, start=2):
        P._check_element(q[at], name, blocks=True)
    named = stream.records_by_kind(q, stream.Quality(P.PLANES, sigstats=True, **P.ALL_ON))
    assert named["sigstats"] is q[-1] and named["fsim"] is q[-2]


@pytest.mark.parametrize("switches", [P.ALL_ON, dict(fsim=True), dict(motion=True, cambi="only"), dict(vif=True, siti=True)])
def test_with_it_off_the_tuple_and_every_call_are_what_they_were(switches):
    """the stand-in of test_stream_pass_host.py has no sigstats_submit: a pass that called it would fail"""
    old, new = P.StandIn(), StandIn()
    q0 = P._run(old, **switches)
    q1 = _run(new, sigstats=False, sigstats_black=None, sigstats_crop=None, **switches)
    assert old.log == new.log and "sigstats_submit" not in [m for _l, m, *_ in new.log]
    assert len(q0) == len(q1)
    for a, b in zip(q0, q1):
        assert (a is None and b is None) or type(a) is type(b)
    q2 = _run(StandIn(), sigstats=True, **switches)
    assert len(q2) == len(q0) + 1 and q2[-1].dtype == E.SIGSTATS_DTYPE


def test_the_parameters_are_validated_on_or_off():
    for on in (False, True, "only"):
        for key in ("sigstats_black", "sigstats_crop"):
            for bad in (-1, 65536, 1.0, "24", False):
                with pytest.raises(ValueError, match="%s must be None or an integer from 0 to 65535" % key):
                    stream.Quality(P.PLANES, sigstats=on, **{key: bad})
    q = stream.Quality(P.PLANES, sigstats_black=np.int64(5))
    assert q.sigstats_black == 5 and type(q.sigstats_black) is int


def test_a_failing_submit_propagates_and_drains_the_lane():
    eng = StandIn(fail="sigstats")
    with pytest.raises(RuntimeError, match="sigstats_submit failed"):
        _run(eng, sigstats=True, gmsd=True)
    assert eng.drained == 1 and sorted(eng.pending) == ["gmsd", "quality"]
