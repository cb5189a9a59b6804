"""The one chain of pre-passes behind run_ffmpeg_metrics and process_video_and_extract_metrics, without a device: every
combination of sync, light, align, shift, colorfit and conform through both entry points, with the frame_* calls and stream.run
replaced by the stand-ins of tests/prepass_chain_cases.py.

tests/golden/prepass_trace.json holds what the commit BEFORE the chain did in every case - both entry points then carried the
sequence written out by hand - recorded by oracle/gen_prepass_trace.py with the same stand-ins.  A case passes when the chain
makes the same calls with the same frames in the same order, hands stream.run the same streams, planes and plan, writes the
same log and ends in the same error."""
import json
import os

import pytest

import prepass_chain_cases as PC
from rtvqa_amd import video_processing as vp

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prepass_trace.json")) as _f:
    _DOC = json.load(_f)
CASES = list(PC.cases())
GOLDEN = dict(zip((PC.case_name(counts, kw) for counts, kw in CASES), PC.unpack(_DOC)))


def test_the_golden_file_holds_every_case_and_no_other():
    assert len(_DOC["cases"]) == len(CASES) == len(GOLDEN) and _DOC["commit"] == "f21e14170dd34e3fcba20a3c4923086f4315e5a7"
    assert len(CASES) == 3 * 2 * 2 * 2 * 2 * 4 + 2 * 2 * 2 * 2 * 2 * 4   # the issue's product, and again without a trim at 10 / 10


def test_the_table_is_the_key_order():
    assert [(p.name, tuple(p.keys)) for p in vp.PREPASSES] == [(name, tuple(keys)) for name, keys in PC.PREPASS_KEYS]


def test_with_everything_off_the_chain_touches_nothing(monkeypatch):
    """no pre-pass: the streams come back as the objects they were - not sliced, not copied, not even looked at -, extra stays
    None (or the scaled pass's two keys), there is no plan and nothing asks for a log"""
    def touched(*a, **kw):
        raise AssertionError("a stream was touched")
    for name in ("_host_stream", "_frame_slice", "_frame_count", "_sync_streams"):
        monkeypatch.setattr(vp, name, touched)
    req = vp._requests({}, config=True)
    assert req == (False, None, None, None, None, False, None)
    ref, dist, bgr, planes = object(), object(), object(), object()
    for extra in (None, {"DIST_RES": "16x16", "SCALE": "bicubic"}):
        streams, out, plan, at, ran = vp._prepass_chain(req, ref, dist, (bgr,), PC.LAYOUT, PC.H, PC.W, (16, 16), planes, {}, None,
                                                        extra=extra)
        assert [id(a) for a in streams] == [id(ref), id(dist), id(bgr)] and out is extra and plan is None and at is planes
        assert ran is False


@pytest.mark.parametrize("counts,kw", CASES, ids=[PC.case_name(counts, kw) for counts, kw in CASES])
def test_both_entry_points_run_the_chain_of_the_parent(counts, kw, tmp_path, monkeypatch):
    got = {entry: PC.trace(entry, kw, tmp_path, monkeypatch.setattr, counts) for entry in PC.ENTRY_POINTS}
    rfm, row = got["run_ffmpeg_metrics"], got["process_video_and_extract_metrics"]
    refused = PC.refusal(kw)
    if refused is not None:   # the request parser's refusals, with the parent's messages and before any call
        assert rfm == row == {"calls": [], "error": refused, "log": None}
    # (a) the call trace, the log and the error of the parent commit
    assert got == GOLDEN[PC.case_name(counts, kw)]
    if refused is not None:
        return
    assert row["error"] is None
    # (b) the keys after "frames" and "pooled_metrics" - and with them the row's last columns, prepass_chain_cases.trace - are
    # the table's order filtered by what is on; (c) nothing on: no extra keys, so no log
    want = PC.keys_of(kw)
    assert [k for k, _v in row["log"] or ()] == want and (row["log"] is None) == (not want)
    # (d) both entry points hand the same frames to every stand-in, in the same order.  run_ffmpeg_metrics alone checks that
    # the two streams are equally long, right after sync's trim: there its chain ends, a prefix of the other's
    calls = [[(c["call"], c["frames"][:2] if c["call"] != "stream.run" else [c["frames"][-1] or c["frames"][0], c["frames"][1]],
               {k: v for k, v in c["args"].items() if k not in ("complexity",)}) for c in t["calls"]] for t in (rfm, row)]
    if rfm["error"] is None:
        assert calls[0] == calls[1] and rfm["log"] == row["log"]
    else:
        assert rfm["error"] == "ref and dist must have the same shape" and counts[0] != counts[1] and not kw.get("sync_apply")
        assert calls[0] == calls[1][:len(calls[0])] and [c[0] for c in calls[0]] == ["frame_sync"] * bool(kw.get("sync"))
        assert rfm["log"] is None
