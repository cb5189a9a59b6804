"""The harness of tests/test_prepass_chain_host.py and of oracle/gen_prepass_trace.py: both entry points over every combination
of the six pre-passes, with the six frame_* pre-pass calls and stream.run replaced by stand-ins that record what they were
handed.  No device is touched.

The clips: 12 reference and 10 distorted frames (and, see CLIPS, 10 and 10), 32 x 32 yuv420p (and the distorted stream's BGR rendition for the complexity
half); every sample of frame i holds i, so a stand-in reads the frame numbers off whatever slice it receives.  The stand-ins
answer canned results of the real shapes, made by the real analysis functions on small hand-made inputs: a sync offset of 2, an
align offset of 0, a shift of (-1, 2), a full-range / limited-range mix-up for the colour fit.

A case's trace is a JSON-ready dict: "calls" (every stand-in call in order: its name, the frame numbers of every stream it
received, its other arguments bound to the real function's signature), "error" (the ValueError that ended the run, or null),
"log" (the written feature log's top-level keys and values after "frames" and "pooled_metrics", null when no log was written)
- which process_video_and_extract_metrics' row must repeat as its last columns, or trace() fails."""
import inspect
import itertools
import json
import os
import zlib

import numpy as np

import colorfit_reference as CR
from rtvqa_amd import align, colorfit, conform, engine, light, shift, stream, sync
from rtvqa_amd import video_processing as vp

H, W = 32, 32
# (reference, distorted) frames.  The first pair is the one of unequal lengths: run_ffmpeg_metrics goes on with it only where
# sync's trim was applied - otherwise its equal-shape check ends the run, which the trace records - so the second, of equal
# lengths, takes that entry point through the paths without a trim.
CLIPS = ((12, 10), (10, 10))
LAYOUT = "yuv420p"
SYNC_OFFSET, SHIFT = 2, (-1, 2)
ENTRY_POINTS = ("run_ffmpeg_metrics", "process_video_and_extract_metrics")
PREPASS_KEYS = (("light", light.LIGHT_KEYS), ("sync", sync.SYNC_KEYS), ("colorfit", colorfit.COLORFIT_KEYS),
                ("align", align.ALIGN_KEYS), ("shift", shift.SHIFT_KEYS), ("conform", conform.CONFORM_KEYS))   # the key order
ROW_HEAD = ("Bitrate (kbps)", "Resolution (px)", "Frame Rate (fps)", "CRF", "Advanced Motion Complexity", "DCT Complexity",
            "Histogram Complexity", "Edge Detection Complexity", "ORB Feature Complexity", "Color Histogram Complexity",
            "Temporal DCT Complexity", "Framerate Variation")   # the row of an empty pass, column_order "fixed"
STAND_INS = ("frame_sync", "frame_light", "frame_align", "frame_shift", "frame_colorfit", "frame_conform")
REAL = {name: getattr(vp, name) for name in STAND_INS}   # (read before anything is patched: the signatures to bind to)


def clip(n, samples=H * W * 3 // 2):
    """[n, samples] uint8 planar frames, frame i all i"""
    return np.repeat(np.arange(n, dtype=np.uint8)[:, None], samples, axis=1)


def bgr(n):
    return np.ascontiguousarray(clip(n, H * W * 3).reshape(n, H, W, 3))


def numbers(a):
    """the frame numbers a stream holds, as [first, count] when they are consecutive (None for no stream)"""
    if a is None:
        return None
    a = np.asarray(a)
    got = [int(v) for v in a.reshape(len(a), -1)[:, 0]]
    assert all((f == v).all() for f, v in zip(a.reshape(len(a), -1), got))
    return [got[0], len(got)] if got and got == list(range(got[0], got[0] + len(got))) else got


def requests():
    """every combination of the six requests, as run_ffmpeg_metrics' keywords"""
    for syn, lit, ali, shi, fit, con in itertools.product(("off", "on", "apply"), (False, True), (False, True), (False, True),
                                                          (False, True), (None, "none", "match", "matrix")):
        kw = {}
        if syn != "off":
            kw.update(sync=True, sync_apply=syn == "apply")
        if lit:
            kw["light"] = True
        if ali:
            kw["align"] = 3
        if shi:
            kw["shift"] = 4
        if fit:
            kw["colorfit"] = True
        if con is not None:
            kw.update(conform=True, conform_color=con)
        yield kw


def cases():
    """(frame counts, requests) of every case: all requests over the first pair of CLIPS, those without a trim over the second"""
    for kw in requests():
        for counts in CLIPS:
            if counts == CLIPS[0] or not kw.get("sync_apply"):
                yield counts, kw


def case_name(counts, kw):
    return "%dx%d:%s" % (counts[0], counts[1], name_of(kw))


def name_of(kw):
    return ",".join("%s=%s" % (k, kw[k]) for k in sorted(kw)) or "plain"


def refusal(kw):
    """the message with which the request parser refuses a combination, or None"""
    if kw.get("conform"):
        if not (kw.get("sync") or kw.get("align") or kw.get("shift") or kw.get("colorfit")):
            return "conform needs at least one of sync, align, shift and colorfit: nothing is applied that was not measured."
        if kw["conform_color"] != "none" and not kw.get("colorfit"):
            return ("conform_color '%s' needs colorfit: no colour map is applied that was not fitted (conform_color 'none' applies "
                    "time and place alone)." % kw["conform_color"])
    return None


def keys_of(kw):
    """the pre-pass keys a run with these requests writes, in the table's order"""
    on = {"light": kw.get("light"), "sync": kw.get("sync"), "colorfit": kw.get("colorfit"), "align": kw.get("align"),
          "shift": kw.get("shift"), "conform": kw.get("conform")}
    return [k for name, keys in PREPASS_KEYS if on[name] for k in keys]


# ---- the canned results ----------------------------------------------------------------------------------------------------------
def _sync_result(n_ref, n_dist, min_overlap):
    diag = [1000 * sync.overlap(k, n_dist, n_ref) + 7 * abs(k) for k in range(-(n_dist - 1), n_ref)]
    diag[SYNC_OFFSET + n_dist - 1] = 0
    best = [min(j + SYNC_OFFSET, n_ref - 1) for j in range(n_dist)]
    out = sync.analyse(diag, best, n_dist, n_ref, min_overlap)
    out.update(ref_sig=np.zeros((n_ref, 256), np.uint8), dist_sig=np.zeros((n_dist, 256), np.uint8),
               diag=np.array(diag, np.uint64), best=np.array(best, np.uint64))
    return out


def _align_result(n, radius):
    sse = np.full((n, 2 * radius + 1), 100, np.uint64)
    sse[:, radius] = 0
    return dict(align.analyse(sse), sse=sse)


def _shift_result(n, radius):
    sse = np.full((n, 2 * radius + 1, 2 * radius + 1), 100, np.uint64)
    sse[:, SHIFT[0] + radius, SHIFT[1] + radius] = 0
    return dict(shift.analyse(sse), sse=sse)


def _light_result(n):
    rec = np.zeros(n, engine.LIGHT_DTYPE)
    rec["count"], rec["max_nits"], rec["avg_nits"], rec["y_avg"] = H * W, 100.0 + np.arange(n), 50.0, 40.0
    rec["pct_nits"][:, light.P9998] = 90.0
    rec["out_709"], rec["out_p3"] = 8, 2
    return rec, light.summarise(rec)


def _colorfit_result(n):
    """two 16 x 16 frames whose distorted side went through full -> limited range; the records repeated to n frames"""
    planes = vp.LAYOUTS[LAYOUT][0](16, 16)
    rng = np.random.RandomState(20261021)
    ref = rng.randint(0, 256, (2, 16 * 16 * 3 // 2)).astype(np.uint8)
    dist = ref.astype(np.float64)
    dist[:, :256] = 16.0 + dist[:, :256] * 219.0 / 255.0
    dist[:, 256:] = 128.0 + (dist[:, 256:] - 128.0) * 224.0 / 255.0
    dist = np.rint(dist).astype(np.uint8)
    two = CR.records(ref, dist, planes)
    rec = np.zeros(n, engine.COLORFIT_DTYPE)
    for i in range(n):
        for field in CR.FIELDS:
            rec[i][field] = two[i % 2][field]
    scale = (n + 1) // 2   # the tables of a clip of n such frames, to within the odd one
    tab = (CR.tables(ref, dist, planes, 8) * scale).astype(np.uint64)
    return rec, tab, colorfit.analyse(rec, 8, "yuv", tab.tolist())


def _digest(plan):
    """what of a plan the pass applies, small enough for the golden file"""
    if plan is None:
        return None
    side = lambda s: {"origin": [list(o) for o in s["origin"]], "index": s["index"],
                      "lut": None if s["lut"] is None else zlib.crc32(json.dumps(s["lut"]).encode()),
                      "matrix": s["matrix"]}
    return {"summary": plan["summary"], "out": [plan["out_height"], plan["out_width"]], "ref": side(plan["ref"]),
            "dist": side(plan["dist"])}


class Harness:
    """the stand-ins, installed with `patch(object, name, value)` (monkeypatch.setattr, or setattr itself)"""

    def __init__(self, patch):
        self.calls = []
        for name in STAND_INS:
            patch(vp, name, getattr(self, name))
        patch(stream, "run", self.run)

    def _note(self, name, streams, args, kwargs):
        sig = inspect.signature(REAL[name])
        bound = sig.bind(*args, **kwargs)
        bound.apply_defaults()
        assert bound.arguments["engine"] is None
        rest = {k: v for k, v in list(bound.arguments.items())[streams:] if v != sig.parameters[k].default}   # (absent: the default)
        self.calls.append({"call": name, "frames": [numbers(a) for a in args[:streams]], "args": rest})
        return bound.arguments

    def frame_sync(self, *a, **kw):
        arg = self._note("frame_sync", 2, a, kw)
        return _sync_result(len(a[0]), len(a[1]), arg["min_overlap"])

    def frame_light(self, *a, **kw):
        self._note("frame_light", 1, a, kw)
        return _light_result(len(a[0]))

    def frame_align(self, *a, **kw):
        arg = self._note("frame_align", 2, a, kw)
        return _align_result(len(a[1]), arg["radius"])

    def frame_shift(self, *a, **kw):
        arg = self._note("frame_shift", 2, a, kw)
        return _shift_result(len(a[1]), arg["radius"])

    def frame_colorfit(self, *a, **kw):
        self._note("frame_colorfit", 2, a, kw)
        return _colorfit_result(len(a[1]))

    def frame_conform(self, *a, **kw):
        """both streams cut to the conformed frame's samples: a frame still holds its number"""
        arg = self._note("frame_conform", 2, a, kw)
        plan = conform.plan(vp.LAYOUTS[arg["layout"]][0], arg["height"], arg["width"], 8, "yuv", shift=arg["shift"],
                            offset=arg["offset"], n_ref=len(a[0]), n_dist=len(a[1]))
        samples = sum(int(p[0]) * int(p[1]) for p in plan["out_planes"])
        ref_i = range(len(a[0])) if plan["ref"]["index"] is None else plan["ref"]["index"]
        dist_i = range(len(a[1])) if plan["dist"]["index"] is None else plan["dist"]["index"]
        return (np.ascontiguousarray(np.asarray(a[0])[list(ref_i), :samples]),
                np.ascontiguousarray(np.asarray(a[1])[list(dist_i), :samples]), plan["summary"])

    def run(self, dist, ref=None, quality=None, complexity=None, batch_size=100, engine=None, on_quality=None, qdist=None,
            device=None):
        """an empty pass: no chunk, no record, empty complexity series"""
        assert engine is None and device is None and quality.dist_planes is None
        self.calls.append({"call": "stream.run", "frames": [numbers(dist), numbers(ref), numbers(qdist)],
                           "args": {"planes": [[int(v) for v in p] for p in quality.planes], "plan": _digest(quality.conform),
                                    "batch_size": batch_size, "complexity": complexity is not None, "writer_sizes": [list(s) for s in on_quality.sizes]}})
        p = len(quality.planes)
        series = {k: [] for k in ("motion", "dct", "temporal", "hist", "edge", "orb", "color")}
        return (np.zeros((0, p), np.uint64), np.zeros((0, p), np.float64)), (series if complexity is not None else None)


def trace(entry, kw, tmp, patch, counts=CLIPS[0]):
    """one entry point over one set of requests and clips of counts = (reference, distorted) frames -> the case's trace (the
    module's docstring)"""
    h = Harness(patch)
    logs = [os.path.join(str(tmp), "%s.log" % k) for k in ("psnr", "ssim", "vmaf")]
    for path in logs:
        if os.path.exists(path):
            os.remove(path)
    ref, dist = clip(counts[0]), clip(counts[1])
    out = {"calls": h.calls, "error": None, "log": None}
    try:
        if entry == "run_ffmpeg_metrics":
            assert vp.run_ffmpeg_metrics(ref, dist, *logs, layout=LAYOUT, height=H, width=W, batch_size=4, **kw) is None
            if os.path.exists(logs[2]):
                out["log"] = _top(json.load(open(logs[2])))
        else:
            seen = []
            real = vp.write_vif_log

            def spy(path, *a, **k):   # (the entry point removes its log: read it as it is written)
                real(path, *a, **k)
                seen.append(_top(json.load(open(path))))

            patch(vp, "write_vif_log", spy)
            try:
                cfg = dict({"crf": 23, "resize_width": 16, "resize_height": 16, "frame_interval": 1, "batch_size": 4, "pixfmt": LAYOUT,
                            "height": H, "width": W}, **kw)
                row = vp.process_video_and_extract_metrics(ref, dist, cfg, csv_file=os.path.join(str(tmp), "row.csv"),
                                                           column_order="fixed", encoded_bgr=bgr(counts[1]))
            finally:
                patch(vp, "write_vif_log", real)
            assert len(seen) <= 1
            out["log"] = seen[0] if seen else None
            # the row: its own columns, then the log's further keys in the log's order, read back from it
            assert list(row) == list(ROW_HEAD) + [k for k, _v in out["log"] or ()], list(row)
            assert all(row[k] == v for k, v in out["log"] or ())
    except ValueError as e:
        out["error"] = str(e)
    return json.loads(json.dumps(out))   # (tuples as lists, as the golden file holds them)


def _top(doc):
    keys = list(doc)
    assert keys[:2] == ["frames", "pooled_metrics"]
    return [[k, doc[k]] for k in keys[2:]]


# ---- the golden file: every distinct thing once ----------------------------------------------------------------------------------
# The 640 traces repeat a few dozen distinct calls and log values.  The file holds each distinct call ("calls"), sequence of
# calls ("chains"), log key with its value ("pairs"), log ("logs") and error ("errors") once, and per case and
# entry point three indices into them, -1 for None: [chain, error, log], cases in the order of cases().
TABLES = ("calls", "chains", "pairs", "logs", "errors")


def pack(traces):
    """[{entry point: trace} per case, in cases()' order] -> the golden file's tables and "cases" """
    doc, seen = {t: [] for t in TABLES}, {t: {} for t in TABLES}

    def index(table, item):
        if item is None:
            return -1
        key = json.dumps(item)
        if key not in seen[table]:
            seen[table][key] = len(doc[table])
            doc[table].append(item)
        return seen[table][key]

    def three(t):
        log = None if t["log"] is None else [index("pairs", p) for p in t["log"]]
        return [index("chains", [index("calls", c) for c in t["calls"]]), index("errors", t["error"]), index("logs", log)]

    doc["cases"] = [[three(case[entry]) for entry in ENTRY_POINTS] for case in traces]
    return doc


def unpack(doc):
    """pack's inverse"""
    def trace_of(chain, error, log):
        return {"calls": [doc["calls"][i] for i in doc["chains"][chain]], "error": None if error < 0 else doc["errors"][error],
                "log": None if log < 0 else [doc["pairs"][i] for i in doc["logs"][log]]}
    return [{entry: trace_of(*three) for entry, three in zip(ENTRY_POINTS, case)} for case in doc["cases"]]


def dump(doc, f):
    """JSON with one call, pair or error per line and eight of the index lists"""
    f.write('{"commit": %s' % json.dumps(doc["commit"]))
    for table in TABLES + ("cases",):
        items = [json.dumps(item, separators=(",", ":")) for item in doc[table]]
        per = 1 if table in ("calls", "pairs", "errors") else 8
        f.write(',\n"%s": [\n%s\n]' % (table, ",\n".join(", ".join(items[i:i + per]) for i in range(0, len(items), per))))
    f.write("}\n")
