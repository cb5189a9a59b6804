"""Interlace and 3:2 pulldown detection from the field statistics of ONE stream (Engine.fields, vqa_fields_metrics), and the
frame-index plans that Engine.weave applies.  Pure host: integers and exact fractions, no float takes part in a decision.

The frame rule is FFmpeg idet's single-frame rule with its default thresholds (intl_thres 1.04 = 26/25, prog_thres 1.5 = 3/2) AS
RECALLED: it is NOT pinned against FFmpeg, no binary being at hand.  idet forms, at frame t, alpha0 and alpha1 from the frame
before and the frame after; here fwd of frame t and bwd of frame t + 1 are those terms (include/vqa.h), so the rule needs the
records of two neighbouring frames and nothing else.  idet's multi-frame history verdict is not built.

Field names: "top" is the field of the even rows (y & 1 == 0), "bottom" of the odd rows.  "tff": the top field is the earlier
one of a frame.
"""
from fractions import Fraction

TYPES = ("tff", "bff", "progressive", "undetermined")
REPEATS = ("both", "top", "bottom", "none")
INTL_THRES = Fraction(26, 25)   # idet's intl_thres 1.04
PROG_THRES = Fraction(3, 2)     # idet's prog_thres 1.5
REPEAT_RATIO = 3                # a field repeats when the other field's SAD is more than this many times its own
PERIOD = 5
# the repeats of one period of 2:3 pulldown, tff, against the frame before: (A,A) (B,B) (B,C) (C,D) (D,D)
PATTERN = ("none", "none", "top", "none", "bottom")
MIN_PERIODS = 2                 # whole periods a cadence must explain
FRAMES_PER_BREAK = 5 * PERIOD   # at most one break per five periods
# (top, bottom) film frame of the five output frames of a period, tff
PULLDOWN = ((0, 0), (1, 1), (1, 2), (2, 3), (3, 3))


def _word(rec, name, f=None):
    v = rec[name]
    return int(v if f is None else v[f])


def frame_type(a0, a1, d):
    """idet's single-frame rule on the integers a0, a1 (the temporal terms of the two field orders) and d (the frame's comb)"""
    if a0 > INTL_THRES * a1:
        return "tff"
    if a1 > INTL_THRES * a0:
        return "bff"
    if a1 > PROG_THRES * d:
        return "progressive"
    return "undetermined"


def frame_repeat(rec):
    """which field of a frame repeats the frame before: "both" | "top" | "bottom" | "none"; None without a predecessor"""
    if not _word(rec, "has_prev"):
        return None
    s0, s1 = _word(rec, "sad", 0), _word(rec, "sad", 1)
    if _word(rec, "changed", 0) == 0 and _word(rec, "changed", 1) == 0:
        return "both"
    if REPEAT_RATIO * s0 < s1:
        return "top"
    if REPEAT_RATIO * s1 < s0:
        return "bottom"
    return "none"


def expected_repeat(t, phase, order="tff"):
    """what frame t of a 3:2 stream of that phase and field order repeats"""
    r = PATTERN[(t + phase) % PERIOD]
    if order == "bff" and r != "none":
        r = "bottom" if r == "top" else "top"
    return r


def _walk(repeat, phase, order):
    """the indices at which the repeat sequence contradicts the cadence, walked from `phase`: at a contradiction the phase is
    taken again from the five frames that start there (the phase that explains most of them, the current one on a tie), so a cut
    costs one break and not one per later frame.  Frames without a predecessor contradict nothing."""
    breaks, p, n = [], phase, len(repeat)
    for t in range(n):
        if repeat[t] is None or repeat[t] == expected_repeat(t, p, order):
            continue
        breaks.append(t)
        best, best_hits = p, -1
        for k in range(PERIOD):
            q = (p + k) % PERIOD
            hits = sum(1 for u in range(t, min(n, t + PERIOD)) if repeat[u] is None or repeat[u] == expected_repeat(u, q, order))
            if hits > best_hits:
                best, best_hits = q, hits
        p = best
    return breaks


def find_cadence(repeat):
    """the repeat sequence -> {"cadence": "3:2", "phase", "order", "breaks"} when ONE of the ten (phase, order) hypotheses explains
    it over at least two whole periods with fewer breaks than every other and at most one break per five periods; else
    {"cadence": "none", "phase": None, "order": None, "breaks": []}"""
    none = {"cadence": "none", "phase": None, "order": None, "breaks": []}
    seen = sum(1 for r in repeat if r is not None)
    if seen < MIN_PERIODS * PERIOD or not any(r in ("top", "bottom") for r in repeat):
        return none
    tried = sorted(((len(b), order, phase, b) for order in ("tff", "bff") for phase in range(PERIOD)
                    for b in (_walk(repeat, phase, order),)), key=lambda x: x[0])
    (n0, order, phase, breaks), n1 = tried[0], tried[1][0]
    if n0 == n1 or n0 * FRAMES_PER_BREAK > seen:
        return none
    return {"cadence": "3:2", "phase": phase, "order": order, "breaks": breaks}


def analyse(records):
    """[n] records of Engine.fields (N.FIELDS_DTYPE; any sequence of mappings with those words) ->
    {"type": per frame, "counts": {type: frames}, "clip_type", "repeat": per frame, "cadence", "phase", "order", "breaks",
    "static"}.
    type[t]: frame_type(a0, a1, d) with a0 = fwd_t[0] + bwd_{t+1}[1], a1 = fwd_t[1] + bwd_{t+1}[0], d = comb_t[0] + comb_t[1]; a
    term whose frame is missing (fwd of a frame without a predecessor, bwd beyond the last frame) is 0.  clip_type: the type of a
    strict majority of the determined frames, "undetermined" without one.  A static clip - every frame with a predecessor
    repeats both fields - is reported as static True, clip_type "undetermined", cadence "none": never guessed."""
    n = len(records)
    types, repeat = [], []
    for t in range(n):
        r = records[t]
        nxt = records[t + 1] if t + 1 < n and _word(records[t + 1], "has_prev") else None
        has = _word(r, "has_prev")
        a0 = (_word(r, "fwd", 0) if has else 0) + (_word(nxt, "bwd", 1) if nxt is not None else 0)
        a1 = (_word(r, "fwd", 1) if has else 0) + (_word(nxt, "bwd", 0) if nxt is not None else 0)
        types.append(frame_type(a0, a1, _word(r, "comb", 0) + _word(r, "comb", 1)))
        repeat.append(frame_repeat(r))
    counts = {k: types.count(k) for k in TYPES}
    seen = [r for r in repeat if r is not None]
    static = bool(seen) and all(r == "both" for r in seen)
    determined = n - counts["undetermined"]
    clip_type = next((k for k in TYPES[:3] if 2 * counts[k] > determined), "undetermined")
    found = find_cadence(repeat)
    if static:
        clip_type, found = "undetermined", find_cadence([])
    return dict(found, type=types, counts=counts, clip_type=clip_type, repeat=repeat, static=static)


def telecine_plan(n_film, phase=0, order="tff"):
    """2:3 pulldown of n_film film frames -> (top_index, bottom_index) for Engine.weave: one period of five output frames is,
    written (top, bottom), (A, A) (B, B) (B, C) (C, D) (D, D) under tff and with the fields exchanged under bff.  Only output
    frames whose two film frames exist are planned; the first `phase` of them are left out, so the stream starts at that phase."""
    _check_plan_args(phase, order)
    top, bottom, k = [], [], 0
    while True:
        q, (a, b) = divmod(k, PERIOD)[0], PULLDOWN[k % PERIOD]
        a, b = 4 * q + a, 4 * q + b
        if max(a, b) >= int(n_film):
            break
        top.append(a if order == "tff" else b)
        bottom.append(b if order == "tff" else a)
        k += 1
    return top[phase:], bottom[phase:]


def ivtc_plan(analysis, n):
    """analyse's answer for a stream of n frames with a found cadence -> (top_index, bottom_index) that weave the film frames
    back: four per period, each film frame's two fields taken from the stream's frames that hold them (A and B from their own
    frames, C from the two mixed frames, D from the last).  Film frames whose fields lie outside 0 .. n - 1 are left out.  The
    plan follows the phase found at the start of the stream: a stream with breaks is planned piece by piece by the caller.
    A ValueError when the cadence is "none"."""
    if analysis.get("cadence") != "3:2":
        raise ValueError("no 3:2 cadence was found: there is nothing to invert")
    phase, order, n = int(analysis["phase"]), analysis["order"], int(n)
    _check_plan_args(phase, order)
    # film frame -> (the period's frame that holds its first field, its second field), first = top under tff
    holds = ((0, 0), (1, 1), (3, 2), (4, 4))
    top, bottom = [], []
    for base in range(-phase, n, PERIOD):
        for first, second in holds:
            a, b = base + first, base + second
            if 0 <= a < n and 0 <= b < n:
                top.append(a if order == "tff" else b)
                bottom.append(b if order == "tff" else a)
    return top, bottom


def field_plan(n, order="tff"):
    """n frames at twice the rate -> (top_index, bottom_index) of the n // 2 interlaced frames that take their earlier field from
    frame 2 j and their later field from frame 2 j + 1; the earlier field is the top one under "tff\""""
    _check_plan_args(0, order)
    early, late = list(range(0, 2 * (int(n) // 2), 2)), list(range(1, 2 * (int(n) // 2), 2))
    return (early, late) if order == "tff" else (late, early)


def _check_plan_args(phase, order):
    if order not in ("tff", "bff"):
        raise ValueError("order must be 'tff' or 'bff' (got %r)" % (order,))
    if isinstance(phase, bool) or not isinstance(phase, int) or not 0 <= phase < PERIOD:
        raise ValueError("phase must be 0 .. 4 (got %r)" % (phase,))


FIELDS_KEYS = ("FIELDS_REF_TYPE", "FIELDS_REF_COMBED", "FIELDS_REF_CADENCE", "FIELDS_REF_REPEATS",
               "FIELDS_DIST_TYPE", "FIELDS_DIST_COMBED", "FIELDS_DIST_CADENCE", "FIELDS_DIST_REPEATS", "FIELDS_MATCH")


def summary_keys(ref, dist):
    """the two streams' analyses -> the nine top-level keys of the log and the row (FIELDS_KEYS, in that order).  COMBED: the
    frames classed tff or bff; REPEATS: the frames that repeat a field or both; MATCH: 1 when type, cadence and phase agree"""
    out = {}
    for side, a in (("REF", ref), ("DIST", dist)):
        out["FIELDS_%s_TYPE" % side] = a["clip_type"]
        out["FIELDS_%s_COMBED" % side] = a["counts"]["tff"] + a["counts"]["bff"]
        out["FIELDS_%s_CADENCE" % side] = a["cadence"]
        out["FIELDS_%s_REPEATS" % side] = sum(1 for r in a["repeat"] if r in ("both", "top", "bottom"))
    out["FIELDS_MATCH"] = int(all(ref[k] == dist[k] for k in ("clip_type", "cadence", "phase")))
    return out
