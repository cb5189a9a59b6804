"""Temporal alignment read off the band of Engine.align / video_processing.frame_align: pure host code over exact integers.

sse is [n, 2R + 1] (uint64 array or nested lists); column c is k = c - R, sse[j][c] the squared error between encoded frame j
and reference frame j + k, NONE where that reference frame does not exist.  Everything here works in Python integers and
fractions: no rounding until psnr_gain, one formula in double."""
import math
from fractions import Fraction

NONE = (1 << 64) - 1   # VQA_ALIGN_NONE

ALIGN_KEYS = ("ALIGN_RADIUS", "ALIGN_OFFSET", "ALIGN_DROPPED", "ALIGN_REPEATED", "ALIGN_PSNR_GAIN")
PSNR_GAIN_CAP = 100.0


def _rows(sse):
    rows = [[int(v) for v in row] for row in sse]
    if not rows or len(rows[0]) % 2 != 1 or any(len(r) != len(rows[0]) for r in rows):
        raise ValueError("sse must be [n, 2 radius + 1] with n >= 1")
    return rows, len(rows[0]) // 2


def offset_of(sse):
    """The constant offset: the k whose column has the smallest mean over its valid entries, compared exactly.  Columns are
    examined in the order (|k|, k) and replaced only on a strict improvement: a tie goes to the smallest |k|, then to the
    negative one.  0 when no entry is valid."""
    rows, R = _rows(sse)
    best, best_k = None, 0
    for k in sorted(range(-R, R + 1), key=lambda k: (abs(k), k)):
        col = [r[k + R] for r in rows if r[k + R] != NONE]
        if not col:
            continue
        mean = Fraction(sum(col), len(col))
        if best is None or mean < best:
            best, best_k = mean, k
    return best_k


def match_path(sse, offset=0):
    """The monotone assignment: m[j] among the valid columns of row j, minimising sum_j sse[j][m[j]] subject to j + m[j]
    non-decreasing (m[j + 1] >= m[j] - 1), as a forward prefix-minimum recurrence, O(n (2R + 1)).  Among equally good
    predecessors k' of k: k itself, then the nearest to k, then the smaller; among equally good ends: the nearest to `offset`,
    then the smaller.  A row without a valid column takes no part (its m is 0) and the rows around it are constrained as if
    every row between them moved with the reference.  -> the list m"""
    rows, R = _rows(sse)
    n, band = len(rows), 2 * R + 1
    live = [j for j in range(n) if any(v != NONE for v in rows[j])]
    m = [0] * n
    if not live:
        return m
    INF = None
    prev_cost, back, prev_j = None, [], None
    for j in live:
        cost = [v if v != NONE else INF for v in rows[j]]
        if prev_cost is None:
            back.append([None] * band)
        else:
            gap = j - prev_j
            # the prefix minimum of prev_cost over columns <= c, with its rightmost position (the nearest to c from below)
            pm, pa, run, arg = [INF] * band, [None] * band, INF, None
            for c in range(band):
                v = prev_cost[c]
                if v is not INF and (run is INF or v <= run):
                    run, arg = v, c
                pm[c], pa[c] = run, arg
            choice, total = [None] * band, [INF] * band
            for c in range(band):
                if cost[c] is INF:
                    continue
                cands = []   # (value, distance to c, column): the order of preference after the value
                if prev_cost[c] is not INF:
                    cands.append((prev_cost[c], 0, c))
                if c > 0 and pm[c - 1] is not INF:
                    cands.append((pm[c - 1], c - pa[c - 1], pa[c - 1]))
                for a in range(c + 1, min(band, c + gap + 1)):   # (one column in the usual case: gap = 1)
                    if prev_cost[a] is not INF:
                        cands.append((prev_cost[a], a - c, a))
                if cands:
                    v, _d, a = min(cands)
                    total[c], choice[c] = v + cost[c], a
            back.append(choice)
            cost = total
            if all(v is INF for v in cost):   # (no band of real frames does this: a row's last valid column moves down by one)
                raise ValueError("row %d has no valid column a monotone path can reach" % j)
        prev_cost, prev_j = cost, j
    ends = [(v, abs(c - R - offset), c) for c, v in enumerate(prev_cost) if v is not INF]
    c = min(ends)[2]
    for at in range(len(live) - 1, -1, -1):
        m[live[at]] = c - R
        c = back[at][c]
    return m


def psnr_gain(sse_given, sse_aligned):
    """10 log10(sse_given / sse_aligned): what the misalignment costs in PSNR.  0.0 when both are 0, capped at +-100.0"""
    if sse_given == sse_aligned:
        return 0.0
    if sse_aligned == 0:
        return PSNR_GAIN_CAP
    if sse_given == 0:
        return -PSNR_GAIN_CAP
    return max(-PSNR_GAIN_CAP, min(PSNR_GAIN_CAP, 10.0 * math.log10(sse_given / sse_aligned)))


def analyse(sse):
    """-> dict: offset (offset_of), match (match_path from it), ref_index (j + match[j]), dropped (the sum of step - 1 over the
    steps of ref_index above 1), repeated (the number of zero steps), mismatched (frames with match != 0), sse_given (the sum of
    the k = 0 column over the frames where it is valid), sse_aligned (the sum along the path over the same frames), psnr_gain."""
    rows, R = _rows(sse)
    off = offset_of(rows)
    m = match_path(rows, off)
    live = [j for j in range(len(rows)) if any(v != NONE for v in rows[j])]
    ref_index = [j + m[j] for j in range(len(rows))]
    steps = [ref_index[b] - ref_index[a] for a, b in zip(live, live[1:])]
    given = [j for j in live if rows[j][R] != NONE]
    sse_given = sum(rows[j][R] for j in given)
    sse_aligned = sum(rows[j][m[j] + R] for j in given)
    return {"offset": off, "match": m, "ref_index": ref_index,
            "dropped": sum(s - 1 for s in steps if s > 1), "repeated": sum(1 for s in steps if s == 0),
            "mismatched": sum(1 for j in live if m[j] != 0),
            "sse_given": sse_given, "sse_aligned": sse_aligned, "psnr_gain": psnr_gain(sse_given, sse_aligned)}


def log_keys(result, radius):
    """analyse's dict -> the five top-level keys of the log and the row (ALIGN_KEYS, in that order)"""
    return {"ALIGN_RADIUS": int(radius), "ALIGN_OFFSET": int(result["offset"]), "ALIGN_DROPPED": int(result["dropped"]),
            "ALIGN_REPEATED": int(result["repeated"]), "ALIGN_PSNR_GAIN": float(result["psnr_gain"])}
