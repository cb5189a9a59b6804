"""Clip-wide sync read off Engine.sig_cross / video_processing.frame_sync: pure host code over exact integers.

diag is [n_dist + n_ref - 1] (uint64 array or list): diag[k + n_dist - 1] is the sum of the squared signature distances of the
pairs (distorted frame j, reference frame j + k), k = -(n_dist - 1) .. n_ref - 1.  best is [n_dist]: (the smallest distance of
distorted frame j << 32) | the smallest reference index that has it.  Everything here works in Python integers and fractions:
no rounding until log_keys, one division in double per key."""
from fractions import Fraction

SYNC_KEYS = ("SYNC_OFFSET", "SYNC_OVERLAP", "SYNC_DISTANCE", "SYNC_RUNNER_UP", "SYNC_FRAMES_OFF", "SYNC_APPLIED")
CELLS = 256   # the bytes of a signature: SYNC_DISTANCE is per cell


def overlap(k, n_dist, n_ref):
    """The number of j with 0 <= j < n_dist and 0 <= j + k < n_ref: the pairs of diagonal k (0 where there is none)."""
    return max(0, min(n_dist, n_ref - k) - max(0, -k))


def _counts(n_dist, n_ref):
    for name, v in (("n_dist", n_dist), ("n_ref", n_ref)):
        if isinstance(v, bool) or int(v) != v or v < 1:
            raise ValueError("%s must be an integer >= 1" % name)
    return int(n_dist), int(n_ref)


def analyse(diag, best, n_dist, n_ref, min_overlap=None, guard=2):
    """-> dict.  The candidates are the k whose overlap is at least min_overlap (default max(1, (min(n_dist, n_ref) + 1) // 2)).
    offset: the candidate with the smallest diag / overlap, compared exactly; candidates are examined in the order (|k|, k) and
    replaced only on a strict improvement, as align.offset_of does.  mean: that quotient (a Fraction).  overlap: its pairs.
    runner_up: (k, mean) of the best candidate with |k - offset| > guard, in the same order, or None.  ambiguous: the runner-up's
    mean equals the best mean - a static clip, a loop: the offset is then a guess and must not be applied.  per_frame:
    (best[j] & 0xffffffff) - j.  frames_off: the j whose per_frame is not offset.  runs: the run-length list (first, count,
    offset) of per_frame.  trim: (ref_lo, dist_lo, length), the slices that pair the two streams at the offset."""
    n_dist, n_ref = _counts(n_dist, n_ref)
    diag, best = [int(v) for v in diag], [int(v) for v in best]
    if len(diag) != n_dist + n_ref - 1:
        raise ValueError("diag must hold n_dist + n_ref - 1 = %d words (got %d)" % (n_dist + n_ref - 1, len(diag)))
    if len(best) != n_dist:
        raise ValueError("best must hold n_dist = %d words (got %d)" % (n_dist, len(best)))
    if min_overlap is None:
        min_overlap = max(1, (min(n_dist, n_ref) + 1) // 2)
    if isinstance(min_overlap, bool) or int(min_overlap) != min_overlap or min_overlap < 1:
        raise ValueError("min_overlap must be null or an integer >= 1")
    if isinstance(guard, bool) or int(guard) != guard or guard < 0:
        raise ValueError("guard must be an integer >= 0")
    cands = [k for k in sorted(range(-(n_dist - 1), n_ref), key=lambda k: (abs(k), k)) if overlap(k, n_dist, n_ref) >= min_overlap]
    if not cands:
        raise ValueError("no offset pairs min_overlap = %d frames of clips of %d and %d frames" % (min_overlap, n_dist, n_ref))

    def mean_of(k):
        return Fraction(diag[k + n_dist - 1], overlap(k, n_dist, n_ref))

    def smallest(ks):
        at, low = None, None
        for k in ks:
            m = mean_of(k)
            if low is None or m < low:
                at, low = k, m
        return at, low

    off, mean = smallest(cands)
    away = [k for k in cands if abs(k - off) > guard]
    runner_up = smallest(away) if away else None
    per_frame = [(b & 0xffffffff) - j for j, b in enumerate(best)]
    runs = []
    for j, k in enumerate(per_frame):
        if runs and runs[-1][2] == k:
            runs[-1] = (runs[-1][0], runs[-1][1] + 1, k)
        else:
            runs.append((j, 1, k))
    return {"offset": off, "mean": mean, "overlap": overlap(off, n_dist, n_ref), "runner_up": runner_up,
            "ambiguous": runner_up is not None and runner_up[1] == mean, "per_frame": per_frame,
            "frames_off": sum(1 for k in per_frame if k != off), "runs": runs,
            "trim": (max(0, off), max(0, -off), overlap(off, n_dist, n_ref))}


def log_keys(result, applied):
    """analyse's dict -> the six top-level keys of the log and the row (SYNC_KEYS, in that order)"""
    up = result["runner_up"]
    return {"SYNC_OFFSET": int(result["offset"]), "SYNC_OVERLAP": int(result["overlap"]),
            "SYNC_DISTANCE": float(result["mean"] / CELLS), "SYNC_RUNNER_UP": float(up[1] / CELLS) if up is not None else -1.0,
            "SYNC_FRAMES_OFF": int(result["frames_off"]), "SYNC_APPLIED": 1 if applied else 0}
