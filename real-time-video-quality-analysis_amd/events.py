"""QC events of a clip from its signal statistics (Engine.sigstats / Quality(sigstats=True)): black frames, frozen frames, scene
cuts and the dark-border box.  Pure host code over the records' integer words - no pixels, no device.  Runs are given in frames:
the pass has no timestamps."""
import numpy as np


def _runs(flags, min_run):
    """maximal runs of set flags of at least min_run frames -> [(first, last), ...]"""
    out, start = [], None
    for i, v in enumerate(list(flags) + [False]):
        if v and start is None:
            start = i
        elif not v and start is not None:
            if i - start >= min_run:
                out.append((start, i - 1))
            start = None
    return out


def signal_events(records, planes_depth, black_share=0.98, freeze_noise=0.001, scene_threshold=10.0, min_run=1,
                  first_has_prev=False):
    """records: the sigstats records of a whole clip, [n, p] or [n] (engine.SIGSTATS_DTYPE); plane 0's are used.  planes_depth: d,
    the bit depth of the samples.  With N = count:
      black[i]        below_black >= black_share N                                    (blackframe's share of dark samples)
      frozen[i]       the frame has a predecessor and sad <= freeze_noise N (2^d - 1)   (freezedetect's mean absolute difference)
      mafd[i]         100 sad / (N 2^d); 0 for a frame with no predecessor            (scdet's measure)
      scene_score[i]  min(mafd[i], |mafd[i] - mafd[i-1]|); 0 for frame 0
      cuts            the frames whose score is >= scene_threshold
      black_runs, frozen_runs   maximal runs of at least min_run frames, as (first, last)
      crop            the union box over the frames that are not black - (min top, max bottom, min left, max right) - or None when
                      every frame is black
    first_has_prev: frame 0 was measured against a prev0 (a clip's first frame has no predecessor: False).
    -> dict of the above; black and frozen as bool [n], mafd and scene_score as float64 [n]."""
    rec = np.asarray(records)
    if rec.ndim == 2:
        rec = rec[:, 0]
    d = int(planes_depth)
    n = len(rec)
    count = rec["count"].astype(np.float64)
    sad = rec["sad"].astype(np.float64)
    has_prev = np.ones(n, bool)
    if n and not first_has_prev:
        has_prev[0] = False
    black = rec["below_black"].astype(np.float64) >= black_share * count
    frozen = has_prev & (sad <= freeze_noise * count * float((1 << d) - 1))
    mafd = np.where(has_prev, 100.0 * sad / (count * float(1 << d)), 0.0) if n else np.zeros(0)
    score = np.zeros(n)
    if n > 1:
        score[1:] = np.minimum(mafd[1:], np.abs(mafd[1:] - mafd[:-1]))
    lit = ~black
    crop = None
    if lit.any():
        crop = (int(rec["top"][lit].min()), int(rec["bottom"][lit].max()), int(rec["left"][lit].min()),
                int(rec["right"][lit].max()))
    return dict(black=black, frozen=frozen, mafd=mafd, scene_score=score,
                cuts=[int(i) for i in np.nonzero(score >= scene_threshold)[0]],
                black_runs=_runs(black, min_run), frozen_runs=_runs(frozen, min_run), crop=crop)
