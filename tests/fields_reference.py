"""A NumPy restatement of include/vqa.h's fields definition and of the weave, written from the text (not from the kernel):
Python integers of arbitrary size under the sums, so nothing here can overflow.

    record(c, p)       the words of one frame against its predecessor (None: it has none)
    records(clip, prev0)   the same over a clip [n, h, w]
    weave(frames, top, bottom)   out[j][y] = frames[(bottom if y & 1 else top)[j]][y] over the leading row axis
"""
import numpy as np

WORDS = ("comb", "fwd", "bwd", "sad", "changed")


def _second_difference(outer, inner):
    """|outer[y-1][x] + outer[y+1][x] - 2 inner[y][x]| for 2 <= y < h - 2 -> int64 [h - 4, w]; row k of it is y = k + 2"""
    o, i = outer.astype(np.int64), inner.astype(np.int64)
    h = o.shape[0]
    return np.abs(o[1:h - 3] + o[3:h - 1] - 2 * i[2:h - 2])


def record(c, p=None):
    """c, p: [h, w] integer planes -> {"comb": [2], "fwd": [2], "bwd": [2], "sad": [2], "changed": [2], "count", "has_prev"}"""
    c = np.asarray(c)
    h, w = c.shape
    out = {k: [0, 0] for k in WORDS}
    out["count"], out["has_prev"] = (h - 4) * w, 0 if p is None else 1
    comb = _second_difference(c, c)
    for f in (0, 1):
        # y = k + 2 has the parity of k
        out["comb"][f] = int(comb[f::2].sum())
    if p is not None:
        p = np.asarray(p)
        fwd, bwd = _second_difference(c, p), _second_difference(p, c)
        diff = c.astype(np.int64) - p.astype(np.int64)
        for f in (0, 1):
            out["fwd"][f] = int(fwd[f::2].sum())
            out["bwd"][f] = int(bwd[f::2].sum())
            out["sad"][f] = int(np.abs(diff[f::2]).sum())
            out["changed"][f] = int((diff[f::2] != 0).sum())
    return out


def records(clip, prev0=None):
    clip = np.asarray(clip)
    return [record(clip[i], clip[i - 1] if i else prev0) for i in range(clip.shape[0])]


def same(got, want):
    """a record of the engine (a NumPy record of N.FIELDS_DTYPE) against one of record(): every word"""
    return all([int(v) for v in np.atleast_1d(got[k])] == [int(v) for v in np.atleast_1d(want[k])]
               for k in WORDS + ("count", "has_prev"))


def weave(frames, top, bottom):
    """frames [n, h, ...] -> [len(top), h, ...]: even rows from frames[top[j]], odd rows from frames[bottom[j]]"""
    frames = np.asarray(frames)
    out = frames[np.asarray(top, np.int64)].copy()
    out[:, 1::2] = frames[np.asarray(bottom, np.int64)][:, 1::2]
    return out
