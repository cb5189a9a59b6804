"""NumPy restatement of the no-reference artefact measures, written from the definition in include/vqa.h (vqa_artifacts_submit),
not from the kernel: the 21 integer words of a plane as Python ints, and the host figures formed from them in double in the
header's order of operations.  It also holds the blur in its UNTELESCOPED form - a 9-tap mean kept as exact ninths (the window
sum, an integer), then neighbour differences - which is how the telescoping dB9(i, j) = |x(i + 4, j) - x(i - 5, j)| is proved
and not assumed (tests/test_artifacts_host.py)."""
import numpy as np

SQRT_HALF_PI = 1.2533141373155003   # the double nearest sqrt(pi / 2), as the header writes it
WORDS = ("edge_h", "edge_v", "blur_f_h", "blur_v_h", "blur_f_v", "blur_v_v", "lap")
DOUBLES = ("blockiness", "blockiness_max", "blur_h", "blur_v", "blur", "noise")


def counts(n):
    """cnt[p] per line of n samples: the boundaries c = 1 .. n - 1 with c mod 8 == p, by enumeration"""
    out = [0] * 8
    for c in range(1, n):
        out[c % 8] += 1
    return out


def _edges(x):
    """edge[p] over the boundaries between columns of x [H, W]"""
    d = np.abs(x[:, 1:] - x[:, :-1])                    # boundary c = 1 .. W - 1 at index c - 1
    return [int(d[:, [c - 1 for c in range(1, x.shape[1]) if c % 8 == p]].sum()) for p in range(8)]


def _blur_cols(x):
    """(blur_f, blur_v) of the direction that differences along axis 1 (the horizontal one), telescoped"""
    w = x.shape[1]
    j = np.arange(5, w - 4)                             # j = 5 .. W - 5
    df = np.abs(x[:, j] - x[:, j - 1])
    db9 = np.abs(x[:, j + 4] - x[:, j - 5])
    return int(df.sum()), int(np.maximum(0, 9 * df - db9).sum())


def _blur_cols_untelescoped(x):
    """the same from the blurred plane itself: B9(i, j) = sum of the 9 samples j - 4 .. j + 4 (nine times the 9-tap mean, an
    exact integer), defined where the window lies inside; nine times the blurred plane's neighbour difference is
    |B9(i, j) - B9(i, j - 1)|, which needs both windows: j = 5 .. W - 5"""
    w = x.shape[1]
    b9 = {j: sum(x[:, j + k] for k in range(-4, 5)) for j in range(4, w - 4)}
    f = v = 0
    for j in range(5, w - 4):
        df = np.abs(x[:, j] - x[:, j - 1])
        db9 = np.abs(b9[j] - b9[j - 1])
        f += int(df.sum())
        v += int(np.maximum(0, 9 * df - db9).sum())
    return f, v


def laplacian_sum(x):
    c = x[1:-1, 1:-1]
    l = (x[:-2, :-2] - 2 * x[:-2, 1:-1] + x[:-2, 2:] - 2 * x[1:-1, :-2] + 4 * c - 2 * x[1:-1, 2:]
         + x[2:, :-2] - 2 * x[2:, 1:-1] + x[2:, 2:])
    return int(np.abs(l).sum())


def words(plane, untelescoped=False):
    """the 21 integer words of one plane [H, W] of integer samples -> dict of Python ints (edge_*: lists of 8)"""
    x = np.asarray(plane).astype(np.int64)
    blur = _blur_cols_untelescoped if untelescoped else _blur_cols
    fh, vh = blur(x)
    fv, vv = blur(np.ascontiguousarray(x.T))
    return dict(edge_h=_edges(x), edge_v=_edges(np.ascontiguousarray(x.T)), blur_f_h=fh, blur_v_h=vh, blur_f_v=fv, blur_v_v=vv,
                lap=laplacian_sum(x))


def _ratios(edge, n, lines):
    cnt = [c * lines for c in counts(n)]
    se, sc = sum(edge), sum(cnt)
    r = []
    for p in range(8):
        m_b = float(edge[p]) / float(cnt[p])
        m_o = float(se - edge[p]) / float(sc - cnt[p])
        den = m_b + m_o
        r.append(0.0 if den == 0.0 else (m_b - m_o) / den)
    return r


def _argmax_low(r):
    best = 0
    for p in range(1, 8):
        if r[p] > r[best]:
            best = p
    return best


def figures(wd, h, w, depth):
    """the host's part: phases and doubles from the words, every operation one IEEE double operation in the header's order"""
    rh, rv = _ratios(wd["edge_h"], w, h), _ratios(wd["edge_v"], h, w)
    ph, pv = _argmax_low(rh), _argmax_low(rv)
    out = dict(phase_h=ph, phase_v=pv, blockiness=(rh[0] + rv[0]) / 2.0, blockiness_max=(rh[ph] + rv[pv]) / 2.0, r_h=rh, r_v=rv)
    for d in ("h", "v"):
        f9 = 9.0 * float(wd["blur_f_" + d])
        out["blur_" + d] = 0.0 if wd["blur_f_" + d] == 0 else (f9 - float(wd["blur_v_" + d])) / f9
    out["blur"] = max(out["blur_h"], out["blur_v"])
    s = float(1 << (depth - 8))
    out["noise"] = (SQRT_HALF_PI * float(wd["lap"])) / ((6.0 * float((w - 2) * (h - 2))) * s)
    return out


def measure(plane, depth):
    """words and figures of one plane -> one dict"""
    x = np.asarray(plane)
    wd = words(x)
    wd.update(figures(wd, x.shape[0], x.shape[1], depth))
    return wd


def record_words(rec):
    """the words of an engine record (ARTIFACTS_DTYPE scalar) as the dict `words` gives"""
    out = {k: int(rec[k]) for k in WORDS[2:]}
    out["edge_h"] = [int(v) for v in rec["edge_h"]]
    out["edge_v"] = [int(v) for v in rec["edge_v"]]
    return out


def ulps(a, b):
    """the distance of two doubles in units of the spacing at the larger one"""
    if a == b:
        return 0.0
    return abs(a - b) / np.spacing(max(abs(a), abs(b)))
