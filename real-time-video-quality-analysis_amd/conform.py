"""Conform: what align, sync, shift and colorfit FOUND, turned into the arguments of Engine.conform_submit (include/vqa.h,
vqa_conform_submit) for both streams of a pair.  Pure host code: Python integers and fractions.Fraction, no GPU and no NumPy
needed to plan.

Geometry.  A shift (dy, dx) in shift.py's sense - distorted (y, x) shows reference (y + dy, x + dx) - leaves a common luma
window of h - |dy| by w - |dx|, rounded DOWN to a multiple of the subsampling on each axis; it sits at (max(0, -dy), max(0, -dx))
in the distorted picture and at (max(0, dy), max(0, dx)) in the reference.  A chroma plane's window is origin >> s and size >> s.
Where dy (or dx) is odd on a subsampled axis one of the two chroma origins is rounded down and the chroma planes stay half a
chroma sample apart: chroma_half reports it, nothing is interpolated.

Time.  A constant offset k (distorted frame j pairs reference frame j + k, sync.py's and align.py's sense) slices both streams as
sync's trim does.  With ref_index (align.analyse's path) the distorted frames keep their order and the reference is gathered;
frames whose partner does not exist are dropped from both.

Colour, applied to the DISTORTED stream only.  Every map is quantised ONCE to 2^-16 fixed point, floor(v 2^16 + 1/2) from exact
Fractions, and applied as vqa_conform_submit states: clip((sum + 2^15) >> 16, 0, peak).  A map whose matrix is diagonal is a
function of the sample alone and is handed over as the table it is, lut[p][c] = clip((M_pp c + b_p + 2^15) >> 16, 0, peak), which
gives the same bytes as the matrix would and takes the copy kernel; any other matrix needs three planes."""
from fractions import Fraction

from . import colorfit as CF

CONFORM_KEYS = ("CONFORM_OFFSET", "CONFORM_DY", "CONFORM_DX", "CONFORM_COLOR", "CONFORM_RES", "CONFORM_FRAMES",
                "CONFORM_CHROMA_HALF")
COLOR_MODES = ("none", "match", "levels", "matrix", "tone")
INVERSE = {"limited_to_full": "full_to_limited", "full_to_limited": "limited_to_full",
           "bt601_to_bt709": "bt709_to_bt601", "bt709_to_bt601": "bt601_to_bt709"}
MAX_COEF, MAX_BIAS = 1 << 20, 1 << 33   # vqa_conform_submit's bounds on the fixed-point matrix
TONE_MAX_DEPTH = 10                     # colorfit's tables have one bin per code up to 10 bits


def fix16(v):
    """floor(v 2^16 + 1/2) of an exact value"""
    return (Fraction(v) * (1 << 17) + 1) // 2


def fixed_matrix(M, b):
    """M [k][k] and b [k] (anything Fraction takes) -> the integer rows [k][k + 1] in 2^-16 fixed point, the offset last; a
    ValueError beyond vqa_conform_submit's bounds"""
    rows = [[int(fix16(v)) for v in row] + [int(fix16(c))] for row, c in zip(M, b)]
    for row in rows:
        if any(abs(v) > MAX_COEF for v in row[:-1]) or abs(row[-1]) > MAX_BIAS:
            raise ValueError("the colour map leaves the fixed-point bounds (|M| <= 16, |b| <= 2^17): %r" % (row,))
    return rows


def is_diagonal(rows):
    return all(v == 0 for k, row in enumerate(rows) for i, v in enumerate(row[:-1]) if i != k)


def diagonal_lut(rows, depth):
    """the tables of a diagonal fixed-point map: lut[p][c] = clip((rows[p][p] c + rows[p][-1] + 2^15) >> 16, 0, peak)"""
    peak = (1 << depth) - 1
    return [[min(max((row[p] * c + row[-1] + (1 << 15)) >> 16, 0), peak) for c in range(peak + 1)] for p, row in enumerate(rows)]


def tone_lut(tables, depth):
    """colorfit's tables [planes][bins][3] (count, sum, sum of squares per code of the stream to correct) -> lut [planes][2^depth].
    A filled bin: floor((2 sum + count) / (2 count)), the mean rounded half up.  Empty bins between two filled ones a < c < b:
    integer linear interpolation rounded half up, floor((2 (l_a (b - c) + l_b (c - a)) + (b - a)) / (2 (b - a))).  Outside the
    filled range: slope 1 from the nearest filled bin.  No filled bin at all: the identity.  Clipped to the peak.  depth <= 10
    only: above, a bin holds several codes."""
    depth = int(depth)
    if depth > TONE_MAX_DEPTH:
        raise ValueError("a tone table is built up to %d bits (got %d): above, colorfit's bins hold several codes" % (TONE_MAX_DEPTH, depth))
    bins, peak = 1 << depth, (1 << depth) - 1
    out = []
    for rows in tables:
        rows = [[int(v) for v in r] for r in rows]
        if len(rows) != bins:
            raise ValueError("a %d-bit table has %d bins (got %d)" % (depth, bins, len(rows)))
        filled = [c for c in range(bins) if rows[c][0] > 0]
        at = {c: (2 * rows[c][1] + rows[c][0]) // (2 * rows[c][0]) for c in filled}
        lut = list(range(bins))
        if filled:
            first, last = filled[0], filled[-1]
            for c in range(first):
                lut[c] = at[first] - (first - c)
            for c in range(last + 1, bins):
                lut[c] = at[last] + (c - last)
            for a, b in zip(filled, filled[1:]):
                for c in range(a + 1, b):
                    lut[c] = (2 * (at[a] * (b - c) + at[b] * (c - a)) + (b - a)) // (2 * (b - a))
            for c in filled:
                lut[c] = at[c]
        out.append([min(max(v, 0), peak) for v in lut])
    return out


def color_map(color, depth, model):
    """color: None | ("match", name) | ("levels", gain[], offset[]) | ("matrix", M, b) | ("tone", tables) ->
    (label, lut or None, matrix or None): lut [planes][2^depth] integers, matrix [3][4] integers"""
    planes = CF._planes_of(model)
    if color is None:
        return "none", None, None
    kind = color[0]
    if kind == "tone":
        lut = tone_lut(color[1], depth)
        if len(lut) != planes:
            raise ValueError("the tone tables must hold the model's %d plane(s)" % planes)
        return "tone", lut, None
    if kind == "match":
        name = color[1]
        if name == "none":
            return "none", None, None
        cat = {n: (M, b) for n, M, b in CF.catalogue(depth, model)}
        if name not in INVERSE or INVERSE[name] not in cat:
            raise ValueError("%r is no mishap of the %r catalogue" % (name, model))
        M, b = cat[INVERSE[name]]
        label = "match:" + name
    elif kind == "levels":
        gain, offset = list(color[1])[:planes], list(color[2])[:planes]
        if len(gain) != planes or len(offset) != planes:
            raise ValueError("levels need a gain and an offset for each of the model's %d plane(s)" % planes)
        M = [[Fraction(gain[i]) if i == j else Fraction(0) for j in range(planes)] for i in range(planes)]
        b, label = offset, "levels"
    elif kind == "matrix":
        M, b, label = [list(r)[:planes] for r in list(color[1])[:planes]], list(color[2])[:planes], "matrix"
        if len(M) != planes or any(len(r) != planes for r in M) or len(b) != planes:
            raise ValueError("a matrix fit needs M [%d][%d] and b [%d]" % (planes, planes, planes))
    else:
        raise ValueError("color must be None or start with one of 'match', 'levels', 'matrix', 'tone' (got %r)" % (kind,))
    rows = fixed_matrix(M, b)
    if is_diagonal(rows):
        return label, diagonal_lut(rows, depth), None
    if planes != 3:
        raise ValueError("a full matrix needs three planes")
    return label, None, rows


def geometry(planes_fn, h, w, shift=(0, 0)):
    """-> dict(out_h, out_w, ref_origin [(y0, x0) per plane], dist_origin, chroma_half, sub [(sy, sx) per plane]).
    planes_fn(h, w): the plane tuples (width, height, ...) of a frame whose luma is h x w."""
    dy, dx = int(shift[0]), int(shift[1])
    full = planes_fn(h, w)
    sub = []
    for p in full:
        pw, ph = int(p[0]), int(p[1])
        if ph not in (h, (h + 1) // 2) or pw not in (w, (w + 1) // 2):
            raise ValueError("plane %dx%d is neither the luma's size nor its half" % (pw, ph))
        sub.append((int(ph != h), int(pw != w)))
    my, mx = 1 << max(s[0] for s in sub), 1 << max(s[1] for s in sub)
    oh, ow = (h - abs(dy)) // my * my, (w - abs(dx)) // mx * mx
    if oh <= 0 or ow <= 0:
        raise ValueError("the shift (%d, %d) leaves no common window of a %dx%d picture" % (dy, dx, w, h))
    dist0, ref0 = (max(0, -dy), max(0, -dx)), (max(0, dy), max(0, dx))
    return {"out_h": oh, "out_w": ow, "sub": sub,
            "ref_origin": [(ref0[0] >> sy, ref0[1] >> sx) for sy, sx in sub],
            "dist_origin": [(dist0[0] >> sy, dist0[1] >> sx) for sy, sx in sub],
            "chroma_half": int(any((sy and dy % 2) or (sx and dx % 2) for sy, sx in sub))}


def timing(n_ref, n_dist, offset=0, ref_index=None):
    """-> (ref frames, dist frames): equally long lists of source frame numbers.  ref_index None: the slices of the constant
    offset (sync's trim); else the distorted frames j whose ref_index[j] exists, in order, and those reference frames."""
    n_ref, n_dist = int(n_ref), int(n_dist)
    if n_ref < 1 or n_dist < 1:
        raise ValueError("n_ref and n_dist must be at least 1")
    if ref_index is None:
        k = int(offset)
        lo_r, lo_d = max(0, k), max(0, -k)
        length = max(0, min(n_dist, n_ref - k) - max(0, -k))
        ref, dist = list(range(lo_r, lo_r + length)), list(range(lo_d, lo_d + length))
    else:
        path = [int(v) for v in ref_index]
        if len(path) != n_dist:
            raise ValueError("ref_index must name a reference frame for each of the %d distorted frames" % n_dist)
        dist = [j for j, i in enumerate(path) if 0 <= i < n_ref]
        ref = [path[j] for j in dist]
    if not ref:
        raise ValueError("no frame of the distorted stream has a partner")
    return ref, dist


def plan(planes_fn, h, w, depth, model, shift=(0, 0), offset=0, ref_index=None, n_ref=None, n_dist=None, color=None):
    """-> dict(ref=..., dist=..., planes, out_planes, summary).  ref and dist are the keyword arguments of
    Engine.conform_submit for the two streams: origin, index (None where it is the identity), lut, matrix (lists of Python
    integers; None on the reference side).  planes / out_planes: planes_fn at the given and at the conformed size.  summary:
    the CONFORM_* keys (CONFORM_KEYS) plus "chroma_half", "frames", "identity" (nothing would change).
    n_ref / n_dist: the streams' frame counts (n_dist defaults to n_ref); None: time is left alone (the pass applies a
    constant offset by its feeds)."""
    depth = int(depth)
    g = geometry(planes_fn, h, w, shift)
    label, lut, matrix = color_map(color, depth, model)
    planes, out_planes = planes_fn(h, w), planes_fn(g["out_h"], g["out_w"])
    if len(planes) != CF._planes_of(model):
        raise ValueError("the %r model has %d planes, planes_fn gives %d" % (model, CF._planes_of(model), len(planes)))
    ref_i = dist_i = None
    frames = None
    if n_ref is not None:
        n_dist = n_ref if n_dist is None else n_dist
        ref_i, dist_i = timing(n_ref, n_dist, offset, ref_index)
        frames = len(ref_i)
        if ref_i == list(range(int(n_ref))):
            ref_i = None
        if dist_i == list(range(int(n_dist))):
            dist_i = None
    elif ref_index is not None:
        raise ValueError("a ref_index path needs n_ref and n_dist")
    summary = {"CONFORM_OFFSET": int(offset), "CONFORM_DY": int(shift[0]), "CONFORM_DX": int(shift[1]), "CONFORM_COLOR": label,
               "CONFORM_RES": "%dx%d" % (g["out_w"], g["out_h"]), "CONFORM_FRAMES": -1 if frames is None else frames,
               "CONFORM_CHROMA_HALF": g["chroma_half"], "chroma_half": g["chroma_half"], "frames": frames,
               "identity": (g["out_h"], g["out_w"]) == (h, w) and lut is None and matrix is None and ref_i is None and dist_i is None}
    return {"ref": {"origin": g["ref_origin"], "index": ref_i, "lut": None, "matrix": None},
            "dist": {"origin": g["dist_origin"], "index": dist_i, "lut": lut, "matrix": matrix},
            "planes": planes, "out_planes": out_planes, "height": h, "width": w, "out_height": g["out_h"], "out_width": g["out_w"],
            "depth": depth, "model": model, "summary": summary}


def log_keys(summary):
    """plan's summary -> the seven top-level keys of the log and the row (CONFORM_KEYS, in that order)"""
    return {k: summary[k] for k in CONFORM_KEYS}
