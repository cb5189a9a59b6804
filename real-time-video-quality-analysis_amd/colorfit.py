"""Colour registration read off the records of Engine.colorfit / video_processing.frame_colorfit: pure host code over exact integers.

A record holds, for one frame pair on the luma grid (include/vqa.h, vqa_colorfit_submit), count = n, sum_r[3], sum_d[3], rr[6]
(the pairs 00, 01, 02, 11, 12, 22), rd[3 i + k] = sum r_i d_k, dd[3] and sse[3]; r is the reference, d the distorted stream.  With
A = [[n, sum_r^T], [sum_r, rr]] and c_k = (sum_d[k], rd[., k]), a map d_k ~ b_k + sum_i M[k][i] r_i leaves, with x = (b_k, M[k][.]),

    sse_k(x) = dd[k] - 2 x . c_k + x^T A x

so every candidate map - the least-squares gain and offset per plane, the least-squares 3 x 3 matrix plus offset, and a short
catalogue of known mishaps - is scored without another look at the pictures.  Everything here works in Python integers and
fractions.Fraction; a float appears only where a result is turned into decibels or a curve.  NO CLIPPING IS MODELLED: samples a
mishap pushed against 0 or the peak stay in the residual of every fit.  Nothing is corrected: the fits are reported."""
import math
from fractions import Fraction

COLORFIT_KEYS = ("COLORFIT_MATCH", "COLORFIT_MATCH_PSNR_GAIN", "COLORFIT_PSNR_GAIN", "COLORFIT_GAIN_Y", "COLORFIT_OFFSET_Y",
                 "COLORFIT_TONE_PSNR_GAIN", "COLORFIT_FRAMES_OFF")
PSNR_GAIN_CAP = 100.0   # JSON has no infinity
MODELS = ("yuv", "bgr", "gray")
_PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))   # rr's order
KR_KB = {"bt601": (Fraction(299, 1000), Fraction(114, 1000)), "bt709": (Fraction(2126, 10000), Fraction(722, 10000))}


def db(a, b):
    """10 log10(a / b) of two exact errors: 0.0 if a == 0, inf if b == 0 < a; the fraction is turned into a float last"""
    if a == 0:
        return 0.0
    if b == 0:
        return math.inf
    return 10.0 * math.log10(Fraction(a) / Fraction(b))


def _capped(v):
    return float(min(PSNR_GAIN_CAP, v))


def _planes_of(model):
    if model not in MODELS:
        raise ValueError("model must be one of %s (got %r)" % (", ".join(repr(m) for m in MODELS), model))
    return 1 if model == "gray" else 3


def moments(record):
    """one record (a row of engine.COLORFIT_DTYPE, or a mapping of its fields) -> its words as Python integers:
    {"n", "sr"[3], "sd"[3], "rr"[3][3] (symmetric), "rd"[3][3] ([i][k]), "dd"[3], "sse"[3]}"""
    def ints(name, count):
        v = [int(x) for x in record[name]]
        if len(v) != count:
            raise ValueError("%s must hold %d words" % (name, count))
        return v

    rr6, rd9 = ints("rr", 6), ints("rd", 9)
    rr = [[0] * 3 for _ in range(3)]
    for v, (i, j) in zip(rr6, _PAIRS):
        rr[i][j] = rr[j][i] = v
    return {"n": int(record["count"]), "sr": ints("sum_r", 3), "sd": ints("sum_d", 3), "rr": rr,
            "rd": [rd9[3 * i:3 * i + 3] for i in range(3)], "dd": ints("dd", 3), "sse": ints("sse", 3)}


def add(a, b):
    """the moments of two sets of positions together"""
    return {"n": a["n"] + b["n"], "sr": [x + y for x, y in zip(a["sr"], b["sr"])], "sd": [x + y for x, y in zip(a["sd"], b["sd"])],
            "rr": [[x + y for x, y in zip(p, q)] for p, q in zip(a["rr"], b["rr"])],
            "rd": [[x + y for x, y in zip(p, q)] for p, q in zip(a["rd"], b["rd"])],
            "dd": [x + y for x, y in zip(a["dd"], b["dd"])], "sse": [x + y for x, y in zip(a["sse"], b["sse"])]}


def sse_of(m, k, offset, row):
    """sse_k(x) for the map d_k ~ offset + sum_i row[i] r_i, exactly; row may be shorter than three (the planes the model has)"""
    row = [Fraction(v) for v in row] + [Fraction(0)] * (3 - len(row))
    b = Fraction(offset)
    xc = b * m["sd"][k] + sum(row[i] * m["rd"][i][k] for i in range(3))
    xax = b * b * m["n"] + 2 * b * sum(row[i] * m["sr"][i] for i in range(3)) + \
        sum(row[i] * row[j] * m["rr"][i][j] for i in range(3) for j in range(3))
    return m["dd"][k] - 2 * xc + xax


def levels(m, k):
    """the least-squares gain and offset of plane k by itself -> (gain, offset, sse_affine); a flat reference plane: gain 1"""
    n = m["n"]
    var = n * m["rr"][k][k] - m["sr"][k] ** 2
    cov = n * m["rd"][k][k] - m["sr"][k] * m["sd"][k]
    centred = m["dd"][k] - Fraction(m["sd"][k] ** 2, n)
    if var == 0:
        return Fraction(1), Fraction(m["sd"][k] - m["sr"][k], n), centred
    gain = Fraction(cov, var)
    return gain, (m["sd"][k] - gain * m["sr"][k]) / n, centred - Fraction(cov * cov, n * var)


def matrix(m, planes):
    """the joint least-squares fit d_k ~ b_k + sum_i M[k][i] r_i over the centred moments -> (M [planes][planes], b [planes],
    sse_matrix [planes]).  V m_k = W[., k] by elimination in the order 0, 1, 2 without exchanges: V is positive semidefinite, so
    a pivot is a Schur complement >= 0, and a zero pivot - a flat plane, or one that is an exact affine function of those before
    it - drops that reference plane: its coefficient is 0 in every fit."""
    n = m["n"]
    V = [[Fraction(n * m["rr"][i][j] - m["sr"][i] * m["sr"][j]) for j in range(planes)] for i in range(planes)]
    W = [[Fraction(n * m["rd"][i][k] - m["sr"][i] * m["sd"][k]) for k in range(planes)] for i in range(planes)]
    W0 = [row[:] for row in W]
    live = [True] * planes
    for i in range(planes):
        if V[i][i] == 0:
            live[i] = False
            continue
        for r in range(i + 1, planes):
            f = V[r][i] / V[i][i]
            if f:
                V[r] = [a - f * b for a, b in zip(V[r], V[i])]
                W[r] = [a - f * b for a, b in zip(W[r], W[i])]
    M = [[Fraction(0)] * planes for _ in range(planes)]
    for k in range(planes):
        for i in reversed(range(planes)):
            if live[i]:
                M[k][i] = (W[i][k] - sum(V[i][j] * M[k][j] for j in range(i + 1, planes))) / V[i][i]
    b = [(m["sd"][k] - sum(M[k][i] * m["sr"][i] for i in range(planes))) / n for k in range(planes)]
    sse = [m["dd"][k] - Fraction(m["sd"][k] ** 2, n) - sum(M[k][i] * W0[i][k] for i in range(planes)) / n for k in range(planes)]
    return M, b, sse


def ypbpr_matrix(src, dst):
    """F_dst F_src^-1: Y'PbPr of the `src` system ("bt601" | "bt709") read as R'G'B' and rewritten in the `dst` system, in
    Fractions from Kr and Kb"""
    def forward(kr, kb):
        kg = 1 - kr - kb
        y = [kr, kg, kb]
        return [y, [(c - v) / (2 * (1 - kb)) for c, v in zip((0, 0, 1), y)], [(c - v) / (2 * (1 - kr)) for c, v in zip((1, 0, 0), y)]]

    def inverse(kr, kb):   # R' = Y' + 2 (1 - Kr) Pr, B' = Y' + 2 (1 - Kb) Pb, G' from Y'
        kg = 1 - kr - kb
        r, b = [Fraction(1), Fraction(0), 2 * (1 - kr)], [Fraction(1), 2 * (1 - kb), Fraction(0)]
        g = [(c - kr * x - kb * z) / kg for c, x, z in zip((1, 0, 0), r, b)]
        return [r, g, b]

    F, G = forward(*KR_KB[dst]), inverse(*KR_KB[src])
    return [[sum(F[i][j] * G[j][k] for j in range(3)) for k in range(3)] for i in range(3)]


def catalogue(depth, model):
    """the known mishaps as exact maps in code space, in the order ties go by -> [(name, M [planes][planes], b [planes])], the map
    being d = b + M r.  s = 2^(depth - 8), P = 2^depth - 1.
      limited_to_full   d_Y = (r_Y - 16 s) P / (219 s), d_C = (r_C - 128 s) P / (224 s) + 128 s
      full_to_limited   its inverse
      bt601_to_bt709    ("yuv" only) the codes were read as BT.601 Y'CbCr and rewritten as BT.709: S F709 F601^-1 S^-1 about the
                        centre (16 s, 128 s, 128 s), S = diag(219, 224, 224)
      bt709_to_bt601    ("yuv" only) the reverse
    "bgr" and "gray" take the two range maps with the luma constants on every plane.  No clipping is modelled."""
    planes = _planes_of(model)
    depth = int(depth)
    if not 8 <= depth <= 16:
        raise ValueError("depth must be 8 .. 16")
    s, P = 1 << (depth - 8), (1 << depth) - 1
    chroma = [False, True, True] if model == "yuv" else [False] * planes

    def diagonal(gains, offsets):
        return [[gains[i] if i == j else Fraction(0) for j in range(planes)] for i in range(planes)], offsets

    l2f = diagonal([Fraction(P, 224 * s) if c else Fraction(P, 219 * s) for c in chroma],
                   [128 * s - Fraction(128 * s * P, 224 * s) if c else -Fraction(16 * s * P, 219 * s) for c in chroma])
    f2l = diagonal([Fraction(224 * s, P) if c else Fraction(219 * s, P) for c in chroma],
                   [128 * s - Fraction(128 * s * 224 * s, P) if c else Fraction(16 * s) for c in chroma])
    out = [("limited_to_full",) + l2f, ("full_to_limited",) + f2l]
    if model == "yuv":
        S, centre = (219, 224, 224), (16 * s, 128 * s, 128 * s)
        for name, src, dst in (("bt601_to_bt709", "bt601", "bt709"), ("bt709_to_bt601", "bt709", "bt601")):
            T = ypbpr_matrix(src, dst)
            M = [[T[i][j] * Fraction(S[i], S[j]) for j in range(3)] for i in range(3)]
            out.append((name, M, [centre[i] - sum(M[i][j] * centre[j] for j in range(3)) for i in range(3)]))
    return out


def match(m, cat, planes):
    """the candidate of the catalogue with the smallest total error (ties: catalogue order), NAMED when it at least halves the
    error - 2 sse_candidate <= sse_given and sse_given > 0: a mishap is named when it accounts for at least as much error as
    everything else together; the factor 2 is the rule's definition -> (name or "none", the candidate's total error or None)"""
    given = sum(m["sse"][:planes])
    best = None
    for name, M, b in cat:
        total = sum(sse_of(m, k, b[k], M[k]) for k in range(planes))
        if best is None or total < best[1]:
            best = (name, total)
    if best is not None and given > 0 and 2 * best[1] <= given:
        return best
    return "none", None


def tone(tables, planes):
    """the tables [planes][bins][3] (count, sum_d, sum_dd) -> (curve [planes][bins] of floats, NaN where a bin is empty;
    sse_lut [planes], exact: the error the best per-code curve would leave)"""
    curve, sse = [], []
    for p in range(planes):
        rows = [[int(v) for v in row] for row in tables[p]]
        curve.append([s / c if c else math.nan for c, s, _q in rows])
        sse.append(sum((q - Fraction(s * s, c) for c, s, q in rows if c), Fraction(0)))
    return curve, sse


def analyse(records, depth, model, tables=None):
    """records: the [n] records of a clip (engine.COLORFIT_DTYPE, or mappings of its fields); depth 8 .. 16; model "yuv" | "bgr"
    | "gray"; tables: None or [planes][bins][3] of the same clip.  The records are summed in Python integers.  -> dict:
      sse_given [planes]         the error as given (integers)
      gain, offset, sse_affine   the per-plane least-squares levels fit and what it would leave (Fractions)
      matrix, matrix_offset, sse_matrix   the joint 3 x 3 fit and what it would leave
      match, match_sse           the named mishap of catalogue(depth, model) or "none" (match), and its total error (None)
      per_frame, frames_off      the same rule on each frame's own record; the frames whose match differs from the clip's
      psnr_gain                  dB(sum sse_given, sum sse_matrix); match_psnr_gain likewise for the named candidate (0.0 for "none")
      with tables: curve, sse_lut, lut_psnr_gain [planes] = dB(sse_given, sse_lut) and tone_psnr_gain [planes] =
        dB(sse_affine, sse_lut): what a per-code curve explains beyond gain and offset - a gamma or transfer mismatch shows
        here, a pure levels error does not."""
    planes = _planes_of(model)
    frames = [moments(r) for r in records]
    if not frames:
        raise ValueError("records must hold at least one frame")
    m = frames[0]
    for f in frames[1:]:
        m = add(m, f)
    if m["n"] <= 0:
        raise ValueError("records must count at least one position")
    cat = catalogue(depth, model)
    given = m["sse"][:planes]
    lev = [levels(m, k) for k in range(planes)]
    M, b, sse_matrix = matrix(m, planes)
    name, match_sse = match(m, cat, planes)
    per_frame = [match(f, cat, planes)[0] for f in frames]
    out = {"planes": planes, "count": m["n"], "sse_given": given,
           "gain": [v[0] for v in lev], "offset": [v[1] for v in lev], "sse_affine": [v[2] for v in lev],
           "matrix": M, "matrix_offset": b, "sse_matrix": sse_matrix,
           "match": name, "match_sse": match_sse, "per_frame": per_frame,
           "frames_off": sum(1 for v in per_frame if v != name),
           "psnr_gain": db(sum(given), sum(sse_matrix)),
           "match_psnr_gain": 0.0 if name == "none" else db(sum(given), match_sse)}
    if tables is not None:
        if len(tables) != planes:
            raise ValueError("tables must be [planes][bins][3] of the model's %d plane(s)" % planes)
        out["curve"], out["sse_lut"] = tone(tables, planes)
        out["lut_psnr_gain"] = [db(given[p], out["sse_lut"][p]) for p in range(planes)]
        out["tone_psnr_gain"] = [db(out["sse_affine"][p], out["sse_lut"][p]) for p in range(planes)]
    return out


def log_keys(result, depth):
    """analyse's dict -> the seven top-level keys of the log and the row (COLORFIT_KEYS, in that order); gains are capped at
    100.0, the offset is on the 8-bit scale (offset / 2^(depth - 8)), the tone gain is plane 0's (0.0 without tables)"""
    tone_gain = result["tone_psnr_gain"][0] if "tone_psnr_gain" in result else 0.0
    return {"COLORFIT_MATCH": str(result["match"]), "COLORFIT_MATCH_PSNR_GAIN": _capped(result["match_psnr_gain"]),
            "COLORFIT_PSNR_GAIN": _capped(result["psnr_gain"]), "COLORFIT_GAIN_Y": float(result["gain"][0]),
            "COLORFIT_OFFSET_Y": float(result["offset"][0] / (1 << (int(depth) - 8))),
            "COLORFIT_TONE_PSNR_GAIN": _capped(tone_gain), "COLORFIT_FRAMES_OFF": int(result["frames_off"])}
