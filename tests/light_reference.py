"""HDR light levels and gamut QC, restated in NumPy from the definition in include/vqa.h (vqa_light_submit), not from the kernel:
the three planes of a pixel -> R'G'B' (tests/itp_reference.py's decode, which is vqa_itp_submit's) -> ONE rounding to 16-bit codes
-> integers only: table look-ups, the BT.2020 luminance in integer division, the gamut test on int64, counts, and the percentiles
BY SORTING the pixels' m >> 4 (the kernel counts a histogram).

  table_pq()                       T[c] = rint(2^20 EOTF_PQ(c / 65535)) with itp_reference's EOTF
  gamut_double(name) / gamut_int   the linear BT.2020 -> BT.709 / P3-D65 matrix from the chromaticities, and rint(2^16 A)
  codes(planes, ..)                three integer planes -> (cR, cG, cB) uint16-valued int64 [h, w] and the clamped mask
  record(planes, .., T, M709, MP3) one frame -> dict of every field of vqa_light_metrics
  encode_2020(rgb_nits, depth)     display light -> limited-range BT.2020 PQ Y'CbCr code values (the false-positive study)
"""
import numpy as np

import itp_reference as IR

BINS = 4096
PERCENTILES = (100, 500, 1000, 2500, 5000, 7500, 9000, 9500, 9900, 9998)
UNIT = 2.0 ** -20
TABLE_LIMIT = 1 << 34
REL_SHIFT, FLOOR = 6, 1 << 32
D65 = (0.3127, 0.3290)
PRIMARIES = {"bt2020": ((0.708, 0.292), (0.170, 0.797), (0.131, 0.046)),
             "bt709": ((0.64, 0.33), (0.30, 0.60), (0.15, 0.06)),
             "p3": ((0.680, 0.320), (0.265, 0.690), (0.150, 0.060))}
BT2087 = [[1.6605, -0.5876, -0.0728], [-0.1246, 1.1329, -0.0083], [-0.0182, -0.1006, 1.1187]]
P3_4DEC = [[1.3436, -0.2822, -0.0614], [-0.0653, 1.0758, -0.0105], [0.0028, -0.0196, 1.0168]]
INT_709 = [[108822, -38512, -4774], [-8163, 74246, -547], [-1190, -6592, 73317]]
INT_P3 = [[88053, -18493, -4024], [-4279, 70503, -688], [185, -1284, 66635]]


def table_pq():
    c = np.arange(65536, dtype=np.float64) / 65535.0
    return np.rint(IR.pq_eotf(c) * 2.0 ** 20).astype(np.uint64)


def rgb_to_xyz(name):
    """the usual construction: the primaries' XYZ at unit Y as columns, scaled so that R = G = B = 1 gives D65"""
    p = np.array([[x / y, 1.0, (1.0 - x - y) / y] for x, y in PRIMARIES[name]]).T
    white = np.array([D65[0] / D65[1], 1.0, (1.0 - D65[0] - D65[1]) / D65[1]])
    return p * np.linalg.solve(p, white)[None, :]


def gamut_double(name):
    """linear BT.2020 RGB -> linear `name` RGB"""
    return np.linalg.solve(rgb_to_xyz(name), rgb_to_xyz("bt2020"))


def gamut_int(name):
    return np.rint(gamut_double(name) * 65536.0).astype(np.int64)


def codes(planes, depth, model, full_range):
    """three integer planes (Y, Cb, Cr with chroma of the luma's size or its ceil-half, or B, G, R) -> cR, cG, cB, clamped"""
    h, w = np.asarray(planes[0]).shape
    p = [np.asarray(planes[0], np.int64)] + [IR.replicate(np.asarray(q, np.int64), h, w) for q in planes[1:]]
    if model == IR.YUV2020:
        r, g, b = IR.rgb_from_yuv(p[0], p[1], p[2], depth, full_range)
    else:
        peak = np.float64((1 << depth) - 1)
        b, g, r = (q.astype(np.float64) / peak for q in p)
    clamped = np.zeros((h, w), bool)
    out = []
    for e in (r, g, b):
        clamped |= (e < 0.0) | (e > 1.0)
        out.append(np.rint(np.minimum(np.maximum(e, 0.0), 1.0) * 65535.0).astype(np.int64))
    return out[0], out[1], out[2], clamped


def outside(m, qr, qg, qb):
    """the gamut test on int64 arrays: min_k S_k < -((qmax << 16) >> 6) - 2^32"""
    m = np.asarray(m, np.int64).reshape(3, 3)
    s = [m[k, 0] * qr + m[k, 1] * qg + m[k, 2] * qb for k in range(3)]
    lo = np.minimum(s[0], np.minimum(s[1], s[2]))
    qmax = np.maximum(qr, np.maximum(qg, qb))
    return lo < -((qmax << 16) >> REL_SHIFT) - FLOOR


def record(planes, depth, model, full_range, table, m709, mp3):
    table = np.asarray(table, np.uint64)
    t = table.astype(np.int64)
    cr, cg, cb, clamped = codes(planes, depth, model, full_range)
    qr, qg, qb = t[cr], t[cg], t[cb]
    m = np.maximum(cr, np.maximum(cg, cb))
    qm = t[m]
    y = (2627 * qr + 6780 * qg + 593 * qb + 5000) // 10000
    n = m.size
    order = np.sort((m >> 4).ravel())                       # percentiles by sorting, not counting
    pct = [int(order[(p * n + 9999) // 10000 - 1]) for p in PERCENTILES]
    sum_q, sum_y = int(qm.sum()), int(y.sum())
    rec = {"count": n, "max_code": [int(cr.max()), int(cg.max()), int(cb.max())], "max_code_rgb": int(m.max()),
           "min_code_rgb": int(m.min()), "reserved": 0, "sum_q": sum_q, "sum_y": sum_y, "max_y": int(y.max()),
           "out_709": int(outside(m709, qr, qg, qb).sum()), "out_p3": int(outside(mp3, qr, qg, qb).sum()),
           "clamped": int(clamped.sum()), "pct_bin": pct}
    rec["max_nits"] = float(table[rec["max_code_rgb"]]) * UNIT
    rec["min_nits"] = float(table[rec["min_code_rgb"]]) * UNIT
    rec["avg_nits"] = float(np.float64(np.uint64(sum_q)) * UNIT / np.float64(n))
    rec["y_avg"] = float(np.float64(np.uint64(sum_y)) * UNIT / np.float64(n))
    rec["y_max"] = float(rec["max_y"]) * UNIT
    rec["maxscl"] = [float(table[c]) * UNIT for c in rec["max_code"]]
    rec["pct_nits"] = [float(table[b << 4]) * UNIT for b in pct]
    rec["share_709"] = rec["out_709"] / n
    rec["share_p3"] = rec["out_p3"] / n
    return rec, np.bincount((m >> 4).ravel(), minlength=BINS).astype(np.uint32)


def records(frames, planes, depth, model, full_range, table, m709, mp3):
    """frames [n, samples] and plane tuples -> per frame (record, histogram)"""
    return [record(p, depth, model, full_range, table, m709, mp3) for p in IR.split_planes(frames, planes)]


def encode_2020(rgb_nits, depth=10):
    """linear BT.2020 display light [.., 3] in cd/m2 -> limited-range PQ Y'CbCr 4:4:4 code values (rounded, clipped to the
    depth), by the inverse of the header's chain"""
    e = IR.pq_inverse(np.clip(np.asarray(rgb_nits, np.float64), 0.0, 10000.0))
    r, g, b = e[..., 0], e[..., 1], e[..., 2]
    y = IR.KR * r + IR.KG * g + IR.KB * b
    cb, cr = (b - y) / 1.8814, (r - y) / 1.4746
    s, peak = 1 << (depth - 8), (1 << depth) - 1
    q = [np.rint(219 * s * y + 16 * s), np.rint(224 * s * cb + 128 * s), np.rint(224 * s * cr + 128 * s)]
    return [np.clip(v, 0, peak).astype(np.int64) for v in q]
