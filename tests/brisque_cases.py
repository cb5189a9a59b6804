"""The shared cases of the BRISQUE tests (tests/test_brisque_host.py, tests/test_gpu_brisque.py): the geometry, depth and layout
grid and the contents.  Seeded; the restatements of every (entry, content) are computed once and shared.

The grid is artifacts_cases.GRID's geometries plus the sizes that cross k_brisque_mscn's 64 x 16 tile at BOTH scales:
  scale 0   by one: 17 rows (17 x 25), 65 columns (33 x 65)
  scale 1   by one: 33 -> 17 rows (33 x 65), 130 -> 65 columns (20 x 130); by two columns: 132 -> 66 (34 x 132, whose 17 rows
            cross by one as well)
4:2:0 at 66 x 98 adds chroma planes of 33 x 49 (scale 1: 17 x 25).  16 x 300 and 300 x 16 have a side above 256: strips longer
than k_brisque_seam's workgroup, and a row of tiles longer than one run of four."""
import functools

import numpy as np

import artifacts_cases as AC
import brisque_reference as R
import motion_cases as K

GRID = list(AC.GRID) + [((34, 132), 8, "gray", 2), ((20, 130), 8, "gray", 2), ((16, 300), 8, "gray", 2), ((300, 16), 8, "gray", 2)]
IDS = ["%dx%d-%s" % (g[0][0], g[0][1], g[2]) for g in GRID]

# natural: smoothed noise plus grain (fits mid-grid); noise: uniform noise (the scale-0 GGD alpha saturates at 10.0: the clamp
# case); flat: a bright near-flat field, peak - 3 .. peak - 1 (where fp32 moments would cancel); zeros; ends: 0 or peak
KINDS = ("natural", "noise", "flat", "zeros", "ends")


def plane(kind, h, w, depth, seed):
    """[h, w] int64 samples"""
    rng = np.random.default_rng(seed)
    peak = (1 << depth) - 1
    if kind == "zeros":
        return np.zeros((h, w), np.int64)
    if kind == "noise":
        return rng.integers(0, peak + 1, (h, w)).astype(np.int64)
    if kind == "ends":
        return rng.integers(0, 2, (h, w)).astype(np.int64) * peak
    if kind == "flat":
        return peak - 3 + rng.integers(0, 3, (h, w)).astype(np.int64)
    a = rng.normal(size=(h + 16, w + 16))
    k = np.ones(3) / 3.0
    for ax in (0, 1):
        a = np.apply_along_axis(lambda v: np.convolve(v, k, "same"), ax, a)
    a = a[8:8 + h, 8:8 + w]
    a = a / a.std()
    x = 0.5 * peak + 0.18 * peak * a + 0.1 * peak * rng.normal(size=(h, w))
    return np.clip(np.rint(x), 0, peak).astype(np.int64)


@functools.lru_cache(maxsize=None)
def clip(layout, h, w, depth, kind, n):
    """n frames in `layout`, every plane of every frame its own seeded content -> (frames, planes)"""
    planes = K.planes_of(layout, h, w)
    dt = np.uint16 if depth > 8 else np.uint8
    isz = np.dtype(dt).itemsize
    size = max(p[2] + (p[1] - 1) * p[3] + (p[0] - 1) * p[4] + isz for p in planes) // isz
    out = np.zeros((n, size), dt)
    for k, p in enumerate(planes):
        pw, ph, off, rs, step = p[:5]
        for i in range(n):
            view = np.lib.stride_tricks.as_strided(out[i, off // isz:], shape=(ph, pw), strides=(rs, step))
            view[...] = plane(kind, ph, pw, depth, 1000 * (h + w + depth) + 10 * i + k)
    if layout == "bgr24":
        out = out.reshape(n, h, w, 3)
    out.setflags(write=False)
    return out, planes


@functools.lru_cache(maxsize=None)
def restated(layout, h, w, depth, kind, n):
    """[frame][plane] -> dict(x, moments (float64), features, flags, ks, words (this file's integers), spans)"""
    f, planes = clip(layout, h, w, depth, kind, n)
    out = []
    for i in range(n):
        row = []
        for p in planes:
            x = K.plane_series(f[i:i + 1], p)[0]
            ft, flags, ks = R.float_features(x, depth)
            row.append(dict(x=x, moments=R.float_moments(x, depth), features=ft, flags=flags, ks=ks,
                            spans=R.alpha_spans(x, depth)))
        out.append(row)
    return out


# The natural-like fits that the admission rule (test_brisque_host.py) does NOT admit for end-to-end alpha comparison, by name:
# (grid id, frame, plane, fit), fit = 5 scale + (0: GGD, 1 .. 4: H, V, D1, D2).  Ten of the eleven are the GGD of scale 1 on a
# plane of at most 33 x 49 samples, whose scale-1 field has at most 425 samples: there alpha sits at 4 .. 6, where the ratio
# curve is flat and the bars move it by 3 .. 5 steps.  Every other fit of the natural-like content is admitted and compared.
NOT_ADMITTED = {("16x16-gray", 1, 0, 5), ("16x16-gray", 2, 0, 5), ("16x16-gray", 2, 0, 8), ("16x16-gray", 3, 0, 7),
                ("17x25-gray", 3, 0, 5), ("66x98-yuv420p", 0, 2, 5), ("66x98-yuv420p", 1, 2, 5), ("66x98-yuv420p", 2, 1, 5),
                ("64x96-yuv420p10le", 0, 1, 5), ("64x96-yuv420p10le", 1, 1, 5), ("64x96-yuv420p10le", 1, 2, 5)}


def rows(h, w, period, peak=255):
    """rows of 0 and of peak, `period` rows each.  Along a row m keeps its sign (a row of peak lies above every mu, a row of 0
    below), so no H product is negative: the H fit of scale 0 degenerates (n_neg == 0) and its bit is set.  period 1: every
    vertical and diagonal neighbour has the other sign, so V, D1 and D2 have no positive product and degenerate too;
    period 2: they see both signs and do not"""
    i = np.arange(h)[:, None]
    return np.broadcast_to(((i // period) & 1) * peak, (h, w)).astype(np.int64)


def gray_frames(planes, depth):
    return AC.gray_frames(planes, depth)


WORD_FIELDS = ("sum_abs_u", "sum_u2", "n_neg", "n_pos", "sum_abs_p", "sq_neg_lo", "sq_neg_hi", "sq_pos_lo", "sq_pos_hi")
FIELDS = WORD_FIELDS + ("flags", "reserved", "features")


def close_moments(got, want, tag):
    """the words' moments (got) against the float64 restatement's (want), each within its bar"""
    for s in (0, 1):
        g, f = got[s], want[s]
        assert abs(g["abs_m"] - f["abs_m"]) <= R.BAR_ABS_M, (tag, s, "abs_m", g["abs_m"], f["abs_m"])
        assert abs(g["m2"] - f["m2"]) <= R.bar_m2(f["abs_m"]), (tag, s, "m2", g["m2"], f["m2"])
        for o in range(4):
            a, b = g["o"][o], f["o"][o]
            assert abs(a["abs_p"] - b["abs_p"]) <= R.bar_abs_p(f["abs_m"]), (tag, s, o, "abs_p", a["abs_p"], b["abs_p"])
            for k in ("sq_neg", "sq_pos"):
                assert abs(a[k] - b[k]) <= R.bar_p2(b["abs_p"]), (tag, s, o, k, a[k], b[k])
            for k in ("n_neg", "n_pos"):
                assert abs(a[k] - b[k]) <= b["near"], (tag, s, o, k, a[k], b[k], b["near"])


# a libsvm model and an svm-scale range file made here: no BRISQUE model ships
def model_text(rng, n_sv=5):
    rows = []
    for _ in range(n_sv):
        idx = sorted(rng.choice(36, 20, replace=False) + 1)
        rows.append("%r " % float(rng.normal()) + " ".join("%d:%r" % (j, float(rng.uniform(-1, 1))) for j in idx))
    return "svm_type epsilon_svr\nkernel_type rbf\ngamma 0.05\nnr_class 2\ntotal_sv %d\nrho -1.5\nSV\n%s\n" % (n_sv, "\n".join(rows))


def range_text(lo, hi, lower=-1.0, upper=1.0):
    return "x\n%r %r\n" % (lower, upper) + "".join("%d %r %r\n" % (j + 1, float(lo[j]), float(hi[j])) for j in range(36))
