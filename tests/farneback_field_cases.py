"""Farneback judged per pixel: the cases, the launchers' geometry restated, the seam table and the two checks.  Seeded; one module, so
that tests/test_farneback_field_host.py (how far is the reference from itself, is the seam table the kernels', do the checks have
teeth?) and tests/test_gpu_farneback_field.py (the device's expansions and flow field against the oracle) see the same bytes.

A case is (shape, content): a batch of three gray frames (as BGR with three equal channels), so two pairs, one chunk, three planes.
What is compared:
  expansions   the five coefficient planes of every plane at every pyramid level, BIT FOR BIT with oracle/vqa_oracle.c
               (co.farneback_expansion): the claim of k_farneback.hip's header;
  flow         the final field of every pair, every pixel and both components, |gpu - C| <= bar(case), where
               bar = MARGIN * e,  e = max |flow_C - flow_64| = the reference's own float32-to-float64 distance on that case
               (co.farneback against no.farneback_mean_mag), floored at the float32 spacing of the case's largest flow component and
               never above CAP.  A case whose own e exceeds CAP is ill-conditioned in the reference itself: EXPANSIONS_ONLY."""
import functools
import os
import re

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- the cases -------------------------------------------------------------------------------------------------------------------
# (h, w), the smallest that crosses everything first:
#   264 x 520  three coarser levels, 132 x 260, 66 x 130, 33 x 65.  Level 0 crosses the column seams 242 / 484 (k_fb_iter), 246 / 492
#              (k_fb_polyexp_march) and 256 / 512 (k_fb_level3, and k_fb_upflow writing it); level 1 crosses 242, 246 and 256; both are
#              exact halvings (k_fb_level3<1>, <2>); levels 2 and 3 take k_fb_level<2,16> with 9 and 19 taps
#   263 x 519  the same level sizes (lrint of 131.5 / 259.5) but w != 2 lw: level 1 takes the bilinear k_fb_level<2,64>
#   70 x 500   one coarser level; wide and short: one strip's worth of rows in every marching kernel
#   97 x 131, 33 x 40, 9 x 9   one coarser level or none: the edge-replication paths.  9 x 9 has no float64 run
#              (oracle/np_oracle.py is valid from 10 x 10: below that OpenCV's unsigned border test wraps)
SHAPES = ((264, 520), (263, 519), (70, 500), (97, 131), (33, 40), (9, 9))
CONTENTS = ("pan", "pan2", "noise")
# pan: a Gaussian-filtered (sigma 2.5) noise texture panned by (2, 1) pixels per frame, built as test_farneback_known_translation_1080p
# builds its frames; pan2: sigma 1.5, panned by (-3, 2); noise: uniform noise, every frame its own
# (sigma, pan x, pan y, seed of the texture).  pan2's seed: with 78 the reference ITSELF is 7.8e-4 apart from its float64 run on
# 264 x 520, in the 15 x 15 neighbourhoods of a few top-border pixels near column 390 whose vertical flow lies within rounding of
# FarnebackUpdateMatrices' in-frame test (the discontinuity test_farneback_border_discontinuity_cases documents); 79, 80 and 81 are
# free of it on every shape (e 6e-7 .. 5.4e-6).  No pixel is excluded anywhere: the content is one the reference is stable on.
PAN = {"pan": (2.5, 2, 1, 77), "pan2": (1.5, -3, 2, 79)}
PAIRS, PLANES = 2, 3
# batch independence is checked on two larger batches of the same frames: 9 pairs, and 44 - the smallest class of batch in which
# k_fb_iter cuts a 264 x 520 frame into other strips than it does for one pair (tests/test_farneback_field_host.py asserts both)
NINE_PAIRS, MANY_PAIRS = 9, 44

MARGIN = 4.0    # the project's margin over the reference's own distance (tests/probe_cases.py)
CAP = 1e-4      # no bar is above this, absolute (flow components of the panned contents are 1 to 3.6)

# Judged on the expansions only, by name: the reference's own float32 and float64 runs are further apart than CAP on these two -
# uniform noise through three coarser levels, where the 2 x 2 system is singular to rounding at many pixels and the flow follows the
# last bit of the box sums (include/vqa.h, flow_mag_mean; test_farneback_ill_conditioned_frames).  e as measured by
# tests/test_farneback_field_host.py, which also asserts that exactly these cases exceed the cap.
EXPANSIONS_ONLY = {((264, 520), "noise"): 2.6e-4, ((263, 519), "noise"): 9.4e-4}

# 9 x 9 has no float64 run to measure e on.  It takes the e of the same content at 33 x 40: the other shape without a coarser level,
# the same kernels (k_fb_level3<1>, one column block, one strip) and the same three iterations from a zero field.
E_FROM = {(9, 9): (33, 40)}


def cases():
    return [(s, c) for s in SHAPES for c in CONTENTS]


def case_id(case):
    return "%dx%d-%s" % (case[0][0], case[0][1], case[1])


@functools.lru_cache(maxsize=None)
def gray_frames(case):
    """-> uint8 [3][h][w], read-only"""
    (h, w), content = case
    rng = np.random.default_rng(9000 + 7 * h + w)
    if content == "noise":
        g = rng.integers(0, 256, (PLANES, h, w), dtype=np.uint8)
    else:
        import scipy.ndimage as ndi
        sigma, px, py, seed = PAN[content]
        a = ndi.gaussian_filter(np.random.default_rng(seed).integers(0, 256, (h + 16, w + 16)).astype(np.float32), sigma)
        a = ((a - a.min()) / (a.max() - a.min()) * 255).astype(np.uint8)
        g = np.stack([a[8 + py * k:8 + py * k + h, 8 + px * k:8 + px * k + w] for k in range(PLANES)])
    g = np.ascontiguousarray(g)
    g.setflags(write=False)
    return g


def bgr_frames(case):
    """the batch as the engine takes it: [3][h][w][3], the three channels equal (BGR2GRAY of (g, g, g) is g: the weights sum to 1 in
    its fixed point; tests/test_farneback_field_host.py asserts it)"""
    return np.ascontiguousarray(np.repeat(gray_frames(case)[..., None], 3, axis=3))


# ---- references, computed once and shared ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def flow_c(case):
    """-> (float32 [pairs][h][w][2], [pairs] mean magnitudes) of oracle/vqa_oracle.c"""
    from oracle import c_oracle as co
    g = gray_frames(case)
    out = [co.farneback(g[p], g[p + 1], want_flow=True) for p in range(PAIRS)]
    f = np.stack([o[1] for o in out])
    f.setflags(write=False)
    return f, tuple(float(o[0]) for o in out)


@functools.lru_cache(maxsize=None)
def flow_64(case):
    """-> float64 [pairs][h][w][2] of oracle/np_oracle.py (valid from 10 x 10)"""
    from oracle import np_oracle as no
    g = gray_frames(case)
    assert min(case[0]) >= 10
    f = np.stack([np.asarray(no.farneback_mean_mag(g[p], g[p + 1], want_flow=True)[1], np.float64) for p in range(PAIRS)])
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def expansion_c(case, plane, level):
    """-> float32 [lh][lw][5] of oracle/vqa_oracle.c"""
    from oracle import c_oracle as co
    r = co.farneback_expansion(gray_frames(case)[plane], level)[0]
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def measured_e(case):
    """the reference's own float32-to-float64 distance on a case (over both pairs, every pixel, both components), with where it lies"""
    d = np.abs(flow_c(case)[0].astype(np.float64) - flow_64(case))
    i = np.unravel_index(int(np.argmax(d)), d.shape)
    return float(d[i]), tuple(int(v) for v in i)


def e_of(case):
    shape, content = case
    return measured_e((E_FROM.get(shape, shape), content))[0]


def judged_on_flow(case):
    return case not in EXPANSIONS_ONLY


def bar_of(case):
    """MARGIN * e, floored at the float32 spacing of the case's largest flow component, never above CAP"""
    floor = float(np.spacing(np.float32(np.abs(flow_c(case)[0]).max())))
    return min(max(MARGIN * e_of(case), floor), CAP)


# ---- the two checks (the host test plants errors in them, the GPU test judges the device with them) -------------------------------
def flow_gap(got, want):
    """-> (largest |got - want| over pixels and components, its (y, x, component))"""
    d = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
    i = np.unravel_index(int(np.argmax(d)), d.shape)
    return float(d[i]), tuple(int(v) for v in i)


def first_difference(got, want):
    """bitwise comparison of two float32 [lh][lw][5] expansions -> None, or (y, x, coefficient) of the first differing value in
    plane-major order (coefficient, row, column: the order the device keeps them in)"""
    a, b = np.ascontiguousarray(got, np.float32).view(np.uint32), np.ascontiguousarray(want, np.float32).view(np.uint32)
    assert a.shape == b.shape, (a.shape, b.shape)
    ne = np.argwhere((a != b).transpose(2, 0, 1))
    if not len(ne):
        return None
    c, y, x = (int(v) for v in ne[0])
    return y, x, c


# ---- the launchers' geometry, restated (csrc/k_farneback.hip, run_farneback in csrc/vqa_capi.hip) ---------------------------------
FI_NT, BS_M, FI_RESTART = 256, 7, 16
FI_OUT = FI_NT - 2 * BS_M            # 242 output columns per workgroup of k_fb_iter
PE_N, PM_NT = 5, 256
PM_OUT = PM_NT - 2 * PE_N            # 246 output columns per workgroup of k_fb_polyexp_march
L3_COLS, UF_COLS, UF_ROWS = 256, 256, 8


def source_constants():
    """the same constants as csrc/k_farneback.hip spells them"""
    txt = open(os.path.join(REPO, "real-time-video-quality-analysis_amd", "csrc", "k_farneback.hip")).read()

    def num(pat):
        return int(re.search(pat, txt).group(1))
    fi_nt = num(r"#define FI_THREADS (\d+)")
    assert re.search(r"constexpr int FI_NT = FI_THREADS, FI_OUT = FI_NT - 14;", txt)
    assert re.search(r"constexpr int PM_NT = (\d+), PM_OUT = PM_NT - 2 \* PE_N;", txt)
    return {"FI_NT": fi_nt, "FI_OUT": fi_nt - 14, "BS_M": num(r"constexpr int BS_M = (\d+);"),
            "FI_RESTART": num(r"#define FI_RESTART_ROWS (\d+)"), "PE_N": num(r"constexpr int PE_N = (\d+);"),
            "PM_NT": num(r"constexpr int PM_NT = (\d+),"), "PM_OUT": num(r"constexpr int PM_NT = (\d+),") - 2 * num(r"constexpr int PE_N = (\d+);"),
            "UF_ROWS": num(r"constexpr int UF_ROWS = (\d+);")}


def _ceil(a, b):
    return -(-a // b)


def lrint(v):
    return int(round(v))   # both round halves to even


def levels_of(h, w):
    k, scale = 0, 1.0
    while k < 3:
        scale *= 0.5
        if w * scale < 32 or h * scale < 32:
            break
        k += 1
    return k


def level_size(h, w, k):
    return lrint(h * 0.5 ** k), lrint(w * 0.5 ** k)


def blur_taps(k):
    sigma = (2.0 ** k - 1) * 0.5
    return max(lrint(sigma * 5) | 1, 3)


def iter_geometry(pairs, h, w):
    """fb_iter_geometry -> (column blocks, strips, rows per strip)"""
    ncb = -(-w // FI_OUT)
    cap = min(max(h // max(FI_RESTART, 32), 1), 64)
    best = None
    for n in range(1, cap + 1):
        qs = _ceil(_ceil(h, n), FI_RESTART) * FI_RESTART
        ne = -(-h // qs)
        cost = -(-(ncb * ne * pairs) // (768 * 256 // FI_NT)) * (qs + 16)
        if best is None or cost < best[0]:
            best = (cost, ne, qs)
    return ncb, best[1], best[2]


def polyexp_geometry(planes, h, w):
    """launch_fb_polyexp -> (column blocks, strips, rows per strip)"""
    ncb = -(-w // PM_OUT)
    ns = -(-2048 // (ncb * planes))
    ns = min(max(ns, 1), max(h // 32, 1))
    qs = -(-h // ns)
    return ncb, -(-h // qs), qs


def _axis(ssize, dsize, is_x):
    """fb_build_axis / fb_axis: the bilinear taps' first source index per destination index"""
    f = ((np.arange(dsize) + 0.5) * (1.0 / (dsize / ssize)) - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    if is_x:
        s = np.clip(s, 0, ssize - 1)
    return s


def _span(first, last, n, tile):
    return max(int(last[min(a + tile, n) - 1] - first[a] + 1) for a in range(n))


def level_kernel(planes, h, w, k):
    """launch_fb_level -> (kernel, tile columns, tile rows) of level k's image"""
    lh, lw = level_size(h, w, k)
    taps = blur_taps(k)
    r = taps >> 1
    halving = w == 2 * lw and h == 2 * lh
    if taps == 3 and (k == 0 or halving):
        nbx = -(-lw // L3_COLS)
        ns = min(max(-(-4096 // (nbx * planes)), 1), max(lh // 32, 1))
        qs = (-(-lh // ns) + 3) & ~3
        return ("k_fb_level3<1>" if k == 0 else "k_fb_level3<2>"), L3_COLS, qs
    assert k > 0   # (the finest level always has three taps)
    if halving:
        sx0, sx1 = 2 * np.arange(lw), 2 * np.arange(lw) + 1
        sy0, sy1 = 2 * np.arange(lh), 2 * np.arange(lh) + 1
    else:
        xo, yo = _axis(w, lw, True), _axis(h, lh, False)
        sx0, sx1 = xo, np.minimum(xo + 1, w - 1)
        sy0, sy1 = np.clip(yo, 0, h - 1), np.clip(yo + 1, 0, h - 1)
    tall = r <= 2
    cap_x = _span(sx0, sx1, lw, 32) + 2 * r
    cap_y = _span(sy0, sy1, lh, 32 if tall else 8) + 2 * r
    nsy = 64 if tall else 16
    lds = (((cap_x + 3) & ~3) + 4) * cap_y + 4 * 64 * cap_y + 4 * 64 * nsy + 4 * 32 + 4 * (64 + nsy)
    if lds > 64 * 1024:
        return "k_fb_blur_h + k_fb_blur_v + k_fb_resize<1>", 256, 16
    ts = 62 if r <= 1 else 64
    return ("k_fb_level<2,64>", ts // 2, ts // 2) if tall else ("k_fb_level<2,16>", ts // 2, 8)


def _cuts(n, step):
    return tuple(range(step, n, step))


@functools.lru_cache(maxsize=None)
def seam_table(shape, pairs=PAIRS):
    """every place where a kernel cuts a plane of this shape: [(level, kernel, 'col' | 'row', position)], position = the first
    column / row of the next block.  (k_fb_iter also restarts its column sums at every multiple of 16 rows inside a strip: listed as
    'restart' rows.)"""
    h, w = shape
    out = []
    levels = levels_of(h, w)
    for k in range(levels + 1):
        lh, lw = level_size(h, w, k)
        name, tc, tr = level_kernel(pairs + 1, h, w, k)
        for x in _cuts(lw, tc):
            out.append((k, name, "col", x))
        for y in _cuts(lh, tr):
            out.append((k, name, "row", y))
        ncb, ns, qs = polyexp_geometry(pairs + 1, lh, lw)
        for x in _cuts(lw, PM_OUT):
            out.append((k, "k_fb_polyexp_march", "col", x))
        for y in _cuts(lh, qs):
            out.append((k, "k_fb_polyexp_march", "row", y))
        ncb, ns, qs = iter_geometry(pairs, lh, lw)
        for x in _cuts(lw, FI_OUT):
            out.append((k, "k_fb_iter", "col", x))
        for y in _cuts(lh, qs):
            out.append((k, "k_fb_iter", "row", y))
        for y in _cuts(lh, FI_RESTART):
            if y % qs:
                out.append((k, "k_fb_iter", "restart", y))
        if k < levels:   # the coarser level's flow is upsampled INTO this level
            for x in _cuts(lw, UF_COLS):
                out.append((k, "k_fb_upflow", "col", x))
            for y in _cuts(lh, UF_ROWS):
                out.append((k, "k_fb_upflow", "row", y))
    return tuple(out)


def seams_beside(shape, level, y, x, kernels=None, reach=1):
    """the seams of `level` that (y, x) lies beside: within `reach` columns / rows of the cut, either side"""
    hits = []
    for k, name, kind, pos in seam_table(shape):
        if k != level or (kernels and name not in kernels):
            continue
        at = x if kind == "col" else y
        if pos - reach <= at < pos + reach:
            hits.append("%s %s %d" % (name, kind, pos))
    return hits


def describe(shape, level, y, x, kernels=None):
    s = seams_beside(shape, level, y, x, kernels, reach=8)
    lh, lw = level_size(shape[0], shape[1], level)
    edge = [n for n, on in (("top", y < 8), ("bottom", y >= lh - 8), ("left", x < 8), ("right", x >= lw - 8)) if on]
    return "(row %d, column %d) of level %d (%d x %d); within 8 of: %s" % (y, x, level, lh, lw, ", ".join(s + edge) or "no seam or edge")


# ---- the magnitude sum, as the kernel forms it ------------------------------------------------------------------------------------
def fixed_point_mean(flow):
    """mean |flow| of a float32 [h][w][2] field the way k_fb_iter<.., MAG> and k_fb_mag_finalize form it: float32 magnitudes
    sqrtf(fx fx + fy fy) (no contraction), each times 2^28 and rounded to the nearest integer (ties to even), summed as integers,
    the total times 2^-28, times 1 / (h w) -> (mean, the integer total)"""
    f = np.asarray(flow, np.float32)
    fx, fy = f[..., 0], f[..., 1]
    m = np.sqrt(fx * fx + fy * fy)                                  # float32 throughout; np.sqrt is correctly rounded
    q = np.rint(m.astype(np.float64) * 268435456.0).astype(np.int64)  # m 2^28 is exact in float32 as well: a power of two
    t = int(q.sum())
    h, w = fx.shape
    return float(t) * (1.0 / 268435456.0) * (1.0 / (float(h) * float(w))), t

