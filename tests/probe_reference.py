"""The reference side of the localised probes (tests/probe_cases.py): D per probe, in float64 and in the float32 restatement.

  D(k) = sum over the map of  value(ref, ref) - value(ref, dist_k)

taken over the windows the patch touches - every other window holds the same numbers in both maps and its difference is exactly 0,
in any arithmetic - so D carries no rounding floor from the rest of the plane.  The maps are those of tests/hbd_reference.py
(Gaussian SSIM, vf_ssim), tests/msssim_reference.py (the pyramid) and tests/vif_reference.py, through their own functions; nothing
they compute is altered.  A `mutate` argument is the teeth test's: it receives the finished maps and returns them broken.

ADM (tests/adm_reference.py) pools cube roots of sums, so D = num[s](ref, ref) - num[s](ref, dist_k) is taken between the totals, as
on the GPU; where the patch reaches no pooled sample every statement sees the same numbers and D is exactly 0.  Motion
(tests/motion_reference.py): D is the pair's sad itself."""
import contextlib
import functools

import numpy as np

import adm_reference as A
import hbd_reference as R
import motion_reference as MO
import msssim_reference as M
import probe_cases as PC
import vif_reference as V


# ---- Gaussian SSIM and the MS-SSIM levels ------------------------------------------------------------------------------------------
def gauss_maps(x, y, data_range, dtype=np.float64, filt=R._filt):
    """-> (cs map, ssim map) of one level: hbd_reference.ssim_gauss's statements (the ssim map's mean is its return value bit for
    bit), with msssim_reference.window_means' contrast-structure term beside them.  x, y: float64 planes in sample units (a
    pyramid level's 2x2 means are dyadic rationals of depth + 8 bits at most: exact in float32 too)"""
    ty = np.dtype(dtype).type
    if ty is np.float64:
        scale, centre = ty(1), ty(0)
    else:
        scale, centre, data_range = ty(255.0 / data_range), ty(128), 255
    x, y = x.astype(dtype) * scale - centre, y.astype(dtype) * scale - centre
    mx, my = filt(x), filt(y)
    sxx = filt(x * x) - mx * mx
    syy = filt(y * y) - my * my
    sxy = filt(x * y) - mx * my
    ux, uy = mx + centre, my + centre
    C1, C2 = ty((.01 * data_range) ** 2), ty((.03 * data_range) ** 2)
    S = ((2 * ux * uy + C1) * (2 * sxy + C2)) / ((ux * ux + uy * uy + C1) * (sxx + syy + C2))
    cs = (2 * sxy + C2) / (sxx + syy + C2)
    return cs.astype(np.float64), S.astype(np.float64)


def _touched(xr, xd, reach):
    """the rows and columns of samples any window that holds a changed sample reads: the changed box grown by `reach`"""
    ys, xs = np.nonzero(xr != xd)
    if ys.size == 0:
        return None
    h, w = xr.shape
    return (slice(max(ys.min() - reach, 0), min(ys.max() + reach + 1, h)), slice(max(xs.min() - reach, 0), min(xs.max() + reach + 1, w)))


def gauss_level_D(xr, xd, data_range, dtype=np.float64, crop=True, mutate=None):
    """-> (D of cs, D of ssim) of one level.  crop: only the windows the changed samples touch are evaluated (the same statements
    on the same numbers as on the whole plane); a mutation wants the whole plane, its seams are plane coordinates"""
    box = _touched(xr, xd, 10) if crop else (slice(None), slice(None))
    if box is None:
        return 0.0, 0.0
    a, b = xr[box], xd[box]
    rr, rd = gauss_maps(a, a, data_range, dtype), gauss_maps(a, b, data_range, dtype)
    if mutate is not None:
        assert not crop
        rr, rd = mutate(a, a, rr), mutate(a, b, rd)
    return float((rr[0] - rd[0]).sum()), float((rr[1] - rd[1]).sum())


@functools.lru_cache(maxsize=None)
def gauss_D(name, depth, dtype="float64"):
    """D of the Gaussian SSIM of every probe of the 140 x 264 plane: -> float64 [probes]"""
    a = PC.ref_plane("gauss", name, depth).astype(np.float64)
    L = (1 << depth) - 1
    out = [gauss_level_D(a, PC.dist_plane("gauss", name, depth, p).astype(np.float64), L, np.dtype(dtype))[1] for p in PC.probes("gauss")]
    return np.array(out)


@functools.lru_cache(maxsize=None)
def ms_D(name, depth, dtype="float64"):
    """D of every level's cs and ssim mean of every probe of the 352 x 528 plane: -> float64 [probes, 2 (cs, ssim), 5]"""
    a = PC.ref_plane("ms", name, depth)
    L = (1 << depth) - 1
    lr = M.pyramid(a)
    out = []
    for p in PC.probes("ms"):
        ld = M.pyramid(PC.dist_plane("ms", name, depth, p))
        out.append(np.array([gauss_level_D(x, y, L, np.dtype(dtype)) for x, y in zip(lr, ld)]).T)
    return np.array(out)


def map_samples(kind, level=0):
    """N of a level: the samples of its map"""
    h, w = PC.plane_of(kind)
    if kind == "ffmpeg":
        return ((h >> 2) - 1) * ((w >> 2) - 1)
    if kind == "vif":
        return (h >> level) * (w >> level)
    for _ in range(level):
        h, w = (h + 1) // 2, (w + 1) // 2
    return (h - 10) * (w - 10)


# ---- vf_ssim -----------------------------------------------------------------------------------------------------------------------
def ffmpeg_map(a, b, depth, dtype=np.float64):
    """the map of 8x8 windows at stride 4 of vf_ssim on int64 planes.  Above 8 bits: hbd_reference.ssim_ffmpeg's statements (double,
    as FFmpeg's ssim_end1x; its return value is this map's mean).  At 8 bits FFmpeg's ssim_end1: the constants are the integers
    416 and 235963 and the four factors are converted to float and combined in float; dtype float32 is that definition itself,
    float64 the same integers in double."""
    h, w = a.shape
    bh, bw = h >> 2, w >> 2
    A = a[:bh * 4, :bw * 4].reshape(bh, 4, bw, 4)
    B = b[:bh * 4, :bw * 4].reshape(bh, 4, bw, 4)
    s = [A.sum((1, 3)), B.sum((1, 3)), (A * A).sum((1, 3)) + (B * B).sum((1, 3)), (A * B).sum((1, 3))]
    s1, s2, ss, s12 = (x[:-1, :-1] + x[:-1, 1:] + x[1:, :-1] + x[1:, 1:] for x in s)
    if depth > 8:
        mx = (1 << depth) - 1
        c1, c2 = .01 * .01 * mx * mx * 64, .03 * .03 * mx * mx * 64 * 63
        s1, s2, ss, s12 = (x.astype(np.float64) for x in (s1, s2, ss, s12))
        vars_ = ss * 64 - s1 * s1 - s2 * s2
        covar = s12 * 64 - s1 * s2
        return (2 * s1 * s2 + c1) * (2 * covar + c2) / ((s1 * s1 + s2 * s2 + c1) * (vars_ + c2))
    c1, c2 = 416, 235963
    vars_ = ss * 64 - s1 * s1 - s2 * s2
    covar = s12 * 64 - s1 * s2
    f = [x.astype(dtype) for x in (2 * s1 * s2 + c1, 2 * covar + c2, s1 * s1 + s2 * s2 + c1, vars_ + c2)]
    return (f[0] * f[1] / (f[2] * f[3])).astype(np.float64)


def ffmpeg_probe_D(a, d, depth, dtype=np.float64, mutate=None):
    rr, rd = ffmpeg_map(a, a, depth, dtype), ffmpeg_map(a, d, depth, dtype)
    if mutate is not None:
        rr, rd = mutate(a, a, rr), mutate(a, d, rd)
    return float((rr - rd).sum())


@functools.lru_cache(maxsize=None)
def ffmpeg_D(name, depth, dtype="float64"):
    """D of vf_ssim of every probe: -> float64 [probes].  Above 8 bits the definition is double: float32 has no meaning there
    and returns the float64 figures"""
    a = PC.ref_plane("ffmpeg", name, depth)
    return np.array([ffmpeg_probe_D(a, PC.dist_plane("ffmpeg", name, depth, p), depth, np.dtype(dtype)) for p in PC.probes("ffmpeg")])


# ---- VIF ---------------------------------------------------------------------------------------------------------------------------
def vif_maps(ref, dist, depth=8, dtype=np.float64):
    """vif_reference.vif's loop, keeping the maps: -> [(num map, den map)] per level (their float64 sums are its num and den)"""
    ty = np.dtype(dtype).type
    sc = ty(1 << (depth - 8))
    x, y = np.asarray(ref).astype(dtype) / sc - ty(128), np.asarray(dist).astype(dtype) / sc - ty(128)
    out = []
    for s in range(V.LEVELS):
        if s:
            x, y = V.next_level(x, s), V.next_level(y, s)
        out.append(V.statistic(x, y, s))
    return out


def vif_probe_D(maps_rr, a, d, depth, dtype=np.float64, mutate=None):
    """-> D of num per level, from the maps of (a, a) (shared by the probes of a plane) and those of (a, d)"""
    maps_rd = vif_maps(a, d, depth, dtype)
    if mutate is not None:
        maps_rd = [mutate(s, m) for s, m in enumerate(maps_rd)]
    return np.array([float(rr[0].sum(dtype=np.float64) - rd[0].sum(dtype=np.float64)) for rr, rd in zip(maps_rr, maps_rd)])


@functools.lru_cache(maxsize=None)
def vif_D(name, depth, dtype="float64"):
    """D of num[s] of every probe: -> float64 [probes, 4].  The totals of a level are a few thousand and each is a float64 sum of
    its map, good to 1e-12: D is taken between the totals, as on the GPU"""
    a = PC.ref_plane("vif", name, depth)
    rr = vif_maps(a, a, depth, np.dtype(dtype))
    return np.array([vif_probe_D(rr, a, PC.dist_plane("vif", name, depth, p), depth, np.dtype(dtype)) for p in PC.probes("vif")])


# ---- ADM ---------------------------------------------------------------------------------------------------------------------------
ADM_MARGIN = 2.0 ** -20      # tests/test_gpu_adm.py's: a sample is unsure when its angle test flips within this relative margin


def adm_sums(ref, dist, depth=8, dtype=np.float64, mutate=None, margin=0.0):
    """adm_reference.adm's loop over the scales, through its own dwt and scale_sums: -> (num [4], den [4], unsure [4], lo [4], hi [4]).
    unsure (margin > 0): the unsure samples of the pooled region grown by one - a sample just outside it still masks one inside;
    lo, hi: the smallest and the largest num[s] among: as computed, the unsure samples' flags all forced off, all forced on
    (adm_reference's machinery; a flag of scale s moves num[s] alone, the a band does not depend on it).
    mutate: the teeth test's, an object with  bands(s, the scale's input, its four bands (a, v, h, d)) -> four bands  and
    patched(s), a context manager held around scale s's scale_sums."""
    ty = np.dtype(dtype).type
    sc = ty(1 << (depth - 8))
    x, y = np.asarray(ref).astype(dtype) / sc - ty(128), np.asarray(dist).astype(dtype) / sc - ty(128)
    num, den, unsure = np.zeros(A.LEVELS), np.zeros(A.LEVELS), np.zeros(A.LEVELS, int)
    forced = np.full((A.LEVELS, 2), np.nan)
    for s in range(A.LEVELS):
        bx, by = A.dwt(x), A.dwt(y)
        if mutate is not None:
            bx, by = mutate.bands(s, x, bx), mutate.bands(s, y, by)
        o, t = (bx[2], bx[1], bx[3]), (by[2], by[1], by[3])
        with (mutate.patched(s) if mutate is not None else contextlib.nullcontext()):
            num[s], den[s], _ = A.scale_sums(o, t, s)
        if margin:
            top, bottom, left, right, _area = A.region(*o[0].shape)
            u = A.decouple(o, t, margin)[2]
            unsure[s] = int(u[max(top - 1, 0):bottom + 1, max(left - 1, 0):right + 1].sum())
            if unsure[s]:
                forced[s] = [A.scale_sums(o, t, s, flag_override=f, margin=margin)[0] for f in (False, True)]
        x, y = bx[0], by[0]
    both = np.vstack([num, forced.T])
    return num, den, unsure, np.nanmin(both, axis=0), np.nanmax(both, axis=0)


@functools.lru_cache(maxsize=None)
def adm_table(kind, name, depth, dtype="float64"):
    """-> (D of num[s] of every probe: float64 [probes, 4]; the unsure samples of every probe's frame: int [probes, 4]; the interval
    [D_lo, D_hi] of the forced-flag runs, D itself where nothing is unsure) - the last three of the float64 run only"""
    a = PC.ref_plane(kind, name, depth)
    dt = np.dtype(dtype)
    margin = ADM_MARGIN if dt == np.float64 else 0.0
    num0 = adm_sums(a, a, depth, dt)[0]
    D, unsure, d_lo, d_hi = [], [], [], []
    for p in PC.probes(kind):
        num, _den, u, lo, hi = adm_sums(a, PC.dist_plane(kind, name, depth, p), depth, dt, margin=margin)
        D.append(num0 - num)
        unsure.append(u)
        d_lo.append(num0 - hi)
        d_hi.append(num0 - lo)
    return np.array(D), np.array(unsure), np.array(d_lo), np.array(d_hi)


def adm_sigma(plane, name, depth, probe, s):
    """the float32 noise D of one item is expected to carry, from the reference alone (probe_cases.MARGIN_OF uses it; the GPU is not
    asked).  e = the rms distance of the float32 run's detail coefficients of scale s from the float64 run's (the roundings of
    2 (s + 1) filter passes).  x = |rf r| - thr of a band then carries rf e, and num = sum_b cbrt(S_b), S_b = sum x^3, moves by
    S_b^(-2/3) sum x^2 dx: over the touched pooled samples, whose roundings are independent between frame 0 and frame k,
    sigma_D^2 = sum over both frames and the three bands of  S_b^(-4/3) (rf_b e)^2 sum_touched x^4.  -> (sigma_D, e, touched)"""
    a = PC.ref_plane(plane, name, depth)

    def bands(img, dt):
        x = img.astype(dt) / dt(1 << (depth - 8)) - dt(128)
        for _ in range(s + 1):
            b = A.dwt(x)
            x = b[0]
        return b
    pair = [(bands(img, np.float64), bands(img, np.float32)) for img in (a, PC.dist_plane(plane, name, depth, probe))]
    e = float(np.sqrt(np.mean([(b32[k].astype(np.float64) - b64[k]) ** 2 for b64, b32 in pair for k in (1, 2, 3)])))
    ref, dist = pair[0][0], pair[1][0]
    touched = (ref[1] != dist[1]) | (ref[2] != dist[2]) | (ref[3] != dist[3])
    top, bottom, left, right, _area = A.region(*touched.shape)
    pooled = np.zeros(touched.shape, bool)
    pooled[top:bottom, left:right] = True
    w = (A.rf(s)[0], A.rf(s)[0], A.rf(s)[1])
    o = (ref[2], ref[1], ref[3])
    var = 0.0
    for b in (ref, dist):
        t = (b[2], b[1], b[3])
        r, flag, _unsure = A.decouple(o, t)
        r = A._apply_flag(r, t, flag)
        thr = A._neighbour_sum(sum(np.abs(w[k] * (t[k] - r[k])) for k in range(3)))
        for k in range(3):
            x = np.maximum(np.abs(w[k] * r[k]) - thr, 0.0)
            var += (x[pooled] ** 3).sum() ** (-4.0 / 3.0) * (w[k] * e) ** 2 * (x[touched & pooled] ** 4).sum()
    return float(np.sqrt(var)), e, int((touched & pooled).sum())


def adm_D(plane, name, depth, dtype="float64"):
    """D of num[s] of every probe of plane "adm" (A) or "adm-b" (B): -> float64 [probes, 4]"""
    return adm_table(plane, name, depth, np.dtype(dtype).name)[0]


def adm_unsure(plane, name, depth):
    """the (scale, probe) items of a case whose touched region holds an unsure sample: -> {(scale, probe): (D_lo, D_hi)}"""
    pr = PC.probes(plane)
    _D, u, lo, hi = adm_table(plane, name, depth)
    return {(int(s), pr[int(k)]): (float(lo[k, s]), float(hi[k, s])) for k, s in zip(*np.nonzero(u))}


def interval(kind, name, depth):
    """-> (lo, hi) [probes, levels]: what D_gpu is held to, before the bar widens it.  D_64 itself, but for ADM's unsure items"""
    if kind in ("adm", "adm-b"):
        return adm_table(kind, name, depth)[2:]
    d = D64(kind, name, depth)
    return d, d


# ---- motion ------------------------------------------------------------------------------------------------------------------------
def motion_blur(x, dtype=np.float64, hmutate=None):
    """motion_reference.blur's statements in `dtype` (float64: its bits): the vertical pass first, then the horizontal one.
    hmutate(v, out) -> out: the teeth test's, it receives the vertical pass and the finished blur"""
    ty = np.dtype(dtype).type

    def one_pass(v, axis):
        n = v.shape[axis]
        out = np.zeros_like(v)
        for k, t in enumerate(MO.TAPS):
            idx = [MO.border_index(i + k - 2, n) for i in range(n)]
            out = out + ty(t) * np.take(v, idx, axis=axis)
        return out
    v = one_pass(np.asarray(x).astype(dtype), 0)
    out = one_pass(v, 1)
    return out if hmutate is None else hmutate(v, out)


def motion_sad(cur, prev, depth, dtype=np.float64, hmutate=None, omutate=None):
    """motion_reference.sad in `dtype`; omutate(|difference map|) -> map is the teeth test's"""
    ty = np.dtype(dtype).type
    xs = [np.asarray(p).astype(dtype) / ty(1 << (depth - 8)) - ty(128) for p in (cur, prev)]
    d = np.abs(motion_blur(xs[0], dtype, hmutate) - motion_blur(xs[1], dtype, hmutate))
    if omutate is not None:
        d = omutate(d)
    return float(d.sum(dtype=np.float64))


@functools.lru_cache(maxsize=None)
def motion_D(name, depth, dtype="float64"):
    """D of every probe: the sad of the pair (p_k, base) itself -> float64 [probes].  float64 is motion_reference.sad"""
    a = PC.ref_plane("motion", name, depth)
    if np.dtype(dtype) == np.float64:
        return np.array([MO.sad(PC.dist_plane("motion", name, depth, p), a, depth) for p in PC.probes("motion")])
    return np.array([motion_sad(PC.dist_plane("motion", name, depth, p), a, depth, np.dtype(dtype)) for p in PC.probes("motion")])


def motion_fixed_point():
    """the fixed-point term of every probe, derived: each output sample the blur of the patch reaches rounds |d| 2^16 to an integer,
    at most 2^-17 each, and every other sample is 0 = 0: -> float64 [probes], absolute on sad"""
    return np.array([PC.motion_touched(p) * PC.MOTION_QUANTUM for p in PC.probes("motion")])


# ---- groups and bars ---------------------------------------------------------------------------------------------------------------
def _table(kind, name, depth, dtype):
    """-> float64 [probes, levels] of a kind (MS-SSIM: cs and ssim are two kinds, "ms-cs" and "ms-ssim"; ADM: "adm" is plane A and
    "adm-b" plane B, the level is the scale)"""
    if kind in ("adm", "adm-b"):
        return adm_D(kind, name, depth, dtype)
    if kind == "motion":
        return motion_D(name, depth, dtype)[:, None]
    if kind == "gauss":
        return gauss_D(name, depth, dtype)[:, None]
    if kind == "ffmpeg":
        return ffmpeg_D(name, depth, dtype)[:, None]
    if kind == "vif":
        return vif_D(name, depth, dtype)
    return ms_D(name, depth, dtype)[:, 0 if kind == "ms-cs" else 1, :]


def base_kind(kind):
    return "ms" if kind.startswith("ms") else kind


def D64(kind, name, depth):
    return _table(kind, name, depth, "float64")


def D32(kind, name, depth):
    return _table(kind, name, depth, "float32")


def kept(kind, level):
    """the indices of the probes of a (kind, level) that are not excluded by name"""
    b = base_kind(kind)
    return [k for k, p in enumerate(PC.probes(b)) if level in PC.levels_of(b, p) and not PC.excluded(b, level, p)]


def ratios(kind, name, depth):
    """|D_32 - D_64| / |D_64| of every (probe, level): -> float64 [probes, levels]"""
    return gap(kind, name, depth, D32(kind, name, depth))


def gap(kind, name, depth, got):
    """the distance of `got` [probes, levels] from D_64 - for one of ADM's unsure items, from the interval of its forced-flag runs -
    over |D_64|: what a bar is compared with"""
    d64 = D64(kind, name, depth)
    lo, hi = interval(kind, name, depth)
    with np.errstate(divide="ignore", invalid="ignore"):      # (a level a small patch does not reach: not judged, see kept())
        return np.maximum(np.maximum(lo - got, got - hi), 0.0) / np.abs(d64)


def slack(kind):
    """what is added to a bar in absolute terms: motion's fixed-point term, -> float64 [probes, 1], in units of D; 0 elsewhere"""
    return motion_fixed_point()[:, None] if kind == "motion" else 0.0


def group_ratio(kind, level, name, depth):
    """r of a group: the largest ratio over the probes that are not excluded"""
    return float(ratios(kind, name, depth)[kept(kind, level), level].max())


def bar(kind, level, name, depth):
    """the GPU's bar of a group: MARGIN r (probe_cases.MARGIN_OF: the groups with a derived margin of their own), floored at FLOOR
    (tests/test_probe_host.py holds it below CAP)"""
    return max(PC.MARGIN_OF.get((kind, level, name, depth), PC.MARGIN) * group_ratio(kind, level, name, depth), PC.FLOOR)
