"""The reference side of the localised probes (tests/probe_cases.py): D per probe, in float64 and in the float32 restatement.

  D(k) = sum over the map of  value(ref, ref) - value(ref, dist_k)

taken over the windows the patch touches - every other window holds the same numbers in both maps and its difference is exactly 0,
in any arithmetic - so D carries no rounding floor from the rest of the plane.  The maps are those of tests/hbd_reference.py
(Gaussian SSIM, vf_ssim), tests/msssim_reference.py (the pyramid) and tests/vif_reference.py, through their own functions; nothing
they compute is altered.  A `mutate` argument is the teeth test's: it receives the finished maps and returns them broken."""
import functools

import numpy as np

import hbd_reference as R
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


# ---- groups and bars ---------------------------------------------------------------------------------------------------------------
def _table(kind, name, depth, dtype):
    """-> float64 [probes, levels] of a kind (MS-SSIM: cs and ssim are two kinds, "ms-cs" and "ms-ssim")"""
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
    d64, d32 = D64(kind, name, depth), D32(kind, name, depth)
    with np.errstate(divide="ignore", invalid="ignore"):      # (a level a small patch does not reach: not judged, see kept())
        return np.abs(d32 - d64) / np.abs(d64)


def group_ratio(kind, level, name, depth):
    """r of a group: the largest ratio over the probes that are not excluded"""
    return float(ratios(kind, name, depth)[kept(kind, level), level].max())


def bar(kind, level, name, depth):
    """the GPU's bar of a group: MARGIN r (probe_cases.MARGIN_OF: the groups with a derived margin of their own), floored at FLOOR
    (tests/test_probe_host.py holds it below CAP)"""
    return max(PC.MARGIN_OF.get((kind, level, name, depth), PC.MARGIN) * group_ratio(kind, level, name, depth), PC.FLOOR)
