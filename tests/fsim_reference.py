"""FSIM / FSIMc (Zhang, Zhang, Mou and Zhang 2011) restated from the definition in include/vqa.h (vqa_fsim_submit), in NumPy:

  filters / noise_factor   the sixteen log-Gabor tables of a grid and the noise factor c_o in the MATLAB form (real(ifft2(filt))
                           sqrt(N), EstSumAn2 + 2 EstSumAiAj), which the library forms by Parseval
  phase_congruency         PC of one Y grid in float64, through np.fft or (dense=True) through explicit DFT matrix products
  fsim_float               the definition in plain float64, nothing quantised -> (fsim, fsimc, PC_r, PC_d)
  pool_words               the integer pooling over GIVEN p maps -> the three words P, A, B; scores_of gives fsim, fsimc from them

A frame is a list of 2-D integer arrays: [Y, U, V] (U, V of the luma's size or its ceil-half in either direction), [B, G, R] or
[Y].  model: "yuv709" | "bgr" | "gray".  Not pinned against the authors' MATLAB (README, Parity)."""
import functools
import math

import numpy as np

import mdsi_reference as MR

T1, T2, T3, LAMBDA = 0.85, 160.0, 200.0, 0.03
FIX = float(1 << 24)
A_ROWS = ((0.299, 0.587, 0.114), (0.596, -0.274, -0.322), (0.211, -0.523, 0.312))   # Y, I, Q over R, G, B
NSCALE = NORIENT = 4
grid = MR.grid


# ---- the filter bank --------------------------------------------------------------------------------------------------------
def _range(n):
    return (np.arange(n) - (n - 1) / 2.0) / (n - 1) if n % 2 else (np.arange(n) - n / 2.0) / n


@functools.lru_cache(maxsize=8)
def filters(hd, wd):
    """-> filt [orientation][scale][hd, wd] float64.  Cached: read-only."""
    x, y = np.meshgrid(_range(wd), _range(hd))
    radius = np.fft.ifftshift(np.sqrt(x * x + y * y))
    theta = np.fft.ifftshift(np.arctan2(-y, x))
    lp = 1.0 / (1.0 + (radius / 0.45) ** 30)
    radius[0, 0] = 1.0
    sint, cost = np.sin(theta), np.cos(theta)
    log_gabor = []
    for s in range(NSCALE):
        fo = 1.0 / (6.0 * 2.0 ** s)
        g = np.exp(-(np.log(radius / fo)) ** 2 / (2.0 * math.log(0.55) ** 2)) * lp
        g[0, 0] = 0.0
        log_gabor.append(g)
    sigma = (math.pi / 4.0) / 1.2
    out = np.empty((NORIENT, NSCALE, hd, wd))
    for o in range(NORIENT):
        a = o * math.pi / 4.0
        ds = sint * math.cos(a) - cost * math.sin(a)
        dc = cost * math.cos(a) + sint * math.sin(a)
        dtheta = np.abs(np.arctan2(ds, dc))
        spread = np.exp(-dtheta ** 2 / (2.0 * sigma ** 2))
        for s in range(NSCALE):
            out[o, s] = log_gabor[s] * spread
    out.setflags(write=False)
    return out


def noise_factor(hd, wd, o):
    """c_o in the file's form: T = c_o sqrt(median)"""
    filt = filters(hd, wd)[o]
    n = hd * wd
    ifa = [np.real(np.fft.ifft2(f)) * math.sqrt(n) for f in filt]
    sum_an2 = sum(float((a * a).sum()) for a in ifa)
    sum_aiaj = sum(float((ifa[i] * ifa[j]).sum()) for i in range(NSCALE) for j in range(i + 1, NSCALE))
    em = float((filt[0] ** 2).sum())
    # EstNoiseEnergy2 = 2 noisePower sumEstSumAn2 + 4 noisePower sumEstSumAiAj, noisePower = (median / ln 2) / EM; tau =
    # sqrt(EstNoiseEnergy2 / 2); T = (tau sqrt(pi / 2) + 2 sqrt((2 - pi / 2) tau^2)) / 1.7
    tau_over_sqrt_med = math.sqrt((2.0 * sum_an2 + 4.0 * sum_aiaj) / (math.log(2.0) * em) / 2.0)
    return tau_over_sqrt_med * (math.sqrt(math.pi / 2.0) + 2.0 * math.sqrt(2.0 - math.pi / 2.0)) / 1.7


@functools.lru_cache(maxsize=8)
def noise_factors(hd, wd):
    return tuple(noise_factor(hd, wd, o) for o in range(NORIENT))


@functools.lru_cache(maxsize=8)
def dft_matrix(n):
    jk = (np.arange(n)[:, None] * np.arange(n)[None, :]) % n
    return np.exp(-2j * math.pi * jk / n)


# ---- phase congruency ---------------------------------------------------------------------------------------------------------
def phase_congruency(y, dense=False, centre=True):
    """PC [hd, wd] of a Y grid.  dense: the transforms as explicit float64 DFT matrix products, W_h X W_w and conj(W_h) . conj(W_w)
    / N; else np.fft.  centre=False skips X = Y - Y(0, 0) (the filters have no DC term: the definition does not change)."""
    y = np.asarray(y, np.float64)
    hd, wd = y.shape
    x = y - y[0, 0] if centre else y
    filt, c = filters(hd, wd), noise_factors(hd, wd)
    if dense:
        wh, ww = dft_matrix(hd), dft_matrix(wd)
        f = wh @ x @ ww
        inv = lambda g: (np.conj(wh) @ g @ np.conj(ww)) / (hd * wd)
    else:
        f = np.fft.fft2(x)
        inv = np.fft.ifft2
    num, den = np.zeros((hd, wd)), np.zeros((hd, wd))
    for o in range(NORIENT):
        eo = [inv(f * filt[o, s]) for s in range(NSCALE)]
        an = sum(np.abs(e) for e in eo)
        se, so = sum(e.real for e in eo), sum(e.imag for e in eo)
        xe = np.sqrt(se * se + so * so) + 1e-4
        me, mo = se / xe, so / xe
        energy = sum((e.real * me + e.imag * mo) - np.abs(e.real * mo - e.imag * me) for e in eo)
        t = c[o] * math.sqrt(float(np.median(np.abs(eo[0]) ** 2)))
        num += np.maximum(energy - t, 0.0)
        den += an
    return np.where(den > 0.0, num / np.where(den > 0.0, den, 1.0), 0.0)


# ---- channels, gradient, similarity ---------------------------------------------------------------------------------------------
def channels(planes, model, depth=8):
    """-> Y, I, Q [hd, wd] float64: colour conversion per pixel, box mean, the channel rows"""
    f = MR.factor(*planes[0].shape)
    r, g, b = (MR.box_sum(c, f) / float(f * f) for c in MR._rgb_float(planes, model, depth))
    y = A_ROWS[0][0] * r + A_ROWS[0][1] * g + A_ROWS[0][2] * b
    if model == "gray":
        return y, np.zeros_like(y), np.zeros_like(y)
    return (y,) + tuple(a[0] * r + a[1] * g + a[2] * b for a in A_ROWS[1:])


def scharr(x):
    """Scharr, zeros outside the grid, in the order include/vqa.h states -> gx, gy"""
    p = np.zeros((x.shape[0] + 2, x.shape[1] + 2), np.float64)
    p[1:-1, 1:-1] = x
    s = lambda dy, dx: p[1 + dy:p.shape[0] - 1 + dy, 1 + dx:p.shape[1] - 1 + dx]
    gx = (((3.0 * s(-1, 1) + 10.0 * s(0, 1)) + 3.0 * s(1, 1)) - ((3.0 * s(-1, -1) + 10.0 * s(0, -1)) + 3.0 * s(1, -1))) / 16.0
    gy = (((3.0 * s(1, -1) + 10.0 * s(1, 0)) + 3.0 * s(1, 1)) - ((3.0 * s(-1, -1) + 10.0 * s(-1, 0)) + 3.0 * s(-1, 1))) / 16.0
    return gx, gy


def similarity(cr, cd, pc_r, pc_d):
    """-> S_L, S_L C from the channels (Y, I, Q) of both images and two PC maps, in the order include/vqa.h states"""
    rx, ry = scharr(cr[0])
    dx, dy = scharr(cd[0])
    qr, qd = rx * rx + ry * ry, dx * dx + dy * dy
    s_g = (2.0 * np.sqrt(qr * qd) + T2) / ((qr + qd) + T2)
    s_pc = (2.0 * (pc_r * pc_d) + T1) / ((pc_r * pc_r + pc_d * pc_d) + T1)
    s_l = s_g * s_pc
    s_i = (2.0 * (cr[1] * cd[1]) + T3) / ((cr[1] * cr[1] + cd[1] * cd[1]) + T3)
    s_q = (2.0 * (cr[2] * cd[2]) + T3) / ((cr[2] * cr[2] + cd[2] * cd[2]) + T3)
    x = s_i * s_q
    c = np.abs(x) ** LAMBDA * np.where(x < 0.0, math.cos(LAMBDA * math.pi), 1.0)
    return s_l, s_l * c


def fsim_float(ref, dist, model, depth=8, dense=False):
    """the definition in float64, nothing quantised -> fsim, fsimc, PC_r, PC_d, S_L, S_L C (P = 0: both scores 1.0)"""
    cr, cd = channels(ref, model, depth), channels(dist, model, depth)
    pc_r, pc_d = phase_congruency(cr[0], dense), phase_congruency(cd[0], dense)
    s_l, s_lc = similarity(cr, cd, pc_r, pc_d)
    pm = np.maximum(pc_r, pc_d)
    tot = float(pm.sum())
    if tot == 0.0:
        return 1.0, 1.0, pc_r, pc_d, s_l, s_lc
    return float((s_l * pm).sum()) / tot, float((s_lc * pm).sum()) / tot, pc_r, pc_d, s_l, s_lc


# ---- the integer pooling --------------------------------------------------------------------------------------------------------
def quantise(pc):
    return np.rint(np.asarray(pc, np.float64) * FIX).astype(np.int64)


def pool_words(ref, dist, model, depth, p_r, p_d):
    """the three words P, A, B (B signed) over GIVEN p maps (int64): PC = p 2^-24, g = rint(S_L 2^24), gc = rint(S_L C 2^24),
    pm = max(p_r, p_d), the sums of pm, (g pm + 2^23) >> 24 and (gc pm + 2^23) >> 24.  Also returns gc's map, for the bound on B."""
    cr, cd = channels_device(ref, model, depth), channels_device(dist, model, depth)
    p_r, p_d = np.asarray(p_r, np.int64), np.asarray(p_d, np.int64)
    s_l, s_lc = similarity(cr, cd, p_r.astype(np.float64) * (1.0 / FIX), p_d.astype(np.float64) * (1.0 / FIX))
    g, gc = np.rint(s_l * FIX).astype(np.int64), np.rint(s_lc * FIX).astype(np.int64)
    pm = np.maximum(p_r, p_d)
    return int(pm.sum()), int(((g * pm + (1 << 23)) >> 24).sum()), int(((gc * pm + (1 << 23)) >> 24).sum())


def scores_of(words):
    p, a, b = words
    return (1.0, 1.0) if p == 0 else (float(a) / float(p), float(b) / float(p))


def matrix(model, depth, f):
    """the twelve doubles of include/vqa.h: mat[Y, I, Q][plane 0, 1, 2, count]; GRAY zeroes the rows of I and Q"""
    s, peak = float(1 << (depth - 8)), float((1 << depth) - 1)
    rgb = [[0.0] * 4 for _ in range(3)]
    o0 = o1 = 0.0
    if model == "bgr":
        k = 255.0 / peak
        rgb[0][2] = k; rgb[1][1] = k; rgb[2][0] = k
    else:
        ky, kc = 255.0 / (219.0 * s), (0.0 if model == "gray" else 255.0 / (224.0 * s))
        rgb[0][0] = ky; rgb[0][2] = 1.5748 * kc
        rgb[1][0] = ky; rgb[1][1] = -0.1873 * kc; rgb[1][2] = -0.4681 * kc
        rgb[2][0] = ky; rgb[2][1] = 1.8556 * kc
        o0, o1 = 16.0 * s, 128.0 * s
    for c in range(3):
        rgb[c][3] = -((o0 * rgb[c][0] + o1 * rgb[c][1]) + o1 * rgb[c][2])
    ff = float(f) * float(f)
    m = [[((a[0] * rgb[0][j] + a[1] * rgb[1][j]) + a[2] * rgb[2][j]) / ff for j in range(4)] for a in A_ROWS]
    if model == "gray":
        m[1], m[2] = [0.0] * 4, [0.0] * 4
    return m


def channels_device(planes, model, depth=8):
    """Y, I, Q in the device's form: integer box sums and the 3 x 4 matrix"""
    h, w = planes[0].shape
    f = MR.factor(h, w)
    full = [planes[0].astype(np.int64)] + [MR.replicate(p, h, w).astype(np.int64) for p in planes[1:]]
    while len(full) < 3:
        full.append(np.zeros((h, w), np.int64))
    s0, s1, s2 = (MR.box_sum(p, f).astype(np.float64) for p in full)
    cnt = MR.box_sum(np.ones((h, w), np.int64), f).astype(np.float64)
    return tuple(((m[0] * s0 + m[1] * s1) + m[2] * s2) + m[3] * cnt for m in matrix(model, depth, f))


def derived_bar(pc_r, pc_d):
    """What may separate the integer pooling from the float pooling on THIS pair of PC maps, 4 N 2^-24 / sum PC_m: p moves a
    sample's PC by at most 2^-25, which moves S_PC by less than 2^-24 (its derivative in either PC is below 2 / 0.85 ... times
    2^-25) and PC_m by 2^-25; g and gc add 2^-25 each and the >> 24 another 2^-25 of a sample's term; a ratio of sums whose
    numerator and denominator terms each move by at most 2 * 2^-24 (S_L, C <= 1) moves by at most 4 N 2^-24 / sum PC_m."""
    pm = np.maximum(pc_r, pc_d)
    tot = float(pm.sum())
    return math.inf if tot == 0.0 else 4.0 * pm.size * 2.0 ** -24 / tot
