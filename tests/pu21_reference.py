"""PU21-PSNR and PU21-SSIM (Mantiuk and Azimi, PCS 2021, the banding_glare fit), restated in NumPy from the definition in
include/vqa.h (vqa_pu21_submit), not from the kernels: the three planes of a pixel -> R'G'B' clamped to [0, 1] -> display light
(itp_reference's chain, which states the same text) -> luminance -> the PU21 encoding V -> PSNR and Gaussian SSIM on V.

  encode(L)                               V on arrays, float64
  light / channels(planes, ..)            a frame given as (Y, Cb, Cr) or (B, G, R) integer planes -> display light; V of Y, R, G, B
  record(ref, dist, ..)                   the UNQUANTISED float64 form: mse_y, mse_rgb, pu_psnr, pu_psnr_rgb, pu_ssim
  quantise(v), sse_words, ssim_word, finalize, record_q
                                          the QUANTISED form: q = rint(V 2^16) once, then everything in Python integers and
                                          doubles in the order the header states: the two-word sums of the squared differences,
                                          the separable Gaussian moments on x = q / 2^16, u = rint(ssim 2^24), the 128-bit join.
"""
import numpy as np

import itp_reference as IR

MIN_DIM = 16
FIX = 2.0 ** 16             # q = rint(V 2^16)
SSIM_FIX = 2.0 ** 24        # u = rint(ssim 2^24)
PEAK = 256.0
P = (0.353487901, 0.3734658629, 8.277049286e-05, 0.9062562627, 0.09150303166, 0.9099517204, 596.3148142)
L_MIN, L_MAX = 0.005, 10000.0
C1, C2 = (0.01 * 256.0) * (0.01 * 256.0), (0.03 * 256.0) * (0.03 * 256.0)
YUV2020, BGR, PQ, HLG = IR.YUV2020, IR.BGR, IR.PQ, IR.HLG
TILE = 16                   # k_pu21_ssim's tile of windows (a fact of the kernel that the tests' sizes follow)
# the bar of pu_ssim, quantised (or the GPU's) against unquantised: see DESIGN.md 4s.  It is MEASURED, not derived: over the case
# grid of pu21_cases.matrix() on the CPU (test_pu21_host.py prints the figure) the largest gap is 1.40e-6, on the 16 x 16 darkstep
# case under HLG.  There the frames are flat at a and b of a few tenths of a PU unit, the luminance term is
# 1 - (a - b)^2 / (a^2 + b^2 + C1), and one rounding of 2^-16 on a - b = 0.3 moves it by 2 * 0.3 * 2^-16 / 6.55 = 1.4e-6: the
# quantisation of q, not the 2^-24 quantum of u (2^-25 on a mean), sets the figure.  The bar is four times the measured gap.
SSIM_BAR = 5.6e-6


def encode(l):
    """cd/m2 -> PU21 units"""
    l = np.clip(np.asarray(l, np.float64), L_MIN, L_MAX)
    lp = np.power(l, P[3])
    return np.maximum(P[6] * (np.power((P[0] + P[1] * lp) / (1.0 + P[2] * lp), P[4]) - P[5]), 0.0)


def light(planes, depth=8, model=YUV2020, transfer=PQ, full_range=False):
    """three integer planes -> display light R, G, B in cd/m2 on the luma grid"""
    if len(planes) != 3:
        raise ValueError("pu21 needs three planes")
    h, w = np.asarray(planes[0]).shape
    if h < MIN_DIM or w < MIN_DIM:
        raise ValueError("frames below %d x %d are not measured" % (MIN_DIM, MIN_DIM))
    a = [np.asarray(planes[0], np.int64)] + [IR.replicate(np.asarray(p, np.int64), h, w) for p in planes[1:]]
    if model == YUV2020:
        r, g, b = IR.rgb_from_yuv(*a, depth=depth, full_range=full_range)
    else:
        peak = float((1 << depth) - 1)
        b, g, r = (x.astype(np.float64) / peak for x in a)
    r, g, b = (np.clip(x, 0.0, 1.0) for x in (r, g, b))
    if transfer == PQ:
        return tuple(IR.pq_eotf(x) for x in (r, g, b))
    if transfer == HLG:
        return IR.hlg_display(r, g, b)
    raise ValueError("transfer")


def channels(planes, depth=8, model=YUV2020, transfer=PQ, full_range=False):
    """-> V of the luminance and of the three display-light channels: (vy, vr, vg, vb), float64 [h, w]"""
    r, g, b = light(planes, depth, model, transfer, full_range)
    y = (IR.KR * r + IR.KG * g) + IR.KB * b
    return tuple(encode(x) for x in (y, r, g, b))


def window():
    e = [float(np.exp(-float((i - 5) * (i - 5)) / 4.5)) for i in range(11)]
    s = 0.0
    for x in e:
        s += x
    return [x / s for x in e]


def filt(v):
    """the 11 x 11 Gaussian over the valid part, separable, horizontal then vertical, each a sum in the order i = 0 .. 10"""
    g = window()
    v = np.asarray(v, np.float64)
    h, w = v.shape
    s = np.zeros((h, w - 10))
    for j in range(11):
        s = s + g[j] * v[:, j:j + w - 10]
    o = np.zeros((h - 10, w - 10))
    for i in range(11):
        o = o + g[i] * s[i:i + h - 10, :]
    return o


def ssim_map(xr, xd):
    """the value of every valid window, float64 [h - 10, w - 10]"""
    xr, xd = np.asarray(xr, np.float64), np.asarray(xd, np.float64)
    mu_r, mu_d = filt(xr), filt(xd)
    var_r, var_d, cov = filt(xr * xr) - mu_r * mu_r, filt(xd * xd) - mu_d * mu_d, filt(xr * xd) - mu_r * mu_d
    num = (2.0 * (mu_r * mu_d) + C1) * (2.0 * cov + C2)
    den = ((mu_r * mu_r + mu_d * mu_d) + C1) * ((var_r + var_d) + C2)
    return num / den


def psnr(mse):
    return float("inf") if mse == 0 else float(10.0 * np.log10(PEAK * PEAK / mse))


def record(ref, dist, depth=8, model=YUV2020, transfer=PQ, full_range=False):
    """one frame pair, UNQUANTISED -> dict"""
    a, b = channels(ref, depth, model, transfer, full_range), channels(dist, depth, model, transfer, full_range)
    mse_y = float(np.mean((a[0] - b[0]) ** 2))
    mse_rgb = float(np.mean(np.stack([(a[k] - b[k]) ** 2 for k in (1, 2, 3)])))
    return {"mse_y": mse_y, "mse_rgb": mse_rgb, "pu_psnr": psnr(mse_y), "pu_psnr_rgb": psnr(mse_rgb),
            "pu_ssim": float(np.mean(ssim_map(a[0], b[0])))}


# ---- the quantised form ----------------------------------------------------------------------------------------------------
def quantise(v):
    return np.rint(np.asarray(v, np.float64) * FIX).astype(np.int64)


def sse_words(qa, qb):
    """integer arrays (any shape) -> (lo, hi): the sums of the low 32 bits and of the bits above them of every squared difference"""
    d = np.asarray(qa, np.int64) - np.asarray(qb, np.int64)
    t = (d * d).reshape(-1)                       # below 2^52
    return int((t & 0xffffffff).sum(dtype=np.uint64)), int((t >> 32).sum(dtype=np.uint64))


def join(lo, hi):
    return (int(hi) << 32) + int(lo)


def u_map(qy_r, qy_d):
    x_r, x_d = np.asarray(qy_r, np.int64).astype(np.float64) / FIX, np.asarray(qy_d, np.int64).astype(np.float64) / FIX
    return np.rint(ssim_map(x_r, x_d) * SSIM_FIX).astype(np.int64)


def ssim_word(qy_r, qy_d):
    """the two q_Y maps -> the signed sum of u = rint(ssim 2^24) over the valid windows"""
    return int(u_map(qy_r, qy_d).sum())


def finalize(words, h, w):
    """(sse_y_lo, sse_y_hi, sse_rgb_lo, sse_rgb_hi, ssim_q) -> the record as vqa_pu21_wait forms it"""
    sy, sc = join(words[0], words[1]), join(words[2], words[3])
    windows = (h - 10) * (w - 10)
    hw = float(h) * float(w)
    mse_y, mse_rgb = float(sy) / (4294967296.0 * hw), float(sc) / (4294967296.0 * (3.0 * hw))
    return {"sse_y_lo": int(words[0]), "sse_y_hi": int(words[1]), "sse_rgb_lo": int(words[2]), "sse_rgb_hi": int(words[3]),
            "ssim_q": int(words[4]), "windows": windows, "mse_y": mse_y, "mse_rgb": mse_rgb, "pu_psnr": psnr(mse_y),
            "pu_psnr_rgb": psnr(mse_rgb), "pu_ssim": float(words[4]) / (SSIM_FIX * float(windows))}


def record_q(ref, dist, depth=8, model=YUV2020, transfer=PQ, full_range=False):
    """one frame pair, QUANTISED -> (record dict, q_Y of ref, q_Y of dist)"""
    a = [quantise(v) for v in channels(ref, depth, model, transfer, full_range)]
    b = [quantise(v) for v in channels(dist, depth, model, transfer, full_range)]
    h, w = a[0].shape
    y = sse_words(a[0], b[0])
    c = sse_words(np.stack(a[1:]), np.stack(b[1:]))
    return finalize(y + c + (ssim_word(a[0], b[0]),), h, w), a[0], b[0]


split_planes = IR.split_planes
