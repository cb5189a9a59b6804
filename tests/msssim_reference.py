"""CPU reference for multi-scale SSIM (Wang, Simoncelli, Bovik 2003) in the 2x2-mean form of tf.image.ssim_multiscale and
pytorch-msssim, float64, written from the definition (include/vqa.h, VQA_SSIM_MS), not from the kernels:

  level 0      the plane's samples as they are
  level s + 1  L[s+1][i][j] = 1/4 sum_{di,dj in {0,1}} L[s][min(2i + di, h_s - 1)][min(2j + dj, w_s - 1)]: an odd level is
               padded by duplicating its last row / column, then every 2x2 block is averaged; dims ceil(dim / 2); the means
               are never rounded (they are dyadic rationals of depth + 2 s bits: exact in float64)
  window       hbd_reference's: 11x11 Gaussian, sigma 1.5, C1 = (.01 L)^2, C2 = (.03 L)^2, population covariances, valid region
  per sample   l = (2 mx my + C1) / (mx^2 + my^2 + C1),  cs = (2 sxy + C2) / (sx^2 + sy^2 + C2),  ssim = l cs
  per level    cs_s = mean cs map,  ssim_s = mean ssim map
  MS-SSIM      prod_{s<4} max(cs_s, 0)^w_s * max(ssim_4, 0)^w_4,  w = WEIGHTS (a negative mean gives 0, not NaN)
"""
import numpy as np

import hbd_reference as R

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
LEVELS = 5
MIN_DIM = 161   # 161 -> 81 -> 41 -> 21 -> 11: level 4 still holds a window


def downsample(x):
    """one pyramid step on a float64 plane"""
    h, w = x.shape
    if h & 1:
        x = np.concatenate([x, x[-1:, :]], axis=0)
    if w & 1:
        x = np.concatenate([x, x[:, -1:]], axis=1)
    return 0.25 * (x[0::2, 0::2] + x[0::2, 1::2] + x[1::2, 0::2] + x[1::2, 1::2])


def pyramid(a):
    """the five levels of a plane (any integer or float array), float64"""
    lv = [np.asarray(a, np.float64)]
    for _ in range(LEVELS - 1):
        lv.append(downsample(lv[-1]))
    return lv


def window_means(x, y, data_range):
    """-> (mean cs map, mean ssim map) of one level (float64 planes)"""
    mx, my = R._filt(x), R._filt(y)
    sxx = R._filt(x * x) - mx * mx
    syy = R._filt(y * y) - my * my
    sxy = R._filt(x * y) - mx * my
    C1, C2 = (.01 * data_range) ** 2, (.03 * data_range) ** 2
    lum = (2 * mx * my + C1) / (mx * mx + my * my + C1)
    cs = (2 * sxy + C2) / (sxx + syy + C2)
    return float(cs.mean()), float((lum * cs).mean())


def combine(cs, ssim):
    """the clamped product of the definition from the ten per-level means"""
    v = 1.0
    for s in range(LEVELS):
        x = float(cs[s] if s < LEVELS - 1 else ssim[s])
        v *= x ** WEIGHTS[s] if x > 0.0 else 0.0
    return v


def terms(cs, ssim):
    """the five clamped per-level terms v_s the product is made of (before the exponents)"""
    return [max(float(cs[s] if s < LEVELS - 1 else ssim[s]), 0.0) for s in range(LEVELS)]


def msssim(a, b, data_range):
    """-> (cs [5], ssim [5], MS-SSIM) of a plane pair"""
    if min(a.shape) < MIN_DIM:
        raise ValueError("multi-scale SSIM needs planes of at least %d x %d" % (MIN_DIM, MIN_DIM))
    cs, ssim = [], []
    for x, y in zip(pyramid(a), pyramid(b)):
        c, s = window_means(x, y, data_range)
        cs.append(c)
        ssim.append(s)
    return np.array(cs), np.array(ssim), combine(cs, ssim)


def frame_msssim(ref, dist, planes, depth):
    """-> (sse list, cs [p,5], ssim [p,5], MS-SSIM [p]) for the planes of one frame pair (flat uint8 / uint16 arrays)"""
    mx = (1 << depth) - 1
    sse, cs, ssim, ms = [], [], [], []
    for p in planes:
        a, b = R.plane(ref, p), R.plane(dist, p)
        sse.append(R.sse(a, b))
        c, s, m = msssim(a, b, mx)
        cs.append(c)
        ssim.append(s)
        ms.append(m)
    return sse, np.array(cs), np.array(ssim), np.array(ms)


def value_bound(cs, ssim, bar=1e-4):
    """What |MS - MS_ref| may be when every per-level mean is within `bar` of the reference's: first order
    sum_s w_s MS / v_s * bar, doubled for the second-order term.  None when a term is within ten bars of the clamp."""
    v = terms(cs, ssim)
    if min(v) < 10 * bar:
        return None
    ms = combine(cs, ssim)
    return 2 * bar * sum(w * ms / t for w, t in zip(WEIGHTS, v))
