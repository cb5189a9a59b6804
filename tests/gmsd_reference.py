"""GMSD (Xue, Zhang, Mou, Bovik 2014) restated in float64 NumPy from the definition in include/vqa.h, step by step, plus the
integer form of the pooling the device uses (u = rint(gms 2^24), exact sums, a 128-bit-wide variance numerator - Python integers
here).  Nothing of the package is imported: this file is the reference the kernel is compared with."""
import math

import numpy as np

MIN_DIM = 16
FIX = 1 << 24
T8 = 170.0


def downsample(x):
    """the 2x2 mean at step 2 with zeros outside the plane: D [ceil(h/2), ceil(w/2)] float64 (S = 4 D is an exact integer)"""
    x = np.asarray(x).astype(np.float64)
    h, w = x.shape
    p = np.zeros((h + (h & 1), w + (w & 1)))
    p[:h, :w] = x
    return (p[0::2, 0::2] + p[1::2, 0::2] + p[0::2, 1::2] + p[1::2, 1::2]) / 4.0


def prewitt(D):
    """-> (gx, gy) at every sample of D, D = 0 outside (conv2 'same': a zero fill, not a clamp)"""
    h, w = D.shape
    p = np.zeros((h + 2, w + 2))
    p[1:-1, 1:-1] = D
    gx = (p[0:h, 2:] + p[1:h + 1, 2:] + p[2:, 2:] - p[0:h, 0:w] - p[1:h + 1, 0:w] - p[2:, 0:w]) / 3.0
    gy = (p[2:, 0:w] + p[2:, 1:w + 1] + p[2:, 2:] - p[0:h, 0:w] - p[0:h, 1:w + 1] - p[0:h, 2:]) / 3.0
    return gx, gy


def grad_sq(D):
    """m^2 = gx^2 + gy^2 = q / 144"""
    gx, gy = prewitt(D)
    return gx * gx + gy * gy


def threshold(depth):
    """T = 170 (peak / 255)^2"""
    k = ((1 << depth) - 1) / 255.0
    return T8 * (k * k)


def gms_map(r, d, depth=8):
    """the similarity map over the downsampled grid, float64, unquantised"""
    mr2, md2 = grad_sq(downsample(r)), grad_sq(downsample(d))
    T = threshold(depth)
    return (2.0 * np.sqrt(mr2) * np.sqrt(md2) + T) / (mr2 + md2 + T)


def pool(g):
    """-> (gmsd, gms_mean): the standard deviation with divisor N - 1 (MATLAB's std2) and the mean"""
    g = np.asarray(g, np.float64).reshape(-1)
    return float(np.std(g, ddof=1)), float(np.mean(g))


def gmsd(r, d, depth=8):
    """-> (gmsd, gms_mean) of one plane pair in float64, unquantised"""
    return pool(gms_map(r, d, depth))


def words(g):
    """the three integer words of a similarity map: (sum u, sum u^2 low, sum u^2 high) with u = rint(g 2^24) - as ONE split of
    the total (the device splits per workgroup; hi 2^32 + lo is the same integer)"""
    u = [int(v) for v in np.rint(np.asarray(g, np.float64).reshape(-1) * FIX)]
    su, su2 = sum(u), sum(v * v for v in u)
    return su, su2 & 0xffffffff, su2 >> 32


def pool_words(su, lo, hi, n):
    """the host's formulas of include/vqa.h on the three words: -> (gmsd, gms_mean)"""
    s2 = (hi << 32) + lo
    num = n * s2 - su * su
    assert num >= 0
    return math.sqrt(num / (n * (n - 1))) / FIX, su / (n * FIX)


def gmsd_fixed(r, d, depth=8):
    """-> (gmsd, gms_mean, (sum u, sum u^2)) through the integer form"""
    g = gms_map(r, d, depth)
    su, lo, hi = words(g)
    a, b = pool_words(su, lo, hi, g.size)
    return a, b, (su, (hi << 32) + lo)
