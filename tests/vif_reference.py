"""CPU reference for VIF (visual information fidelity, Sheikh & Bovik 2006, pixel domain) on four scales - the vif_scale0..3
features of VMAF - float64, written from the definition (include/vqa.h, vqa_vif_submit), not from the kernels:

  samples      x = R / 2^(depth-8) - 128,  y = D / 2^(depth-8) - 128
  filter s     n = 2^(4-s) + 1 taps (17, 9, 5, 3),  t[k] = exp(-(k - n//2)^2 / (2 (n/5)^2)) / sum;  columns first, then rows
  borders      index i < 0 reads -i;  index i >= n reads 2n - i - 1;  every level keeps its full size
  level s > 0  level s-1 filtered with the filter of scale s, even rows and even columns kept: dims floor(dim / 2)
  per level    mu1 = F(x), mu2 = F(y), s1 = max(F(xx) - mu1^2, 0), s2 = max(F(yy) - mu2^2, 0), s12 = F(xy) - mu1 mu2
  per sample   (eps 1e-10, nsq 2, smi 4 / 255^2)   g = s12 / (s1 + eps);  sv = s2 - g s12;
               s1 < eps: g = 0, sv = s2, s1 = 0;   s2 < eps: g = 0, sv = 0;   g < 0: sv = s2, g = 0;
               sv = max(sv, eps);  g = min(g, 100);
               num = log2(1 + g^2 s1 / (sv + nsq)),  den = log2(1 + s1 / nsq);   s12 < 0: num = 0;
               s1 < nsq: num = 1 - s2 smi, den = 1
  results      num_s = sum num, den_s = sum den, scale_s = num_s / den_s (1 when den_s = 0), vif = sum num_s / sum den_s
"""
import numpy as np

LEVELS = 4
MIN_DIM = 16
EPS, NSQ, SMI, GAIN_LIMIT = 1e-10, 2.0, 4.0 / (255.0 * 255.0), 100.0


def taps(s, dtype=np.float64):
    n = (1 << (4 - s)) + 1
    k = np.arange(n, dtype=np.float64) - n // 2
    g = np.exp(-(k * k) / (2.0 * (n / 5.0) ** 2))
    return (g / g.sum()).astype(dtype)


def border_index(i, n):
    """the sample an index outside [0, n) reads"""
    if i < 0:
        return -i
    if i >= n:
        return 2 * n - i - 1
    return i


def _gather(n, r):
    return np.array([border_index(i, n) for i in range(-r, n + r)])


def filt(x, t):
    """separable filter of a plane in its own type, same size: columns (vertical pass) first, then rows"""
    r = len(t) // 2
    h, w = x.shape
    xv = x[_gather(h, r), :]
    v = np.zeros_like(x)
    for k in range(len(t)):
        v = v + t[k] * xv[k:k + h, :]
    vh = v[:, _gather(w, r)]
    out = np.zeros_like(x)
    for k in range(len(t)):
        out = out + t[k] * vh[:, k:k + w]
    return out


def next_level(x, s):
    """level s from level s - 1"""
    h, w = x.shape
    return filt(x, taps(s, x.dtype))[0:2 * (h // 2):2, 0:2 * (w // 2):2]


def statistic(x, y, s):
    """-> (num map, den map) of one level, in the type of x"""
    ty = x.dtype.type
    eps, nsq, smi, zero, one = ty(EPS), ty(NSQ), ty(SMI), ty(0), ty(1)
    t = taps(s, x.dtype)
    mu1, mu2 = filt(x, t), filt(y, t)
    s1 = np.maximum(filt(x * x, t) - mu1 * mu1, zero)
    s2 = np.maximum(filt(y * y, t) - mu2 * mu2, zero)
    s12 = filt(x * y, t) - mu1 * mu2
    g = s12 / (s1 + eps)
    sv = s2 - g * s12
    c = s1 < eps
    g, sv, s1 = np.where(c, zero, g), np.where(c, s2, sv), np.where(c, zero, s1)
    c = s2 < eps
    g, sv = np.where(c, zero, g), np.where(c, zero, sv)
    c = g < 0
    sv, g = np.where(c, s2, sv), np.where(c, zero, g)
    sv = np.maximum(sv, eps)
    g = np.minimum(g, ty(GAIN_LIMIT))
    num = np.log2(one + g * g * s1 / (sv + nsq))
    den = np.log2(one + s1 / nsq)
    num = np.where(s12 < 0, zero, num)
    c = s1 < nsq
    num, den = np.where(c, one - s2 * smi, num), np.where(c, one, den)
    return num, den


def vif(ref, dist, depth=8, dtype=np.float64):
    """-> (num [4], den [4], scale [4], vif) of one plane pair (integer arrays of `depth` bits); dtype float32: the same
    statements in that type (the maps; their sums are taken in float64)"""
    ref, dist = np.asarray(ref), np.asarray(dist)
    if ref.shape != dist.shape or ref.ndim != 2:
        raise ValueError("two planes of one shape")
    if min(ref.shape) < MIN_DIM:
        raise ValueError("VIF on four scales needs planes of at least %d x %d" % (MIN_DIM, MIN_DIM))
    ty = np.dtype(dtype).type
    sc = ty(1 << (depth - 8))
    x, y = ref.astype(dtype) / sc - ty(128), dist.astype(dtype) / sc - ty(128)
    num, den = np.zeros(LEVELS), np.zeros(LEVELS)
    for s in range(LEVELS):
        if s:
            x, y = next_level(x, s), next_level(y, s)
        n, d = statistic(x, y, s)
        num[s], den[s] = n.sum(dtype=np.float64), d.sum(dtype=np.float64)
    scale = np.where(den == 0, 1.0, num / np.where(den == 0, 1.0, den))
    total = den.sum()
    return num, den, scale, (num.sum() / total if total else 1.0)


def level_dims(h, w):
    out = [(h, w)]
    for _ in range(LEVELS - 1):
        h, w = h // 2, w // 2
        out.append((h, w))
    return out
