"""CPU reference for ADM (detail loss metric, Li et al. 2011, on a four-level db2 wavelet pyramid) - the adm2 and adm_scale0..3
features of VMAF - written from the definition (include/vqa.h, vqa_adm_submit), not from the kernels.  float64 by default; the
`dtype` argument runs the same statement in float32 (what the device computes in, up to the order of its sums).

  samples      x = R / 2^(depth-8) - 128,  y = D / 2^(depth-8) - 128
  DWT          H x W -> four bands of ceil(H/2) x ceil(W/2); output i reads inputs |2i-1|, 2i, 2i+1, 2i+2 with taps 0..3 of LO / HI,
               an index k >= n reads 2n - k - 1; vertical pass first (L, Hh), then a = lo(L), v = hi(L), h = lo(Hh), d = hi(Hh);
               scale s+1 is the DWT of the a band of scale s
  decoupling   per band k = clamp(t / (o + 1e-30), 0, 1), r = k o;  dp = oh th + ov tv;
               flag = dp >= 0 and dp^2 >= cos^2(1 deg) (oh^2 + ov^2)(th^2 + tv^2);
               flag and r > 0: r = min(100 r, t);  flag and r < 0: r = max(100 r, t);  a_band = t - r
  CSF          rf_s[h] = rf_s[v] = 1 / Q(s, 1), rf_s[d] = 1 / Q(s, 2)
  masking      thr = sum_bands [ |rf a_band| / 15 + sum over the 8 neighbours of |rf a_band| / 30 ]; neighbour -1 reads 1, n reads n-1
  region       left = int(bw 0.1 - 0.5), top = int(bh 0.1 - 0.5); rows [top, bh - top), columns [left, bw - left)
  pooling      num_s = sum_bands [ cbrt(sum_region max(|rf r| - thr, 0)^3) + cbrt(area / 32) ]
               den_s = sum_bands [ cbrt(sum_region |rf o|^3) + cbrt(area / 32) ]
  results      scale_s = num_s / den_s;  adm2 = N / D, N = sum num_s, D = sum den_s, each 0 below 1e-10 h w / (1920 1080); 1 when D = 0
"""
import numpy as np

LEVELS = 4
MIN_DIM = 16
LO = (0.482962913144690, 0.836516303737469, 0.224143868041857, -0.129409522550921)
HI = (-0.129409522550921, -0.224143868041857, 0.836516303737469, -0.482962913144690)
GAIN_LIMIT = 100.0
COS2_1DEG = np.cos(np.pi / 180.0) ** 2
AMP = ((0.62171, 0.67234, 0.72709, 0.67234), (0.34537, 0.41317, 0.49428, 0.41317),
       (0.18004, 0.22727, 0.28688, 0.22727), (0.091401, 0.11792, 0.15214, 0.11792))
ORIENT_GAIN = (1.501, 1.0, 0.534, 1.0)


def csf_q(lam, theta):
    rho = 3.0 * 1080.0 * np.pi / 180.0
    return 2.0 * 0.495 * 10.0 ** (0.466 * np.log10((2.0 ** (lam + 1)) * 0.401 * ORIENT_GAIN[theta] / rho) ** 2) / AMP[lam][theta]


def rf(s):
    """-> (rf[h] = rf[v], rf[d]) of scale s"""
    return 1.0 / csf_q(s, 1), 1.0 / csf_q(s, 2)


def dwt_index(i, n):
    """the four input indices output i of a length-n pass reads, in tap order"""
    return [(k if k < n else 2 * n - k - 1) for k in (abs(2 * i - 1), 2 * i, 2 * i + 1, 2 * i + 2)]


def _pass(x, taps, axis):
    n = x.shape[axis]
    idx = np.array([dwt_index(i, n) for i in range((n + 1) // 2)])   # [out, 4]
    out = None
    for k in range(4):
        term = x.dtype.type(taps[k]) * np.take(x, idx[:, k], axis=axis)
        out = term if out is None else out + term
    return out


def dwt(x):
    """-> (a, v, h, d) of one level"""
    L, Hh = _pass(x, LO, 0), _pass(x, HI, 0)
    return _pass(L, LO, 1), _pass(L, HI, 1), _pass(Hh, LO, 1), _pass(Hh, HI, 1)


def level_dims(h, w):
    """band dims of scales 0..3"""
    out = []
    for _ in range(LEVELS):
        h, w = (h + 1) // 2, (w + 1) // 2
        out.append((h, w))
    return out


def region(bh, bw):
    """-> (top, bottom, left, right, area)"""
    left, top = int(bw * 0.1 - 0.5), int(bh * 0.1 - 0.5)
    return top, bh - top, left, bw - left, (bh - 2 * top) * (bw - 2 * left)


def border_index(i, n):
    """the neighbour an index outside [0, n) reads (VIF's border rule)"""
    if i < 0:
        i = -i
    if i >= n:
        i = 2 * n - i - 1
    return i


def _neighbour_sum(m):
    """(1/15) m + (1/30) sum of the 8 neighbours"""
    bh, bw = m.shape
    ry = np.array([border_index(i, bh) for i in range(-1, bh + 1)])
    rx = np.array([border_index(i, bw) for i in range(-1, bw + 1)])
    e = m[ry][:, rx]
    t = m.dtype.type
    nb = None
    for dy in range(3):
        for dx in range(3):
            if dy == 1 and dx == 1:
                continue
            term = e[dy:dy + bh, dx:dx + bw]
            nb = term if nb is None else nb + term
    return m * t(1.0 / 15.0) + nb * t(1.0 / 30.0)


def decouple(o, t, margin=0.0):
    """o, t: (h, v, d) bands of ref and dist -> (r [3] before the flag is applied, flag map, unsure map)
    unsure (margin > 0): the samples whose flag changes when dp and the two magnitudes move by a relative `margin`"""
    ty = o[0].dtype.type
    r = []
    for ob, tb in zip(o, t):
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            k = np.clip(tb / (ob + ty(1e-30)), ty(0), ty(1))
        r.append(k * ob)
    dp = o[0] * t[0] + o[1] * t[1]
    om, tm = o[0] * o[0] + o[1] * o[1], t[0] * t[0] + t[1] * t[1]
    lhs, rhs = dp * dp, ty(COS2_1DEG) * om * tm
    flag = (dp >= 0) & (lhs >= rhs)
    unsure = np.zeros(flag.shape, bool)
    if margin:
        e = (1.0 + margin) ** 2   # dp enters squared, the two magnitudes once each
        unsure = ((dp >= 0) & (lhs * e >= rhs / e)) != ((dp >= 0) & (lhs / e >= rhs * e))
    return r, flag, unsure


def _apply_flag(r, t, flag):
    ty = r[0].dtype.type
    out = []
    for rb, tb in zip(r, t):
        up = np.minimum(rb * ty(GAIN_LIMIT), tb)
        dn = np.maximum(rb * ty(GAIN_LIMIT), tb)
        out.append(np.where(flag & (rb > 0), up, np.where(flag & (rb < 0), dn, rb)))
    return out


def scale_sums(o, t, s, flag_override=None, margin=0.0):
    """one scale from its (h, v, d) bands -> (num, den, unsure count)"""
    ty = o[0].dtype.type
    rfs = rf(s)
    w = (ty(rfs[0]), ty(rfs[0]), ty(rfs[1]))
    r, flag, unsure = decouple(o, t, margin)
    if flag_override is not None:
        flag = np.where(unsure, flag_override, flag)
    r = _apply_flag(r, t, flag)
    m = None
    for b in range(3):
        term = np.abs(w[b] * (t[b] - r[b]))
        m = term if m is None else m + term
    thr = _neighbour_sum(m)
    bh, bw = o[0].shape
    top, bottom, left, right, area = region(bh, bw)
    c = np.cbrt(area / 32.0)
    num = den = 0.0
    for b in range(3):
        x = np.maximum(np.abs(w[b] * r[b]) - thr, ty(0))[top:bottom, left:right]
        y = np.abs(w[b] * o[b])[top:bottom, left:right]
        num += np.cbrt(float(np.sum((x * x * x).astype(np.float64)))) + c
        den += np.cbrt(float(np.sum((y * y * y).astype(np.float64)))) + c
    return num, den, int(unsure[top:bottom, left:right].sum())


def adm(ref, dist, depth=8, dtype=np.float64, margin=0.0):
    """-> (num [4], den [4], scale [4], adm2) of one plane pair (integer arrays of `depth` bits).
    margin > 0: -> also (unsure [5], lo [5], hi [5]): per scale the count of region samples whose angle test flips when dp and the
    two magnitudes move by a relative `margin`, and the smallest / largest scale value among: as computed, those samples' flags
    all forced off, all forced on.  Entry 4 is adm2 (its count is the total)."""
    ref, dist = np.asarray(ref), np.asarray(dist)
    if ref.shape != dist.shape or ref.ndim != 2:
        raise ValueError("two planes of one shape")
    if min(ref.shape) < MIN_DIM:
        raise ValueError("ADM on four scales needs planes of at least %d x %d" % (MIN_DIM, MIN_DIM))
    ty = np.dtype(dtype).type
    sc = ty(1 << (depth - 8))
    x, y = ref.astype(dtype) / sc - ty(128), dist.astype(dtype) / sc - ty(128)
    num, den = np.zeros(LEVELS), np.zeros(LEVELS)
    unsure, lo, hi = np.zeros(LEVELS + 1, int), np.zeros(LEVELS + 1), np.zeros(LEVELS + 1)
    forced = np.zeros((2, 2, LEVELS))   # [off, on][num, den][scale]
    for s in range(LEVELS):
        xa, xv, xh, xd = dwt(x)
        ya, yv, yh, yd = dwt(y)
        o, t = (xh, xv, xd), (yh, yv, yd)
        num[s], den[s], unsure[s] = scale_sums(o, t, s, margin=margin)
        if margin:
            a = [scale_sums(o, t, s, flag_override=f, margin=margin) for f in (False, True)]
            v = [n / d for n, d, _ in a] + [num[s] / den[s]]
            lo[s], hi[s] = min(v), max(v)
            forced[:, :, s] = [[n, d] for n, d, _ in a]
        x, y = xa, ya
    scale = num / den
    h, w = ref.shape
    floor = 1e-10 * h * w / (1920.0 * 1080.0)
    N, D = num.sum(), den.sum()
    N, D = (0.0 if N < floor else N), (0.0 if D < floor else D)
    adm2 = 1.0 if D == 0 else N / D
    if margin:
        v = [adm2] + [forced[k, 0].sum() / forced[k, 1].sum() for k in (0, 1)]
        unsure[LEVELS], lo[LEVELS], hi[LEVELS] = unsure[:LEVELS].sum(), min(v), max(v)
        return num, den, scale, adm2, unsure, lo, hi
    return num, den, scale, adm2
