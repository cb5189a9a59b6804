"""CIEDE2000 (CIE 142-2001; Sharma, Wu and Dalal 2005), restated in NumPy from the definition in include/vqa.h
(vqa_ciede_submit), not from the kernel: the three planes of a pixel -> CIELAB -> dE00, no clamping anywhere.

  de00(lab1, lab2, weights, dtype)      the difference formula on Lab arrays [.., 3]
  lab_from_yuv / lab_from_bgr           the two colour models on integer samples
  frame(planes, ..) / de_mean(..)       a whole frame pair given as (Y, U, V) or (B, G, R) integer planes
dtype=np.float64 is the text as it stands.  dtype=np.float32 evaluates every step in float32 (NumPy's own libm, not the
kernel's): its gap to the float64 run is what fp32 costs, and decides which contents enter the GPU matrix.
"""
import numpy as np

MIN_DIM = 16
FIX = 2.0 ** 20            # a pixel's dE00 is rounded to 2^-20
SATURATE = 4096.0          # and saturated at 2^12
YUV709, BGR = 0, 1
M = ((0.4124, 0.3576, 0.1805), (0.2126, 0.7152, 0.0722), (0.0193, 0.1192, 0.9505))
WHITE = (0.9505, 1.0000, 1.0890)      # the matrix's row sums


def quantum_bar():
    """the bound include/vqa.h derives for the fixed-point rounding on de_mean: half a quantum"""
    return 0.5 / FIX


def _srgb_linear(c, dt):
    big = c > dt(0.04045)
    safe = np.where(big, c, dt(1.0))
    return np.where(big, np.power((safe + dt(0.055)) / dt(1.055), dt(2.4)), c / dt(12.92)).astype(dt)


def _f(t, dt):
    big = t > dt(0.008856)
    safe = np.where(big, t, dt(1.0))
    return np.where(big, np.cbrt(safe), dt(7.787) * t + dt(16.0) / dt(116.0)).astype(dt)


def lab_from_rgb(r, g, b, dtype=np.float64):
    """non-linear R'G'B' (any reals) -> Lab [.., 3]"""
    dt = dtype
    r, g, b = (_srgb_linear(np.asarray(x, dt), dt) for x in (r, g, b))
    xyz = [(dt(M[i][0]) * r + dt(M[i][1]) * g + dt(M[i][2]) * b) / dt(WHITE[i]) for i in range(3)]
    fx, fy, fz = (_f(t.astype(dt), dt) for t in xyz)
    return np.stack([dt(116.0) * fy - dt(16.0), dt(500.0) * (fx - fy), dt(200.0) * (fy - fz)], axis=-1).astype(dt)


def lab_from_yuv(y, u, v, depth=8, dtype=np.float64):
    """integer Y, U, V of one size (chroma already replicated) -> Lab"""
    dt = dtype
    s = 1 << (depth - 8)
    yy = (np.asarray(y, np.int64) - 16 * s).astype(dt) / dt(219 * s)
    uu = (np.asarray(u, np.int64) - 128 * s).astype(dt) / dt(224 * s)
    vv = (np.asarray(v, np.int64) - 128 * s).astype(dt) / dt(224 * s)
    return lab_from_rgb(yy + dt(1.5748) * vv, yy - dt(0.1873) * uu - dt(0.4681) * vv, yy + dt(1.8556) * uu, dt)


def lab_from_bgr(b, g, r, depth=8, dtype=np.float64):
    dt = dtype
    peak = dt((1 << depth) - 1)
    return lab_from_rgb(*(np.asarray(x, np.int64).astype(dt) / peak for x in (r, g, b)), dtype=dt)


def de00(lab1, lab2, weights=(1.0, 1.0, 1.0), dtype=np.float64):
    """dE00 of include/vqa.h on Lab arrays [.., 3]; angles in degrees"""
    dt = dtype
    lab1, lab2 = np.asarray(lab1, dt), np.asarray(lab2, dt)
    L1, a1, b1 = lab1[..., 0], lab1[..., 1], lab1[..., 2]
    L2, a2, b2 = lab2[..., 0], lab2[..., 1], lab2[..., 2]
    kl, kc, kh = (dt(k) for k in weights)
    d2r = dt(np.pi / 180.0)

    def ratio(c):                      # sqrt(c^7 / (c^7 + 25^7)), the powers by multiplication
        c2 = c * c
        c7 = c2 * c2 * c2 * c
        return np.sqrt(c7 / (c7 + dt(25.0 ** 7)))

    c1, c2 = np.sqrt(a1 * a1 + b1 * b1), np.sqrt(a2 * a2 + b2 * b2)
    g = dt(0.5) * (dt(1.0) - ratio(dt(0.5) * (c1 + c2)))
    ap1, ap2 = (dt(1.0) + g) * a1, (dt(1.0) + g) * a2
    cp1, cp2 = np.sqrt(ap1 * ap1 + b1 * b1), np.sqrt(ap2 * ap2 + b2 * b2)

    def hue(b, ap):
        h = np.degrees(np.arctan2(b, ap)).astype(dt)
        h = np.where(h < 0, h + dt(360.0), h)
        return np.where((ap == 0) & (b == 0), dt(0.0), h).astype(dt)

    h1, h2 = hue(b1, ap1), hue(b2, ap2)
    dL, dC, cc = L2 - L1, cp2 - cp1, cp1 * cp2
    dh = h2 - h1
    dh = np.where(dh > 180, dh - dt(360.0), np.where(dh < -180, dh + dt(360.0), dh))
    dh = np.where(cc == 0, dt(0.0), dh).astype(dt)
    dH = dt(2.0) * np.sqrt(cc) * np.sin(dt(0.5) * dh * d2r)
    lm, cm = dt(0.5) * (L1 + L2), dt(0.5) * (cp1 + cp2)
    hs = h1 + h2
    hm = np.where(np.abs(h1 - h2) <= 180, dt(0.5) * hs, np.where(hs < 360, dt(0.5) * (hs + dt(360.0)), dt(0.5) * (hs - dt(360.0))))
    hm = np.where(cc == 0, hs, hm).astype(dt)
    t = (dt(1.0) - dt(0.17) * np.cos((hm - dt(30.0)) * d2r) + dt(0.24) * np.cos(dt(2.0) * hm * d2r)
         + dt(0.32) * np.cos((dt(3.0) * hm + dt(6.0)) * d2r) - dt(0.20) * np.cos((dt(4.0) * hm - dt(63.0)) * d2r))
    x = (hm - dt(275.0)) / dt(25.0)
    dtheta = dt(30.0) * np.exp(-(x * x))
    rc = dt(2.0) * ratio(cm)
    l2 = (lm - dt(50.0)) * (lm - dt(50.0))
    sl = dt(1.0) + dt(0.015) * l2 / np.sqrt(dt(20.0) + l2)
    sc = dt(1.0) + dt(0.045) * cm
    sh = dt(1.0) + dt(0.015) * cm * t
    rt = -np.sin(dt(2.0) * dtheta * d2r) * rc
    tl, tc, th = dL / (kl * sl), dC / (kc * sc), dH / (kh * sh)
    v = tl * tl + tc * tc + th * th + rt * tc * th
    out = np.sqrt(np.maximum(v, dt(0.0)))
    assert out.dtype == dt, out.dtype
    return out


def replicate(c, h, w):
    """a chroma plane of the luma's size or its ceil-half in either direction -> [h, w] by replication: (i >> sv, j >> sh)"""
    c = np.asarray(c)
    ch, cw = c.shape[-2:]
    if ch not in (h, (h + 1) // 2) or cw not in (w, (w + 1) // 2):
        raise ValueError("a chroma plane is the luma's size or its ceil-half")
    sv, sh = int(ch != h), int(cw != w)
    return c[..., np.arange(h) >> sv, :][..., np.arange(w) >> sh]


def frame(ref, dist, depth=8, model=YUV709, weights=(1.0, 1.0, 1.0), dtype=np.float64):
    """ref, dist: three integer planes each, (Y, U, V) or (B, G, R) -> the per-pixel dE00 [h, w], as float64, exactly 0 where the
    integer triples are equal"""
    h, w = np.asarray(ref[0]).shape
    if h < MIN_DIM or w < MIN_DIM:
        raise ValueError("frames below %d x %d are not measured" % (MIN_DIM, MIN_DIM))
    if len(ref) != 3 or len(dist) != 3:
        raise ValueError("ciede needs three planes")
    a = [np.asarray(ref[0], np.int64)] + [replicate(np.asarray(p, np.int64), h, w) for p in ref[1:]]
    b = [np.asarray(dist[0], np.int64)] + [replicate(np.asarray(p, np.int64), h, w) for p in dist[1:]]
    conv = lab_from_yuv if model == YUV709 else lab_from_bgr
    de = de00(conv(*a, depth=depth, dtype=dtype), conv(*b, depth=depth, dtype=dtype), weights, dtype).astype(np.float64)
    same = (a[0] == b[0]) & (a[1] == b[1]) & (a[2] == b[2])
    return np.where(same, 0.0, np.minimum(de, SATURATE))


def score(de_mean):
    return float(45.0 - 20.0 * np.log10(de_mean)) if de_mean > 0 else float("inf")


def de_mean(ref, dist, depth=8, model=YUV709, weights=(1.0, 1.0, 1.0), dtype=np.float64):
    """-> the mean dE00 over the luma grid of one frame pair"""
    return float(frame(ref, dist, depth, model, weights, dtype).mean())


def de_mean_fixed(ref, dist, depth=8, model=YUV709, weights=(1.0, 1.0, 1.0)):
    """the float64 run with every pixel's value rounded to the 2^-20 quantum and added as integers: what the record's bits would
    be from exact arithmetic"""
    de = frame(ref, dist, depth, model, weights)
    return float(int(np.rint(de * FIX).astype(np.int64).sum()) / FIX / de.size)


def split_planes(frames, planes):
    """frames [n, samples] (or [n, h, w, 3] packed) and plane tuples (w, h, offset, row_stride, step[, depth]) -> per frame a
    list of three integer planes"""
    flat = np.asarray(frames).reshape(len(frames), -1)
    item = flat.dtype.itemsize
    out = []
    for f in flat:
        ps = []
        for (w, h, off, rs, step) in (p[:5] for p in planes):
            idx = (off + np.arange(h)[:, None] * rs + np.arange(w)[None, :] * step) // item
            ps.append(f[idx].astype(np.int64))
        out.append(ps)
    return out
