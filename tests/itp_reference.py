"""dE_ITP (Recommendation ITU-R BT.2124; ICtCp and the PQ / HLG transfer functions of BT.2100), restated in NumPy from the
definition in include/vqa.h (vqa_itp_submit), not from the kernel: the three planes of a pixel -> R'G'B' clamped to [0, 1] ->
display light -> ICtCp -> 720 sqrt(dI^2 + dT^2 + dCp^2).

  pq_eotf / pq_inverse / hlg_display      the transfer functions on arrays
  itp_from_rgb / itp_from_yuv / itp_from_bgr   a colour -> (I, T, Cp) [.., 3]
  frame(ref, dist, ..)                    a whole frame pair given as (Y, Cb, Cr) or (B, G, R) integer planes -> dE per pixel
  words(de) / record(..)                  the quantised form: per-pixel rint(dE 2^20), integer sum and maximum
dtype=np.float64 is the text as it stands.  dtype=np.float32 evaluates every step in float32: its gap to the float64 run is what
fp32 would cost the kernel, and it is the reason the kernel is double (test_itp_host.py records it).
"""
import numpy as np

MIN_DIM = 16
FIX = 2.0 ** 20            # a pixel's dE is rounded to 2^-20
YUV2020, BGR = 0, 1
PQ, HLG = 0, 1
M1, M2 = 2610.0 / 16384.0, 2523.0 / 4096.0 * 128.0
C1, C2, C3 = 3424.0 / 4096.0, 2413.0 / 4096.0 * 32.0, 2392.0 / 4096.0 * 32.0
HLG_A, HLG_B, HLG_C = 0.17883277, 0.28466892, 0.55991073
KR, KG, KB = 0.2627, 0.6780, 0.0593
BAR = 2.0 ** -20           # the GPU's bar on de_mean and de_max against the unquantised float64 run: half of it is the quantum's
#                            half (derived), the other half room for last-ulp differences between two libraries' pow / exp


def pq_eotf(e, dtype=np.float64):
    """a PQ signal in [0, 1] -> cd/m2"""
    dt = dtype
    ep = np.power(np.asarray(e, dt), dt(1.0 / M2))
    num = np.maximum(ep - dt(C1), dt(0.0))
    den = dt(C2) - dt(C3) * ep
    return (dt(10000.0) * np.power(num / den, dt(1.0 / M1))).astype(dt)


def pq_inverse(x, dtype=np.float64):
    """cd/m2 in [0, 10000] -> the PQ signal"""
    dt = dtype
    yp = np.power(np.asarray(x, dt) / dt(10000.0), dt(M1))
    return np.power((dt(C1) + dt(C2) * yp) / (dt(1.0) + dt(C3) * yp), dt(M2)).astype(dt)


def hlg_scene(e, dtype=np.float64):
    """an HLG signal in [0, 1] -> scene light in [0, 1]"""
    dt = dtype
    e = np.asarray(e, dt)
    low = e <= dt(0.5)
    safe = np.where(low, dt(0.5), e)
    return np.where(low, e * e / dt(3.0), (np.exp((safe - dt(HLG_C)) / dt(HLG_A)) + dt(HLG_B)) / dt(12.0)).astype(dt)


def hlg_display(r, g, b, dtype=np.float64):
    """HLG signals -> display light of a 1000 cd/m2 display (gamma 1.2, black level 0), per channel"""
    dt = dtype
    er, eg, eb = (hlg_scene(x, dt) for x in (r, g, b))
    ys = (dt(KR) * er + dt(KG) * eg) + dt(KB) * eb
    k = np.where(ys > 0, dt(1000.0) * np.power(np.where(ys > 0, ys, dt(1.0)), dt(0.2)), dt(0.0)).astype(dt)
    return k * er, k * eg, k * eb


def itp_from_light(r, g, b, dtype=np.float64):
    """display light R, G, B in cd/m2 -> (I, T, Cp) [.., 3]"""
    dt = dtype
    l = ((dt(1688.0) * r + dt(2146.0) * g) + dt(262.0) * b) / dt(4096.0)
    m = ((dt(683.0) * r + dt(2951.0) * g) + dt(462.0) * b) / dt(4096.0)
    s = ((dt(99.0) * r + dt(309.0) * g) + dt(3688.0) * b) / dt(4096.0)
    l, m, s = (pq_inverse(x, dt) for x in (l, m, s))
    i = dt(0.5) * (l + m)
    t = dt(0.5) * (((dt(6610.0) * l - dt(13613.0) * m) + dt(7003.0) * s) / dt(4096.0))
    p = ((dt(17933.0) * l - dt(17390.0) * m) - dt(543.0) * s) / dt(4096.0)
    return np.stack([i, t, p], axis=-1).astype(dt)


def itp_from_rgb(r, g, b, transfer=PQ, dtype=np.float64):
    """non-linear R'G'B' (any reals; clamped to [0, 1] here) -> (I, T, Cp) [.., 3]"""
    dt = dtype
    r, g, b = (np.clip(np.asarray(x, dt), dt(0.0), dt(1.0)) for x in (r, g, b))
    if transfer == PQ:
        fr, fg, fb = (pq_eotf(x, dt) for x in (r, g, b))
    elif transfer == HLG:
        fr, fg, fb = hlg_display(r, g, b, dt)
    else:
        raise ValueError("transfer")
    return itp_from_light(fr, fg, fb, dt)


def rgb_from_yuv(y, cb, cr, depth=8, full_range=False, dtype=np.float64):
    """integer Y, Cb, Cr of one size -> R', G', B' (unclamped), BT.2020 non-constant luminance"""
    dt = dtype
    s, peak = 1 << (depth - 8), (1 << depth) - 1
    y, cb, cr = (np.asarray(x, np.int64) for x in (y, cb, cr))
    if full_range:
        yy, bb, rr = y.astype(dt) / dt(peak), (cb - (1 << (depth - 1))).astype(dt) / dt(peak), (cr - (1 << (depth - 1))).astype(dt) / dt(peak)
    else:
        yy, bb, rr = (y - 16 * s).astype(dt) / dt(219 * s), (cb - 128 * s).astype(dt) / dt(224 * s), (cr - 128 * s).astype(dt) / dt(224 * s)
    r = yy + dt(1.4746) * rr
    b = yy + dt(1.8814) * bb
    g = ((yy - dt(KR) * r) - dt(KB) * b) / dt(KG)
    return r, g, b


def itp_from_yuv(y, cb, cr, depth=8, transfer=PQ, full_range=False, dtype=np.float64):
    return itp_from_rgb(*rgb_from_yuv(y, cb, cr, depth, full_range, dtype), transfer=transfer, dtype=dtype)


def itp_from_bgr(b, g, r, depth=8, transfer=PQ, full_range=False, dtype=np.float64):
    dt = dtype
    peak = dt((1 << depth) - 1)
    return itp_from_rgb(*(np.asarray(x, np.int64).astype(dt) / peak for x in (r, g, b)), transfer=transfer, dtype=dt)


def delta(a, b, dtype=np.float64):
    """(I, T, Cp) arrays [.., 3] -> dE_ITP"""
    dt = dtype
    d = np.asarray(a, dt) - np.asarray(b, dt)
    return (dt(720.0) * np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])).astype(dt)


def replicate(c, h, w):
    """a chroma plane of the luma's size or its ceil-half in either direction -> [h, w] by replication: (i >> sv, j >> sh)"""
    c = np.asarray(c)
    ch, cw = c.shape[-2:]
    if ch not in (h, (h + 1) // 2) or cw not in (w, (w + 1) // 2):
        raise ValueError("a chroma plane is the luma's size or its ceil-half")
    sv, sh = int(ch != h), int(cw != w)
    return c[..., np.arange(h) >> sv, :][..., np.arange(w) >> sh]


def frame(ref, dist, depth=8, model=YUV2020, transfer=PQ, full_range=False, dtype=np.float64):
    """ref, dist: three integer planes each, (Y, Cb, Cr) or (B, G, R) -> the per-pixel dE_ITP [h, w], as float64, exactly 0 where
    the integer triples are equal"""
    h, w = np.asarray(ref[0]).shape
    if h < MIN_DIM or w < MIN_DIM:
        raise ValueError("frames below %d x %d are not measured" % (MIN_DIM, MIN_DIM))
    if len(ref) != 3 or len(dist) != 3:
        raise ValueError("itp needs three planes")
    a = [np.asarray(ref[0], np.int64)] + [replicate(np.asarray(p, np.int64), h, w) for p in ref[1:]]
    b = [np.asarray(dist[0], np.int64)] + [replicate(np.asarray(p, np.int64), h, w) for p in dist[1:]]
    conv = itp_from_yuv if model == YUV2020 else itp_from_bgr
    de = delta(conv(*a, depth=depth, transfer=transfer, full_range=full_range, dtype=dtype),
               conv(*b, depth=depth, transfer=transfer, full_range=full_range, dtype=dtype), dtype).astype(np.float64)
    same = (a[0] == b[0]) & (a[1] == b[1]) & (a[2] == b[2])
    return np.where(same, 0.0, de)


def words(de):
    """the per-pixel values -> (sum_q, max_q): rint(dE 2^20) added and maximised as integers"""
    q = np.rint(np.asarray(de, np.float64) * FIX).astype(np.int64)
    return int(q.sum()), int(q.max())


def record(ref, dist, depth=8, model=YUV2020, transfer=PQ, full_range=False, dtype=np.float64):
    """one frame pair -> dict: de_mean and de_max unquantised, and the quantised form (sum_q, max_q, q_mean, q_max)"""
    de = frame(ref, dist, depth, model, transfer, full_range, dtype)
    sq, mq = words(de)
    return {"de_mean": float(de.mean()), "de_max": float(de.max()), "sum_q": sq, "max_q": mq,
            "q_mean": sq / FIX / de.size, "q_max": mq / FIX}


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
