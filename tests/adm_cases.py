"""The plane pairs the ADM tests measure: natural content (synth.s_natural) under four distortions, in every layout of the parity
matrix.  One module, so that the host test can check on the CPU - for exactly the pairs the GPU test compares - that the
reference's own float32 run stays within half the bar of its float64 run (the decoupling's angle test is a discontinuity: a
pair on which float32 already flips samples says nothing about the kernels)."""
import numpy as np

import vif_reference as V

KINDS = ("blur", "noise", "quant", "sharp")
# geometry (h, w), depth, layout, seed
GRID = [((1080, 1920), 8, "yuv420p", 1088), ((270, 480), 10, "yuv420p10le", 280), ((120, 160), 12, "yuv444p12le", 132),
        ((100, 140), 16, "gray16le", 116), ((163, 201), 8, "gray", 171), ((47, 35), 8, "gray", 55), ((16, 16), 8, "gray", 24),
        ((90, 110), 8, "bgr24", 98)]
IDS = ["%dx%d-%s" % (g[0][0], g[0][1], g[2]) for g in GRID]
ROI = dict(H=120, W=160, h=75, w=93, y0=9, x0=13, seed=5, n=2)


def planes_of(layout, h, w):
    from rtvqa_amd import video_processing as vp
    return vp.LAYOUTS[layout][0](h, w)


def natural(h, w, depth, seed):
    """one plane of synth.py's natural content (texture octaves, moving rectangles), scaled to `depth` bits"""
    from rtvqa_amd import synth
    g = synth.s_natural(1, h, w, seed=seed)[0][:, :, seed % 3].astype(np.int64)
    if depth > 8:
        rng = np.random.default_rng(seed)
        g = g * (1 << (depth - 8)) + rng.integers(0, 1 << (depth - 8), g.shape)   # the low bits carry content too
    return g


def distort(a, kind, depth, seed):
    mx = (1 << depth) - 1
    rng = np.random.default_rng(seed + 99)
    f = a.astype(np.float64)
    if kind == "blur":
        b = V.filt(f, V.taps(2))
    elif kind == "noise":
        b = f + rng.standard_normal(a.shape) * 6 * (1 << (depth - 8))
    elif kind == "quant":
        q = 16 << (depth - 8)
        b = (a // q) * q + q // 2
    elif kind == "sharp":
        b = f + 0.8 * (f - V.filt(f, V.taps(2)))
    else:
        raise ValueError(kind)
    return np.clip(np.rint(b), 0, mx).astype(np.int64)


def frames(layout, h, w, depth, kind, seed, n=1):
    """n frame pairs in `layout`: -> (ref, dist, planes) with [n, samples] arrays ([n, h, w, 3] for bgr24)"""
    planes = planes_of(layout, h, w)
    dt = np.uint16 if depth > 8 else np.uint8
    isz = np.dtype(dt).itemsize
    size = max(p[2] + (p[1] - 1) * p[3] + (p[0] - 1) * p[4] + isz for p in planes) // isz
    out = [np.zeros((n, size), dt), np.zeros((n, size), dt)]
    for i in range(n):
        for k, p in enumerate(planes):
            pw, ph, off, rs, step = p[:5]
            a = natural(ph, pw, depth, seed * 131 + i * 7 + k)
            pair = (a, distort(a, kind, depth, seed + i))
            for o, v in zip(out, pair):
                view = np.lib.stride_tricks.as_strided(o[i, off // isz:], shape=(ph, pw), strides=(rs, step))
                view[...] = v
    if layout == "bgr24":
        out = [o.reshape(n, h, w, 3) for o in out]
    return out[0], out[1], planes


def flat(a):
    return a.reshape(a.shape[0], -1)


def plane_of(frame, p, isz):
    pw, ph, off, rs, step = p[:5]
    return np.lib.stride_tricks.as_strided(frame[off // isz:], shape=(ph, pw), strides=(rs, step)).astype(np.int64)


def roi_frames(kind):
    """-> (r, d of the padded frames [2, H * W], the window's plane tuple, the window alone as contiguous frames rr, dc)"""
    c = ROI
    r, d, _ = frames("gray", c["H"], c["W"], 8, kind, seed=c["seed"], n=c["n"])
    roi = [(c["w"], c["h"], c["y0"] * c["W"] + c["x0"], c["W"], 1)]
    cut = lambda a: np.ascontiguousarray(a.reshape(c["n"], c["H"], c["W"])[:, c["y0"]:c["y0"] + c["h"], c["x0"]:c["x0"] + c["w"]]).reshape(c["n"], -1)
    return r, d, roi, cut(r), cut(d)


def parity_pairs():
    """every (tag, ref plane, dist plane, depth) the GPU parity tests compare"""
    for (geom, depth, layout, seed), tag in zip(GRID, IDS):
        for kind in KINDS:
            r, d, planes = frames(layout, geom[0], geom[1], depth, kind, seed)
            isz = r.dtype.itemsize
            for p, pl in enumerate(planes):
                yield "%s %s plane %d" % (tag, kind, p), plane_of(flat(r)[0], pl, isz), plane_of(flat(d)[0], pl, isz), depth
    for kind in KINDS:
        _r, _d, _roi, rr, dc = roi_frames(kind)
        for i in range(ROI["n"]):
            yield "roi %s frame %d" % (kind, i), rr[i].reshape(ROI["h"], ROI["w"]).astype(np.int64), \
                dc[i].reshape(ROI["h"], ROI["w"]).astype(np.int64), 8
