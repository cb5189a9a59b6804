"""XPSNR as include/vqa.h states it (vqa_xpsnr_submit), restated in NumPy for the tests: the integer words as int64 arrays, the
blocks through np.add.reduceat, the host part with Python floats over the blocks in ascending k.  Written from the header's
text, not from the kernels."""
import math

import numpy as np


def geometry(w, h):
    """-> dict(B, nbx, nby, bv, gw, gh, rho) of a w x h luma plane"""
    rho = (w * h) / (3840.0 * 2160.0)
    B = max(4, 4 * int(math.floor(32.0 * math.sqrt(rho) + 0.5)))
    bv = 1 if w * h <= 2048 * 1152 else 2
    return dict(B=B, nbx=-(-w // B), nby=-(-h // B), bv=bv, gw=w // bv, gh=h // bv, rho=rho)


def block_size(w, h):
    return geometry(w, h)["B"]


def activity_grid(luma, bv):
    """G: the luma itself, or its 2 x 2 sums on floor(h / 2) x floor(w / 2) (the last row / column of an odd plane is dropped)"""
    a = np.asarray(luma).astype(np.int64)
    if bv == 1:
        return a
    gh, gw = a.shape[0] // 2, a.shape[1] // 2
    a = a[:2 * gh, :2 * gw]
    return a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2]


def _blocks(a, step_y, step_x, nby, nbx):
    """block sums of `a` on a grid of step_y x step_x from (0, 0), padded with empty blocks to nby x nbx"""
    a = np.asarray(a, np.int64)
    s = np.add.reduceat(np.add.reduceat(a, np.arange(0, a.shape[0], step_y), axis=0), np.arange(0, a.shape[1], step_x), axis=1)
    out = np.zeros((nby, nbx), np.int64)
    out[:s.shape[0], :s.shape[1]] = s
    return out


def _interior(gh, gw):
    m = np.zeros((gh, gw), np.int64)
    m[1:gh - 1, 1:gw - 1] = 1
    return m


def counts(w, h):
    """n_k [nby, nbx]: the origins (rows 1 .. gh - 2, columns 1 .. gw - 2 of G) each block owns"""
    g = geometry(w, h)
    s = g["B"] // g["bv"]
    return _blocks(_interior(g["gh"], g["gw"]), s, s, g["nby"], g["nbx"])


def act_words(luma, prev=None):
    """-> (sa, ta) int64 [nby, nbx] of a reference luma plane and the one before it (None: ta = 0)"""
    h, w = np.asarray(luma).shape
    g = geometry(w, h)
    G = activity_grid(luma, g["bv"])
    f = np.zeros_like(G)
    f[1:-1, 1:-1] = (12 * G[1:-1, 1:-1] - 2 * (G[:-2, 1:-1] + G[2:, 1:-1] + G[1:-1, :-2] + G[1:-1, 2:])
                     - (G[:-2, :-2] + G[:-2, 2:] + G[2:, :-2] + G[2:, 2:]))
    s = g["B"] // g["bv"]
    sa = _blocks(np.abs(f), s, s, g["nby"], g["nbx"])
    if prev is None:
        return sa, np.zeros_like(sa)
    d = np.abs(G - activity_grid(prev, g["bv"])) * _interior(g["gh"], g["gw"])
    return sa, _blocks(d, s, s, g["nby"], g["nbx"])


def sse_words(r, d, w, h):
    """-> sse [nby, nbx] of one plane pair; w x h: the LUMA's size, which fixes the grid and this plane's block size"""
    g = geometry(w, h)
    r, d = np.asarray(r).astype(np.int64), np.asarray(d).astype(np.int64)
    ph, pw = r.shape
    assert pw in (w, (w + 1) // 2) and ph in (h, (h + 1) // 2)
    bw = g["B"] if pw == w else g["B"] // 2
    bh = g["B"] if ph == h else g["B"] // 2
    return _blocks((r - d) ** 2, bh, bw, g["nby"], g["nbx"])


def activity(sa, ta, n, w, h, depth):
    """a_k as Python floats, ascending k"""
    g = geometry(w, h)
    a_min, s = 2.0 ** (depth - 6), g["bv"] * g["bv"]
    out = []
    for x, y, c in zip(sa.reshape(-1).tolist(), ta.reshape(-1).tolist(), n.reshape(-1).tolist()):
        a = float(x + 2 * y) / float(s * c) if c > 0 else a_min
        out.append(max(a, a_min))
    return out


def average(w, h, depth):
    return math.sqrt(16.0 * 2.0 ** (2 * depth - 9) / math.sqrt(max(1e-5, geometry(w, h)["rho"])))


def pool(sse, act, w, h, pw, ph, depth):
    """-> (wsse, xpsnr) of one plane from its block words and the frame's a_k"""
    tot = 0.0
    for e, a in zip(sse.reshape(-1).tolist(), act):
        tot += float(e) / a
    wsse = average(w, h, depth) * tot
    peak = float((1 << depth) - 1)
    return wsse, (10.0 * math.log10((float(pw * ph) * (peak * peak)) / wsse) if wsse > 0 else math.inf)


def frame(ref_planes, dist_planes, prev_luma, depth):
    """one frame: lists of 2-D planes (luma first) -> dict(sa, ta, n, sse [p, nby, nbx], act, wsse [p], xpsnr [p], total [p])"""
    h, w = np.asarray(ref_planes[0]).shape
    sa, ta = act_words(ref_planes[0], prev_luma)
    n = counts(w, h)
    act = activity(sa, ta, n, w, h, depth)
    sse = np.stack([sse_words(r, d, w, h) for r, d in zip(ref_planes, dist_planes)])
    pooled = [pool(sse[p], act, w, h, np.asarray(r).shape[1], np.asarray(r).shape[0], depth) for p, r in enumerate(ref_planes)]
    return dict(sa=sa, ta=ta, n=n, sse=sse, act=act, wsse=[x[0] for x in pooled], xpsnr=[x[1] for x in pooled],
                total=[int(sse[p].sum()) for p in range(len(ref_planes))])


def psnr(r, d, depth):
    r, d = np.asarray(r).astype(np.int64), np.asarray(d).astype(np.int64)
    sse = int(((r - d) ** 2).sum())
    peak = float((1 << depth) - 1)
    return 10.0 * math.log10(float(r.size) * (peak * peak) / float(sse)) if sse else math.inf
