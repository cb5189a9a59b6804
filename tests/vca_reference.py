"""VCA's texture features E, h and L in plain float64 NumPy, written from the definition in include/vqa.h (vqa_vca_submit) and
from nothing else: the orthonormal 32 x 32 DCT-II of every whole block of a plane of raw integer samples, the weighted sum of
the absolute AC coefficients, the block's sample sum, and the three per-frame figures on the 8-bit scale.  `quantise=True`
rounds the block words as the definition's integer words do (qH_k, qL_k) and forms the figures from their integer sums; without
it nothing is rounded: that is what the device is measured against."""
import numpy as np

B = 32


def dct_matrix():
    """T[u][x] = c_u cos(pi (2x + 1) u / 64), c_0 = sqrt(1 / 32), c_u = sqrt(2 / 32)"""
    u = np.arange(B, dtype=np.float64)[:, None]
    x = np.arange(B, dtype=np.float64)[None, :]
    t = np.cos(np.pi * (2.0 * x + 1.0) * u / 64.0) * np.sqrt(2.0 / B)
    t[0, :] = np.sqrt(1.0 / B)
    return t


def weights():
    """w(u, v) = exp(|(u v / 1024)^2 - 1|); the DC coefficient is left out of the sum: its weight here is 0"""
    u = np.arange(B, dtype=np.float64)
    uv = np.outer(u, u) / 1024.0
    w = np.exp(np.abs(uv * uv - 1.0))
    w[0, 0] = 0.0
    return w


T, W = dct_matrix(), weights()


def grid(h, w):
    return h // B, w // B   # nby, nbx


def dct_block(x):
    """D = T X T^t of one 32 x 32 block"""
    return T @ np.asarray(x, np.float64) @ T.T


def blocks(plane):
    """one plane of raw integer samples [h, w] -> (H [nby, nbx] float64, S [nby, nbx] int64)"""
    p = np.asarray(plane).astype(np.int64)
    nby, nbx = grid(*p.shape)
    x = p[:nby * B, :nbx * B].reshape(nby, B, nbx, B).transpose(0, 2, 1, 3)
    d = np.einsum("uy,abyx,vx->abuv", T, x.astype(np.float64), T)
    return (np.abs(d) * W).sum(axis=(2, 3)), x.sum(axis=(2, 3))


def quantise_h(hk, depth):
    return np.rint(hk * float(1 << (24 - depth))).astype(np.int64)


def quantise_l(s):
    return np.rint(np.sqrt(s.astype(np.float64)) * 16777216.0).astype(np.int64)


def features(planes, depth, prev=None, quantise=False):
    """planes: [n, h, w] raw samples of one plane of n consecutive frames; prev: the plane of the frame before frame 0, or None.
    -> dict: e, h, l [n] float64 on the 8-bit scale; H [n, nby, nbx] (H_k, unquantised), S [n, nby, nbx]; with quantise also the
    integer words e_sum, h_sum, l_sum [n] and qh [n, nby, nbx]."""
    planes = np.asarray(planes)
    n = planes.shape[0]
    sc = 1.0 / float(1 << (depth - 8))
    hs, ss = zip(*(blocks(planes[i]) for i in range(n)))
    hk, s = np.stack(hs), np.stack(ss)
    c = float(hk.shape[1] * hk.shape[2])
    hp = blocks(prev)[0] if prev is not None else None
    out = dict(H=hk, S=s)
    if quantise:
        q = 1.0 / float(1 << (24 - depth))
        qh, ql = quantise_h(hk, depth), quantise_l(s)
        qp = quantise_h(hp, depth) if hp is not None else None
        e_sum = qh.sum(axis=(1, 2))
        l_sum = ql.sum(axis=(1, 2))
        h_sum = np.zeros(n, np.int64)
        for i in range(n):
            before = qh[i - 1] if i > 0 else qp
            if before is not None:
                h_sum[i] = np.abs(qh[i] - before).sum()
        out.update(qh=qh, e_sum=e_sum, h_sum=h_sum, l_sum=l_sum,
                   e=sc * e_sum.astype(np.float64) * q / (1024.0 * c), h=sc * h_sum.astype(np.float64) * q / (1024.0 * c),
                   l=np.sqrt(sc / 32.0) * l_sum.astype(np.float64) * (1.0 / 16777216.0) / c)
        return out
    e = sc * hk.sum(axis=(1, 2)) / (1024.0 * c)
    hh = np.zeros(n)
    for i in range(n):
        before = hk[i - 1] if i > 0 else hp
        if before is not None:
            hh[i] = sc * np.abs(hk[i] - before).sum() / (1024.0 * c)
    l = np.sqrt(sc / 32.0) * np.sqrt(s.astype(np.float64)).sum(axis=(1, 2)) / c
    out.update(e=e, h=hh, l=l)
    return out


def bar(value):
    """the project's 1e-4 for its float metrics, relative above 1 and absolute below, on the 8-bit scale"""
    return 1e-4 * np.maximum(1.0, np.abs(value))
