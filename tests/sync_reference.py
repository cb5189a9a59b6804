"""The restatement of vqa_sig_submit's and vqa_sig_cross_submit's definitions (include/vqa.h) in NumPy.  Signatures: the cells by
slicing, the sums in uint64, the quotient by `//`.  The cross: D[j][i] = sum (d - r)^2 formed DIRECTLY in int64 - no Gram
matrix, no shift, no energies, so it shares no algebra with the kernels - diag by walking the diagonals, best by argmin, whose
first hit is the tie rule."""
import numpy as np

from align_reference import plane_series  # noqa: F401  (the samples of one plane tuple of every frame -> int64 [n, h, w])

G = 16
BYTES = 256


def signatures(planes, depth=8):
    """planes: [n, h, w] samples (any integer type, h, w >= 16) -> uint8 [n, 256]"""
    p = np.asarray(planes)
    n, h, w = p.shape
    assert h >= G and w >= G
    out = np.empty((n, BYTES), np.uint8)
    for a in range(G):
        r0, r1 = a * h // G, (a + 1) * h // G
        for b in range(G):
            c0, c1 = b * w // G, (b + 1) * w // G
            s = p[:, r0:r1, c0:c1].reshape(n, -1).sum(axis=1, dtype=np.uint64)
            count = np.uint64(((r1 - r0) * (c1 - c0)) << (depth - 8))
            out[:, G * a + b] = np.minimum(s // count, np.uint64(255)).astype(np.uint8)
    return out


def distances(dist_sig, ref_sig):
    """-> int64 [n_dist, n_ref], D[j][i] = sum_k (dist_sig[j][k] - ref_sig[i][k])^2, row by row"""
    d, r = np.asarray(dist_sig).astype(np.int64), np.asarray(ref_sig).astype(np.int64)
    out = np.empty((d.shape[0], r.shape[0]), np.int64)
    for j in range(d.shape[0]):
        e = r - d[j]
        out[j] = (e * e).sum(axis=1)
    return out


def cross(dist_sig, ref_sig):
    """-> (diag uint64 [n_dist + n_ref - 1], best uint64 [n_dist])"""
    D = distances(dist_sig, ref_sig)
    n_dist, n_ref = D.shape
    diag = np.zeros(n_dist + n_ref - 1, np.uint64)
    for k in range(-(n_dist - 1), n_ref):
        total = 0
        for j in range(max(0, -k), min(n_dist, n_ref - k)):
            total += int(D[j, j + k])
        diag[k + n_dist - 1] = total
    at = D.argmin(axis=1)   # the first of equal minima: the smallest reference index
    best = np.array([(int(D[j, at[j]]) << 32) | int(at[j]) for j in range(n_dist)], np.uint64)
    return diag, best


def cross_fast(dist_sig, ref_sig):
    """cross for the large count cases: the same D, the diagonals through np.trace's integer sum instead of a Python loop"""
    D = distances(dist_sig, ref_sig)
    n_dist, n_ref = D.shape
    diag = np.array([int(np.trace(D, offset=k, dtype=np.int64)) for k in range(-(n_dist - 1), n_ref)], np.uint64)
    at = D.argmin(axis=1)
    best = (D[np.arange(n_dist), at].astype(np.uint64) << np.uint64(32)) | at.astype(np.uint64)
    return diag, best
