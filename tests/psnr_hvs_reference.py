"""PSNR-HVS (Egiazarian et al. 2006) and PSNR-HVS-M (Ponomarenko et al. 2007), restated in NumPy from the definition in
include/vqa.h (vqa_psnr_hvs_submit), not from the kernel: the published MATLAB form per plane, non-overlapping 8x8 blocks, on
the raw integer samples.

  psnr_hvs(R, D, depth, dtype=np.float64)   the text as it stands, in float64: two DCTs and their difference, variances by
                                            mean-and-subtract, everything summed in float64 with no quantisation.
  psnr_hvs(.., dtype=np.float32)            the arithmetic the header says the device uses, in float32: the variances from the
                                            exact integer sums (their quotients in float64, once), u as the DCT of the integer
                                            difference, m / msk as m (Q / 10)^2, per-block sums in float32 (NumPy's own order of
                                            addition, not the kernel's), the blocks' sums added in float64.  Its gap to the
                                            float64 run is what fp32 costs, and decides which contents enter the GPU matrix.
"""
import numpy as np

MIN_DIM = 16
FIX = 2.0 ** 20          # a block's two sums are rounded to 2^-20
Q = np.array([[16, 11, 10, 16, 24, 40, 51, 61], [12, 12, 14, 19, 26, 58, 60, 55], [14, 13, 16, 24, 40, 57, 69, 56],
              [14, 17, 22, 29, 51, 87, 80, 62], [18, 22, 37, 56, 68, 109, 103, 77], [24, 35, 55, 64, 81, 104, 113, 92],
              [49, 64, 78, 87, 103, 121, 120, 101], [72, 92, 95, 98, 112, 100, 103, 99]], np.float64)
CSF_SCALE = 25.735088


def tables(dtype=np.float64):
    """-> (C [8,8], csf [8,8], msk [8,8]) formed in float64 and rounded once to dtype"""
    k = np.arange(8, dtype=np.float64)
    c = np.sqrt(2.0 / 8.0) * np.cos((2.0 * k[None, :] + 1.0) * k[:, None] * np.pi / 16.0)
    c[0] = np.sqrt(1.0 / 8.0)
    return c.astype(dtype), (CSF_SCALE / Q).astype(dtype), ((10.0 / Q) ** 2).astype(dtype)


def quantum_bar():
    """the bound include/vqa.h derives for the fixed-point rounding on S: half a quantum per block over 64 coefficients"""
    return 0.5 / FIX / 64.0


def _blocks(p):
    """[h, w] -> [bh, bw, 8, 8] int64, whole blocks only"""
    p = np.asarray(p, np.int64)
    h, w = p.shape
    if h < MIN_DIM or w < MIN_DIM:
        raise ValueError("planes below %d x %d are not measured" % (MIN_DIM, MIN_DIM))
    bh, bw = h // 8, w // 8
    return p[:bh * 8, :bw * 8].reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3)


def _dct(z, c):
    """C z C^T of every block, in z's type"""
    return np.einsum("ij,abjk,lk->abil", c, z, c).astype(z.dtype)


def _vari64(x):
    n = x.shape[-1] * x.shape[-2]
    mu = x.mean(axis=(-2, -1), keepdims=True)
    return ((x - mu) ** 2).sum(axis=(-2, -1)) * (n / (n - 1.0))


def _pop64(z):
    g = _vari64(z)
    q = _vari64(z[..., :4, :4]) + _vari64(z[..., :4, 4:]) + _vari64(z[..., 4:, :4]) + _vari64(z[..., 4:, 4:])
    return np.where(g > 0, q / np.where(g > 0, g, 1.0), 0.0)


def _pop_int(zi):
    """pop from the exact integer sums: n s2 - s1^2 = (n - 1) vari, an integer; the quotients in float64, once"""
    def nvar(x):
        n = x.shape[-1] * x.shape[-2]
        return n * (x * x).sum(axis=(-2, -1)) - x.sum(axis=(-2, -1)) ** 2      # int64: below 2^44
    nb = nvar(zi)
    nq = nvar(zi[..., :4, :4]) + nvar(zi[..., :4, 4:]) + nvar(zi[..., 4:, :4]) + nvar(zi[..., 4:, 4:])
    vb, vq = nb.astype(np.float64) / 63.0, nq.astype(np.float64) / 15.0
    return np.where(nb > 0, vq / np.where(nb > 0, vb, 1.0), 0.0)


def block_sums(ref, dist, dtype=np.float64):
    """-> (hvs [bh, bw], hvsm [bh, bw]): every block's two sums of 64 terms, as float64"""
    c, csf, msk = tables(dtype)
    a, b = _blocks(ref), _blocks(dist)
    za, zb = _dct(a.astype(dtype), c), _dct(b.astype(dtype), c)
    ac = np.ones((8, 8), bool)
    ac[0, 0] = False

    def m_of(zi, zd):
        e = ((zd * zd * msk)[..., ac]).sum(axis=-1, dtype=dtype)
        pop = _pop64(zi.astype(np.float64)) if dtype == np.float64 else _pop_int(zi)
        return (np.sqrt(e * pop.astype(dtype)) / dtype(32.0)).astype(dtype)
    m = np.maximum(m_of(a, za), m_of(b, zb))
    if dtype == np.float64:
        u = np.abs(za - zb)
        thr = m[..., None, None] / msk
    else:
        u = np.abs(_dct((a - b).astype(dtype), c))
        thr = m[..., None, None] * ((Q / 10.0) ** 2).astype(dtype)
    thr[..., 0, 0] = 0
    hvs = ((u * csf) ** 2).reshape(u.shape[:2] + (64,)).sum(axis=-1, dtype=dtype)
    um = np.maximum(u - thr, dtype(0))
    hvsm = ((um * csf) ** 2).reshape(u.shape[:2] + (64,)).sum(axis=-1, dtype=dtype)
    return hvs.astype(np.float64), hvsm.astype(np.float64)


def db(s, depth=8):
    peak = float((1 << depth) - 1)
    return float(10.0 * np.log10(peak * peak / s)) if s > 0 else float("inf")


def psnr_hvs(ref, dist, depth=8, dtype=np.float64):
    """-> (S_hvs, S_hvsm, psnr_hvs dB, psnr_hvsm dB) of one plane pair"""
    hvs, hvsm = block_sums(ref, dist, dtype)
    n_c = 64.0 * hvs.size
    s, sm = float(hvs.sum() / n_c), float(hvsm.sum() / n_c)
    return s, sm, db(s, depth), db(sm, depth)


def psnr_hvs_fixed(ref, dist, depth=8):
    """the float64 run with every block's sums rounded to the 2^-20 quantum and added as integers: what the record's bits
    would be from exact arithmetic.  -> (S_hvs, S_hvsm)"""
    hvs, hvsm = block_sums(ref, dist, np.float64)
    n_c = 64.0 * hvs.size
    return tuple(float(sum(int(v) for v in np.rint(x.reshape(-1) * FIX)) / FIX / n_c) for x in (hvs, hvsm))
