"""CPU reference for PSNR's SSE and the two SSIM definitions on 8..16-bit planar frames (float64 / exact integers).

Written from the definitions, not from the kernels:
  sse           sum over the plane of (ref - dist)^2, exact (FFmpeg vf_psnr's per-component sum)
  ssim_ffmpeg   libavfilter/vf_ssim.c at high depth: ssim_4x4xn_16bit (4x4 block sums s1, s2, ss, s12 as int64),
                ssim_endn_16bit (a sample pools a 2x2 group of blocks, 8x8 window at stride 4), ssim_end1x (double:
                c1 = .01*.01*max*max*64, c2 = .03*.03*max*max*64*63, max = 2^depth - 1), mean over (W/4-1)(H/4-1)
                samples (ssim_plane_16bit)
  ssim_gauss    scikit-image structural_similarity(gaussian_weights=True, sigma=1.5, use_sample_covariance=False,
                data_range=L): 11x11 Gaussian window (truncate 3.5), K1 .01, K2 .03, mean over the valid region
                (the window fully inside the plane), L = 2^depth - 1
Frames are flat [samples] arrays and planes (width, height, offset, row_stride, pixel_step[, depth]) tuples in BYTES, as the
engine takes them.
"""
import numpy as np


def plane(frame, p):
    """the (h, w) samples of plane tuple p inside one flat frame (uint8 or uint16), as int64"""
    w, h, off, rs, step = p[:5]
    isz = frame.dtype.itemsize
    flat = np.ascontiguousarray(frame).reshape(-1)
    assert off % isz == 0 and rs % isz == 0 and step % isz == 0
    v = np.lib.stride_tricks.as_strided(flat[off // isz:], shape=(h, w), strides=(rs, step), writeable=False)
    return v.astype(np.int64)


def sse(a, b):
    d = a - b
    return int((d * d).sum())


def ssim_ffmpeg(a, b, mx):
    """vf_ssim at max = mx on int64 planes; NaN when the plane has fewer than 2x2 blocks"""
    h, w = a.shape
    bh, bw = h >> 2, w >> 2
    if bh < 2 or bw < 2:
        return float("nan")
    A = a[:bh * 4, :bw * 4].reshape(bh, 4, bw, 4)
    B = b[:bh * 4, :bw * 4].reshape(bh, 4, bw, 4)
    s = [A.sum((1, 3)), B.sum((1, 3)), (A * A).sum((1, 3)) + (B * B).sum((1, 3)), (A * B).sum((1, 3))]

    def pool(x):   # the 2x2 group of blocks of every sample, int64 (exact)
        return x[:-1, :-1] + x[:-1, 1:] + x[1:, :-1] + x[1:, 1:]
    s1, s2, ss, s12 = (pool(x).astype(np.float64) for x in s)
    c1 = .01 * .01 * mx * mx * 64
    c2 = .03 * .03 * mx * mx * 64 * 63
    vars_ = ss * 64 - s1 * s1 - s2 * s2
    covar = s12 * 64 - s1 * s2
    v = (2 * s1 * s2 + c1) * (2 * covar + c2) / ((s1 * s1 + s2 * s2 + c1) * (vars_ + c2))
    return float(v.sum() / ((bh - 1) * (bw - 1)))


def _gauss11(dtype=np.float64):
    k = np.arange(11) - 5
    g = np.exp(-(k * k) / (2 * 1.5 * 1.5))
    return (g / g.sum()).astype(dtype)


def _filt(x):
    """separable 11x11 Gaussian, valid region, in the type of x"""
    g = _gauss11(x.dtype)
    h, w = x.shape
    v = sum(g[k] * x[k:k + h - 10, :] for k in range(11))
    return sum(g[k] * v[:, k:k + w - 10] for k in range(11))


def ssim_gauss(a, b, data_range, dtype=np.float64):
    """skimage's Gaussian SSIM at data range L on int64 planes; NaN below 11x11.  dtype float32: the same statements in that
    type on samples mapped to x 255 / L - 128 (data range 255), the means moved back by 128 for the luminance term - the range
    a float32 evaluation works in (include/vqa.h); SSIM does not change under the map, the float64 default does not apply it."""
    if a.shape[0] < 11 or a.shape[1] < 11:
        return float("nan")
    ty = np.dtype(dtype).type
    if ty is np.float64:
        scale, centre = ty(1), ty(0)
    else:
        scale, centre, data_range = ty(255.0 / data_range), ty(128), 255
    x, y = a.astype(dtype) * scale - centre, b.astype(dtype) * scale - centre
    mx, my = _filt(x), _filt(y)
    sxx = _filt(x * x) - mx * mx
    syy = _filt(y * y) - my * my
    sxy = _filt(x * y) - mx * my
    ux, uy = mx + centre, my + centre
    C1, C2 = ty((.01 * data_range) ** 2), ty((.03 * data_range) ** 2)
    S = ((2 * ux * uy + C1) * (2 * sxy + C2)) / ((ux * ux + uy * uy + C1) * (sxx + syy + C2))
    return float(S.astype(np.float64).mean())


def frame_quality(ref, dist, planes, mode, depth):
    """-> (sse list, ssim list) per plane of one frame pair (flat uint8 / uint16 arrays)"""
    mx = (1 << depth) - 1
    out_sse, out_ssim = [], []
    for p in planes:
        a, b = plane(ref, p), plane(dist, p)
        out_sse.append(sse(a, b))
        out_ssim.append(ssim_gauss(a, b, mx) if mode == "gauss" else ssim_ffmpeg(a, b, mx))
    return out_sse, out_ssim
