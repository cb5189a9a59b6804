"""The contents and bars of the CIEDE2000 parity matrix, shared by tests/test_ciede_host.py (is the reference's own float32 run
stable on a content?) and tests/test_gpu_ciede.py (the GPU against the float64 reference), so that both see the same bytes.
Integer-only and seeded.  The list is fixed here: nothing is left out by a test, and all of it must pass the admission."""
import numpy as np

import motion_cases as K

# geometry (h, w), depth, layout: the minimum (one workgroup); odd luma with 9 x 12 chroma, ragged patches, the sample-by-sample
# path; the one-load-per-row path over more than one workgroup (20 x 34 patches); 4:2:2; 10, 12 and 16 bits (70 columns of
# 16-bit samples are no whole patches: sample by sample); packed BGR (pixel step 3: sample by sample)
GRID = [((16, 16), 8, "yuv444p"), ((17, 23), 8, "yuv420p"), ((40, 136), 8, "yuv420p"), ((72, 88), 8, "yuv422p"),
        ((72, 88), 10, "yuv420p10le"), ((40, 56), 12, "yuv444p12le"), ((50, 70), 16, "yuv444p16le"), ((40, 56), 8, "bgr24")]
IDS = ["%dx%d-%s" % (g[0][0], g[0][1], g[2]) for g in GRID]
N_FRAMES = 2
DISTORTIONS = ("noise4", "plane1+6")       # the +-4-level noise of the PSNR-HVS tests; a pure offset of U (G of bgr24) by 6 levels
WEIGHTS = ((1.0, 1.0, 1.0), (0.65, 1.0, 4.0))
ADMIT = 1e-5                   # the reference's float32 run against its float64 run on de_mean
GPU_BAR = 1e-4                 # the family's relative bar (VIF, ADM, PSNR-HVS); the fixed-point term 2^-21 is added to it


def model_of(layout):
    import ciede_reference as R
    return R.BGR if layout == "bgr24" else R.YUV709


def pair_clip(layout, h, w, depth, seed, n, kind="natural", distortion="noise4"):
    """n frame pairs: the suite's reference clip and a distorted copy -> (ref, dist, planes)"""
    r, planes = K.clip(layout, h, w, depth, kind, seed=seed, n=n)
    u, L = 1 << (depth - 8), (1 << depth) - 1
    if distortion == "noise4":
        rng = np.random.default_rng(seed + 1)
        d = np.clip(r.astype(np.int64) + rng.integers(-4, 5, r.shape) * u + (rng.integers(0, u, r.shape) if depth > 8 else 0), 0, L)
        return r, d.astype(r.dtype), planes
    if distortion != "plane1+6":
        raise ValueError(distortion)
    d = r.copy()
    flat = d.reshape(n, -1)
    pw, ph, off, rs, step = planes[1][:5]
    isz = r.dtype.itemsize
    for i in range(n):
        view = np.lib.stride_tricks.as_strided(flat[i, off // isz:], shape=(ph, pw), strides=(rs, step))
        view[...] = np.clip(view.astype(np.int64) + 6 * u, 0, L).astype(r.dtype)
    return r, d, planes


def matrix():
    """every (geometry, depth, layout, distortion) of the GPU parity matrix"""
    return [(g, d, lay, dis) for (g, d, lay) in GRID for dis in DISTORTIONS]


def matrix_ids():
    return ["%dx%d-%s-%s" % (g[0], g[1], lay, dis) for (g, d, lay, dis) in matrix()]


def case(geom, depth, layout, distortion):
    h, w = geom
    return pair_clip(layout, h, w, depth, seed=h + w, n=N_FRAMES, distortion=distortion)


# ---- the further contents the GPU tests hold to the parity bar, beside the matrix: admitted like it ---------------------------
GRAY = [(depth, chroma) for depth in (8, 10) for chroma in ("444", "420")]
GRAY_GEOM = (34, 52)
ROI_FRAME, ROI_N = (60, 80), 3
ROIS = [(9, 13, 35, 45), (8, 16, 36, 48)]      # (y0, x0, h, w): an unaligned window (sample by sample); an aligned one


def gray_offset(depth, chroma):
    """a gray clip (U = V = 128 s) and its copy with the luma raised by 5 s: the 4:4:4 and the 4:2:0 version hold the same picture
    -> (ref, dist, planes)"""
    from rtvqa_amd.engine import yuv_planes
    s, dt = 1 << (depth - 8), (np.uint16 if depth > 8 else np.uint8)
    h, w = GRAY_GEOM
    y = np.clip(K.plane_clip(N_FRAMES, h, w, depth, "natural", 3), 16 * s, 200 * s)
    pl = yuv_planes(h, w, chroma, depth)
    f = np.full((N_FRAMES, sum(p[0] * p[1] for p in pl)), 128 * s, dt)
    f[:, :h * w] = y.reshape(N_FRAMES, -1)
    g = f.copy()
    g[:, :h * w] += 5 * s
    return f, g, pl


def roi_source():
    """the 4:4:4 clip the windows are cut from, as [n, 3 * H, W] (plane k starts k * H rows further down) -> (ref, dist)"""
    H, W = ROI_FRAME
    g, gd, _ = pair_clip("yuv444p", H, W, 8, seed=5, n=ROI_N)
    return g.reshape(ROI_N, 3 * H, W), gd.reshape(ROI_N, 3 * H, W)


def roi_cut(window):
    """the window's samples as frames of their own -> (ref, dist, planes)"""
    H, W = ROI_FRAME
    y0, x0, hh, ww = window
    cut = [np.ascontiguousarray(x.reshape(ROI_N, 3, H, W)[:, :, y0:y0 + hh, x0:x0 + ww]).reshape(ROI_N, -1) for x in roi_source()]
    return cut[0], cut[1], [(ww, hh, k * hh * ww, ww, 1) for k in range(3)]


def extras():
    """-> [(tag, ref, dist, planes, depth)]: every content outside matrix() that a GPU test compares with the reference"""
    out = [("gray+5 %d bits %s" % (d, c),) + gray_offset(d, c) + (d,) for (d, c) in GRAY]
    return out + [("window %d,%d %dx%d" % w,) + roi_cut(w) + (8,) for w in ROIS]
