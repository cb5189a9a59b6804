"""Engine — thin Python owner of one vqa_ctx (one HIP device, one stream).

Host-side plumbing only: it hands pointers to the C ABI (include/vqa.h) and
turns the result records into NumPy arrays.  All pixel arithmetic happens in
the HIP kernels; nothing here computes a metric on the CPU.
"""
import ctypes as C
import math

import numpy as np

from . import _native as N

# numpy mirror of vqa_frame_metrics (layout checked against ctypes at import)
FRAME_DTYPE = np.dtype([
    ("hist_gray", np.uint32, (256,)),
    ("hist_bgr", np.uint32, (3, 256)),
    ("sum_gray2", np.uint64),
    ("dct_energy", np.float64),
    ("temporal_dct_l1", np.float64),
    ("sad_sum", np.uint64),
    ("sad_blocks", np.uint32),
    ("mv_d2_hist", np.uint32, (129,)),
    ("edge_count", np.uint32),
    ("edge_strong", np.uint32),
    ("edge_weak", np.uint32),
    ("has_prev", np.uint32),
    ("hyst_steps", np.uint32), ("orb_keypoints", np.uint32), ("orb_response", np.uint32), ("hyst_overflow", np.uint32),
    ("flow_mag_mean", np.float64),
], align=True)
PLANE_DTYPE = np.dtype([("sse", np.uint64), ("ssim", np.float64)], align=True)
assert FRAME_DTYPE.itemsize == C.sizeof(N.VqaFrameMetrics), (FRAME_DTYPE.itemsize, C.sizeof(N.VqaFrameMetrics))
VIF_DTYPE = np.dtype([("num", np.float64, (4,)), ("den", np.float64, (4,)), ("scale", np.float64, (4,)), ("vif", np.float64)],
                     align=True)
assert PLANE_DTYPE.itemsize == C.sizeof(N.VqaPlaneMetrics)
assert VIF_DTYPE.itemsize == C.sizeof(N.VqaVifMetrics)
ADM_DTYPE = np.dtype([("num", np.float64, (4,)), ("den", np.float64, (4,)), ("scale", np.float64, (4,)), ("adm2", np.float64)],
                     align=True)
assert ADM_DTYPE.itemsize == C.sizeof(N.VqaAdmMetrics)
MOTION_DTYPE = np.dtype([("sad", np.float64), ("motion", np.float64)], align=True)
assert MOTION_DTYPE.itemsize == C.sizeof(N.VqaMotionMetrics)
SITI_DTYPE = np.dtype([("grad_sum", np.float64), ("grad_sq", np.uint64), ("diff_sum", np.int64), ("diff_sq", np.uint64),
                       ("si", np.float64), ("ti", np.float64)], align=True)
assert SITI_DTYPE.itemsize == C.sizeof(N.VqaSitiMetrics)
PSNR_HVS_DTYPE = np.dtype([("s_hvs", np.float64), ("s_hvsm", np.float64), ("psnr_hvs", np.float64), ("psnr_hvsm", np.float64)],
                          align=True)
assert PSNR_HVS_DTYPE.itemsize == C.sizeof(N.VqaPsnrHvsMetrics)
CIEDE_DTYPE = np.dtype([("de_sum", np.float64), ("de_mean", np.float64), ("ciede2000", np.float64)], align=True)
assert CIEDE_DTYPE.itemsize == C.sizeof(N.VqaCiedeMetrics)
GMSD_DTYPE = np.dtype([("sum_u", np.uint64), ("sum_u2_lo", np.uint64), ("sum_u2_hi", np.uint64), ("count", np.int64),
                       ("gms_mean", np.float64), ("gmsd", np.float64)], align=True)
assert GMSD_DTYPE.itemsize == C.sizeof(N.VqaGmsdMetrics)
CAMBI_DTYPE = np.dtype([("top", np.uint64, (5,)), ("k", np.int64, (5,)), ("masked", np.int64, (5,)), ("pool", np.float64, (5,)),
                        ("cambi", np.float64)], align=True)
assert CAMBI_DTYPE.itemsize == C.sizeof(N.VqaCambiMetrics)
XPSNR_DTYPE = np.dtype([("sse", np.uint64), ("wsse", np.float64), ("xpsnr", np.float64), ("block", np.int32), ("nbx", np.int32),
                        ("nby", np.int32)], align=True)
assert XPSNR_DTYPE.itemsize == C.sizeof(N.VqaXpsnrMetrics)
HAARPSI_DTYPE = np.dtype([("den", np.uint64), ("num_lo", np.uint64), ("num_hi", np.uint64), ("similarity", np.float64),
                          ("haarpsi", np.float64)], align=True)
assert HAARPSI_DTYPE.itemsize == C.sizeof(N.VqaHaarpsiMetrics)
VCA_DTYPE = np.dtype([("e_sum", np.uint64), ("h_sum", np.uint64), ("l_sum", np.uint64), ("nbx", np.int32), ("nby", np.int32),
                      ("e", np.float64), ("h", np.float64), ("l", np.float64)], align=True)
assert VCA_DTYPE.itemsize == C.sizeof(N.VqaVcaMetrics)
ARTIFACTS_DTYPE = np.dtype([("edge_h", np.uint64, (8,)), ("edge_v", np.uint64, (8,)), ("blur_f_h", np.uint64),
                            ("blur_v_h", np.uint64), ("blur_f_v", np.uint64), ("blur_v_v", np.uint64), ("lap", np.uint64),
                            ("phase_h", np.int32), ("phase_v", np.int32), ("blockiness", np.float64),
                            ("blockiness_max", np.float64), ("blur_h", np.float64), ("blur_v", np.float64),
                            ("blur", np.float64), ("noise", np.float64)], align=True)
assert ARTIFACTS_DTYPE.itemsize == C.sizeof(N.VqaArtifactsMetrics)
BRISQUE_DTYPE = np.dtype([("sum_abs_u", np.uint64, (2,)), ("sum_u2", np.uint64, (2,))] +
                         [(k, np.uint64, (2, 4)) for k in ("n_neg", "n_pos", "sum_abs_p", "sq_neg_lo", "sq_neg_hi",
                                                          "sq_pos_lo", "sq_pos_hi")] +
                         [("flags", np.uint32), ("reserved", np.uint32), ("features", np.float64, (36,))], align=True)
assert BRISQUE_DTYPE.itemsize == C.sizeof(N.VqaBrisqueMetrics)
MDSI_DTYPE = np.dtype([("sum_pos", np.uint64), ("sum_neg", np.uint64), ("n_neg", np.uint64), ("sum_dev", np.uint64),
                       ("count", np.int64), ("factor", np.int32), ("reserved", np.int32), ("dev", np.float64),
                       ("mdsi", np.float64)], align=True)
assert MDSI_DTYPE.itemsize == C.sizeof(N.VqaMdsiMetrics)
ITP_DTYPE = np.dtype([("sum_q", np.uint64), ("max_q", np.uint64), ("de_sum", np.float64), ("de_mean", np.float64),
                      ("de_max", np.float64)], align=True)
assert ITP_DTYPE.itemsize == C.sizeof(N.VqaItpMetrics)
PU21_DTYPE = np.dtype([("sse_y_lo", np.uint64), ("sse_y_hi", np.uint64), ("sse_rgb_lo", np.uint64), ("sse_rgb_hi", np.uint64),
                       ("ssim_q", np.int64), ("windows", np.int64), ("mse_y", np.float64), ("mse_rgb", np.float64),
                       ("pu_psnr", np.float64), ("pu_psnr_rgb", np.float64), ("pu_ssim", np.float64)], align=True)
assert PU21_DTYPE.itemsize == C.sizeof(N.VqaPu21Metrics)
FSIM_DTYPE = np.dtype([("sum_pc", np.uint64), ("sum_sim", np.uint64), ("sum_simc", np.uint64), ("count", np.int64),
                       ("factor", np.int32), ("flags", np.uint32), ("fsim", np.float64), ("fsimc", np.float64)], align=True)
assert FSIM_DTYPE.itemsize == C.sizeof(N.VqaFsimMetrics) == 56
SIGSTATS_DTYPE = np.dtype([("count", np.int64), ("sum", np.uint64), ("sum_sq", np.uint64), ("min", np.uint32), ("max", np.uint32),
                           ("low", np.uint32), ("median", np.uint32), ("high", np.uint32), ("or_mask", np.uint32),
                           ("and_mask", np.uint32), ("bits_used", np.int32), ("below_black", np.uint64), ("under", np.uint64),
                           ("over_luma", np.uint64), ("over_chroma", np.uint64), ("above_peak", np.uint64), ("sad", np.uint64),
                           ("changed", np.uint64), ("top", np.int32), ("bottom", np.int32), ("left", np.int32),
                           ("right", np.int32), ("mean", np.float64), ("stdev", np.float64), ("dif", np.float64)], align=True)
assert SIGSTATS_DTYPE.itemsize == C.sizeof(N.VqaSigstatsMetrics) == 152
LIGHT_DTYPE = np.dtype([("count", np.int64), ("max_code", np.uint32, (3,)), ("max_code_rgb", np.uint32), ("min_code_rgb", np.uint32),
                        ("reserved", np.uint32), ("sum_q", np.uint64), ("sum_y", np.uint64), ("max_y", np.uint64),
                        ("out_709", np.uint64), ("out_p3", np.uint64), ("clamped", np.uint64), ("pct_bin", np.uint32, (10,)),
                        ("max_nits", np.float64), ("min_nits", np.float64), ("avg_nits", np.float64), ("y_avg", np.float64),
                        ("y_max", np.float64), ("maxscl", np.float64, (3,)), ("pct_nits", np.float64, (10,)),
                        ("share_709", np.float64), ("share_p3", np.float64)], align=True)
assert LIGHT_DTYPE.itemsize == C.sizeof(N.VqaLightMetrics) == 280
COLORFIT_DTYPE = np.dtype([("count", np.uint64), ("sum_r", np.uint64, (3,)), ("sum_d", np.uint64, (3,)), ("rr", np.uint64, (6,)),
                           ("rd", np.uint64, (9,)), ("dd", np.uint64, (3,)), ("sse", np.uint64, (3,))], align=True)
assert COLORFIT_DTYPE.itemsize == C.sizeof(N.VqaColorfitMetrics) == 224
# the plane-batch kinds, each a batch of its own: the Engine's pending slot -> (submit, wait, record dtype, record ctype)
_BATCHES = {
    "_pending_q": ("vqa_quality_submit", "vqa_quality_wait", PLANE_DTYPE, N.VqaPlaneMetrics),
    "_pending_v": ("vqa_vif_submit", "vqa_vif_wait", VIF_DTYPE, N.VqaVifMetrics),
    "_pending_a": ("vqa_adm_submit", "vqa_adm_wait", ADM_DTYPE, N.VqaAdmMetrics),
    "_pending_m": ("vqa_motion_submit", "vqa_motion_wait", MOTION_DTYPE, N.VqaMotionMetrics),
    "_pending_s": ("vqa_siti_submit", "vqa_siti_wait", SITI_DTYPE, N.VqaSitiMetrics),
    "_pending_h": ("vqa_psnr_hvs_submit", "vqa_psnr_hvs_wait", PSNR_HVS_DTYPE, N.VqaPsnrHvsMetrics),
    "_pending_e": ("vqa_ciede_submit", "vqa_ciede_wait", CIEDE_DTYPE, N.VqaCiedeMetrics),   # (one entry per frame)
    "_pending_g": ("vqa_gmsd_submit", "vqa_gmsd_wait", GMSD_DTYPE, N.VqaGmsdMetrics),
    "_pending_b": ("vqa_cambi_submit", "vqa_cambi_wait", CAMBI_DTYPE, N.VqaCambiMetrics),   # (one stream)
    "_pending_x": ("vqa_xpsnr_submit", "vqa_xpsnr_wait", XPSNR_DTYPE, N.VqaXpsnrMetrics),   # (a pair and the frame before it)
    "_pending_w": ("vqa_haarpsi_submit", "vqa_haarpsi_wait", HAARPSI_DTYPE, N.VqaHaarpsiMetrics),
    "_pending_t": ("vqa_vca_submit", "vqa_vca_wait", VCA_DTYPE, N.VqaVcaMetrics),   # (one stream and the frame before it)
    "_pending_r": ("vqa_artifacts_submit", "vqa_artifacts_wait", ARTIFACTS_DTYPE, N.VqaArtifactsMetrics),   # (one stream)
    "_pending_n": ("vqa_brisque_submit", "vqa_brisque_wait", BRISQUE_DTYPE, N.VqaBrisqueMetrics),   # (one stream)
    "_pending_d": ("vqa_mdsi_submit", "vqa_mdsi_wait", MDSI_DTYPE, N.VqaMdsiMetrics),   # (one entry per frame)
    "_pending_i": ("vqa_itp_submit", "vqa_itp_wait", ITP_DTYPE, N.VqaItpMetrics),   # (one entry per frame)
    "_pending_u": ("vqa_pu21_submit", "vqa_pu21_wait", PU21_DTYPE, N.VqaPu21Metrics),   # (one entry per frame)
    "_pending_f": ("vqa_fsim_submit", "vqa_fsim_wait", FSIM_DTYPE, N.VqaFsimMetrics),   # (one entry per frame)
    "_pending_z": ("vqa_sigstats_submit", "vqa_sigstats_wait", SIGSTATS_DTYPE, N.VqaSigstatsMetrics),   # (one stream and the frame before it)
}


def check_xpsnr_planes(planes):
    """vqa_xpsnr_submit's layout rules, as a ValueError before anything is uploaded: a planar layout (pixel step of one sample)
    whose first plane is the luma, every other plane of its size or its ceil-half in either direction, all at least 16 x 16"""
    bps = 2 if planes_depth(planes) > 8 else 1
    w0, h0 = int(planes[0][0]), int(planes[0][1])
    for p in planes:
        w, h = int(p[0]), int(p[1])
        if int(p[4]) != bps:
            raise ValueError("xpsnr needs a planar layout whose first plane is the luma (packed layouts such as bgr24 have none)")
        if w not in (w0, (w0 + 1) // 2) or h not in (h0, (h0 + 1) // 2):
            raise ValueError("xpsnr needs planes of the luma's size or half of it (%dx%d against %dx%d)" % (w, h, w0, h0))
        if w < N.XPSNR_MIN_DIM or h < N.XPSNR_MIN_DIM:
            raise ValueError("xpsnr needs planes of at least %d x %d (got %dx%d)" % (N.XPSNR_MIN_DIM, N.XPSNR_MIN_DIM, w, h))


def check_vca_planes(planes):
    """vqa_vca_submit's layout rules, as a ValueError before anything is uploaded: a planar layout (pixel step of one sample),
    every plane at least 32 x 32"""
    bps = 2 if planes_depth(planes) > 8 else 1
    for p in planes:
        w, h = int(p[0]), int(p[1])
        if int(p[4]) != bps:
            raise ValueError("vca needs a planar layout (packed layouts such as bgr24 are not measured)")
        if w < N.VCA_BLOCK or h < N.VCA_BLOCK:
            raise ValueError("vca needs planes of at least %d x %d (got %dx%d)" % (N.VCA_BLOCK, N.VCA_BLOCK, w, h))


def vca_grid(width, height):
    """VCA's block grid of a width x height plane -> (nbx, nby): its whole 32 x 32 blocks"""
    return int(width) // N.VCA_BLOCK, int(height) // N.VCA_BLOCK


def mdsi_factor(h, w):
    """MDSI's downsampling factor of an h x w plane 0 as include/vqa.h states it: max(1, floor(min(h, w) / 256 + 0.5)) -
    MATLAB's round, so 640 gives 3 - in integers"""
    return max(1, (min(int(h), int(w)) + 128) // 256)


def xpsnr_grid(width, height):
    """XPSNR's block grid of a width x height luma plane as include/vqa.h states it -> (B, nbx, nby):
    B = max(4, 4 floor(32 sqrt(rho) + 0.5)) with rho = W H / (3840 * 2160), and ceil(W / B) x ceil(H / B) blocks."""
    rho = (int(width) * int(height)) / (3840.0 * 2160.0)
    b = max(4, 4 * int(math.floor(32.0 * math.sqrt(rho) + 0.5)))
    return b, -(-int(width) // b), -(-int(height) // b)


def scale_filter(filter):
    """a filter of the resampler by name ("bilinear" | "bicubic" | "lanczos") or id -> its id (N.SCALE_*)"""
    if isinstance(filter, str) and filter in N.SCALE_FILTERS:
        return N.SCALE_FILTERS[filter]
    if not isinstance(filter, (str, bool)) and filter in N.SCALE_FILTERS.values():
        return int(filter)
    raise ValueError("scale filter must be one of %s (got %r)" % (", ".join(repr(k) for k in N.SCALE_FILTERS), filter))


def colorfit_bins(depth):
    """the bins of one plane's transfer table of vqa_colorfit_submit: 1 << min(depth, 10)"""
    return 1 << min(int(depth), 10)


def light_table(transfer="pq"):
    """T[65536] uint64 of vqa_light_table: the display light of a 16-bit code in 2^-20 cd/m2.  "pq" (or N.ITP_PQ); "hlg" is a
    ValueError - HLG's display light is not a per-channel function (the OOTF needs Ys), and CTA-861.3's figures are HDR10's.
    Needs no GPU."""
    if transfer in ("hlg", N.ITP_HLG) and not isinstance(transfer, bool):
        raise ValueError("light levels are not built for 'hlg': its display light is not a per-channel function (the OOTF needs "
                         "Ys) and CTA-861.3's figures are HDR10's; transfer must be 'pq'")
    if isinstance(transfer, bool) or transfer not in ("pq", N.ITP_PQ):
        raise ValueError("transfer must be 'pq'")
    table = np.zeros(65536, np.uint64)
    N.check(N.load().vqa_light_table(N.ITP_PQ, table.ctypes.data_as(C.POINTER(C.c_uint64))), "vqa_light_table")
    return table


def check_light_table(table):
    """a caller's table -> contiguous uint64 [65536]; a ValueError for another type or shape, a table that decreases anywhere or
    an entry of 2^34 or more (vqa_light_submit refuses the same with VQA_ERR_INVALID).  Needs no GPU."""
    table = np.ascontiguousarray(table)
    if table.dtype != np.uint64 or table.shape != (65536,):
        raise ValueError("table must be uint64 [65536]")
    if int(table[-1]) >= N.LIGHT_TABLE_LIMIT or (table[1:] < table[:-1]).any():
        raise ValueError("table must not decrease and must stay below 2^34")
    return table


def light_gamut(name):
    """rint(2^16 A) as int64 [3, 3], A the linear BT.2020 -> "bt709" | "p3" matrix (vqa_light_gamut): rows R, G, B of the
    gamut, columns R, G, B of BT.2020.  Needs no GPU."""
    if not isinstance(name, str) or name not in N.LIGHT_GAMUTS:
        raise ValueError("gamut must be 'bt709' or 'p3'")
    m = np.zeros(9, np.int64)
    N.check(N.load().vqa_light_gamut(N.LIGHT_GAMUTS[name], m.ctypes.data_as(C.POINTER(C.c_int64))), "vqa_light_gamut")
    return m.reshape(3, 3)


def planes_span(planes):
    """bytes from a frame's first byte to the end of its last plane"""
    bps = 2 if planes_depth(planes) > 8 else 1
    return max(int(p[2]) + (int(p[1]) - 1) * int(p[3]) + (int(p[0]) - 1) * int(p[4]) + bps for p in planes)


def check_scale_planes(planes, out_planes):
    """vqa_scale_submit's rules for the two plane lists, as a ValueError before anything is uploaded: one to four planes, the
    same count and depth on both sides, every plane of both at least 16 x 16 with h w <= 2^28, per axis 1/4 <= out / in <= 8"""
    if not 1 <= len(planes) <= 4 or len(planes) != len(out_planes):
        raise ValueError("scale needs one to four planes and as many on both sides (got %d and %d)" % (len(planes), len(out_planes)))
    if planes_depth(planes) != planes_depth(out_planes):
        raise ValueError("scale keeps the sample depth (got %d and %d bits): converting depths is Engine.convert's"
                         % (planes_depth(planes), planes_depth(out_planes)))
    for p in list(planes) + list(out_planes):
        w, h = int(p[0]), int(p[1])
        if w < N.SCALE_MIN_DIM or h < N.SCALE_MIN_DIM or w * h > N.SCALE_MAX_SAMPLES:
            raise ValueError("scale needs planes of at least %d x %d and at most 2^28 samples (got %dx%d)"
                             % (N.SCALE_MIN_DIM, N.SCALE_MIN_DIM, w, h))
    for a, b in zip(planes, out_planes):
        for n_in, n_out in ((int(a[0]), int(b[0])), (int(a[1]), int(b[1]))):
            if n_in > N.SCALE_MAX_DOWN * n_out or n_out > N.SCALE_MAX_UP * n_in:
                raise ValueError("scale ratios lie between 1/%d and %d per axis (got %d -> %d)"
                                 % (N.SCALE_MAX_DOWN, N.SCALE_MAX_UP, n_in, n_out))


def check_conform_args(planes, out_planes, origin=None, index=None, lut=None, matrix=None):
    """vqa_conform_submit's rules for its lists and arrays, as a ValueError before anything is uploaded -> (origin int32
    [n_planes, 2] or None, index int32 [n_out] or None, lut [n_planes, 2^depth] of the sample type or None, matrix int64 [3, 4]
    or None), each contiguous.  Needs no GPU."""
    if not 1 <= len(planes) <= 4 or len(planes) != len(out_planes):
        raise ValueError("conform needs one to four planes and as many on both sides (got %d and %d)" % (len(planes), len(out_planes)))
    depth = planes_depth(planes)
    if depth != planes_depth(out_planes):
        raise ValueError("conform keeps the sample depth (got %d and %d bits): converting depths is Engine.convert's"
                         % (depth, planes_depth(out_planes)))
    for i, q in enumerate(out_planes):
        w, h, least = int(q[0]), int(q[1]), N.CONFORM_MIN_DIM if i == 0 else N.CONFORM_MIN_DIM // 2
        if w < least or h < least or w * h > N.SCALE_MAX_SAMPLES:
            raise ValueError("conform writes planes of at least %d x %d and at most 2^28 samples (plane %d: %dx%d)"
                             % (least, least, i, w, h))
    if origin is not None:
        origin = np.ascontiguousarray(np.asarray(origin, np.int64).reshape(-1, 2))
        if origin.shape[0] != len(planes):
            raise ValueError("origin needs one (y0, x0) per plane")
    for i, (p, q) in enumerate(zip(planes, out_planes)):
        y0, x0 = (int(origin[i, 0]), int(origin[i, 1])) if origin is not None else (0, 0)
        if y0 < 0 or x0 < 0 or y0 + int(q[1]) > int(p[1]) or x0 + int(q[0]) > int(p[0]):
            raise ValueError("the window of plane %d (%dx%d at y0 %d, x0 %d) leaves its source plane (%dx%d)"
                             % (i, int(q[0]), int(q[1]), y0, x0, int(p[0]), int(p[1])))
    if origin is not None:
        origin = origin.astype(np.int32)
    if index is not None:
        index = np.asarray(index)
        if index.ndim != 1 or index.size == 0 or not np.issubdtype(index.dtype, np.integer):
            raise ValueError("index must be a non-empty one-dimensional integer array")
        index = np.ascontiguousarray(index, np.int32)
    sample = np.uint16 if depth > 8 else np.uint8
    if lut is not None:
        lut = np.asarray(lut)
        if not np.issubdtype(lut.dtype, np.integer) or lut.shape != (len(planes), 1 << depth):
            raise ValueError("lut must be an integer array [%d, %d] (got %s %s)" % (len(planes), 1 << depth, lut.dtype, lut.shape))
        if int(lut.min()) < 0 or int(lut.max()) > (1 << depth) - 1:
            raise ValueError("lut entries must lie in 0 .. %d" % ((1 << depth) - 1))
        lut = np.ascontiguousarray(lut, sample)
    if matrix is not None:
        if len(planes) != 3:
            raise ValueError("a matrix needs three planes (got %d)" % len(planes))
        matrix = np.asarray(matrix)
        if matrix.shape != (3, 4) or not np.issubdtype(matrix.dtype, np.integer):
            raise ValueError("matrix must be an integer [3, 4] array in 2^-16 fixed point")
        matrix = np.ascontiguousarray(matrix, np.int64)
        if int(np.abs(matrix[:, :3]).max()) > N.CONFORM_MAX_COEF or int(np.abs(matrix[:, 3]).max()) > N.CONFORM_MAX_BIAS:
            raise ValueError("matrix coefficients are bounded by 2^20 and its offsets by 2^33 (2^-16 fixed point)")
    return origin, index, lut, matrix


CONVERT_CHROMA = ("box", "linear")      # vqa_convert_submit's chroma filters, by id
CONVERT_SITING = ("center", "left")     # its horizontal sitings
CONVERT_RANGE = ("limited", "full")     # its ranges


def convert_options(chroma="linear", siting="center", range="limited"):
    """the three options of convert by name -> their ids (N.CHROMA_*, N.SITING_*, N.RANGE_*); a ValueError for anything else"""
    ids = []
    for what, names, v in (("chroma", CONVERT_CHROMA, chroma), ("siting", CONVERT_SITING, siting), ("range", CONVERT_RANGE, range)):
        if not isinstance(v, str) or v not in names:
            raise ValueError("convert %s must be one of %s (got %r)" % (what, ", ".join(repr(k) for k in names), v))
        ids.append(names.index(v))
    return tuple(ids)


def convert_relation(n_s, n_d):
    """the relation of one axis by include/vqa.h's rule: "same" | "up" | "down", or None where there is none"""
    n_s, n_d = int(n_s), int(n_d)
    if n_d == n_s:
        return "same"
    if n_s == (n_d + 1) >> 1:
        return "up"
    if n_d == (n_s + 1) >> 1:
        return "down"
    return None


def check_convert_planes(planes, out_planes):
    """vqa_convert_submit's rules for the two plane lists, as a ValueError before anything is uploaded: one to four planes and
    as many on both sides, one depth per list, plane 0 of both at least 16 x 16 and the others at least 8 x 8 with h w <= 2^28,
    per plane and axis the same size, twice (2 n or 2 n - 1) or half (rounded up) of it.  Needs no GPU."""
    if not 1 <= len(planes) <= 4 or len(planes) != len(out_planes):
        raise ValueError("convert needs one to four planes and as many on both sides (got %d and %d)" % (len(planes), len(out_planes)))
    planes_depth(planes), planes_depth(out_planes)
    for side, lst in (("source", planes), ("destination", out_planes)):
        for i, q in enumerate(lst):
            w, h, least = int(q[0]), int(q[1]), N.CONVERT_MIN_DIM if i == 0 else N.CONVERT_MIN_DIM // 2
            if w < least or h < least or w * h > N.SCALE_MAX_SAMPLES:
                raise ValueError("convert needs planes of at least %d x %d and at most 2^28 samples (%s plane %d: %dx%d)"
                                 % (least, least, side, i, w, h))
    for i, (a, b) in enumerate(zip(planes, out_planes)):
        for axis, n_s, n_d in (("width", a[0], b[0]), ("height", a[1], b[1])):
            if convert_relation(n_s, n_d) is None:
                raise ValueError("convert takes a plane to the same size, twice or half of it per axis (plane %d %s: %d -> %d): "
                                 "chroma ratios other than 1 and 2 are not built" % (i, axis, int(n_s), int(n_d)))


def scale_tables(filter, n_in, n_out):
    """vqa_scale_tables: one axis' tables of the resampler as the library builds them on the host (no GPU needed) ->
    (k int32 [n_out, ksize], xmin int32 [n_out], count int32 [n_out])"""
    lib, fid = N.load(), scale_filter(filter)
    ks = C.c_int(0)
    N.check(lib.vqa_scale_tables(fid, int(n_in), int(n_out), None, None, None, C.byref(ks)), "vqa_scale_tables")
    k = np.zeros((int(n_out), ks.value), np.int32)
    xmin, count = np.zeros(int(n_out), np.int32), np.zeros(int(n_out), np.int32)
    i32 = C.POINTER(C.c_int32)
    N.check(lib.vqa_scale_tables(fid, int(n_in), int(n_out), k.ctypes.data_as(i32), xmin.ctypes.data_as(i32),
                                 count.ctypes.data_as(i32), C.byref(ks)), "vqa_scale_tables")
    return k, xmin, count


class DeviceFrames:
    """n packed BGR24 frames resident in device memory (itemsize 2: frames of uint16 samples, for the quality kernels'
    9..16-bit planes; strides are in bytes)."""

    def __init__(self, ptr, n, h, w, frame_stride=None, row_stride=None, owner=None, channels=3, itemsize=1):
        self.ptr, self.n, self.h, self.w = int(ptr), int(n), int(h), int(w)
        self.channels = channels
        self.itemsize = int(itemsize)
        self.row_stride = int(row_stride) if row_stride else self.w * channels * self.itemsize
        self.frame_stride = int(frame_stride) if frame_stride else self.row_stride * self.h
        self._owner = owner  # keeps the allocation (torch tensor / DeviceBuffer) alive

    @classmethod
    def from_torch(cls, t):
        """Wrap a CUDA(HIP) uint8 (or uint16) torch tensor of shape [n,h,w,3] (or [n,h,w]) without copying."""
        assert t.is_cuda and t.dtype.__str__() in ("torch.uint8", "torch.uint16") and t.is_contiguous()
        ch = t.shape[3] if t.dim() == 4 else 1
        return cls(t.data_ptr(), t.shape[0], t.shape[1], t.shape[2], owner=t, channels=ch, itemsize=t.element_size())

    def frame(self, i):
        return DeviceFrames(self.ptr + i * self.frame_stride, 1, self.h, self.w, self.frame_stride, self.row_stride,
                            owner=self._owner, channels=self.channels, itemsize=self.itemsize)

    def slice(self, a, b):
        return DeviceFrames(self.ptr + a * self.frame_stride, b - a, self.h, self.w, self.frame_stride,
                            self.row_stride, owner=self._owner, channels=self.channels, itemsize=self.itemsize)

    def roi(self, y0, y1, x0, x1):
        """The window rows y0..y1, columns x0..x1 of every frame, in place (same memory, padded rows)."""
        assert 0 <= y0 < y1 <= self.h and 0 <= x0 < x1 <= self.w
        return DeviceFrames(self.ptr + y0 * self.row_stride + x0 * self.channels * self.itemsize, self.n, y1 - y0, x1 - x0,
                            self.frame_stride, self.row_stride, owner=self._owner, channels=self.channels,
                            itemsize=self.itemsize)


class DeviceBuffer:
    def __init__(self, engine, nbytes):
        self.engine, self.nbytes = engine, int(nbytes)
        p = C.c_void_p()
        N.check(engine.lib.vqa_alloc_device(engine.ctx, self.nbytes, C.byref(p)), "vqa_alloc_device", engine.ctx)
        self.ptr = p.value

    def free(self):
        if self.ptr:
            self.engine.lib.vqa_free_device(self.engine.ctx, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def bgr_planes(h, w):
    """B, G, R channels of packed BGR24 as three full-size planes."""
    return [(w, h, c, 3 * w, 3) for c in range(3)]


def gray_planes(h, w):
    return [(w, h, 0, w, 1)]


def yuv420p_planes(h, w):
    cw, ch = (w + 1) // 2, (h + 1) // 2
    return [(w, h, 0, w, 1), (cw, ch, w * h, cw, 1), (cw, ch, w * h + cw * ch, cw, 1)]


def yuv_planes(h, w, chroma="420", depth=8):
    """Y, U, V of one planar frame (chroma "420" | "422" | "444"; "mono": Y only) at `depth` bits: 8 -> uint8 samples
    (5-tuples, what yuv420p_planes / gray_planes give), 9..16 -> little-endian uint16 samples (6-tuples carrying the
    depth; offsets and strides in bytes).  Planes follow each other without padding, as FFmpeg's planar formats."""
    if chroma not in ("420", "422", "444", "mono"):
        raise ValueError("chroma must be '420', '422', '444' or 'mono' (got %r)" % (chroma,))
    depth = int(depth)
    if depth != 8 and not 9 <= depth <= 16:
        raise ValueError("depth must be 8 or 9..16 (got %d)" % depth)
    bps = 2 if depth > 8 else 1
    sizes = [(w, h)]
    if chroma != "mono":
        cw = (w + 1) // 2 if chroma in ("420", "422") else w
        ch = (h + 1) // 2 if chroma == "420" else h
        sizes += [(cw, ch), (cw, ch)]
    out, off = [], 0
    for pw, ph in sizes:
        out.append((pw, ph, off, pw * bps, bps) + ((depth,) if depth > 8 else ()))
        off += pw * ph * bps
    return out


def mono_planes(h, w, depth=8):
    """One gray plane of `depth` bits (gray10le, gray16le ...: uint16 samples above 8 bits)."""
    return yuv_planes(h, w, "mono", depth)


def planes_depth(planes):
    """The sample depth of a plane list: 8 for 5-tuples (and a 6th element 0 / 8), else the 6th element; one depth per list."""
    depths = {(int(p[5]) if len(p) > 5 else 0) or 8 for p in planes}
    if len(depths) != 1:
        raise ValueError("the planes of one submit must share a sample depth (got %s)" % sorted(depths))
    return depths.pop()


def plane_descs(planes):
    """Plane tuples (width, height, offset, row_stride, pixel_step[, bit_depth]) -> a ctypes vqa_plane_desc array."""
    descs = (N.VqaPlaneDesc * len(planes))()
    for i, p in enumerate(planes):
        w, h, off, rs, step = p[:5]
        descs[i].width, descs[i].height, descs[i].offset = w, h, off
        descs[i].row_stride, descs[i].pixel_step = rs, step
        descs[i].bit_depth = int(p[5]) if len(p) > 5 else 0
    return descs


class Engine:
    def __init__(self, device=0):
        self.lib = N.load()
        ctx = C.c_void_p()
        st = self.lib.vqa_create(int(device), C.byref(ctx))
        if st != N.VQA_OK:
            raise N.VqaError(st, "vqa_create(device=%d)" % device)
        self.ctx = ctx
        self.device = int(device)

    def close(self):
        if getattr(self, "ctx", None):
            for p in getattr(self, "_pinned", []):
                self.lib.vqa_free_pinned(self.ctx, p)
            self._pinned = []
            self.lib.vqa_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- memory ----------------------------------------------------------
    def upload(self, arr):
        """Copy a host uint8 array [n,h,w,3] (or [n,h,w]) to device memory.  A uint16 array (9..16-bit planar frames, e.g.
        [n, samples]) keeps its samples: DeviceFrames with itemsize 2."""
        arr = np.asarray(arr)
        arr = np.ascontiguousarray(arr, dtype=np.uint16 if arr.dtype == np.uint16 else np.uint8)
        if arr.ndim == 2:
            arr = arr[:, None, :]
        buf = DeviceBuffer(self, arr.nbytes)
        N.check(self.lib.vqa_copy_h2d(self.ctx, buf.ptr, arr.ctypes.data, arr.nbytes), "vqa_copy_h2d", self.ctx)
        N.check(self.lib.vqa_sync(self.ctx), "vqa_sync", self.ctx)
        ch = arr.shape[3] if arr.ndim == 4 else 1
        return DeviceFrames(buf.ptr, arr.shape[0], arr.shape[1], arr.shape[2], owner=buf, channels=ch, itemsize=arr.itemsize)

    def alloc_pinned(self, shape, dtype=np.uint8):
        """A NumPy array backed by page-locked host memory (hipHostMalloc): H2D from it is a true async DMA.
        The memory lives until the engine is closed."""
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = C.c_void_p()
        N.check(self.lib.vqa_alloc_pinned(self.ctx, max(nbytes, 1), C.byref(p)), "vqa_alloc_pinned", self.ctx)
        self._pinned = getattr(self, "_pinned", [])
        self._pinned.append(p.value)
        raw = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(max(nbytes, 1),))
        return raw[:nbytes].view(dtype).reshape(shape)

    def free_pinned(self, arr):
        """Give back an array alloc_pinned returned (it must not be used afterwards)."""
        p = arr.ctypes.data if hasattr(arr, "ctypes") else int(arr)
        if p in getattr(self, "_pinned", []):
            self._pinned.remove(p)
            N.check(self.lib.vqa_free_pinned(self.ctx, p), "vqa_free_pinned", self.ctx)

    def is_pinned(self, arr):
        """True if the array's memory - ALL of it, first byte to last - is page-locked and known to HIP (alloc_pinned, torch
        pin_memory, hipHostRegister): a submit / h2d from it is an asynchronous DMA; pageable memory, and an array that
        only starts inside a registered region, is staged through a pinned ring (stream.py)."""
        if getattr(arr, "nbytes", 0) == 0:
            return False
        if any(st < 0 for st in arr.strides):
            return False
        span = sum((n - 1) * st for n, st in zip(arr.shape, arr.strides)) + arr.itemsize  # first byte .. last byte of a strided view
        out = C.c_int(0)
        N.check(self.lib.vqa_host_is_pinned(self.ctx, arr.ctypes.data, span, C.byref(out)), "vqa_host_is_pinned", self.ctx)
        return bool(out.value)

    def h2d_async(self, dst_ptr, src_ptr, nbytes):
        """Enqueue a host-to-device copy on the engine's stream (a true DMA when the source is pinned)."""
        if nbytes:
            N.check(self.lib.vqa_copy_h2d(self.ctx, int(dst_ptr), int(src_ptr), int(nbytes)), "vqa_copy_h2d", self.ctx)

    def sync(self):
        N.check(self.lib.vqa_sync(self.ctx), "vqa_sync", self.ctx)

    def wait_for(self, other):
        """vqa_stream_wait: what is enqueued on this engine from now on starts after what `other` (an engine of the same device,
        e.g. the pass's copy lane) has enqueued so far - a device-side dependency, the host does not wait."""
        N.check(self.lib.vqa_stream_wait(self.ctx, other.ctx), "vqa_stream_wait", self.ctx)

    def drain(self):
        """Wait out whatever this engine still has pending (a quality, a VIF, an ADM, a motion, an SI/TI, a PSNR-HVS, a CIEDE2000, a GMSD, a CAMBI, an XPSNR, a HaarPSI, a VCA, an artefacts, a BRISQUE, an MDSI, a dE_ITP, a PU21, an FSIM, a sigstats, a scale and / or a complexity batch), discard the results and
        synchronise its streams: after a failure in the caller's loop nothing reads the caller's buffers any more and the
        engine is usable again.  Never raises."""
        for pend in list(_BATCHES) + ["_pending_c", "_pending_k", "_pending_l", "_pending_j", "_pending_o", "_pending_sg", "_pending_sx", "_pending_cf", "_pending_cm", "_pending_cv", "_pending_fd", "_pending_wv"]:
            try:
                if getattr(self, pend, None):
                    {"_pending_c": self.complexity_wait, "_pending_x": self.xpsnr_wait, "_pending_t": self.vca_wait,
                     "_pending_z": self.sigstats_wait, "_pending_k": self.scale_wait,
                     "_pending_l": self.align_wait, "_pending_j": self.shift_wait,
                     "_pending_o": self.light_wait, "_pending_sg": self.signature_wait,
                     "_pending_sx": self.sig_cross_wait, "_pending_cf": self.colorfit_wait,
                     "_pending_cm": self.conform_wait, "_pending_cv": self.convert_wait,
                     "_pending_fd": self.fields_wait, "_pending_wv": self.weave_wait}.get(pend, lambda: self._batch_wait(pend))()
            except Exception:
                setattr(self, pend, None)
        try:
            self.sync()
        except Exception:
            pass

    def trim(self):
        """vqa_trim: give back every scratch buffer, the result staging and every cached table of this (idle) engine.
        The next submit re-grows what it needs; results are unaffected."""
        N.check(self.lib.vqa_trim(self.ctx), "vqa_trim", self.ctx)

    # ---- options (include/vqa.h: none of them changes a result) --------------
    def set_option(self, option, value):
        N.check(self.lib.vqa_set_option(self.ctx, int(option), int(value)), "vqa_set_option", self.ctx)

    def get_option(self, option):
        v = C.c_int(0)
        N.check(self.lib.vqa_get_option(self.ctx, int(option), C.byref(v)), "vqa_get_option", self.ctx)
        return v.value

    def set_overlap(self, on):
        """Block-SAD and the Canny chain on side streams inside a complexity submit (default on)."""
        self.set_option(N.OPT_OVERLAP, 1 if on else 0)

    @property
    def stream(self):
        return self.lib.vqa_stream(self.ctx)

    # ---- complexity --------------------------------------------------------
    def make_params(self, resize=None, canny=(100, 200), sad_range=7, dct_mode=N.DCT_AUTO, motion_mode=N.MOTION_SAD):
        p = N.VqaParams()
        self.lib.vqa_default_params(C.byref(p))
        if resize:
            p.resize_w, p.resize_h = int(resize[0]), int(resize[1])
        p.canny_low, p.canny_high = int(canny[0]), int(canny[1])
        p.sad_range = int(sad_range)
        p.dct_mode = int(dct_mode)
        p.motion_mode = int(motion_mode)
        return p

    @staticmethod
    def _frames_args(frames, prev0):
        if isinstance(frames, DeviceFrames):
            if prev0 is not None and not isinstance(prev0, DeviceFrames):
                raise TypeError("prev0 must live where frames live (device)")
            pp = prev0.ptr if prev0 is not None else None
            return (frames.ptr, pp, N.VQA_MEM_DEVICE, frames.n, frames.h, frames.w, frames.frame_stride,
                    frames.row_stride, (frames, prev0))
        arr = np.asarray(frames)
        if arr.dtype != np.uint8:  # a silent cast would turn float frames in 0..1 into all-zero planes
            raise ValueError("frames must be uint8 (got %s): decoded 8-bit BGR frames, as cv2.VideoCapture.read yields" % arr.dtype)
        if arr.ndim == 3:
            arr = arr[None]
        if arr.ndim != 4 or arr.shape[3] != 3:
            raise ValueError("frames must be uint8 [n,h,w,3] packed BGR")
        # a strided selection of whole frames (clip[k-1::k]) and a region of interest (clip[:, y0:y1, x0:x1])
        # are passed as they are: frame_stride / row_stride do the stepping
        h_, w_ = arr.shape[1], arr.shape[2]
        st = arr.strides
        if not (st[2:] == (3, 1) and st[1] >= w_ * 3 and (arr.shape[0] == 1 or st[0] >= (h_ - 1) * st[1] + w_ * 3)):
            arr = np.ascontiguousarray(arr)
        rstride = arr.strides[1] if h_ > 1 else w_ * 3
        keep = [arr]
        pp = None
        if prev0 is not None:
            p0 = np.asarray(prev0)
            if p0.dtype != np.uint8:
                raise ValueError("prev0 must be uint8 (got %s)" % p0.dtype)
            if p0.shape != arr.shape[1:]:
                raise ValueError("prev0 must have the frames' geometry")
            if not (p0.strides[1:] == (3, 1) and (h_ == 1 or p0.strides[0] == rstride)):
                if rstride != w_ * 3:  # one row stride serves frames and prev0: fall back to compact copies
                    arr = np.ascontiguousarray(arr)
                    rstride = w_ * 3
                    keep[0] = arr
                p0 = np.ascontiguousarray(p0)
            keep.append(p0)
            pp = p0.ctypes.data
        n, h, w, _ = arr.shape
        fstride = arr.strides[0] if n > 1 else max(h * rstride, 1)
        return (arr.ctypes.data, pp, N.VQA_MEM_HOST, n, h, w, fstride, rstride, keep)

    def complexity_submit(self, frames, prev0=None, mask=N.M_ALL, params=None):
        fp, pp, kind, n, h, w, fs, rs, keep = self._frames_args(frames, prev0)
        params = params or self.make_params()
        st = self.lib.vqa_complexity_submit(self.ctx, fp, pp, kind, n, h, w, fs, rs, mask, C.byref(params))
        N.check(st, "vqa_complexity_submit", self.ctx)
        self._pending_c = (n, keep)
        return n

    def complexity_wait(self):
        n, _keep = self._pending_c
        out = np.zeros(n, dtype=FRAME_DTYPE)
        st = self.lib.vqa_complexity_wait(self.ctx, out.ctypes.data_as(C.POINTER(N.VqaFrameMetrics)), n)
        self._pending_c = None
        N.check(st, "vqa_complexity_wait", self.ctx)
        return out

    def complexity(self, frames, prev0=None, mask=N.M_ALL, params=None, **kw):
        """Run the selected complexity kernels over a batch; returns a structured array (FRAME_DTYPE)."""
        if params is None:
            params = self.make_params(**kw)
        self.complexity_submit(frames, prev0, mask, params)
        return self.complexity_wait()

    # ---- quality -----------------------------------------------------------
    def quality_submit(self, ref, dist, planes, ssim_mode=N.SSIM_GAUSS, frame_bytes=None):
        """planes: (width, height, offset, row_stride, pixel_step[, bit_depth]) per plane, in bytes.  8-bit planes read uint8
        frames; 9..16-bit planes (yuv_planes(.., depth=10) ...) read uint16 frames (host arrays or DeviceFrames of itemsize 2),
        passed through as they are: a frame of the other sample type is a ValueError, not a cast."""
        self._batch_submit("_pending_q", self._pair_args(ref, dist, planes, frame_bytes), planes, ssim_mode)

    @staticmethod
    def _stream_arg(a, planes, device, what="frames"):
        """one stream of a plane-batch submit, resident where `device` says -> (pointer, what to keep alive: the DeviceFrames or
        the contiguous host array).  Its samples must be what the planes' depth says: the other type is an error, not a cast."""
        depth = planes_depth(planes)
        wide, want = depth > 8, "uint16" if depth > 8 else "uint8"
        if device:
            if (a.itemsize == 2) != wide:
                raise ValueError("%d-bit planes need frames of %s samples (got DeviceFrames of itemsize %d)" % (depth, want, a.itemsize))
            return a.ptr, a
        a = np.asarray(a)
        if wide != (a.dtype == np.uint16):
            raise ValueError("%d-bit planes need %s %s (got %s)" % (depth, "a " + want if what == "prev0" else want, what, a.dtype))
        a = np.ascontiguousarray(a, dtype=np.uint16 if wide else np.uint8)
        return a.ctypes.data, a

    def _pair_args(self, ref, dist, planes, frame_bytes=None):
        """the (ref, dist) pair of a quality / VIF / ADM / PSNR-HVS / CIEDE2000 / GMSD / HaarPSI / MDSI / dE_ITP / PU21 / FSIM submit -> (ref ptr, dist ptr, mem kind, n, frame strides, what to keep alive)"""
        dev = isinstance(ref, DeviceFrames)
        if dev:
            assert isinstance(dist, DeviceFrames) and ref.n == dist.n
        rp, ref = self._stream_arg(ref, planes, dev)
        dp, dist = self._stream_arg(dist, planes, dev)
        if dev:
            return rp, dp, N.VQA_MEM_DEVICE, ref.n, ref.frame_stride, dist.frame_stride, (ref, dist)
        if ref.shape != dist.shape:
            raise ValueError("ref and dist must have the same shape")
        n = ref.shape[0]
        fs = frame_bytes or (ref.nbytes // n)
        return rp, dp, N.VQA_MEM_HOST, n, fs, fs, (ref, dist)

    def _batch_submit(self, slot, streams, planes, *mode, n=None):
        """streams: what _pair_args / _ref_args / _one_stream_args gave - the C arguments up to the frame strides, then what to
        keep alive.  n: the batch's frames; None: the fourth argument, where _pair_args and _ref_args have it"""
        *args, keep = streams
        sub = _BATCHES[slot][0]
        st = getattr(self.lib, sub)(self.ctx, *args, plane_descs(planes), len(planes), *mode)
        N.check(st, sub, self.ctx)
        setattr(self, slot, (args[3] if n is None else n, len(planes), keep))

    def _batch_wait(self, slot):
        """-> the pending batch's [n, n_planes] records; the slot is free again whatever the status"""
        _sub, wait, dtype, ctype = _BATCHES[slot]
        n, npl, _keep = getattr(self, slot)
        out = np.zeros(n * npl, dtype=dtype)
        st = getattr(self.lib, wait)(self.ctx, out.ctypes.data_as(C.POINTER(ctype)), n * npl)
        setattr(self, slot, None)
        N.check(st, wait, self.ctx)
        return out.reshape(n, npl)

    def quality_wait(self, scales=False):
        """-> [n, n_planes] records (PLANE_DTYPE).  scales=True (after an SSIM_MS submit only): -> (records, cs, ssim) with the
        per-scale means as float64 [n, n_planes, 5], level 0 first (vqa_quality_wait_ms)."""
        if not scales:
            return self._batch_wait("_pending_q")
        n, npl, _keep = self._pending_q
        out = np.zeros(n * npl, dtype=PLANE_DTYPE)
        sc = np.zeros((n * npl, 2, N.MS_LEVELS), np.float64)   # vqa_ms_scales: cs[5], ssim[5]
        st = self.lib.vqa_quality_wait_ms(self.ctx, out.ctypes.data_as(C.POINTER(N.VqaPlaneMetrics)),
                                          sc.ctypes.data_as(C.POINTER(N.VqaMsScales)), n * npl)
        if st != N.VQA_ERR_STATE:   # (a refusal for a batch that is not multi-scale leaves the batch pending)
            self._pending_q = None
        N.check(st, "vqa_quality_wait_ms", self.ctx)
        return (out.reshape(n, npl), np.ascontiguousarray(sc[:, 0]).reshape(n, npl, N.MS_LEVELS),
                np.ascontiguousarray(sc[:, 1]).reshape(n, npl, N.MS_LEVELS))

    def quality(self, ref, dist, planes, ssim_mode=N.SSIM_GAUSS, frame_bytes=None, scales=False):
        """SSE + SSIM per plane for n frame pairs; returns [n, n_planes] structured array (PLANE_DTYPE).  ssim_mode SSIM_MS:
        the ssim field is MS-SSIM (planes of at least 161 x 161), and scales=True adds the per-scale cs and ssim means."""
        self.quality_submit(ref, dist, planes, ssim_mode, frame_bytes)
        return self.quality_wait(scales)

    # ---- VIF ---------------------------------------------------------------
    def vif_submit(self, ref, dist, planes, frame_bytes=None):
        """VIF on four scales for n frame pairs (vqa_vif_submit): the arrays / DeviceFrames and plane tuples of
        quality_submit; every plane at least 16 x 16.  A batch of its own: it may follow a quality_submit of the same frames
        before either is waited for."""
        self._batch_submit("_pending_v", self._pair_args(ref, dist, planes, frame_bytes), planes)

    def vif_wait(self):
        """-> [n, n_planes] records (VIF_DTYPE): num[4], den[4], scale[4] (libvmaf's vif_scale0..3) and vif."""
        return self._batch_wait("_pending_v")

    def vif(self, ref, dist, planes, frame_bytes=None):
        """VIF per plane on four scales for n frame pairs; returns [n, n_planes] structured array (VIF_DTYPE)."""
        self.vif_submit(ref, dist, planes, frame_bytes)
        return self.vif_wait()

    # ---- ADM ---------------------------------------------------------------
    def adm_submit(self, ref, dist, planes, frame_bytes=None):
        """ADM on four scales for n frame pairs (vqa_adm_submit): the arrays / DeviceFrames and plane tuples of
        quality_submit; every plane at least 16 x 16.  A batch of its own: it may follow a quality_submit and a vif_submit of
        the same frames before any of them is waited for."""
        self._batch_submit("_pending_a", self._pair_args(ref, dist, planes, frame_bytes), planes)

    def adm_wait(self):
        """-> [n, n_planes] records (ADM_DTYPE): num[4], den[4], scale[4] (libvmaf's adm_scale0..3) and adm2."""
        return self._batch_wait("_pending_a")

    def adm(self, ref, dist, planes, frame_bytes=None):
        """ADM per plane on four scales for n frame pairs; returns [n, n_planes] structured array (ADM_DTYPE)."""
        self.adm_submit(ref, dist, planes, frame_bytes)
        return self.adm_wait()

    # ---- VMAF's motion feature -------------------------------------------------
    def _ref_args(self, ref, planes, prev0, frame_bytes=None):
        """the reference frames (and the frame before them) of a motion or an SI/TI submit -> (ref ptr, prev0 ptr or None, mem kind, n,
        frame stride, what to keep alive)"""
        dev = isinstance(ref, DeviceFrames)
        if prev0 is not None and isinstance(prev0, DeviceFrames) != dev:
            raise TypeError("prev0 must live where ref lives (%s)" % ("device" if dev else "host"))
        rp, ref = self._stream_arg(ref, planes, dev)
        pp, p0 = self._stream_arg(prev0, planes, dev, "prev0") if prev0 is not None else (None, None)
        if dev:
            return rp, pp, N.VQA_MEM_DEVICE, ref.n, ref.frame_stride, (ref, p0)
        n = ref.shape[0]
        if p0 is not None and p0.nbytes != ref.nbytes // n:
            raise ValueError("prev0 must have the frames' layout (%d bytes, got %d)" % (ref.nbytes // n, p0.nbytes))
        return rp, pp, N.VQA_MEM_HOST, n, frame_bytes or (ref.nbytes // n), (ref, p0)

    def motion_submit(self, ref, planes, prev0=None, frame_bytes=None):
        """VMAF's motion feature for n reference frames (vqa_motion_submit): frame i against frame i - 1, frame 0 against
        prev0 (None: it has no predecessor and scores 0).  The arrays / DeviceFrames and plane tuples of vif_submit - the
        reference stream alone; every plane at least 16 x 16.  A batch of its own: it may follow a quality_submit, a vif_submit
        and an adm_submit of the same frames before any of them is waited for."""
        self._batch_submit("_pending_m", self._ref_args(ref, planes, prev0, frame_bytes), planes)

    def motion_wait(self):
        """-> [n, n_planes] records (MOTION_DTYPE): sad, the sum of |blur(frame) - blur(previous frame)| over the plane, and
        motion = sad / (h w), libvmaf's `motion`.  (motion2 needs the next frame: tails.motion2 over the whole clip.)"""
        return self._batch_wait("_pending_m")

    def motion(self, ref, planes, prev0=None, frame_bytes=None):
        """VMAF's motion feature per plane for n reference frames; returns [n, n_planes] structured array (MOTION_DTYPE)."""
        self.motion_submit(ref, planes, prev0, frame_bytes)
        return self.motion_wait()

    # ---- ITU-T P.910 spatial and temporal information -----------------------------
    def siti_submit(self, ref, planes, prev0=None, frame_bytes=None):
        """P.910's SI and TI for n reference frames (vqa_siti_submit): Sobel on the interior of frame i, and frame i against
        frame i - 1, frame 0 against prev0 (None: it has no predecessor and its ti is 0).  The arguments of motion_submit - the
        reference stream alone; every plane at least 16 x 16.  A batch of its own: it may follow a quality_submit, a vif_submit,
        an adm_submit and a motion_submit of the same frames before any of them is waited for."""
        self._batch_submit("_pending_s", self._ref_args(ref, planes, prev0, frame_bytes), planes)

    def siti_wait(self):
        """-> [n, n_planes] records (SITI_DTYPE): the four integer sums (grad_sum in 2^-32 fixed point, as a double), si and ti
        on the 8-bit scale.  (P.910's clip values are the maxima over the frames.)"""
        return self._batch_wait("_pending_s")

    def siti(self, ref, planes, prev0=None, frame_bytes=None):
        """P.910's SI and TI per plane for n reference frames; returns [n, n_planes] structured array (SITI_DTYPE)."""
        self.siti_submit(ref, planes, prev0, frame_bytes)
        return self.siti_wait()

    # ---- PSNR-HVS and PSNR-HVS-M ------------------------------------------------
    def psnr_hvs_submit(self, ref, dist, planes, frame_bytes=None):
        """PSNR-HVS and PSNR-HVS-M for n frame pairs (vqa_psnr_hvs_submit): the arrays / DeviceFrames and plane tuples of
        quality_submit; every plane at least 16 x 16, and only its whole 8x8 blocks are looked at.  A batch of its own: it may
        follow a quality_submit, a vif_submit, an adm_submit, a motion_submit and a siti_submit of the same frames before any of
        them is waited for."""
        self._batch_submit("_pending_h", self._pair_args(ref, dist, planes, frame_bytes), planes)

    def psnr_hvs_wait(self):
        """-> [n, n_planes] records (PSNR_HVS_DTYPE): s_hvs and s_hvsm, the two CSF-weighted mean squared errors, and psnr_hvs
        and psnr_hvsm in dB (inf for identical planes)."""
        return self._batch_wait("_pending_h")

    def psnr_hvs(self, ref, dist, planes, frame_bytes=None):
        """PSNR-HVS and PSNR-HVS-M per plane for n frame pairs; returns [n, n_planes] structured array (PSNR_HVS_DTYPE)."""
        self.psnr_hvs_submit(ref, dist, planes, frame_bytes)
        return self.psnr_hvs_wait()

    # ---- CIEDE2000 --------------------------------------------------------------
    @staticmethod
    def ciede_model(planes):
        """the colour model a plane list implies: CIEDE_BGR for three planes whose pixel step is 3 samples (packed bgr24 and its
        16-bit kin), CIEDE_YUV709 otherwise"""
        bps = 2 if planes_depth(planes) > 8 else 1
        return N.CIEDE_BGR if len(planes) == 3 and all(int(p[4]) == 3 * bps for p in planes) else N.CIEDE_YUV709

    def ciede_submit(self, ref, dist, planes, model=None, weights=N.CIEDE_WEIGHTS_CIE, frame_bytes=None):
        """CIEDE2000 for n frame pairs (vqa_ciede_submit): the arrays / DeviceFrames and plane tuples of quality_submit, exactly
        THREE planes taken together per pixel - Y, U, V (BT.709 limited range; U and V of the luma's size or its ceil-half in
        either direction) or B, G, R; luma at least 16 x 16.  model: N.CIEDE_YUV709 | N.CIEDE_BGR | None (ciede_model(planes)).
        weights: (kL, kC, kH), positive and finite; (1, 1, 1) is the CIE standard, N.CIEDE_WEIGHTS_LIBVMAF = (0.65, 1, 4) what
        libvmaf's ciede2000 feature is believed to use (unverified).  A batch of its own, like psnr_hvs_submit."""
        if model is None:
            model = self.ciede_model(planes)
        if weights is not None and len(weights) != 3:
            raise ValueError("weights must be (kL, kC, kH)")
        k = (C.c_double * 3)(*[float(x) for x in weights]) if weights is not None else None
        *args, keep = self._pair_args(ref, dist, planes, frame_bytes)
        st = self.lib.vqa_ciede_submit(self.ctx, *args, plane_descs(planes), len(planes), int(model), k)
        N.check(st, "vqa_ciede_submit", self.ctx)
        self._pending_e = (args[3], 1, keep)

    def ciede_wait(self):
        """-> [n] records (CIEDE_DTYPE), one per frame: de_sum, de_mean (the mean dE00 over the luma grid) and ciede2000 =
        45 - 20 log10(de_mean) (inf for identical frames)."""
        return self._batch_wait("_pending_e").reshape(-1)

    def ciede(self, ref, dist, planes, model=None, weights=N.CIEDE_WEIGHTS_CIE, frame_bytes=None):
        """CIEDE2000 per frame for n frame pairs; returns [n] structured array (CIEDE_DTYPE)."""
        self.ciede_submit(ref, dist, planes, model, weights, frame_bytes)
        return self.ciede_wait()

    # ---- GMSD --------------------------------------------------------------------
    def gmsd_submit(self, ref, dist, planes, frame_bytes=None):
        """GMSD for n frame pairs (vqa_gmsd_submit): the arrays / DeviceFrames and plane tuples of quality_submit, every plane
        measured by itself and at least 16 x 16.  A batch of its own, like psnr_hvs_submit."""
        self._batch_submit("_pending_g", self._pair_args(ref, dist, planes, frame_bytes), planes)

    def gmsd_wait(self):
        """-> [n, n_planes] records (GMSD_DTYPE): the three integer words (sum_u, sum_u2_lo, sum_u2_hi), count, gms_mean and
        gmsd (exactly 1 and 0 for identical planes)."""
        return self._batch_wait("_pending_g")

    def gmsd(self, ref, dist, planes, frame_bytes=None):
        """GMSD per plane for n frame pairs; returns [n, n_planes] structured array (GMSD_DTYPE)."""
        self.gmsd_submit(ref, dist, planes, frame_bytes)
        return self.gmsd_wait()

    # ---- HaarPSI -----------------------------------------------------------------
    def haarpsi_submit(self, ref, dist, planes, frame_bytes=None):
        """HaarPSI for n frame pairs (vqa_haarpsi_submit): the arrays / DeviceFrames and plane tuples of quality_submit, every
        plane measured by itself and at least 16 x 16.  A batch of its own, like gmsd_submit."""
        self._batch_submit("_pending_w", self._pair_args(ref, dist, planes, frame_bytes), planes)

    def haarpsi_wait(self):
        """-> [n, n_planes] records (HAARPSI_DTYPE): the three integer words (den, num_lo, num_hi), similarity and haarpsi
        (exactly 1 for identical planes)."""
        return self._batch_wait("_pending_w")

    def haarpsi(self, ref, dist, planes, frame_bytes=None):
        """HaarPSI per plane for n frame pairs; returns [n, n_planes] structured array (HAARPSI_DTYPE)."""
        self.haarpsi_submit(ref, dist, planes, frame_bytes)
        return self.haarpsi_wait()

    # ---- XPSNR --------------------------------------------------------------------
    def xpsnr_submit(self, ref, dist, planes, prev0=None, frame_bytes=None):
        """XPSNR for n frame pairs (vqa_xpsnr_submit): the arrays / DeviceFrames and plane tuples of quality_submit - a planar
        layout whose first plane is the luma, the others of its size or its ceil-half, every plane at least 16 x 16 - and prev0
        as in siti_submit: the REFERENCE frame before frame 0, resident where the frames are (None: frame 0 has no predecessor
        and its temporal activity is 0).  A batch of its own, like gmsd_submit."""
        check_xpsnr_planes(planes)
        rp, dp, kind, n, rfs, dfs, keep = self._pair_args(ref, dist, planes, frame_bytes)
        dev = kind == N.VQA_MEM_DEVICE
        if prev0 is not None and isinstance(prev0, DeviceFrames) != dev:
            raise TypeError("prev0 must live where ref lives (%s)" % ("device" if dev else "host"))
        pp, p0 = self._stream_arg(prev0, planes, dev, "prev0") if prev0 is not None else (None, None)
        if p0 is not None and not dev and p0.nbytes != keep[0].nbytes // n:
            raise ValueError("prev0 must have the frames' layout (%d bytes, got %d)" % (keep[0].nbytes // n, p0.nbytes))
        self._batch_submit("_pending_x", (rp, dp, pp, kind, n, rfs, dfs, keep + (p0,)), planes, n=n)
        self._xpsnr_luma = (int(planes[0][0]), int(planes[0][1]))   # of the pending batch: the block grid follows from it

    def xpsnr_wait(self, blocks=False):
        """-> [n, n_planes] records (XPSNR_DTYPE): sse (the plain total), wsse, xpsnr in dB (inf for identical planes), block,
        nbx, nby.  blocks=True: -> (records, map) with the integer words behind them, map = dict(sa, ta, n as uint64
        [n, nby, nbx]; sse as uint64 [n, n_planes, nby, nbx]; act as float64 [n, nby, nbx], the blocks' a_k before the floor
        a_min: (sa + 2 ta) / (s n), 0 where n = 0)."""
        n, npl, _keep = self._pending_x
        w, h = self._xpsnr_luma
        _b, nbx, nby = xpsnr_grid(w, h)
        nb = nbx * nby
        rec = np.zeros(n * npl, dtype=XPSNR_DTYPE)
        words = np.zeros((n, (3 + npl) * nb), np.uint64) if blocks else None
        st = self.lib.vqa_xpsnr_wait(self.ctx, rec.ctypes.data_as(C.POINTER(N.VqaXpsnrMetrics)), n * npl,
                                     words.ctypes.data_as(C.POINTER(C.c_uint64)) if blocks else None, words.size if blocks else 0)
        self._pending_x = None
        N.check(st, "vqa_xpsnr_wait", self.ctx)
        rec = rec.reshape(n, npl)
        if not blocks:
            return rec
        tri = words[:, :3 * nb].reshape(n, nby, nbx, 3)
        sa, ta, cnt = (np.ascontiguousarray(tri[..., i]) for i in range(3))
        s = 1.0 if w * h <= 2048 * 1152 else 4.0
        act = np.divide((sa + 2 * ta).astype(np.float64), s * cnt.astype(np.float64), out=np.zeros(sa.shape, np.float64),
                        where=cnt > 0)
        return rec, dict(sa=sa, ta=ta, n=cnt, sse=np.ascontiguousarray(words[:, 3 * nb:]).reshape(n, npl, nby, nbx), act=act)

    def xpsnr(self, ref, dist, planes, prev0=None, blocks=False, frame_bytes=None):
        """XPSNR per plane for n frame pairs; returns [n, n_planes] structured array (XPSNR_DTYPE), with blocks=True also the
        weight map (xpsnr_wait)."""
        self.xpsnr_submit(ref, dist, planes, prev0, frame_bytes)
        return self.xpsnr_wait(blocks)

    # ---- VCA texture features -------------------------------------------------------
    def vca_submit(self, ref, planes, prev0=None, frame_bytes=None):
        """VCA's E, h and L for n reference frames (vqa_vca_submit): the weighted 32 x 32 block DCT of every plane of frame i, and
        its blocks against those of frame i - 1, frame 0 against prev0 (None: it has no predecessor and its h is 0).  The
        arguments of siti_submit - the reference stream alone; a planar layout, every plane at least 32 x 32.  A batch of its
        own, like siti_submit."""
        check_vca_planes(planes)
        self._batch_submit("_pending_t", self._ref_args(ref, planes, prev0, frame_bytes), planes)
        self._vca_grids = [vca_grid(p[0], p[1]) for p in planes]   # of the pending batch

    def vca_wait(self, blocks=False):
        """-> [n, n_planes] records (VCA_DTYPE): the three integer words e_sum, h_sum, l_sum, the block grid nbx, nby, and e, h, l
        on the 8-bit scale.  blocks=True: -> (records, maps) with the block map behind them, maps = one dict(qh, s as uint64
        [n, nby, nbx]) per plane."""
        n, npl, _keep = self._pending_t
        nb = [gx * gy for gx, gy in self._vca_grids]
        rec = np.zeros(n * npl, dtype=VCA_DTYPE)
        words = np.zeros((n, 2 * sum(nb)), np.uint64) if blocks else None
        st = self.lib.vqa_vca_wait(self.ctx, rec.ctypes.data_as(C.POINTER(N.VqaVcaMetrics)), n * npl,
                                   words.ctypes.data_as(C.POINTER(C.c_uint64)) if blocks else None, words.size if blocks else 0)
        self._pending_t = None
        N.check(st, "vqa_vca_wait", self.ctx)
        rec = rec.reshape(n, npl)
        if not blocks:
            return rec
        maps, at = [], 0
        for (gx, gy), c in zip(self._vca_grids, nb):
            pairs = words[:, at:at + 2 * c].reshape(n, gy, gx, 2)
            maps.append(dict(qh=np.ascontiguousarray(pairs[..., 0]), s=np.ascontiguousarray(pairs[..., 1])))
            at += 2 * c
        return rec, maps

    def vca(self, ref, planes, prev0=None, blocks=False, frame_bytes=None):
        """VCA's texture features per plane for n reference frames; returns [n, n_planes] structured array (VCA_DTYPE), with
        blocks=True also the block maps (vca_wait)."""
        self.vca_submit(ref, planes, prev0, frame_bytes)
        return self.vca_wait(blocks)

    def _one_stream_args(self, frames, planes, frame_bytes=None):
        """the frames of a submit that reads one stream and no frame before it -> (ptr, mem kind, n, frame stride, what to keep
        alive)"""
        dev = isinstance(frames, DeviceFrames)
        fp, frames = self._stream_arg(frames, planes, dev)
        if dev:
            return fp, N.VQA_MEM_DEVICE, frames.n, frames.frame_stride, frames
        n = frames.shape[0]
        return fp, N.VQA_MEM_HOST, n, frame_bytes or (frames.nbytes // n), frames

    # ---- CAMBI ---------------------------------------------------------------------
    def cambi_submit(self, frames, planes, frame_bytes=None):
        """CAMBI, the banding index, for n frames of ONE stream (vqa_cambi_submit): an array / DeviceFrames and the plane tuples
        of quality_submit, every plane measured by itself and at least 16 x 16.  A batch of its own, like gmsd_submit."""
        streams = self._one_stream_args(frames, planes, frame_bytes)
        self._batch_submit("_pending_b", streams, planes, n=streams[2])

    def cambi_wait(self):
        """-> [n, n_planes] records (CAMBI_DTYPE): per scale the integer words top, k and masked, pool = top / (k 2^16), and
        cambi (exactly 0 for a plane without banding)."""
        return self._batch_wait("_pending_b")

    def cambi(self, frames, planes, frame_bytes=None):
        """CAMBI per plane for n frames; returns [n, n_planes] structured array (CAMBI_DTYPE)."""
        self.cambi_submit(frames, planes, frame_bytes)
        return self.cambi_wait()

    # ---- blockiness, blur and noise -------------------------------------------------
    def artifacts_submit(self, frames, planes, frame_bytes=None):
        """No-reference blockiness, blur and noise for n frames of ONE stream (vqa_artifacts_submit): the arguments of
        cambi_submit - an array / DeviceFrames (uint16 above 8 bits; a dtype that does not match the depth is a ValueError) and
        the plane tuples of quality_submit, every plane measured by itself and at least 16 x 16.  A batch of its own, like
        cambi_submit."""
        streams = self._one_stream_args(frames, planes, frame_bytes)
        self._batch_submit("_pending_r", streams, planes, n=streams[2])

    def artifacts_wait(self):
        """-> [n, n_planes] records (ARTIFACTS_DTYPE): the 21 integer words edge_h[8], edge_v[8], blur_f_h, blur_v_h, blur_f_v,
        blur_v_v, lap; phase_h, phase_v; blockiness, blockiness_max, blur_h, blur_v, blur, noise (include/vqa.h)."""
        return self._batch_wait("_pending_r")

    def artifacts(self, frames, planes, frame_bytes=None):
        """Blockiness, blur and noise per plane for n frames; returns [n, n_planes] structured array (ARTIFACTS_DTYPE)."""
        self.artifacts_submit(frames, planes, frame_bytes)
        return self.artifacts_wait()

    # ---- BRISQUE's natural-scene statistics ------------------------------------------
    def brisque_submit(self, frames, planes, frame_bytes=None):
        """BRISQUE's 36 natural-scene statistics for n frames of ONE stream (vqa_brisque_submit): the arguments of cambi_submit
        - an array / DeviceFrames (uint16 above 8 bits; a dtype that does not match the depth is a ValueError) and the plane
        tuples of quality_submit, every plane measured by itself and at least 16 x 16.  A batch of its own, like cambi_submit."""
        streams = self._one_stream_args(frames, planes, frame_bytes)
        self._batch_submit("_pending_n", streams, planes, n=streams[2])

    def brisque_wait(self):
        """-> [n, n_planes] records (BRISQUE_DTYPE): the 60 integer words ([scale] or [scale, orientation]), flags and
        features [36] (include/vqa.h)."""
        return self._batch_wait("_pending_n")

    def brisque(self, frames, planes, frame_bytes=None):
        """BRISQUE's features per plane for n frames; returns [n, n_planes] structured array (BRISQUE_DTYPE)."""
        self.brisque_submit(frames, planes, frame_bytes)
        return self.brisque_wait()

    # ---- MDSI -------------------------------------------------------------------
    @staticmethod
    def mdsi_model(planes):
        """the colour model a plane list implies: MDSI_GRAY for one plane, MDSI_BGR for three planes whose pixel step is 3
        samples (packed bgr24 and its 16-bit kin), MDSI_YUV709 otherwise"""
        if len(planes) == 1:
            return N.MDSI_GRAY
        bps = 2 if planes_depth(planes) > 8 else 1
        return N.MDSI_BGR if len(planes) == 3 and all(int(p[4]) == 3 * bps for p in planes) else N.MDSI_YUV709

    def mdsi_submit(self, ref, dist, planes, model=None, frame_bytes=None):
        """MDSI for n frame pairs (vqa_mdsi_submit): the arrays / DeviceFrames and plane tuples of ciede_submit - THREE planes
        taken together per pixel, Y, U, V (BT.709 limited range; U and V of the luma's size or its ceil-half in either direction)
        or B, G, R - or ONE plane Y; plane 0 at least 16 x 16.  model: N.MDSI_YUV709 | N.MDSI_BGR | N.MDSI_GRAY | None
        (mdsi_model(planes)).  (ref, dist) is ordered: the metric is not symmetric.  A batch of its own, like ciede_submit."""
        if model is None:
            model = self.mdsi_model(planes)
        *args, keep = self._pair_args(ref, dist, planes, frame_bytes)
        st = self.lib.vqa_mdsi_submit(self.ctx, *args, plane_descs(planes), len(planes), int(model))
        N.check(st, "vqa_mdsi_submit", self.ctx)
        self._pending_d = (args[3], 1, keep)

    def mdsi_wait(self):
        """-> [n] records (MDSI_DTYPE), one per frame: the four integer words, count, factor, dev (the mean absolute deviation;
        exactly 0 for identical frames) and mdsi = dev^(1/4)."""
        return self._batch_wait("_pending_d").reshape(-1)

    def mdsi(self, ref, dist, planes, model=None, frame_bytes=None):
        """MDSI per frame for n frame pairs; returns [n] structured array (MDSI_DTYPE)."""
        self.mdsi_submit(ref, dist, planes, model, frame_bytes)
        return self.mdsi_wait()

    # ---- dE_ITP ------------------------------------------------------------------
    @staticmethod
    def itp_model(planes):
        """the colour model a plane list implies: ITP_BGR for three planes whose pixel step is 3 samples (packed bgr24 and its
        16-bit kin), ITP_YUV2020 otherwise"""
        bps = 2 if planes_depth(planes) > 8 else 1
        return N.ITP_BGR if len(planes) == 3 and all(int(p[4]) == 3 * bps for p in planes) else N.ITP_YUV2020

    @staticmethod
    def itp_transfer(transfer):
        """"pq" | "hlg" (or N.ITP_PQ | N.ITP_HLG) -> the transfer's number; anything else is a ValueError"""
        if isinstance(transfer, str) and transfer in N.ITP_TRANSFERS:
            return N.ITP_TRANSFERS[transfer]
        if isinstance(transfer, int) and not isinstance(transfer, bool) and transfer in N.ITP_TRANSFERS.values():
            return transfer
        raise ValueError("transfer must be 'pq' or 'hlg'")

    def itp_submit(self, ref, dist, planes, model=None, transfer="pq", full_range=False, frame_bytes=None):
        """dE_ITP (ITU-R BT.2124) for n frame pairs (vqa_itp_submit): the arrays / DeviceFrames and plane tuples of ciede_submit,
        exactly THREE planes taken together per pixel - Y, Cb, Cr (BT.2020 non-constant luminance; Cb and Cr of the luma's size or
        its ceil-half in either direction) or B, G, R; luma at least 16 x 16.  model: N.ITP_YUV2020 | N.ITP_BGR | None
        (itp_model(planes)).  transfer: "pq" | "hlg" (BT.2100; HLG on a 1000 cd/m2 display).  full_range: False (limited, the
        default) | True; it has no effect on B, G, R.  A batch of its own, like ciede_submit."""
        if model is None:
            model = self.itp_model(planes)
        transfer = self.itp_transfer(transfer)
        if not isinstance(full_range, (bool, np.bool_)):
            raise ValueError("full_range must be True or False")
        *args, keep = self._pair_args(ref, dist, planes, frame_bytes)
        st = self.lib.vqa_itp_submit(self.ctx, *args, plane_descs(planes), len(planes), int(model), transfer, int(full_range))
        N.check(st, "vqa_itp_submit", self.ctx)
        self._pending_i = (args[3], 1, keep)

    def itp_wait(self):
        """-> [n] records (ITP_DTYPE), one per frame: the two integer words sum_q and max_q (2^-20 units), de_sum, de_mean (the
        mean dE_ITP over the luma grid; exactly 0 for identical frames) and de_max (the largest dE_ITP of a pixel)."""
        return self._batch_wait("_pending_i").reshape(-1)

    def itp(self, ref, dist, planes, model=None, transfer="pq", full_range=False, frame_bytes=None):
        """dE_ITP per frame for n frame pairs; returns [n] structured array (ITP_DTYPE)."""
        self.itp_submit(ref, dist, planes, model, transfer, full_range, frame_bytes)
        return self.itp_wait()

    # ---- PU21-PSNR / PU21-SSIM ------------------------------------------------------
    def pu21_submit(self, ref, dist, planes, model=None, transfer="pq", full_range=False, frame_bytes=None):
        """PU21-PSNR and PU21-SSIM for n frame pairs (vqa_pu21_submit): the arrays / DeviceFrames, plane tuples, colour models,
        transfers and ranges of itp_submit, exactly THREE planes taken together per pixel; luma at least 16 x 16.  model:
        N.ITP_YUV2020 | N.ITP_BGR | None (itp_model(planes)).  transfer: "pq" | "hlg".  full_range: False (limited, the default) |
        True; it has no effect on B, G, R.  A batch of its own, like itp_submit."""
        if model is None:
            model = self.itp_model(planes)
        transfer = self.itp_transfer(transfer)
        if not isinstance(full_range, (bool, np.bool_)):
            raise ValueError("full_range must be True or False")
        *args, keep = self._pair_args(ref, dist, planes, frame_bytes)
        st = self.lib.vqa_pu21_submit(self.ctx, *args, plane_descs(planes), len(planes), int(model), transfer, int(full_range))
        N.check(st, "vqa_pu21_submit", self.ctx)
        self._pending_u = (args[3], 1, keep)
        self._pu21_shape = (args[3], 2, int(planes[0][1]), int(planes[0][0]))

    def pu21_wait(self):
        """-> [n] records (PU21_DTYPE), one per frame: the five integer words (sse_y_lo, sse_y_hi, sse_rgb_lo, sse_rgb_hi,
        ssim_q), windows, mse_y, mse_rgb, pu_psnr, pu_psnr_rgb (inf for identical frames) and pu_ssim (exactly 1 for them)."""
        return self._batch_wait("_pending_u").reshape(-1)

    def pu21_maps(self):
        """LAB LIBRARY ONLY: the two q_Y maps of the last PU21 batch, after its wait -> [n, 2, h, w] uint32 (ref, dist)"""
        fn = getattr(self.lib, "vqa_pu21_lab_read_maps", None)
        if fn is None or fn.argtypes is None:
            raise RuntimeError("the PU21 maps can be read back from the lab library only")
        out = np.empty(self._pu21_shape, np.uint32)
        N.check(fn(self.ctx, out.ctypes.data_as(C.POINTER(C.c_uint32)), out.size), "vqa_pu21_lab_read_maps", self.ctx)
        return out

    def pu21(self, ref, dist, planes, model=None, transfer="pq", full_range=False, frame_bytes=None, maps=False):
        """PU21-PSNR and PU21-SSIM per frame for n frame pairs; returns [n] structured array (PU21_DTYPE); on the lab library
        maps=True returns (records, q_Y [n, 2, h, w] uint32)."""
        self.pu21_submit(ref, dist, planes, model, transfer, full_range, frame_bytes)
        rec = self.pu21_wait()
        return (rec, self.pu21_maps()) if maps else rec

    # ---- FSIM / FSIMc ------------------------------------------------------------
    def fsim_submit(self, ref, dist, planes, model=None, frame_bytes=None):
        """FSIM and FSIMc for n frame pairs (vqa_fsim_submit): the arrays / DeviceFrames, plane tuples and colour models of
        mdsi_submit - THREE planes of one depth taken together per pixel, or ONE plane Y; plane 0 at least 16 x 16 and the
        downsampled grid at most 1024 either way.  model: N.FSIM_YUV709 | N.FSIM_BGR | N.FSIM_GRAY | None (mdsi_model(planes):
        the enums agree).  A batch of its own, like mdsi_submit."""
        if model is None:
            model = self.mdsi_model(planes)
        *args, keep = self._pair_args(ref, dist, planes, frame_bytes)
        st = self.lib.vqa_fsim_submit(self.ctx, *args, plane_descs(planes), len(planes), int(model))
        N.check(st, "vqa_fsim_submit", self.ctx)
        self._pending_f = (args[3], 1, keep)
        f = mdsi_factor(int(planes[0][1]), int(planes[0][0]))
        self._fsim_shape = (args[3], 2, -(-int(planes[0][1]) // f), -(-int(planes[0][0]) // f))

    def fsim_wait(self):
        """-> [n] records (FSIM_DTYPE), one per frame: the three integer words (sum_pc, sum_sim, sum_simc), count, factor,
        flags (bit 0: no phase congruency anywhere), fsim and fsimc (both exactly 1 for identical frames)."""
        return self._batch_wait("_pending_f").reshape(-1)

    def fsim_maps(self):
        """LAB LIBRARY ONLY: the two p maps of the last FSIM batch, after its wait -> [n, 2, hd, wd] uint32 (ref, dist)"""
        fn = getattr(self.lib, "vqa_fsim_lab_read_maps", None)
        if fn is None or fn.argtypes is None:
            raise RuntimeError("the FSIM maps can be read back from the lab library only")
        out = np.empty(self._fsim_shape, np.uint32)
        N.check(fn(self.ctx, out.ctypes.data_as(C.POINTER(C.c_uint32)), out.size), "vqa_fsim_lab_read_maps", self.ctx)
        return out

    def fsim(self, ref, dist, planes, model=None, frame_bytes=None, maps=False):
        """FSIM and FSIMc per frame for n frame pairs; returns [n] structured array (FSIM_DTYPE); on the lab library maps=True
        returns (records, p [n, 2, hd, wd] uint32)."""
        self.fsim_submit(ref, dist, planes, model, frame_bytes)
        rec = self.fsim_wait()
        return (rec, self.fsim_maps()) if maps else rec

    # ---- signal statistics --------------------------------------------------------
    @staticmethod
    def _sigstats_level(name, value):
        """a level of sigstats_submit -> the C argument: None is the default (negative), else an integer 0 .. 65535"""
        if value is None:
            return -1
        if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not 0 <= int(value) <= N.SIGSTATS_MAX_LEVEL:
            raise ValueError("%s must be None or an integer from 0 to %d" % (name, N.SIGSTATS_MAX_LEVEL))
        return int(value)

    def sigstats_submit(self, frames, planes, prev0=None, black_level=None, crop_level=None, frame_bytes=None):
        """Signal statistics for n frames of ONE stream (vqa_sigstats_submit): per plane the exact histogram's count, sum, sum of
        squares, min, max, the 10 % / 50 % / 90 % order statistics, the level counts, the bit masks, the dark-border box, and sad /
        changed of frame i against frame i - 1, frame 0 against prev0 (None: it has no predecessor and both are 0).  The
        arguments of siti_submit; every plane at least 16 x 16, packed bgr24 included.  black_level, crop_level: None (32 and 24
        on the 8-bit scale) or an integer 0 .. 65535 in sample units.  A batch of its own, like siti_submit."""
        levels = self._sigstats_level("black_level", black_level), self._sigstats_level("crop_level", crop_level)
        self._batch_submit("_pending_z", self._ref_args(frames, planes, prev0, frame_bytes), planes, *levels)
        self._sigstats_sides = [(int(p[1]), int(p[0])) for p in planes]   # (h, w) of the pending batch

    def sigstats_wait(self, profiles=False):
        """-> [n, n_planes] records (SIGSTATS_DTYPE).  profiles=True: -> (records, sums) with the profiles behind them, sums = one
        dict(rows as uint64 [n, h], cols as uint64 [n, w]) per plane: the row and column sums the box was read off."""
        n, npl, _keep = self._pending_z
        rec = np.zeros(n * npl, dtype=SIGSTATS_DTYPE)
        words = np.zeros((n, sum(h + w for h, w in self._sigstats_sides)), np.uint64) if profiles else None
        st = self.lib.vqa_sigstats_wait(self.ctx, rec.ctypes.data_as(C.POINTER(N.VqaSigstatsMetrics)), n * npl,
                                        1 if profiles else 0, words.ctypes.data_as(C.POINTER(C.c_uint64)) if profiles else None,
                                        words.size if profiles else 0)
        self._pending_z = None
        N.check(st, "vqa_sigstats_wait", self.ctx)
        rec = rec.reshape(n, npl)
        if not profiles:
            return rec
        sums, at = [], 0
        for h, w in self._sigstats_sides:
            sums.append(dict(rows=np.ascontiguousarray(words[:, at:at + h]), cols=np.ascontiguousarray(words[:, at + h:at + h + w])))
            at += h + w
        return rec, sums

    def sigstats(self, frames, planes, prev0=None, black_level=None, crop_level=None, profiles=False, frame_bytes=None):
        """Signal statistics per plane for n frames; returns [n, n_planes] structured array (SIGSTATS_DTYPE), with profiles=True
        also the row and column sums (sigstats_wait)."""
        self.sigstats_submit(frames, planes, prev0, black_level, crop_level, frame_bytes)
        return self.sigstats_wait(profiles)

    # ---- the resampler ---------------------------------------------------------------
    def scale_submit(self, frames, planes, out_planes, filter="bicubic", out=None, frame_bytes=None, out_frame_bytes=None):
        """Resample n frames of ONE stream from `planes` to `out_planes` on the device (vqa_scale_submit): Pillow's
        Image.resize arithmetic, plane i into plane i, filter "bilinear" | "bicubic" | "lanczos".  frames: an array /
        DeviceFrames as cambi_submit takes them (a sample type that does not match the depth is a ValueError, never a cast).
        out: a caller's DeviceFrames to write (its frame stride holds unless out_frame_bytes is given), or None: a new
        DeviceBuffer of n * out_frame_bytes (default: the span of out_planes).  -> the DeviceFrames of the scaled stream, which
        every submit of THIS engine accepts with out_planes at once: the stream orders it behind the resampler, no scale_wait
        is needed in between.  A batch of its own, like cambi_submit."""
        fid = scale_filter(filter)
        check_scale_planes(planes, out_planes)
        fp, kind, n, fs, keep = self._one_stream_args(frames, planes, frame_bytes)
        out, ofs = self._out_frames(n, out_planes, out, out_frame_bytes)
        st = self.lib.vqa_scale_submit(self.ctx, fp, kind, n, fs, plane_descs(planes), out.ptr, ofs, plane_descs(out_planes),
                                       len(planes), fid)
        N.check(st, "vqa_scale_submit", self.ctx)
        self._pending_k = (n, (keep, out))
        return out

    def scale_wait(self):
        """Wait for the pending scale batch: the scaled frames are complete (another engine, or a copy to the host, may read
        them)."""
        st = self.lib.vqa_scale_wait(self.ctx)
        self._pending_k = None
        N.check(st, "vqa_scale_wait", self.ctx)

    def scale(self, frames, planes, out_planes, filter="bicubic", out=None, frame_bytes=None, out_frame_bytes=None):
        """scale_submit and scale_wait -> the DeviceFrames of the scaled stream."""
        res = self.scale_submit(frames, planes, out_planes, filter, out, frame_bytes, out_frame_bytes)
        self.scale_wait()
        return res

    def _out_frames(self, n, out_planes, out, out_frame_bytes):
        """the destination of a scale, conform, convert or weave submit -> (DeviceFrames of n frames, its frame stride in
        bytes): a fresh allocation for out None, else the caller's DeviceFrames, checked against out_planes and cut to n frames"""
        itemsize = 2 if planes_depth(out_planes) > 8 else 1
        span = planes_span(out_planes)
        if out is None:
            ofs = int(out_frame_bytes) if out_frame_bytes else span
            if ofs < span:
                raise ValueError("out_frame_bytes (%d) is smaller than a frame of out_planes (%d)" % (ofs, span))
            buf = DeviceBuffer(self, n * ofs)
            out = DeviceFrames(buf.ptr, n, 1, ofs // itemsize, frame_stride=ofs, owner=buf, channels=1, itemsize=itemsize)
        else:
            if not isinstance(out, DeviceFrames):
                raise TypeError("out must be DeviceFrames (device memory)")
            if out.itemsize != itemsize:
                raise ValueError("%d-bit planes need an out of %s samples (got DeviceFrames of itemsize %d)"
                                 % (planes_depth(out_planes), "uint16" if itemsize == 2 else "uint8", out.itemsize))
            if out.n < n:
                raise ValueError("out holds %d frames, the batch has %d" % (out.n, n))
            ofs = int(out_frame_bytes) if out_frame_bytes else out.frame_stride
            if ofs < span:
                raise ValueError("a frame of out (%d bytes) is smaller than a frame of out_planes (%d)" % (ofs, span))
            if out.n != n or ofs != out.frame_stride:
                out = DeviceFrames(out.ptr, n, out.h, out.w, ofs, out.row_stride, owner=out, channels=out.channels,
                                   itemsize=itemsize)
        return out, ofs

    # ---- conform: the found registration, applied -------------------------------------------
    def conform_submit(self, frames, planes, out_planes, origin=None, index=None, lut=None, matrix=None, out=None,
                       frame_bytes=None, out_frame_bytes=None):
        """A registered copy of n_in frames of ONE stream on the device (vqa_conform_submit): out[j][p][y][x] is a function of
        in[index[j]][p][y0_p + y][x0_p + x].  frames: an array / DeviceFrames as scale_submit takes them (a sample type that
        does not match the depth is a ValueError, never a cast).  out_planes: the windows' sizes, strides and pads.  origin:
        None or one (y0, x0) per plane.  index: None (identity) or the source frame of every output frame.  lut: None or
        [n_planes, 2^depth] of the sample type, applied first.  matrix: None or int64 [3, 4] in 2^-16 fixed point (three
        planes).  out / out_frame_bytes: as for scale_submit.  -> the DeviceFrames of the conformed stream, which every submit
        of THIS engine accepts with out_planes at once; conform_wait is needed only before another engine or the host reads
        them.  A batch of its own, like scale_submit."""
        args = check_conform_args(planes, out_planes, origin, index, lut, matrix)
        origin_a, index_a, lut_a, matrix_a = args
        fp, kind, n_in, fs, keep = self._one_stream_args(frames, planes, frame_bytes)
        if index_a is not None and index_a.size and (int(index_a.min()) < 0 or int(index_a.max()) >= n_in):
            raise ValueError("index must name source frames 0 .. %d" % (n_in - 1))
        n = n_in if index_a is None else int(index_a.size)
        if not 1 <= n <= N.CONFORM_MAX_OUT:
            raise ValueError("a conform submit writes 1 .. %d frames (got %d)" % (N.CONFORM_MAX_OUT, n))
        out, ofs = self._out_frames(n, out_planes, out, out_frame_bytes)
        i32, i64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        st = self.lib.vqa_conform_submit(
            self.ctx, fp, kind, n_in, fs, plane_descs(planes), out.ptr, ofs, plane_descs(out_planes), len(planes),
            origin_a.ctypes.data_as(i32) if origin_a is not None else None,
            index_a.ctypes.data_as(i32) if index_a is not None else None, n,
            lut_a.ctypes.data if lut_a is not None else None,
            matrix_a.ctypes.data_as(i64) if matrix_a is not None else None)
        N.check(st, "vqa_conform_submit", self.ctx)
        self._pending_cm = (n, (keep, out))
        return out

    def conform_wait(self):
        """Wait for the pending conform batch: the conformed frames are complete (another engine, or a copy to the host, may
        read them)."""
        st = self.lib.vqa_conform_wait(self.ctx)
        self._pending_cm = None
        N.check(st, "vqa_conform_wait", self.ctx)

    def conform(self, frames, planes, out_planes, origin=None, index=None, lut=None, matrix=None, out=None, frame_bytes=None,
                out_frame_bytes=None):
        """conform_submit and conform_wait -> the DeviceFrames of the conformed stream."""
        res = self.conform_submit(frames, planes, out_planes, origin, index, lut, matrix, out, frame_bytes, out_frame_bytes)
        self.conform_wait()
        return res

    # ---- convert: another sample depth and / or chroma layout ----------------------------------
    def convert_submit(self, frames, planes, out_planes, chroma="linear", siting="center", range="limited", out=None,
                       frame_bytes=None, out_frame_bytes=None):
        """n frames of ONE stream written at another sample depth and / or chroma layout on the device (vqa_convert_submit):
        plane i of `planes` into plane i of `out_planes`, per axis the same size, twice or half of it (include/vqa.h), integer
        arithmetic with one rounding.  chroma "box" | "linear", siting "center" | "left" (the horizontal axis of "linear"),
        range "limited" | "full".  frames: an array / DeviceFrames as scale_submit takes them (a sample type that does not
        match the depth of `planes` is a ValueError, never a cast).  out / out_frame_bytes: as for scale_submit, at the sample
        type of out_planes.  -> the DeviceFrames of the converted stream, which every submit of THIS engine accepts with
        out_planes at once; convert_wait is needed only before another engine or the host reads them.  A batch of its own,
        like conform_submit."""
        ids = convert_options(chroma, siting, range)
        check_convert_planes(planes, out_planes)
        fp, kind, n, fs, keep = self._one_stream_args(frames, planes, frame_bytes)
        if not 1 <= n <= N.CONVERT_MAX_FRAMES:
            raise ValueError("a convert submit takes 1 .. %d frames (got %d)" % (N.CONVERT_MAX_FRAMES, n))
        out, ofs = self._out_frames(n, out_planes, out, out_frame_bytes)
        st = self.lib.vqa_convert_submit(self.ctx, fp, kind, n, fs, plane_descs(planes), out.ptr, ofs, plane_descs(out_planes),
                                         len(planes), *ids)
        N.check(st, "vqa_convert_submit", self.ctx)
        self._pending_cv = (n, (keep, out))
        return out

    def convert_wait(self):
        """Wait for the pending convert batch: the converted frames are complete (another engine, or a copy to the host, may
        read them)."""
        st = self.lib.vqa_convert_wait(self.ctx)
        self._pending_cv = None
        N.check(st, "vqa_convert_wait", self.ctx)

    def convert(self, frames, planes, out_planes, chroma="linear", siting="center", range="limited", out=None, frame_bytes=None,
                out_frame_bytes=None):
        """convert_submit and convert_wait -> the DeviceFrames of the converted stream."""
        res = self.convert_submit(frames, planes, out_planes, chroma, siting, range, out, frame_bytes, out_frame_bytes)
        self.convert_wait()
        return res

    # ---- fields: interlace and pulldown statistics; weave: frames out of fields -----------------
    def fields_submit(self, frames, planes, prev0=None, plane=0, frame_bytes=None):
        """The field statistics of planes[plane] of n frames of ONE stream (vqa_fields_submit): comb, fwd, bwd, sad and changed
        per row parity, frame i against frame i - 1 and frame 0 against prev0 (None: it has no predecessor, its pair words are 0
        and has_prev is 0).  frames / prev0: as motion_submit takes them (a sample type that does not match the depth is a
        ValueError, never a cast), roi and strided views included.  The plane is at least 16 x 16: a ValueError before anything
        is uploaded.  A batch of its own, like signature_submit."""
        one = [planes[plane]]
        w, h = int(one[0][0]), int(one[0][1])
        if w < N.FIELDS_MIN_DIM or h < N.FIELDS_MIN_DIM:
            raise ValueError("fields needs a plane of at least %d x %d (got %dx%d)" % (N.FIELDS_MIN_DIM, N.FIELDS_MIN_DIM, w, h))
        fp, pp, kind, n, fs, keep = self._ref_args(frames, one, prev0, frame_bytes)
        if not 1 <= n <= N.FIELDS_MAX_FRAMES:
            raise ValueError("a fields submit takes 1 .. %d frames (got %d)" % (N.FIELDS_MAX_FRAMES, n))
        st = self.lib.vqa_fields_submit(self.ctx, fp, pp, kind, n, fs, plane_descs(one))
        N.check(st, "vqa_fields_submit", self.ctx)
        self._pending_fd = (n, keep)

    def fields_wait(self):
        """-> [n] records (N.FIELDS_DTYPE): exact integers; fields.analyse reads the field order and the cadence off them."""
        n, _keep = getattr(self, "_pending_fd", None) or (1, None)   # (nothing pending: the library says so)
        out = np.zeros(n, dtype=N.FIELDS_DTYPE)
        st = self.lib.vqa_fields_wait(self.ctx, out.ctypes.data_as(C.POINTER(N.VqaFieldsMetrics)), n)
        self._pending_fd = None
        N.check(st, "vqa_fields_wait", self.ctx)
        return out

    def fields(self, frames, planes, prev0=None, plane=0, frame_bytes=None):
        """fields_submit and fields_wait -> [n] records (N.FIELDS_DTYPE)"""
        self.fields_submit(frames, planes, prev0, plane, frame_bytes)
        return self.fields_wait()

    def weave_submit(self, frames, planes, top_index, bottom_index, out=None, frame_bytes=None, out_frame_bytes=None):
        """Frames out of the fields of other frames on the device (vqa_weave_submit): the even rows of every plane of output
        frame j come from source frame top_index[j], the odd rows from source frame bottom_index[j].  frames: an array /
        DeviceFrames as conform_submit takes them; `planes` describes both sides.  The indices name source frames 0 .. n - 1 and
        are equally long: a ValueError otherwise.  out / out_frame_bytes: as for conform_submit.  -> the DeviceFrames of the
        woven stream, which every submit of THIS engine accepts with `planes` at once; weave_wait is needed only before another
        engine or the host reads them.  A batch of its own, like conform_submit."""
        if not 1 <= len(planes) <= 4:
            raise ValueError("weave needs one to four planes (got %d)" % len(planes))
        for i, q in enumerate(planes):
            w, h, least = int(q[0]), int(q[1]), N.WEAVE_MIN_DIM if i == 0 else N.WEAVE_MIN_DIM // 2
            if w < least or h < least:
                raise ValueError("weave needs planes of at least %d x %d (plane %d: %dx%d)" % (least, least, i, w, h))
        top, bot = (np.ascontiguousarray(a, dtype=np.int32).reshape(-1) for a in (top_index, bottom_index))
        if top.size != bot.size or not 1 <= top.size <= N.WEAVE_MAX_OUT:
            raise ValueError("top_index and bottom_index must be equally long, 1 .. %d entries (got %d and %d)"
                             % (N.WEAVE_MAX_OUT, top.size, bot.size))
        fp, kind, n_in, fs, keep = self._one_stream_args(frames, planes, frame_bytes)
        if min(int(top.min()), int(bot.min())) < 0 or max(int(top.max()), int(bot.max())) >= n_in:
            raise ValueError("top_index and bottom_index must name source frames 0 .. %d" % (n_in - 1))
        n = int(top.size)
        out, ofs = self._out_frames(n, planes, out, out_frame_bytes)
        i32 = C.POINTER(C.c_int32)
        st = self.lib.vqa_weave_submit(self.ctx, fp, kind, n_in, fs, plane_descs(planes), out.ptr, ofs, plane_descs(planes),
                                       len(planes), top.ctypes.data_as(i32), bot.ctypes.data_as(i32), n)
        N.check(st, "vqa_weave_submit", self.ctx)
        self._pending_wv = (n, (keep, out))
        return out

    def weave_wait(self):
        """Wait for the pending weave batch: the woven frames are complete (another engine, or a copy to the host, may read
        them)."""
        st = self.lib.vqa_weave_wait(self.ctx)
        self._pending_wv = None
        N.check(st, "vqa_weave_wait", self.ctx)

    def weave(self, frames, planes, top_index, bottom_index, out=None, frame_bytes=None, out_frame_bytes=None):
        """weave_submit and weave_wait -> the DeviceFrames of the woven stream."""
        res = self.weave_submit(frames, planes, top_index, bottom_index, out, frame_bytes, out_frame_bytes)
        self.weave_wait()
        return res

    # ---- temporal alignment ------------------------------------------------------------
    def align_submit(self, ref, dist, planes, radius=8, offset=0, plane=0, frame_bytes=None, dist_frame_bytes=None):
        """The squared error of planes[plane] between distorted frame j and reference frame j + offset + k, k = -radius ..
        radius (vqa_align_submit).  ref, dist: uint8 / uint16 arrays (the first axis is the frame; the other type than the
        planes' depth says is a ValueError, not a cast) or DeviceFrames, roi and strided views included - the two streams may
        hold different numbers of frames.  frame_bytes: the frame stride of host arrays (dist_frame_bytes: the distorted
        stream's, where it differs).  planes[plane] is what is measured, at least 1 x 1.  A batch of its own, like gmsd_submit."""
        one = [planes[plane]]
        dev = isinstance(ref, DeviceFrames)
        if dev and not isinstance(dist, DeviceFrames):
            raise TypeError("ref and dist must both be DeviceFrames or both be arrays")
        rp, ref = self._stream_arg(ref, one, dev)
        dp, dist = self._stream_arg(dist, one, dev)
        if dev:
            n_ref, n_dist, rfs, dfs, kind = ref.n, dist.n, ref.frame_stride, dist.frame_stride, N.VQA_MEM_DEVICE
        else:
            n_ref, n_dist, kind = ref.shape[0], dist.shape[0], N.VQA_MEM_HOST
            if not n_ref or not n_dist:
                raise ValueError("ref and dist must hold at least one frame each")
            rfs = int(frame_bytes) if frame_bytes else ref.nbytes // n_ref
            dfs = int(dist_frame_bytes) if dist_frame_bytes else (int(frame_bytes) if frame_bytes else dist.nbytes // n_dist)
        st = self.lib.vqa_align_submit(self.ctx, rp, n_ref, dp, n_dist, kind, rfs, dfs, plane_descs(one), int(offset), int(radius))
        N.check(st, "vqa_align_submit", self.ctx)
        self._pending_l = (n_dist, 2 * int(radius) + 1, (ref, dist))

    def align_wait(self):
        """-> uint64 [n_dist, 2 radius + 1]: column c is k = c - radius; N.ALIGN_NONE where the reference frame does not exist."""
        n, band, _keep = getattr(self, "_pending_l", None) or (1, 1, None)   # (nothing pending: the library says so)
        out = np.zeros((n, band), np.uint64)
        st = self.lib.vqa_align_wait(self.ctx, out.ctypes.data_as(C.POINTER(C.c_uint64)), out.size)
        self._pending_l = None
        N.check(st, "vqa_align_wait", self.ctx)
        return out

    def align(self, ref, dist, planes, radius=8, offset=0, plane=0, frame_bytes=None, dist_frame_bytes=None):
        """align_submit and align_wait -> uint64 [n_dist, 2 radius + 1]; align.analyse reads offset, drops and repeats off it."""
        self.align_submit(ref, dist, planes, radius, offset, plane, frame_bytes, dist_frame_bytes)
        return self.align_wait()

    # ---- spatial registration ----------------------------------------------------------
    def shift_submit(self, ref, dist, planes, radius=4, margin=None, plane=0, frame_bytes=None, dist_frame_bytes=None):
        """The squared error of planes[plane] between distorted frame j and reference frame j read at every shift (dy, dx),
        dy, dx = -radius .. radius, over the core that lies `margin` (default: radius) samples inside the plane
        (vqa_shift_submit).  ref, dist: uint8 / uint16 arrays of as many frames (the first axis is the frame; the other type
        than the planes' depth says is a ValueError, not a cast) or DeviceFrames, roi and strided views included.
        frame_bytes: the frame stride of host arrays (dist_frame_bytes: the distorted stream's, where it differs).  A batch
        of its own, like align_submit."""
        one = [planes[plane]]
        dev = isinstance(ref, DeviceFrames)
        if dev and not isinstance(dist, DeviceFrames):
            raise TypeError("ref and dist must both be DeviceFrames or both be arrays")
        rp, ref = self._stream_arg(ref, one, dev)
        dp, dist = self._stream_arg(dist, one, dev)
        if dev:
            n, n_dist, rfs, dfs, kind = ref.n, dist.n, ref.frame_stride, dist.frame_stride, N.VQA_MEM_DEVICE
        else:
            n, n_dist, kind = ref.shape[0], dist.shape[0], N.VQA_MEM_HOST
            if not n:
                raise ValueError("ref and dist must hold at least one frame each")
            rfs = int(frame_bytes) if frame_bytes else ref.nbytes // n
            dfs = int(dist_frame_bytes) if dist_frame_bytes else (int(frame_bytes) if frame_bytes else dist.nbytes // max(n_dist, 1))
        if n != n_dist:
            raise ValueError("ref and dist must hold the same number of frames")
        radius = int(radius)
        margin = radius if margin is None else int(margin)
        st = self.lib.vqa_shift_submit(self.ctx, rp, dp, n, kind, rfs, dfs, plane_descs(one), radius, margin)
        N.check(st, "vqa_shift_submit", self.ctx)
        self._pending_j = (n, 2 * radius + 1, (ref, dist))

    def shift_wait(self):
        """-> uint64 [n, 2 radius + 1, 2 radius + 1]: entry [j][a][b] is the shift (dy, dx) = (a - radius, b - radius)."""
        n, side, _keep = getattr(self, "_pending_j", None) or (1, 1, None)   # (nothing pending: the library says so)
        out = np.zeros((n, side, side), np.uint64)
        st = self.lib.vqa_shift_wait(self.ctx, out.ctypes.data_as(C.POINTER(C.c_uint64)), out.size)
        self._pending_j = None
        N.check(st, "vqa_shift_wait", self.ctx)
        return out

    def shift(self, ref, dist, planes, radius=4, margin=None, plane=0, frame_bytes=None, dist_frame_bytes=None):
        """shift_submit and shift_wait -> uint64 [n, 2 radius + 1, 2 radius + 1]; shift.analyse reads the shift and its cost off it."""
        self.shift_submit(ref, dist, planes, radius, margin, plane, frame_bytes, dist_frame_bytes)
        return self.shift_wait()

    # ---- HDR light levels and gamut QC ---------------------------------------------------
    light_table = staticmethod(light_table)
    light_gamut = staticmethod(light_gamut)

    def light_submit(self, frames, planes, model=None, transfer="pq", full_range=False, table=None, histogram=False,
                     frame_bytes=None):
        """MaxCLL / MaxFALL's per-frame words, light statistics and gamut counts for n frames of ONE stream (vqa_light_submit): an
        array / DeviceFrames and the plane tuples of itp_submit, exactly THREE planes taken together per pixel - Y, Cb, Cr (BT.2020
        non-constant luminance) or B, G, R; luma at least 16 x 16.  model: N.ITP_YUV2020 | N.ITP_BGR | None (itp_model(planes)).
        table: uint64 [65536], the display light of a 16-bit code in 2^-20 cd/m2, non-decreasing and below 2^34; None:
        light_table(transfer) ("pq" only).  full_range: False (limited, the default) | True; no effect on B, G, R.
        histogram: keep the [n, 4096] histograms for light_wait.  A batch of its own, like itp_submit."""
        if model is None:
            model = self.itp_model(planes)
        if not isinstance(full_range, (bool, np.bool_)):
            raise ValueError("full_range must be True or False")
        if table is None:
            table = light_table(transfer)
        table = check_light_table(table)
        fp, kind, n, fs, keep = self._one_stream_args(frames, planes, frame_bytes)
        st = self.lib.vqa_light_submit(self.ctx, fp, kind, n, fs, plane_descs(planes), len(planes), int(model), int(full_range),
                                       table.ctypes.data_as(C.POINTER(C.c_uint64)), 1 if histogram else 0)
        N.check(st, "vqa_light_submit", self.ctx)
        self._pending_o = (n, bool(histogram), keep)

    def light_wait(self):
        """-> [n] records (LIGHT_DTYPE), one per frame; after a submit with histogram=True: (records, uint32 [n, 4096])."""
        n, want, _keep = getattr(self, "_pending_o", None) or (1, False, None)   # (nothing pending: the library says so)
        rec = np.zeros(n, dtype=LIGHT_DTYPE)
        hist = np.zeros((n, N.LIGHT_BINS), np.uint32) if want else None
        st = self.lib.vqa_light_wait(self.ctx, rec.ctypes.data_as(C.POINTER(N.VqaLightMetrics)), n,
                                     hist.ctypes.data_as(C.POINTER(C.c_uint32)) if want else None)
        self._pending_o = None
        N.check(st, "vqa_light_wait", self.ctx)
        return (rec, hist) if want else rec

    def light(self, frames, planes, model=None, transfer="pq", full_range=False, table=None, histogram=False, frame_bytes=None):
        """light_submit and light_wait -> [n] records (LIGHT_DTYPE), with histogram=True also the histograms;
        light.summarise reads MaxCLL, MaxFALL and the shares off the records."""
        self.light_submit(frames, planes, model, transfer, full_range, table, histogram, frame_bytes)
        return self.light_wait()

    # ---- colour registration ------------------------------------------------------------
    def colorfit_submit(self, ref, dist, planes, tables=False, frame_bytes=None):
        """The joint integer moments of the planes of n frame pairs and, with tables=True, ONE set of per-code transfer tables
        for the whole submit (vqa_colorfit_submit): the arrays / DeviceFrames and plane tuples of ciede_submit, ONE or THREE
        planes taken together on the luma grid, chroma replicated; luma at least 16 x 16; at most N.COLORFIT_MAX_FRAMES frames,
        and with tables n h w <= 2^31.  A batch of its own, like ciede_submit."""
        *args, keep = self._pair_args(ref, dist, planes, frame_bytes)
        st = self.lib.vqa_colorfit_submit(self.ctx, *args, plane_descs(planes), len(planes), 1 if tables else 0)
        N.check(st, "vqa_colorfit_submit", self.ctx)
        words = len(planes) * colorfit_bins(planes_depth(planes)) * 3 if tables else 0
        self._pending_cf = (args[3], len(planes), words, keep)

    def colorfit_wait(self):
        """-> ([n] records (COLORFIT_DTYPE), uint64 [n_planes, bins, 3] tables (count, sum_d, sum_dd) or None)."""
        n, npl, words, _keep = getattr(self, "_pending_cf", None) or (1, 1, 0, None)   # (nothing pending: the library says so)
        rec = np.zeros(n, dtype=COLORFIT_DTYPE)
        tab = np.zeros(words, np.uint64) if words else None
        st = self.lib.vqa_colorfit_wait(self.ctx, rec.ctypes.data_as(C.POINTER(N.VqaColorfitMetrics)), n,
                                        tab.ctypes.data_as(C.POINTER(C.c_uint64)) if words else None, words)
        self._pending_cf = None
        N.check(st, "vqa_colorfit_wait", self.ctx)
        return rec, (tab.reshape(npl, -1, 3) if words else None)

    def colorfit(self, ref, dist, planes, tables=False, frame_bytes=None):
        """colorfit_submit and colorfit_wait -> (records, tables or None); colorfit.analyse reads the fits off them."""
        self.colorfit_submit(ref, dist, planes, tables, frame_bytes)
        return self.colorfit_wait()

    # ---- clip-wide sync: frame signatures and their all-pairs distance ------------------
    def signature_submit(self, frames, planes, plane=0, frame_bytes=None):
        """The 256-byte signature of planes[plane] of n frames of ONE stream (vqa_sig_submit): the floor of the mean of each
        cell of a 16 x 16 grid, brought to 8 bits.  frames: a uint8 / uint16 array (the first axis is the frame; the other type
        than the planes' depth says is a ValueError, not a cast) or DeviceFrames, roi and strided views included.  The plane
        is at least 16 x 16; at most N.SIG_MAX_BATCH frames per submit.  A batch of its own, like cambi_submit."""
        one = [planes[plane]]
        fp, kind, n, fs, keep = self._one_stream_args(frames, one, frame_bytes)
        st = self.lib.vqa_sig_submit(self.ctx, fp, kind, n, fs, plane_descs(one))
        N.check(st, "vqa_sig_submit", self.ctx)
        self._pending_sg = (n, keep)

    def signature_wait(self):
        """-> uint8 [n, 256]: byte 16 a + b is cell (a, b)."""
        n, _keep = getattr(self, "_pending_sg", None) or (1, None)   # (nothing pending: the library says so)
        out = np.zeros((n, N.SIG_BYTES), np.uint8)
        st = self.lib.vqa_sig_wait(self.ctx, out.ctypes.data, n)
        self._pending_sg = None
        N.check(st, "vqa_sig_wait", self.ctx)
        return out

    def signature(self, frames, planes, plane=0, frame_bytes=None):
        """signature_submit and signature_wait -> uint8 [n, 256]"""
        self.signature_submit(frames, planes, plane, frame_bytes)
        return self.signature_wait()

    def sig_cross_submit(self, dist_sig, ref_sig):
        """Every distorted signature against every reference signature (vqa_sig_cross_submit): two uint8 [n, 256] host arrays
        of at most N.SIG_MAX_FRAMES rows each.  A batch of its own."""
        d, r = (np.ascontiguousarray(a) for a in (dist_sig, ref_sig))
        for a in (d, r):
            if a.dtype != np.uint8 or a.ndim != 2 or a.shape[1] != N.SIG_BYTES or not a.shape[0]:
                raise ValueError("signatures must be uint8 [n, %d] with n >= 1 (got %s %s)" % (N.SIG_BYTES, a.dtype, a.shape))
        st = self.lib.vqa_sig_cross_submit(self.ctx, d.ctypes.data, d.shape[0], r.ctypes.data, r.shape[0])
        N.check(st, "vqa_sig_cross_submit", self.ctx)
        self._pending_sx = (d.shape[0], r.shape[0], (d, r))

    def sig_cross_wait(self):
        """-> (diag uint64 [n_dist + n_ref - 1], best uint64 [n_dist]): diag[k + n_dist - 1] is the sum of the squared
        distances of the pairs (j, j + k); best[j] is (the smallest distance << 32) | its smallest reference index."""
        nd, nr, _keep = getattr(self, "_pending_sx", None) or (1, 1, None)   # (nothing pending: the library says so)
        diag, best = np.zeros(nd + nr - 1, np.uint64), np.zeros(nd, np.uint64)
        st = self.lib.vqa_sig_cross_wait(self.ctx, diag.ctypes.data_as(C.POINTER(C.c_uint64)), diag.size,
                                         best.ctypes.data_as(C.POINTER(C.c_uint64)), best.size)
        self._pending_sx = None
        N.check(st, "vqa_sig_cross_wait", self.ctx)
        return diag, best

    def sig_cross(self, dist_sig, ref_sig):
        """sig_cross_submit and sig_cross_wait -> (diag, best); sync.analyse reads the offset and the re-pairing off them."""
        self.sig_cross_submit(dist_sig, ref_sig)
        return self.sig_cross_wait()

    def download(self, dev, dtype=None):
        """Copy DeviceFrames back -> a host array [n, frame_stride / itemsize] (uint8, or uint16 for itemsize 2)."""
        dt = np.dtype(dtype) if dtype is not None else np.dtype(np.uint16 if dev.itemsize == 2 else np.uint8)
        out = np.empty((dev.n, dev.frame_stride // dt.itemsize), dt)
        if out.nbytes:
            # through page-locked memory, like every result the library copies back: the device never writes pageable pages
            pin = self.alloc_pinned(out.shape, dt)
            try:
                N.check(self.lib.vqa_copy_d2h(self.ctx, pin.ctypes.data, dev.ptr, out.nbytes), "vqa_copy_d2h", self.ctx)
                N.check(self.lib.vqa_sync(self.ctx), "vqa_sync", self.ctx)
                out[...] = pin
            finally:
                self.free_pinned(pin)
        return out

    # ---- per-kernel timing ---------------------------------------------------
    def profile(self, on=True):
        N.check(self.lib.vqa_profile_enable(self.ctx, 1 if on else 0), "vqa_profile_enable", self.ctx)

    def profile_read(self, reset=False):
        """-> {kernel name: (total_ms, launches)} for kernels launched since the last reset."""
        out = {}
        for k in N.K_IDS_EXTANT:
            ms, cnt = C.c_double(0), C.c_int64(0)
            N.check(self.lib.vqa_profile_read(self.ctx, k, C.byref(ms), C.byref(cnt), 1 if reset else 0),
                    "vqa_profile_read", self.ctx)
            if cnt.value:
                out[self.lib.vqa_kernel_name(k).decode()] = (ms.value, cnt.value)
        return out

    # ---- debug -------------------------------------------------------------
    def debug_plane(self, which, frame, h, w):
        out = np.empty((h, w), np.uint8)
        st = self.lib.vqa_debug_read_plane(self.ctx, which, frame, out.ctypes.data, h, w)
        N.check(st, "vqa_debug_read_plane", self.ctx)
        return out

    def debug_farneback_flow(self, pair, h, w):
        """The final flow field [h][w][2] (dx, dy) of pair `pair` of the last Farneback submit (its last chunk)."""
        out = np.empty((h, w, 2), np.float32)
        st = self.lib.vqa_debug_read_farneback(self.ctx, 0, pair, 0, out.ctypes.data, h, w)
        N.check(st, "vqa_debug_read_farneback", self.ctx)
        return out

    def debug_farneback_expansion(self, plane, level, lh, lw):
        """The polynomial expansion of gray plane `plane` (0 = prev0, q = frame q - 1) at pyramid level `level` of the last
        Farneback submit, as [lh][lw][5] like OpenCV keeps it (the device keeps, and the C call returns, five planes)."""
        out = np.empty((5, lh, lw), np.float32)
        st = self.lib.vqa_debug_read_farneback(self.ctx, 1, plane, level, out.ctypes.data, lh, lw)
        N.check(st, "vqa_debug_read_farneback", self.ctx)
        return np.ascontiguousarray(out.transpose(1, 2, 0))
