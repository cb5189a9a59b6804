"""ctypes binding of include/vqa.h (libvqa_hip.so).

There is NO fallback: if the HIP library is missing or no gfx950 device is
visible, importing the library or creating a context raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# VQA_LIB_PATH: load another build of the same ABI (the lab build csrc/lab/libvqa_hip_lab.so for A/B re-measurement and
# fault injection, or a probe build); default = the shipped in-tree library
LIB_PATH = os.environ.get("VQA_LIB_PATH") or os.path.join(_HERE, "csrc", "libvqa_hip.so")
LAB_LIB_PATH = os.path.join(_HERE, "csrc", "lab", "libvqa_hip_lab.so")

VQA_ABI_VERSION = 8
VQA_TABLE_CACHE_GEOMETRIES = 16

VQA_OK = 0
VQA_ERR_INVALID = -1
VQA_ERR_NO_DEVICE = -2
VQA_ERR_HIP = -3
VQA_ERR_OOM = -4
VQA_ERR_UNSUPPORTED = -5
VQA_ERR_STATE = -6
VQA_ERR_INCOMPLETE = -7

VQA_MEM_HOST = 0
VQA_MEM_DEVICE = 1

M_GRAY_HIST = 1 << 0
M_COLOR_HIST = 1 << 1
M_DCT = 1 << 2
M_TEMPORAL_DCT = 1 << 3
M_EDGE = 1 << 4
M_MOTION = 1 << 5
M_ORB = 1 << 6
M_ALL = 0x7F

# The kernel ids of include/vqa.h, each written once: (name, id, what vqa_kernel_name answers), ascending, a line per feature.
# csrc/vqa_capi.hip's KERNELS holds the same rows; a new kernel takes the next id after the last and adds its row to both.
K_TABLE = (
    ("K_GRAY_HIST", 0, "k_bgr2gray_hist"), ("K_RESIZE", 1, "k_resize_planes"), ("K_DCT8", 2, "k_dct8"), ("K_DCT_FULL", 3, "k_dct_full"),
    ("K_CANNY_NMS", 4, "k_canny_nms"), ("K_CANNY_HYST", 5, "k_canny_hyst"), ("K_SAD", 6, "k_block_sad"),
    ("K_SSIM_GAUSS", 7, "k_ssim_gauss"), ("K_SSIM_FFMPEG", 8, "k_ssim_ffmpeg"), ("K_ORB", 9, "k_orb64"),
    ("K_FARNEBACK", 10, "farneback(pyramid)"), ("K_MS_PYRAMID", 11, "k_ms_pyramid"),
    ("K_VIF", 12, "k_vif_stats"), ("K_VIF_DECIMATE", 13, "k_vif_decimate"),
    ("K_ADM", 16, "k_adm_scale"), ("K_ADM_REDUCE", 17, "k_adm_reduce"),
    ("K_MOTION", 19, "k_motion_sad"),
    ("K_SITI", 21, "k_siti"),
    ("K_PSNR_HVS", 23, "k_psnr_hvs"),
    ("K_CIEDE", 25, "k_ciede"),
    ("K_GMSD", 27, "k_gmsd"),
    ("K_CAMBI_MASK", 29, "k_cambi_mask"), ("K_CAMBI_DECIMATE", 30, "k_cambi_decimate"), ("K_CAMBI_CONTRAST", 31, "k_cambi_contrast"),
    ("K_CAMBI_TOPK", 32, "k_cambi_topk"),
    ("K_XPSNR_ACT", 34, "k_xpsnr_act"), ("K_XPSNR_SSE", 35, "k_xpsnr_sse"),
    ("K_HAARPSI", 37, "k_haarpsi"),
    ("K_VCA_BLOCKS", 39, "k_vca_blocks"), ("K_VCA_SUM", 40, "k_vca_sum"),
    ("K_ARTIFACTS", 42, "k_artifacts"),
    ("K_BRISQUE_HALF", 44, "k_brisque_half"), ("K_BRISQUE_MSCN", 45, "k_brisque_mscn"), ("K_BRISQUE_SEAM", 46, "k_brisque_seam"),
    ("K_MDSI_MAP", 48, "k_mdsi_map"), ("K_MDSI_DEV", 49, "k_mdsi_dev"),
    ("K_ITP", 51, "k_itp"),
    ("K_PU21_ENCODE", 53, "k_pu21_encode"), ("K_PU21_SSIM", 54, "k_pu21_ssim"),
    ("K_FSIM_LUMA", 56, "k_fsim_luma"), ("K_FSIM_DFT", 57, "k_fsim_dft"), ("K_FSIM_ENERGY", 58, "k_fsim_energy"),
    ("K_FSIM_MEDIAN", 59, "k_fsim_median"), ("K_FSIM_PC", 60, "k_fsim_pc"), ("K_FSIM_POOL", 61, "k_fsim_pool"),
    ("K_SIGSTATS_ACCUM", 63, "k_sigstats_accum"), ("K_SIGSTATS_SCAN", 64, "k_sigstats_scan"),
    ("K_SCALE", 66, "k_scale"),
    ("K_ALIGN_CROSS", 68, "k_align_cross"),
    ("K_SHIFT", 70, "k_shift"),
    ("K_LIGHT_ACCUM", 72, "k_light_accum"), ("K_LIGHT_SCAN", 73, "k_light_scan"),
    ("K_SIG", 75, "k_sig"), ("K_SIG_DIAG", 76, "k_sig_diag"), ("K_SIG_BEST", 77, "k_sig_best"),
)
# The frozen markers: where the id list ended when each feature shipped.  No kernel has a marker's id, but for K_COUNT's: the
# first kernel added after it, K_VIF, took id 12.  K_EAVE is one past the last id.
K_MARKERS = {"K_COUNT": 12, "K_COUNT_ALL": 14, "K_COUNT_EXT": 18, "K_END": 20, "K_LAST": 22, "K_PAST": 24, "K_BEYOND": 26,
             "K_LIMIT": 28, "K_TERMINUS": 33, "K_BOUND": 36, "K_FINIS": 38, "K_CLOSE": 41, "K_STOP": 43, "K_EDGE": 47, "K_BRINK": 50,
             "K_VERGE": 52, "K_RIM": 55, "K_HEM": 62, "K_FRINGE": 65, "K_MARGIN": 67, "K_LEDGE": 69, "K_SILL": 71, "K_LINTEL": 74,
             "K_EAVE": 78}
globals().update({name: k for name, k, _ in K_TABLE}, **K_MARKERS)   # K_GRAY_HIST = 0, ..., K_EAVE = 78
K_NAMES = {k: kernel for _, k, kernel in K_TABLE}
K_IDS_EXTANT = tuple(K_NAMES)                     # every id vqa_profile_read and vqa_kernel_name know
K_IDS_CAMBI = tuple(k for name, k, _ in K_TABLE if name.startswith("K_CAMBI_"))
# the id lists as earlier features shipped them, each under the name that feature gave it: the ids below that feature's marker
globals().update({ids: tuple(k for k in K_IDS_EXTANT if k < K_MARKERS[marker]) for ids, marker in (
    ("K_IDS", "K_COUNT_EXT"), ("K_IDS_ALL", "K_END"), ("K_IDS_KNOWN", "K_LAST"), ("K_IDS_EVERY", "K_PAST"),
    ("K_IDS_NAMED", "K_BEYOND"), ("K_IDS_LISTED", "K_LIMIT"), ("K_IDS_TOLD", "K_TERMINUS"), ("K_IDS_GIVEN", "K_BOUND"),
    ("K_IDS_SHOWN", "K_FINIS"), ("K_IDS_OPEN", "K_CLOSE"), ("K_IDS_FULL", "K_STOP"), ("K_IDS_WHOLE", "K_EDGE"),
    ("K_IDS_TOTAL", "K_BRINK"), ("K_IDS_SUM", "K_VERGE"), ("K_IDS_GRAND", "K_RIM"), ("K_IDS_ENTIRE", "K_HEM"),
    ("K_IDS_COMPLETE", "K_FRINGE"), ("K_IDS_PRESENT", "K_MARGIN"), ("K_IDS_CURRENT", "K_LEDGE"), ("K_IDS_LATEST", "K_SILL"),
    ("K_IDS_NEWEST", "K_LINTEL"))})

OPT_OVERLAP, OPT_HYST_STATS = 0, 1
FLAVOUR_AB_VARIANTS, FLAVOUR_TEST_SEAMS = 1, 2

DCT_AUTO, DCT_BLOCK8, DCT_FULL = 0, 1, 2
SSIM_GAUSS, SSIM_FFMPEG, SSIM_MS = 0, 1, 2
MS_LEVELS = 5
MS_MIN_DIM = 161   # SSIM_MS: level 4 of every plane must hold an 11x11 window (161 -> 81 -> 41 -> 21 -> 11)
MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
VIF_LEVELS = 4
VIF_MIN_DIM = 16   # vqa_vif_submit: level 3 of a 16 x 16 plane is 2 x 2, every reflection stays inside its level
ADM_LEVELS = 4
ADM_MIN_DIM = 16   # vqa_adm_submit: the bands of scale 3 of a 16 x 16 plane are 1 x 1
MOTION_MIN_DIM = 16   # vqa_motion_submit: the limit of VIF and ADM, whose planes it shares
SITI_MIN_DIM = 16   # vqa_siti_submit: the limit of VIF, ADM and motion, whose planes it shares
PSNR_HVS_MIN_DIM = 16   # vqa_psnr_hvs_submit: the limit of the family, whose planes it shares
CIEDE_MIN_DIM = 16   # vqa_ciede_submit: the luma grid's limit (the chroma planes of 4:2:0 may be 8 x 8)
GMSD_MIN_DIM = 16   # vqa_gmsd_submit: the limit of the family, whose planes it shares
CAMBI_MIN_DIM = 16   # vqa_cambi_submit: the limit of the family, whose planes it shares
XPSNR_MIN_DIM = 16   # vqa_xpsnr_submit: the limit of the family, whose planes it shares
HAARPSI_MIN_DIM = 16   # vqa_haarpsi_submit: the limit of the family, whose planes it shares
VCA_BLOCK = 32   # vqa_vca_submit: the side of a block, and of the smallest plane
ARTIFACTS_MIN_DIM = 16   # vqa_artifacts_submit: the limit of the family, whose planes it shares
BRISQUE_MIN_DIM = 16   # vqa_brisque_submit: the limit of the family, whose planes it shares
BRISQUE_Q = 16         # vqa_brisque_metrics: u = rint(m 2^16)
BRISQUE_FEATURES = 36
MDSI_MIN_DIM = 16   # vqa_mdsi_submit: plane 0's limit (the chroma planes of 4:2:0 may be 8 x 8)
MDSI_YUV709, MDSI_BGR, MDSI_GRAY = 0, 1, 2   # vqa_mdsi_submit's colour models
MDSI_FIX_G = 1 << 24  # vqa_mdsi_metrics: g = rint(GCS 2^24)
MDSI_FIX_Z = 1 << 28  # vqa_mdsi_metrics: the words are sums in 2^-28 units
ITP_MIN_DIM = 16   # vqa_itp_submit: the luma grid's limit (the chroma planes of 4:2:0 may be 8 x 8)
ITP_YUV2020, ITP_BGR = 0, 1   # vqa_itp_submit's colour models
ITP_PQ, ITP_HLG = 0, 1        # vqa_itp_submit's transfer functions
ITP_TRANSFERS = {"pq": ITP_PQ, "hlg": ITP_HLG}
ITP_FIX = 1 << 20  # vqa_itp_metrics: q = rint(dE_ITP 2^20)
FSIM_MIN_DIM = 16   # vqa_fsim_submit: plane 0's limit (the chroma planes of 4:2:0 may be 8 x 8)
FSIM_MAX_GRID = 1024   # vqa_fsim_submit: the limit of either side of the downsampled grid
FSIM_YUV709, FSIM_BGR, FSIM_GRAY = 0, 1, 2   # vqa_fsim_submit's colour models
FSIM_FIX = 1 << 24  # vqa_fsim_metrics: p = rint(PC 2^24), g = rint(S_L 2^24)
SIGSTATS_MIN_DIM = 16   # vqa_sigstats_submit: the limit of the family, whose planes it shares
SIGSTATS_MAX_LEVEL = 65535   # vqa_sigstats_submit: the largest black_level and crop_level
SCALE_MIN_DIM = 16   # vqa_scale_submit: the limit of the family, on both sides
SCALE_BILINEAR, SCALE_BICUBIC, SCALE_LANCZOS = 0, 1, 2   # vqa_scale_submit's filters
SCALE_FILTERS = {"bilinear": SCALE_BILINEAR, "bicubic": SCALE_BICUBIC, "lanczos": SCALE_LANCZOS}
SCALE_BITS = 22      # the tables are integers in 2^-22 fixed point
SCALE_MAX_DOWN, SCALE_MAX_UP = 4, 8   # per axis 1/4 <= out / in <= 8
SCALE_MAX_SAMPLES = 1 << 28   # h w of every plane of both lists
ALIGN_NONE = (1 << 64) - 1    # vqa_align_wait: the word of a pair whose reference frame does not exist
ALIGN_MAX_RADIUS = 32         # vqa_align_submit: the largest band radius
ALIGN_MAX_DIST, ALIGN_MAX_REF = 32768, 32768 + 64   # vqa_align_submit: the frames of one submit
SHIFT_MAX_RADIUS = 16         # vqa_shift_submit: the largest radius of the square band of shifts
SHIFT_MAX_FRAMES = 32768      # vqa_shift_submit: the frames of one submit
SHIFT_ROWS, SHIFT_FLUSH = 8, 512   # k_shift: the reference rows of a workgroup's visit, and its matrix steps between two flushes
SIG_GRID, SIG_BYTES = 16, 256     # vqa_sig_submit: the grid of cells and the bytes of a signature
SIG_MAX_BATCH = 32768         # vqa_sig_submit: the frames of one submit
SIG_MAX_FRAMES = 262144       # vqa_sig_cross_submit: the signatures of either side
LIGHT_MIN_DIM = 16            # vqa_light_submit: the luma grid's limit (the chroma planes of 4:2:0 may be 8 x 8)
LIGHT_BINS = 4096             # vqa_light_metrics: the histogram of m >> 4
LIGHT_PERCENTILES = (100, 500, 1000, 2500, 5000, 7500, 9000, 9500, 9900, 9998)   # pct_bin's ranks, per ten thousand
LIGHT_FIX = 1 << 20           # the table's unit: 2^-20 cd/m2
LIGHT_TABLE_LIMIT = 1 << 34   # every table entry is below it
LIGHT_GAMUT_709, LIGHT_GAMUT_P3 = 0, 1   # vqa_light_gamut's gamuts
LIGHT_GAMUTS = {"bt709": LIGHT_GAMUT_709, "p3": LIGHT_GAMUT_P3}
LIGHT_GAMUT_REL_SHIFT, LIGHT_GAMUT_FLOOR = 6, 1 << 32   # outside: min S < -((qmax << 16) >> 6) - 2^32
LIGHT_WALK, LIGHT_SUB_FRAMES = 8, 16384   # k_light_accum: chunks of 256 patches per workgroup; frames of one sub-slice
COLORFIT_MIN_DIM = 16         # vqa_colorfit_submit: the luma grid's limit (the chroma planes of 4:2:0 may be 8 x 8)
COLORFIT_MAX_FRAMES = 32768   # vqa_colorfit_submit: the frames of one submit
COLORFIT_MAX_BINS = 1024      # the bins of one plane's transfer table: 1 << min(depth, 10)
COLORFIT_TABLE_POSITIONS = 1 << 31   # n h w of a submit with tables
CONFORM_MIN_DIM = 16          # vqa_conform_submit: plane 0 of the destination (the other planes: 8, the chroma of 4:2:0)
CONFORM_MAX_OUT = 32768       # vqa_conform_submit: the output frames of one submit
CONFORM_MAX_COEF, CONFORM_MAX_BIAS = 1 << 20, 1 << 33   # |M[k][i]|, i < 3, and |M[k][3]| of its matrix (2^-16 fixed point)
CONVERT_MIN_DIM = 16          # vqa_convert_submit: plane 0 of both sides (the other planes: 8, the chroma of 4:2:0)
CONVERT_MAX_FRAMES = 32768    # vqa_convert_submit: the frames of one submit
FIELDS_MIN_DIM = 16           # vqa_fields_submit: the measured plane
FIELDS_MAX_FRAMES = 32768     # vqa_fields_submit: the frames of one submit
FIELDS_BAND_ROWS = 32         # k_fields_accum: the rows a lane marches (tests straddle it)
WEAVE_MIN_DIM = 16            # vqa_weave_submit: plane 0 (the other planes: 8, the chroma of 4:2:0)
WEAVE_MAX_OUT = 32768         # vqa_weave_submit: the output frames of one submit
CHROMA_BOX, CHROMA_LINEAR = 0, 1       # vqa_convert_submit's chroma filters
SITING_CENTER, SITING_LEFT = 0, 1      # its horizontal sitings (LINEAR only)
RANGE_LIMITED, RANGE_FULL = 0, 1       # its ranges
PU21_MIN_DIM = 16  # vqa_pu21_submit: the luma grid's limit (the chroma planes of 4:2:0 may be 8 x 8)
PU21_FIX = 1 << 16       # vqa_pu21_metrics: q = rint(V 2^16)
PU21_SSIM_FIX = 1 << 24  # vqa_pu21_metrics: u = rint(ssim 2^24)
PU21_SSIM_TILE = 16      # k_pu21_ssim: a workgroup owns 16 x 16 windows
HAARPSI_FIX = 1 << 30  # vqa_haarpsi_metrics: num is a sum of u wI with u = rint(2^30 sigmoid)
HAARPSI_ALPHA = 4.2    # the paper's alpha
CAMBI_SCALES = 5
CAMBI_FIX = 1 << 16  # vqa_cambi_metrics: top is a sum of u, contrasts in steps of 2^-16
CAMBI_WEIGHTS = (16, 8, 4, 2, 1)   # of pool_0 .. pool_4; cambi = their weighted sum / 31
GMSD_FIX = 1 << 24  # vqa_gmsd_metrics: the words are sums of u = rint(gms 2^24) and of u^2
CIEDE_YUV709, CIEDE_BGR = 0, 1   # vqa_ciede_submit's colour models
CIEDE_WEIGHTS_CIE = (1.0, 1.0, 1.0)       # kL, kC, kH of the CIE standard: the default
CIEDE_WEIGHTS_LIBVMAF = (0.65, 1.0, 4.0)  # what libvmaf's ciede2000 feature is believed to use (unverified: README)
MOTION_SAD, MOTION_FARNEBACK = 0, 1


class VqaParams(C.Structure):
    _fields_ = [("resize_w", C.c_int32), ("resize_h", C.c_int32),
                ("canny_low", C.c_int32), ("canny_high", C.c_int32),
                ("sad_range", C.c_int32), ("dct_mode", C.c_int32),
                ("motion_mode", C.c_int32), ("reserved", C.c_int32 * 9)]


class VqaFrameMetrics(C.Structure):
    _fields_ = [("hist_gray", C.c_uint32 * 256),
                ("hist_bgr", (C.c_uint32 * 256) * 3),
                ("sum_gray2", C.c_uint64),
                ("dct_energy", C.c_double),
                ("temporal_dct_l1", C.c_double),
                ("sad_sum", C.c_uint64),
                ("sad_blocks", C.c_uint32),
                ("mv_d2_hist", C.c_uint32 * 129),
                ("edge_count", C.c_uint32),
                ("edge_strong", C.c_uint32),
                ("edge_weak", C.c_uint32),
                ("has_prev", C.c_uint32),
                ("hyst_steps", C.c_uint32), ("orb_keypoints", C.c_uint32), ("orb_response", C.c_uint32), ("hyst_overflow", C.c_uint32),
                ("flow_mag_mean", C.c_double)]


class VqaPlaneDesc(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32),
                ("offset", C.c_int64), ("row_stride", C.c_int64),
                ("pixel_step", C.c_int32), ("bit_depth", C.c_int32)]


class VqaPlaneMetrics(C.Structure):
    _fields_ = [("sse", C.c_uint64), ("ssim", C.c_double)]


class VqaMsScales(C.Structure):
    _fields_ = [("cs", C.c_double * 5), ("ssim", C.c_double * 5)]


class VqaVifMetrics(C.Structure):
    _fields_ = [("num", C.c_double * 4), ("den", C.c_double * 4), ("scale", C.c_double * 4), ("vif", C.c_double)]


class VqaAdmMetrics(C.Structure):
    _fields_ = [("num", C.c_double * 4), ("den", C.c_double * 4), ("scale", C.c_double * 4), ("adm2", C.c_double)]


class VqaMotionMetrics(C.Structure):
    _fields_ = [("sad", C.c_double), ("motion", C.c_double)]


class VqaSitiMetrics(C.Structure):
    _fields_ = [("grad_sum", C.c_double), ("grad_sq", C.c_uint64), ("diff_sum", C.c_int64), ("diff_sq", C.c_uint64),
                ("si", C.c_double), ("ti", C.c_double)]


class VqaPsnrHvsMetrics(C.Structure):
    _fields_ = [("s_hvs", C.c_double), ("s_hvsm", C.c_double), ("psnr_hvs", C.c_double), ("psnr_hvsm", C.c_double)]


class VqaCiedeMetrics(C.Structure):
    _fields_ = [("de_sum", C.c_double), ("de_mean", C.c_double), ("ciede2000", C.c_double)]


class VqaGmsdMetrics(C.Structure):
    _fields_ = [("sum_u", C.c_uint64), ("sum_u2_lo", C.c_uint64), ("sum_u2_hi", C.c_uint64), ("count", C.c_int64),
                ("gms_mean", C.c_double), ("gmsd", C.c_double)]


class VqaCambiMetrics(C.Structure):
    _fields_ = [("top", C.c_uint64 * 5), ("k", C.c_int64 * 5), ("masked", C.c_int64 * 5), ("pool", C.c_double * 5),
                ("cambi", C.c_double)]


class VqaXpsnrMetrics(C.Structure):
    _fields_ = [("sse", C.c_uint64), ("wsse", C.c_double), ("xpsnr", C.c_double), ("block", C.c_int32), ("nbx", C.c_int32),
                ("nby", C.c_int32)]


class VqaVcaMetrics(C.Structure):
    _fields_ = [("e_sum", C.c_uint64), ("h_sum", C.c_uint64), ("l_sum", C.c_uint64), ("nbx", C.c_int32), ("nby", C.c_int32),
                ("e", C.c_double), ("h", C.c_double), ("l", C.c_double)]


class VqaArtifactsMetrics(C.Structure):
    _fields_ = [("edge_h", C.c_uint64 * 8), ("edge_v", C.c_uint64 * 8), ("blur_f_h", C.c_uint64), ("blur_v_h", C.c_uint64),
                ("blur_f_v", C.c_uint64), ("blur_v_v", C.c_uint64), ("lap", C.c_uint64), ("phase_h", C.c_int32),
                ("phase_v", C.c_int32), ("blockiness", C.c_double), ("blockiness_max", C.c_double), ("blur_h", C.c_double),
                ("blur_v", C.c_double), ("blur", C.c_double), ("noise", C.c_double)]


class VqaBrisqueMetrics(C.Structure):
    _fields_ = [("sum_abs_u", C.c_uint64 * 2), ("sum_u2", C.c_uint64 * 2)] + \
               [(k, (C.c_uint64 * 4) * 2) for k in ("n_neg", "n_pos", "sum_abs_p", "sq_neg_lo", "sq_neg_hi", "sq_pos_lo",
                                                     "sq_pos_hi")] + \
               [("flags", C.c_uint32), ("reserved", C.c_uint32), ("features", C.c_double * 36)]


class VqaMdsiMetrics(C.Structure):
    _fields_ = [("sum_pos", C.c_uint64), ("sum_neg", C.c_uint64), ("n_neg", C.c_uint64), ("sum_dev", C.c_uint64),
                ("count", C.c_int64), ("factor", C.c_int32), ("reserved", C.c_int32), ("dev", C.c_double), ("mdsi", C.c_double)]


class VqaItpMetrics(C.Structure):
    _fields_ = [("sum_q", C.c_uint64), ("max_q", C.c_uint64), ("de_sum", C.c_double), ("de_mean", C.c_double),
                ("de_max", C.c_double)]


class VqaPu21Metrics(C.Structure):
    _fields_ = [("sse_y_lo", C.c_uint64), ("sse_y_hi", C.c_uint64), ("sse_rgb_lo", C.c_uint64), ("sse_rgb_hi", C.c_uint64),
                ("ssim_q", C.c_int64), ("windows", C.c_int64), ("mse_y", C.c_double), ("mse_rgb", C.c_double),
                ("pu_psnr", C.c_double), ("pu_psnr_rgb", C.c_double), ("pu_ssim", C.c_double)]


class VqaFsimMetrics(C.Structure):
    _fields_ = [("sum_pc", C.c_uint64), ("sum_sim", C.c_uint64), ("sum_simc", C.c_uint64), ("count", C.c_int64),
                ("factor", C.c_int32), ("flags", C.c_uint32), ("fsim", C.c_double), ("fsimc", C.c_double)]


class VqaLightMetrics(C.Structure):
    _fields_ = [("count", C.c_int64), ("max_code", C.c_uint32 * 3), ("max_code_rgb", C.c_uint32), ("min_code_rgb", C.c_uint32),
                ("reserved", C.c_uint32), ("sum_q", C.c_uint64), ("sum_y", C.c_uint64), ("max_y", C.c_uint64),
                ("out_709", C.c_uint64), ("out_p3", C.c_uint64), ("clamped", C.c_uint64), ("pct_bin", C.c_uint32 * 10),
                ("max_nits", C.c_double), ("min_nits", C.c_double), ("avg_nits", C.c_double), ("y_avg", C.c_double),
                ("y_max", C.c_double), ("maxscl", C.c_double * 3), ("pct_nits", C.c_double * 10), ("share_709", C.c_double),
                ("share_p3", C.c_double)]


class VqaColorfitMetrics(C.Structure):
    _fields_ = [("count", C.c_uint64), ("sum_r", C.c_uint64 * 3), ("sum_d", C.c_uint64 * 3), ("rr", C.c_uint64 * 6),
                ("rd", C.c_uint64 * 9), ("dd", C.c_uint64 * 3), ("sse", C.c_uint64 * 3)]


class VqaFieldsMetrics(C.Structure):
    _fields_ = [("comb", C.c_uint64 * 2), ("fwd", C.c_uint64 * 2), ("bwd", C.c_uint64 * 2), ("sad", C.c_uint64 * 2),
                ("changed", C.c_uint64 * 2), ("count", C.c_uint64), ("has_prev", C.c_uint64)]


# vqa_fields_metrics as a NumPy record: what Engine.fields returns
FIELDS_DTYPE = np.dtype([("comb", np.uint64, (2,)), ("fwd", np.uint64, (2,)), ("bwd", np.uint64, (2,)), ("sad", np.uint64, (2,)),
                         ("changed", np.uint64, (2,)), ("count", np.uint64), ("has_prev", np.uint64)], align=True)


class VqaSigstatsMetrics(C.Structure):
    _fields_ = [("count", C.c_int64), ("sum", C.c_uint64), ("sum_sq", C.c_uint64), ("min", C.c_uint32), ("max", C.c_uint32),
                ("low", C.c_uint32), ("median", C.c_uint32), ("high", C.c_uint32), ("or_mask", C.c_uint32),
                ("and_mask", C.c_uint32), ("bits_used", C.c_int32), ("below_black", C.c_uint64), ("under", C.c_uint64),
                ("over_luma", C.c_uint64), ("over_chroma", C.c_uint64), ("above_peak", C.c_uint64), ("sad", C.c_uint64),
                ("changed", C.c_uint64), ("top", C.c_int32), ("bottom", C.c_int32), ("left", C.c_int32), ("right", C.c_int32),
                ("mean", C.c_double), ("stdev", C.c_double), ("dif", C.c_double)]


class VqaHaarpsiMetrics(C.Structure):
    _fields_ = [("den", C.c_uint64), ("num_lo", C.c_uint64), ("num_hi", C.c_uint64), ("similarity", C.c_double),
                ("haarpsi", C.c_double)]


# every symbol include/vqa.h declares: (restype, argtypes)
_u8p = C.c_void_p
SIGNATURES = {
    "vqa_abi_version": (C.c_int, []),
    "vqa_strerror": (C.c_char_p, [C.c_int]),
    "vqa_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "vqa_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "vqa_destroy": (C.c_int, [C.c_void_p]),
    "vqa_trim": (C.c_int, [C.c_void_p]),
    "vqa_last_hip_error": (C.c_char_p, [C.c_void_p]),
    "vqa_default_params": (None, [C.POINTER(VqaParams)]),
    "vqa_build_flavour": (C.c_int, []),
    "vqa_set_option": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "vqa_get_option": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "vqa_alloc_pinned": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "vqa_free_pinned": (C.c_int, [C.c_void_p, C.c_void_p]),
    "vqa_host_is_pinned": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_int)]),
    "vqa_alloc_device": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "vqa_free_device": (C.c_int, [C.c_void_p, C.c_void_p]),
    "vqa_copy_h2d": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "vqa_copy_d2h": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "vqa_sync": (C.c_int, [C.c_void_p]),
    "vqa_stream_wait": (C.c_int, [C.c_void_p, C.c_void_p]),
    "vqa_stream": (C.c_void_p, [C.c_void_p]),
    "vqa_complexity_submit": (C.c_int, [C.c_void_p, _u8p, _u8p, C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.c_int64, C.c_int64, C.c_uint32, C.POINTER(VqaParams)]),
    "vqa_complexity_wait": (C.c_int, [C.c_void_p, C.POINTER(VqaFrameMetrics), C.c_int]),
    "vqa_quality_submit": (C.c_int, [C.c_void_p, _u8p, _u8p, C.c_int, C.c_int, C.c_int64, C.c_int64,
                                     C.POINTER(VqaPlaneDesc), C.c_int, C.c_int]),
    "vqa_quality_wait": (C.c_int, [C.c_void_p, C.POINTER(VqaPlaneMetrics), C.c_int]),
    "vqa_quality_wait_ms": (C.c_int, [C.c_void_p, C.POINTER(VqaPlaneMetrics), C.POINTER(VqaMsScales), C.c_int]),
    "vqa_vif_submit": (C.c_int, [C.c_void_p, _u8p, _u8p, C.c_int, C.c_int, C.c_int64, C.c_int64,
                                 C.POINTER(VqaPlaneDesc), C.c_int]),
    "vqa_vif_wait": (C.c_int, [C.c_void_p, C.POINTER(VqaVifMetrics), C.c_int]),
    "vqa_adm_submit": (C.c_int, [C.c_void_p, _u8p, _u8p, C.c_int, C.c_int, C.c_int64, C.c_int64,
                                 C.POINTER(VqaPlaneDesc), C.c_int]),
    "vqa_adm_wait": (C.c_int, [C.c_void_p, C.POINTER(VqaAdmMetrics), C.c_int]),
    "vqa_motion_submit": (C.c_int, [C.c_void_p, _u8p, _u8p, C.c_int, C.c_int, C.c_int64, C.POINTER(VqaPlaneDesc), C.c_int]),
    "vqa_motion_wait": (C.c_int, [C.c_void_p, C.POINTER(VqaMotionMetrics), C.c_int]),
    "vqa_siti_submit": (C.c_int, [C.c_void_p, _u8p, _u8p, C.c_int, C.c_int, C.c_int64, C.POINTER(VqaPlaneDesc), C.c_int]),
    "vqa_siti_wait": (C.c_int, [C.c_void_p, C.POINTER(VqaSitiMetrics), C.c_int]),
    "vqa_psnr_hvs_submit": (C.c_int, [C.c_void_p, _u8p, _u8p, C.c_int, C.c_int, C.c_int64, C.c_int64, C.POINTER(VqaPlaneDesc), C.c_int]),
    "vqa_psnr_hvs_wait": (C.c_int, [C.c_void_p, C.POINTER(VqaPsnrHvsMetrics), C.c_int]),
    "vqa_ciede_submit": (C.c_int, [C.c_void_p, _u8p, _u8p, C.c_int, C.c_int, C.c_int64, C.c_int64, C.POINTER(VqaPlaneDesc), C.c_int,
                                   C.c_int, C.POINTER(C.c_double)]),
    "vqa_ciede_wait": (C.c_int, [C.c_void_p, C.POINTER(VqaCiedeMetrics), C.c_int]),
    "vqa_gmsd_submit": (C.c_int, [C.c_void_p, _u8p, _u8p, C.c_int, C.c_int, C.c_int64, C.c_int64, C.POINTER(VqaPlaneDesc), C.c_int]),
    "vqa_gmsd_wait": (C.c_int, [C.c_void_p, C.POINTER(VqaGmsdMetrics), C.c_int]),
    "vqa_cambi_submit": (C.c_int, [C.c_void_p, _u8p, C.c_int, C.c_int, C.c_int64, C.POINTER(VqaPlaneDesc), C.c_int]),
    "vqa_cambi_wait": (C.c_int, [C.c_void_p, C.POINTER(VqaCambiMetrics), C.c_int]),
    "vqa_xpsnr_submit": (C.c_int, [C.c_void_p, _u8p, _u8p, _u8p, C.c_int, C.c_int, C.c_int64, C.c_int64, C.POINTER(VqaPlaneDesc),
                                   C.c_int]),
    "vqa_xpsnr_wait": (C.c_int, [C.c_void_p, C.POINTER(VqaXpsnrMetrics), C.c_int, C.POINTER(C.c_uint64), C.c_int64]),
    "vqa_haarpsi_submit": (C.c_int, [C.c_void_p, _u8p, _u8p, C.c_int, C.c_int, C.c_int64, C.c_int64, C.POINTER(VqaPlaneDesc), C.c_int]),
    "vqa_haarpsi_wait": (C.c_int, [C.c_void_p, C.POINTER(VqaHaarpsiMetrics), C.c_int]),
    "vqa_vca_submit": (C.c_int, [C.c_void_p, _u8p, _u8p, C.c_int, C.c_int, C.c_int64, C.POINTER(VqaPlaneDesc), C.c_int]),
    "vqa_vca_wait": (C.c_int, [C.c_void_p, C.POINTER(VqaVcaMetrics), C.c_int, C.POINTER(C.c_uint64), C.c_int64]),
    "vqa_artifacts_submit": (C.c_int, [C.c_void_p, _u8p, C.c_int, C.c_int, C.c_int64, C.POINTER(VqaPlaneDesc), C.c_int]),
    "vqa_artifacts_wait": (C.c_int, [C.c_void_p, C.POINTER(VqaArtifactsMetrics), C.c_int]),
    "vqa_brisque_submit": (C.c_int, [C.c_void_p, _u8p, C.c_int, C.c_int, C.c_int64, C.POINTER(VqaPlaneDesc), C.c_int]),
    "vqa_brisque_wait": (C.c_int, [C.c_void_p, C.POINTER(VqaBrisqueMetrics), C.c_int]),
    "vqa_mdsi_submit": (C.c_int, [C.c_void_p, _u8p, _u8p, C.c_int, C.c_int, C.c_int64, C.c_int64, C.POINTER(VqaPlaneDesc), C.c_int,
                                  C.c_int]),
    "vqa_mdsi_wait": (C.c_int, [C.c_void_p, C.POINTER(VqaMdsiMetrics), C.c_int]),
    "vqa_mdsi_factor": (C.c_int, [C.c_int, C.c_int]),
    "vqa_itp_submit": (C.c_int, [C.c_void_p, _u8p, _u8p, C.c_int, C.c_int, C.c_int64, C.c_int64, C.POINTER(VqaPlaneDesc), C.c_int,
                                 C.c_int, C.c_int, C.c_int]),
    "vqa_itp_wait": (C.c_int, [C.c_void_p, C.POINTER(VqaItpMetrics), C.c_int]),
    "vqa_pu21_submit": (C.c_int, [C.c_void_p, _u8p, _u8p, C.c_int, C.c_int, C.c_int64, C.c_int64, C.POINTER(VqaPlaneDesc), C.c_int,
                                  C.c_int, C.c_int, C.c_int]),
    "vqa_pu21_wait": (C.c_int, [C.c_void_p, C.POINTER(VqaPu21Metrics), C.c_int]),
    "vqa_pu21_encode": (C.c_double, [C.c_double]),
    "vqa_fsim_submit": (C.c_int, [C.c_void_p, _u8p, _u8p, C.c_int, C.c_int, C.c_int64, C.c_int64, C.POINTER(VqaPlaneDesc), C.c_int,
                                  C.c_int]),
    "vqa_fsim_wait": (C.c_int, [C.c_void_p, C.POINTER(VqaFsimMetrics), C.c_int]),
    "vqa_fsim_noise_factor": (C.c_double, [C.c_int, C.c_int, C.c_int]),
    "vqa_fsim_filter": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    "vqa_sigstats_submit": (C.c_int, [C.c_void_p, _u8p, _u8p, C.c_int, C.c_int, C.c_int64, C.POINTER(VqaPlaneDesc), C.c_int, C.c_int,
                                      C.c_int]),
    "vqa_sigstats_wait": (C.c_int, [C.c_void_p, C.POINTER(VqaSigstatsMetrics), C.c_int, C.c_int, C.POINTER(C.c_uint64), C.c_int64]),
    "vqa_scale_submit": (C.c_int, [C.c_void_p, _u8p, C.c_int, C.c_int, C.c_int64, C.POINTER(VqaPlaneDesc), C.c_void_p, C.c_int64,
                                   C.POINTER(VqaPlaneDesc), C.c_int, C.c_int]),
    "vqa_scale_wait": (C.c_int, [C.c_void_p]),
    "vqa_scale_tables": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                   C.POINTER(C.c_int)]),
    "vqa_align_submit": (C.c_int, [C.c_void_p, _u8p, C.c_int, _u8p, C.c_int, C.c_int, C.c_int64, C.c_int64, C.POINTER(VqaPlaneDesc),
                                   C.c_int, C.c_int]),
    "vqa_align_wait": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_int64]),
    "vqa_shift_submit": (C.c_int, [C.c_void_p, _u8p, _u8p, C.c_int, C.c_int, C.c_int64, C.c_int64, C.POINTER(VqaPlaneDesc), C.c_int,
                                   C.c_int]),
    "vqa_shift_wait": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_int64]),
    "vqa_light_submit": (C.c_int, [C.c_void_p, _u8p, C.c_int, C.c_int, C.c_int64, C.POINTER(VqaPlaneDesc), C.c_int, C.c_int, C.c_int,
                                   C.POINTER(C.c_uint64), C.c_int]),
    "vqa_light_wait": (C.c_int, [C.c_void_p, C.POINTER(VqaLightMetrics), C.c_int, C.POINTER(C.c_uint32)]),
    "vqa_light_table": (C.c_int, [C.c_int, C.POINTER(C.c_uint64)]),
    "vqa_light_gamut": (C.c_int, [C.c_int, C.POINTER(C.c_int64)]),
    "vqa_sig_submit": (C.c_int, [C.c_void_p, _u8p, C.c_int, C.c_int, C.c_int64, C.POINTER(VqaPlaneDesc)]),
    "vqa_sig_wait": (C.c_int, [C.c_void_p, _u8p, C.c_int]),
    "vqa_sig_cross_submit": (C.c_int, [C.c_void_p, _u8p, C.c_int, _u8p, C.c_int]),
    "vqa_sig_cross_wait": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_int64, C.POINTER(C.c_uint64), C.c_int64]),
    "vqa_colorfit_submit": (C.c_int, [C.c_void_p, _u8p, _u8p, C.c_int, C.c_int, C.c_int64, C.c_int64, C.POINTER(VqaPlaneDesc), C.c_int,
                                      C.c_int]),
    "vqa_colorfit_wait": (C.c_int, [C.c_void_p, C.POINTER(VqaColorfitMetrics), C.c_int, C.POINTER(C.c_uint64), C.c_int64]),
    "vqa_conform_submit": (C.c_int, [C.c_void_p, _u8p, C.c_int, C.c_int, C.c_int64, C.POINTER(VqaPlaneDesc), C.c_void_p, C.c_int64,
                                     C.POINTER(VqaPlaneDesc), C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int,
                                     C.c_void_p, C.POINTER(C.c_int64)]),
    "vqa_conform_wait": (C.c_int, [C.c_void_p]),
    "vqa_convert_submit": (C.c_int, [C.c_void_p, _u8p, C.c_int, C.c_int, C.c_int64, C.POINTER(VqaPlaneDesc), C.c_void_p, C.c_int64,
                                     C.POINTER(VqaPlaneDesc), C.c_int, C.c_int, C.c_int, C.c_int]),
    "vqa_convert_wait": (C.c_int, [C.c_void_p]),
    "vqa_fields_submit": (C.c_int, [C.c_void_p, _u8p, _u8p, C.c_int, C.c_int, C.c_int64, C.POINTER(VqaPlaneDesc)]),
    "vqa_fields_wait": (C.c_int, [C.c_void_p, C.POINTER(VqaFieldsMetrics), C.c_int]),
    "vqa_weave_submit": (C.c_int, [C.c_void_p, _u8p, C.c_int, C.c_int, C.c_int64, C.POINTER(VqaPlaneDesc), C.c_void_p, C.c_int64,
                                   C.POINTER(VqaPlaneDesc), C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int]),
    "vqa_weave_wait": (C.c_int, [C.c_void_p]),
    "vqa_profile_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "vqa_profile_read": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_int]),
    "vqa_kernel_name": (C.c_char_p, [C.c_int]),
    "vqa_debug_read_plane": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _u8p, C.c_int, C.c_int]),
    "vqa_debug_read_farneback": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int]),
    "vqa_comm_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_void_p)]),
    "vqa_comm_unique_id": (C.c_int, [C.c_void_p, C.c_size_t]),
    "vqa_comm_create_rank": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "vqa_comm_destroy": (C.c_int, [C.c_void_p]),
    "vqa_comm_size": (C.c_int, [C.c_void_p]),
    "vqa_comm_last_error": (C.c_char_p, [C.c_void_p]),
    "vqa_comm_debug_trace": (C.c_char_p, []),
    "vqa_allreduce": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.c_int]),
}

_lib = None


class VqaError(RuntimeError):
    def __init__(self, status, where, detail=""):
        self.status = status
        msg = "%s failed: %s (%d)" % (where, _strerror(status), status)
        if detail:
            msg += " — " + detail
        super().__init__(msg)


def _strerror(status):
    try:
        return load().vqa_strerror(status).decode()
    except Exception:
        return "status %d" % status


# symbols of the lab build alone (vqa_build_flavour() & FLAVOUR_TEST_SEAMS); include/vqa.h declares them under VQA_TEST_SEAMS
LAB_SIGNATURES = {
    "vqa_pu21_lab_read_maps": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_int64]),
    "vqa_fsim_lab_read_maps": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_int64]),
}


def load():
    """Load libvqa_hip.so and bind every declared symbol.  Raises if the
    library has not been built (run `python -c 'import __graft_entry__ as g; g.build()'`)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "HIP extension not built: %s is missing. Build it with `make -C %s` "
            "(there is no CPU fallback)." % (LIB_PATH, os.path.dirname(LIB_PATH)))
    # PyTorch-ROCm bundles its own libamdhip64.so.7.  If torch is importable, load it
    # first so this process holds ONE HIP runtime (the dynamic linker then resolves
    # our DT_NEEDED libamdhip64.so.7 to the copy torch already mapped).
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL if hasattr(C, "RTLD_GLOBAL") else 0)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    for name, (res, args) in LAB_SIGNATURES.items():   # the lab build's own symbols: absent from the shipped library
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype = res
            fn.argtypes = args
    if lib.vqa_abi_version() != VQA_ABI_VERSION:
        raise ImportError("libvqa_hip.so ABI %d != binding ABI %d" % (lib.vqa_abi_version(), VQA_ABI_VERSION))
    _lib = lib
    return lib


def check(status, where, ctx=None):
    if status != VQA_OK:
        detail = ""
        if ctx is not None and status in (VQA_ERR_HIP, VQA_ERR_OOM, VQA_ERR_INCOMPLETE):
            detail = load().vqa_last_hip_error(ctx).decode()
        raise VqaError(status, where, detail)


# ---------------------------------------------------------------------------
# roctx ranges (SURVEY.md section 5 "Tracing": rocprofv3 --marker-trace): named ranges around the host-side stages of a pass,
# so a trace shows gather / upload / submit / wait / tails per chunk and lane next to the kernels and copies.  The marker
# library is looked for only when a profiler is attached (rocprofv3 preloads its tool library) or VQA_ROCTX=1 asks for it;
# everywhere else - and when the library is absent - trace_range() is a no-op that costs one attribute test.
# ---------------------------------------------------------------------------
_roctx = None


def _roctx_wanted():
    v = os.environ.get("VQA_ROCTX")
    if v is not None:
        return v not in ("", "0")
    return "rocprofiler" in os.environ.get("LD_PRELOAD", "") or "ROCP_TOOL_LIBRARIES" in os.environ


def _roctx_load():
    global _roctx
    if _roctx is None:
        _roctx = False
        if _roctx_wanted():
            for name in ("librocprofiler-sdk-roctx.so", "librocprofiler-sdk-roctx.so.1", "libroctx64.so", "libroctx64.so.4"):
                for where in ("", "/opt/rocm/lib/"):
                    try:
                        lib = C.CDLL(where + name)
                        lib.roctxRangePushA.argtypes = [C.c_char_p]
                        lib.roctxRangePushA.restype = C.c_int
                        lib.roctxRangePop.restype = C.c_int
                        _roctx = lib
                        return _roctx
                    except (OSError, AttributeError):
                        continue
    return _roctx


class _Range:
    __slots__ = ("name",)

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        _roctx.roctxRangePushA(self.name)

    def __exit__(self, *a):
        _roctx.roctxRangePop()
        return False


class _NoRange:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


_NO_RANGE = _NoRange()


def trace_range(name, *args):
    """with trace_range("vqa:upload k=%d lane=%d", k, lane): ... - a roctx range when markers are on, else nothing"""
    lib = _roctx if _roctx is not None else _roctx_load()
    if not lib:
        return _NO_RANGE
    return _Range((name % args if args else name).encode())


def roctx_active():
    return bool(_roctx if _roctx is not None else _roctx_load())
