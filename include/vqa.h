/*
 * vqa.h — C ABI of the MI355X-native per-frame video complexity / quality engine.
 *
 * This is the drop-in boundary for the ONE hot path of
 * zaki699/Real-Time-Video-Quality-Analysis (reference @ 2024-10-16):
 *
 *   complexity_metrics.py:246-310  calculate_average_scene_complexity
 *   complexity_metrics.py:128-148  process_in_batches        (the data-parallel map)
 *   complexity_metrics.py:313-579  process_*_frame           (the per-frame kernels)
 *   video_processing.py:270-297    run_ffmpeg_metrics        (PSNR + SSIM)
 *
 * The reference has no FFI of its own (it is Python over opencv_python and an
 * ffmpeg subprocess); the entry points below are what a ctypes binding for that
 * path binds (INTEGRATION.md shows the stub).  Plain pointers and sizes only —
 * no torch / numpy types.  Every function returns VQA_OK (0) or a negative
 * vqa_status; nothing throws.
 *
 * Threading: one vqa_ctx per device per host thread (a thread may own several: two that
 * measure alternate chunks and one that only copies, tied together by vqa_stream_wait, is
 * the pipeline this library is built for).  A ctx owns one HIP stream,
 * its scratch planes and a pinned result staging area; it is NOT thread-safe.
 * Different contexts may be used from different threads at the same time.
 * Buffers handed to a *_submit call must stay alive and unmodified until the
 * matching *_wait returns.
 * Process-wide state, all of it: (1) the HIP runtime; (2) the table of RCCL entry
 * points, filled once by the first vqa_comm_create* / vqa_comm_unique_id call
 * (a C++11 function-local static: concurrent first calls are safe); (3) immutable
 * function-local constants.  Everything mutable - scratch, cached tables, launch
 * geometry derived from the device (queried in vqa_create), options, error text -
 * is a field of the ctx.
 *
 * Memory: a ctx keeps what it has grown - scratch planes sized by the largest batch
 * seen (Farneback: up to ~13.5 GiB), result staging, and small per-geometry tables
 * (at most VQA_TABLE_CACHE_GEOMETRIES entries of each kind, least recently used
 * evicted) - so that a steady stream of batches allocates nothing.  vqa_trim gives
 * all of it back without destroying the ctx (the reference holds nothing between
 * calls: a process pool per call, complexity_metrics.py:143-147).
 *
 * There is NO CPU fallback: vqa_create fails with VQA_ERR_NO_DEVICE when no
 * gfx950 device is visible.
 *
 * Environment.  The shipped library reads exactly ONE environment variable, once per
 * vqa_create: VQA_OVERLAP (0 / 1) = the initial value of VQA_OPT_OVERLAP below (a
 * scheduling choice; results are identical either way).  No environment variable
 * selects a kernel or changes an arithmetic path.  (The Python binding additionally
 * honours VQA_LIB_PATH to load another build of this ABI, VQA_DEVICE / LOCAL_RANK for the default
 * device, VQA_MOTION for the default motion definition and VQA_ROCTX for roctx ranges.)  A separate
 * LAB build (`make -C csrc lab` -> lab/libvqa_hip_lab.so, vqa_build_flavour() != 0)
 * keeps superseded kernels and test seams behind VQA_*_VARIANT / VQA_COMM_FAKE_RCCL /
 * VQA_HYST_MAX_ROUNDS / VQA_HYST_RESCUE_MAX_ROUNDS / VQA_FAIL_ENSURE_AT / VQA_FB_CHUNK_BYTES; it is for re-measurement and fault
 * injection only and is never loaded by default.
 */
#ifndef VQA_H
#define VQA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define VQA_API __attribute__((visibility("default")))
#else
#define VQA_API
#endif

#define VQA_ABI_VERSION 8
#define VQA_TABLE_CACHE_GEOMETRIES 16

typedef enum vqa_status {
    VQA_OK = 0,
    VQA_ERR_INVALID = -1,     /* bad argument (NULL, non-positive size, bad mask ...)   */
    VQA_ERR_NO_DEVICE = -2,   /* no HIP device / device index out of range              */
    VQA_ERR_HIP = -3,         /* a HIP runtime call failed (vqa_last_hip_error)         */
    VQA_ERR_OOM = -4,         /* device or pinned allocation failed                     */
    VQA_ERR_UNSUPPORTED = -5, /* valid request this build does not implement            */
    VQA_ERR_STATE = -6,       /* wait without submit, submit while one is pending ...   */
    VQA_ERR_INCOMPLETE = -7   /* a result would be inexact and is withheld: vqa_complexity_wait when a frame's Canny
                                 hysteresis did not reach its fixpoint (vqa_last_hip_error names the frame)            */
} vqa_status;

typedef struct vqa_ctx vqa_ctx;

/* where a frame pointer handed to *_submit lives */
typedef enum vqa_mem_kind {
    VQA_MEM_HOST = 0,   /* pageable or pinned host memory: the engine copies H2D on its stream */
    VQA_MEM_DEVICE = 1  /* device memory on the ctx's device (vqa_alloc_device, torch data_ptr) */
} vqa_mem_kind;

/* ---- metric selection (one bit per reference kernel) --------------------- */
#define VQA_M_GRAY_HIST     (1u << 0) /* process_histogram_frame        complexity_metrics.py:392-416 */
#define VQA_M_COLOR_HIST    (1u << 1) /* process_color_histogram_frame  complexity_metrics.py:418-475 */
#define VQA_M_DCT           (1u << 2) /* process_dct_frame              complexity_metrics.py:346-364 */
#define VQA_M_TEMPORAL_DCT  (1u << 3) /* process_temporal_dct_frame     complexity_metrics.py:543-579 */
#define VQA_M_EDGE          (1u << 4) /* process_edge_frame             complexity_metrics.py:477-504 */
#define VQA_M_MOTION        (1u << 5) /* process_frame_complexity       complexity_metrics.py:313-343
                                         (block-SAD substitute for Farneback)         */
#define VQA_M_ORB           (1u << 6) /* process_orb_frame_for_parallel complexity_metrics.py:367-389
                                         (always on the 64x64 thumbnail, as the reference hard-codes) */
#define VQA_M_ALL           0x7Fu

/* dct_mode */
#define VQA_DCT_AUTO   0 /* FULL when resize_w*resize_h <= 128*128, else BLOCK8            */
#define VQA_DCT_BLOCK8 1 /* 8x8 block DCT-II (north_star).  Energy == full-frame energy     */
#define VQA_DCT_FULL   2 /* one full-frame DCT-II, exactly what cv2.dct computes            */

/* motion_mode (what VQA_M_MOTION computes) */
#define VQA_MOTION_SAD       0 /* 16x16 block-SAD full search (north_star; default)          */
#define VQA_MOTION_FARNEBACK 1 /* cv2.calcOpticalFlowFarneback(.., 0.5, 3, 15, 3, 5, 1.2, 0)
                                  mean magnitude — what the reference computes (:340-343).
                                  Scratch on the device: 59 bytes per pixel and pair of a chunk,
                                  chunks of up to 12 GiB (64 pairs of 1080p = 7.8 GB) and never
                                  more than 80 % of what the device has free (halved again if the
                                  reservation still fails), kept by the ctx until vqa_trim /
                                  vqa_destroy                                                  */

/* ssim_mode */
#define VQA_SSIM_GAUSS  0 /* 11x11 Gaussian window, sigma 1.5 (north_star)                  */
#define VQA_SSIM_FFMPEG 1 /* FFmpeg vf_ssim: integer 8x8 window, stride 4 (what the
                             reference's subprocess really computes, video_processing.py:276) */
#define VQA_SSIM_MS     2 /* multi-scale SSIM (Wang, Simoncelli, Bovik 2003) over the Gaussian window, in the 2x2-mean form of
                             tf.image.ssim_multiscale / pytorch-msssim: five levels, level s+1 = the exact mean of each 2x2
                             block of level s (an odd level's last row / column duplicated first; dims ceil(dim / 2)), per
                             level the means cs_s, ssim_s of the window's contrast-structure and full maps, and
                             MS-SSIM = prod_{s<4} max(cs_s,0)^w_s * max(ssim_4,0)^w_4, w = (.0448,.2856,.3001,.2363,.1333)
                             (a negative mean gives 0).  Level 4 must hold a window: every plane of the submit must be at
                             least 161 x 161 (a 4:2:0 frame 321 x 321), VQA_ERR_UNSUPPORTED below; depths, alignment and
                             mixed depths are refused as for VQA_SSIM_GAUSS.  Scratch on the device: 2.7 bytes per pixel of
                             the largest group of same-geometry planes of a batch (levels 1..4 of both images as fp32 sums),
                             kept by the ctx until vqa_trim / vqa_destroy                                                 */

typedef struct vqa_params {
    int32_t resize_w, resize_h; /* cv2.resize target; 0 or == frame size -> native (copy)  */
    int32_t canny_low, canny_high; /* cv2.Canny thresholds; reference uses 100, 200 (:503)  */
    int32_t sad_range;          /* block-SAD search radius R, 0..7 (default 7)              */
    int32_t dct_mode;           /* VQA_DCT_*                                                */
    int32_t motion_mode;        /* VQA_MOTION_*                                             */
    int32_t reserved[9];        /* must be zero                                             */
} vqa_params;

/* Per-frame results of the complexity kernels.  Integer fields are exact
 * (bit-identical to the CPU reference); double fields carry float sums.    */
typedef struct vqa_frame_metrics {
    uint32_t hist_gray[256];     /* calcHist of gray(resize(frame))        (:404-412)       */
    uint32_t hist_bgr[3][256];   /* calcHist of resize(frame) channels B,G,R (:430,455-457) */
    uint64_t sum_gray2;          /* exact sum of squares of the DCT input plane (Parseval)  */
    double   dct_energy;         /* sum(dct(resize(gray(frame)))**2)       (:358-364)       */
    double   temporal_dct_l1;    /* sum|dct(prev) - dct(curr)|; 0 if no previous frame      */
    uint64_t sad_sum;            /* sum over blocks of the winning SAD                      */
    uint32_t sad_blocks;         /* number of 16x16 blocks measured; 0 if no previous frame */
    uint32_t mv_d2_hist[129];    /* blocks per winning dx^2+dy^2                            */
    uint32_t edge_count;         /* np.sum(cv2.Canny(gray,low,high) > 0)   (:503-504)       */
    uint32_t edge_strong;        /* pixels above `high` that survive NMS                    */
    uint32_t edge_weak;          /* NMS survivors in (low, high]                            */
    uint32_t has_prev;           /* 1 if a previous frame was available                     */
    uint32_t hyst_steps;         /* diagnostics only (scheduling-dependent): relaxation steps summed over tile visits;
                                    0 unless VQA_OPT_HYST_STATS is set on the ctx (it costs an atomic per visit) */
    uint32_t orb_keypoints;      /* len(ORB_create().detectAndCompute(gray64)[0])  (:385-389)  */
    uint32_t orb_response;       /* FAST score of that keypoint, 0 when there is none       */
    uint32_t hyst_overflow;      /* how the Canny hysteresis of this frame ended.  0: the tail reached the fixpoint (every frame
                                    seen so far).  2: the tail stopped at its round bound and the rescue pass completed the
                                    fixpoint on the device - edge_count is exact either way.  1 is never returned: a frame that
                                    neither pass finished makes vqa_complexity_wait fail with VQA_ERR_INCOMPLETE and zero the
                                    records - edge_count is a bit-exact count or there is no count (complexity_metrics.py:503-504) */
    double   flow_mag_mean;      /* VQA_MOTION_FARNEBACK: np.mean(|flow|) (:342-343); else 0.  Bar: 1e-4 relative against
                                    the CPU restatement of cv2.calcOpticalFlowFarneback, EXCEPT on frames where a border
                                    pixel's flow lies within float rounding of FarnebackUpdateMatrices' in-frame test
                                    (a discontinuity of the algorithm: either side is a valid evaluation; seen on
                                    35x31 / 129x34 noise frames, 4e-4 on the mean) - there 2e-3.
                                    Independent of how frames are batched (round 6): the running column sums of the flow
                                    iteration restart at every multiple of 16 rows - the only rows where a row strip may
                                    begin - and the magnitudes are summed in 2^-28 fixed point, so the strip count a launch
                                    picks from its number of pairs changes speed, never a bit (rounds 4-5: <= 1e-6 between
                                    batch sizes).  Every field of this record is independent of the batch. */
} vqa_frame_metrics;

/* One plane inside a frame buffer (planar YUV plane, or one channel of packed BGR with pixel_step = 3).
 * bit_depth (ABI 8; the padding word of ABI 7): 0 or 8 = uint8 samples, exactly the ABI 7 behaviour; 9..16 = little-endian
 * uint16 samples of that depth (yuv420p10le and its kin), whose offset, row_stride and pixel_step must be even.  One depth
 * per vqa_quality_submit: planes of a submit that mix depths, a depth outside {0, 8..16} and an odd 16-bit offset, stride
 * or step are VQA_ERR_INVALID.  Samples above max = 2^depth - 1 are read as they are, not clipped (as FFmpeg's psnr / ssim
 * filters read them).  The metrics follow FFmpeg for that depth: vf_psnr's peak is max (the caller's stats lines), vf_ssim's
 * constants are .01^2 max^2 64 and .03^2 max^2 64 63 with double end formulas, and the Gaussian SSIM takes data range
 * L = max (C1 = (.01 L)^2, C2 = (.03 L)^2).
 * Magnitudes: offset, row_stride and the frame strides of every submit are honoured at any magnitude the allocation holds - a
 * frame, a plane or a row may start beyond byte 2^31 or 2^32 of its stream (a resident clip of a few hundred 2160p frames does);
 * every kind forms these addresses in 64 bits.  The one refusal: VQA_SSIM_GAUSS and VQA_SSIM_MS address the rows of a plane with
 * 32 bits and return VQA_ERR_UNSUPPORTED for a plane whose height * row_stride + width * pixel_step reaches 2^31 (its frames
 * and its offset may still lie anywhere).  A plane whose last byte, offset + height * row_stride + width * pixel_step, does not
 * fit int64_t is VQA_ERR_INVALID.  Every depth from 9 to 16 is a tested input of every kind, not only 10, 12 and 16.          */
typedef struct vqa_plane_desc {
    int32_t width, height;
    int64_t offset;      /* bytes from the start of the frame                 */
    int64_t row_stride;  /* bytes between rows                                */
    int32_t pixel_step;  /* bytes between horizontally adjacent samples       */
    int32_t bit_depth;   /* 0 / 8: uint8 samples; 9..16: little-endian uint16 */
} vqa_plane_desc;

typedef struct vqa_plane_metrics {
    uint64_t sse;   /* sum (ref - dist)^2 over the plane — FFmpeg psnr's per-component sum (exact at every depth) */
    double   ssim;  /* mean SSIM of the plane in the selected ssim_mode (VQA_SSIM_MS: the plane's MS-SSIM).  Independent of how frames are batched: the Gaussian
                       kernel sums the SSIM map in 2^-27 fixed point (integer sums are associative, so the strip geometry a
                       launch picks from its workgroup count cannot show; rounds 1-5 summed floats and differed by <= 1e-8
                       between batch sizes); vf_ssim's samples are summed in double, exactly for planes below ~2^28
                       samples.  The same frame pair gives the same bits in any batch; sse is exact */
} vqa_plane_metrics;

/* The per-scale means behind one VQA_SSIM_MS value (vqa_quality_wait_ms): level 0 is the plane, level 4 the coarsest.
 * ssim[0] is, bit for bit, what VQA_SSIM_GAUSS returns for the plane.  Independent of the batch, as vqa_plane_metrics.ssim. */
typedef struct vqa_ms_scales {
    double cs[5];    /* mean of the contrast-structure map (2 s_xy + C2) / (s_x^2 + s_y^2 + C2) of each level */
    double ssim[5];  /* mean of the SSIM map of each level                                                   */
} vqa_ms_scales;

/* VIF (visual information fidelity, Sheikh & Bovik 2006, pixel domain) of one plane pair on four scales: the vif_scale0..3
 * features of VMAF (vqa_vif_submit / vqa_vif_wait; the definition is stated there).  Level 0 is the plane, level 3 the
 * coarsest.  num and den are the device's integer totals times 2^-27: every per-sample term is rounded to 2^-27 and summed in
 * signed 64 bits.  A term is below 64 in magnitude for any 16-bit input (s1 < 2^30 and g <= 100 give num < 43; samples inside
 * their depth's range give s1 <= 2^14 and num < 27; 1 - s2 smi may be slightly negative), so a plane of 2^28 samples sums to
 * less than 2^61 and cannot overflow.  Integer sums are associative: the same pair gives the same bits in any batch.      */
typedef struct vqa_vif_metrics {
    double num[4], den[4]; /* sum over the level of the per-sample numerator / denominator terms     */
    double scale[4];       /* num[s] / den[s] (1 when den[s] == 0): libvmaf's vif_scale0..3          */
    double vif;            /* sum_s num[s] / sum_s den[s] (1 when the denominator is 0)              */
} vqa_vif_metrics;

/* ADM (detail loss metric, Li et al. 2011, on a four-level db2 wavelet pyramid) of one plane pair: the adm2 and adm_scale0..3
 * features of VMAF (vqa_adm_submit / vqa_adm_wait; the definition is stated there).  Scale 0 is the finest.
 * Sums: per scale the device adds six sums of cubes over the pooled region (three bands, numerator and denominator).  A cube
 * max(|rf r| - thr, 0)^3 or |rf o|^3 is below 242 at scale 0 and 4.7e7 at scale 3 for samples inside their depth's range
 * (|band| <= 128 * 1.6731^(2 (s + 1)), rf <= 0.0457), and below 7.7e14 for ARBITRARY 16-bit samples (depth 9: 255 times the
 * range); the region of scale s has at most 2^(28 - 2 (s + 1)) samples, so a total stays below 1e21.  That span (values of
 * interest from 1e-9 up) does not fit one 64-bit fixed-point scale, so the sums are NOT integers: every workgroup owns a
 * fixed 32 x 16 tile of the bands - the tiling depends on the plane's geometry alone -, adds its cubes in a fixed order
 * (fp32 per thread, doubles across the workgroup) and stores one partial; the partials of a plane are then added in double in
 * a fixed order.  The same pair therefore gives the same num / den bits at any place of any batch, from host or device memory.
 * The cube roots and quotients are formed in double on the host by vqa_adm_wait.                                        */
typedef struct vqa_adm_metrics {
    double num[4], den[4]; /* sum over the three bands of cbrt(sum of cubes over the region) + cbrt(area / 32)  */
    double scale[4];       /* num[s] / den[s] (den[s] > 0 always): libvmaf's adm_scale0..3                      */
    double adm2;           /* sum_s num[s] / sum_s den[s] (each sum 0 below 1e-10 h w / (1920 * 1080); 1 when the
                              denominator is 0)                                                                 */
} vqa_adm_metrics;

/* VMAF's motion feature of one reference plane against the same plane of the frame before (vqa_motion_submit / vqa_motion_wait;
 * the definition is stated there).  sad is the device's integer total times 2^-16: every per-sample term |d| is rounded to 2^-16
 * (at most 2^-17 away) and summed in signed 64 bits - VIF's scheme.  |d| < 2^15 for ANY 16-bit input (depth 9: samples reach
 * 65535 / 2 - 128), so a term is below 2^31 and a plane of 2^28 samples sums to less than 2^59: no overflow.  Integer sums are
 * associative: the same pair of frames gives the same bits at any place of any batch, from host or device memory.  The
 * division by h w is made in double on the host by vqa_motion_wait.                                                        */
typedef struct vqa_motion_metrics {
    double sad;     /* sum over the plane of |blur(frame i) - blur(frame i-1)|; 0 without a predecessor      */
    double motion;  /* sad / (h w): libvmaf's `motion` of the frame                                          */
} vqa_motion_metrics;

/* ITU-T P.910 spatial and temporal information of one reference plane (vqa_siti_submit / vqa_siti_wait; the definition and the
 * bounds of the sums are stated there).  The four sums are the device's integers - grad_sum is its 2^-32 fixed-point total,
 * (double) hi + (double) lo 2^-32 -, so the same frame (with its predecessor) gives the same bits at any place of any batch, from
 * host or device memory; si and ti are formed from them in double on the host by vqa_siti_wait.                            */
typedef struct vqa_siti_metrics {
    double   grad_sum; /* sum over the interior of sqrt(gx^2 + gy^2), each term rounded to 2^-32                   */
    uint64_t grad_sq;  /* sum over the interior of gx^2 + gy^2                                                    */
    int64_t  diff_sum; /* sum over the plane of R_i - R_{i-1}; 0 without a predecessor                            */
    uint64_t diff_sq;  /* sum over the plane of (R_i - R_{i-1})^2; 0 without a predecessor                        */
    double   si;       /* population standard deviation of the Sobel magnitude over the interior, 8-bit scale     */
    double   ti;       /* population standard deviation of the frame difference over the plane, 8-bit scale; 0
                          without a predecessor                                                                   */
} vqa_siti_metrics;

/* PSNR-HVS and PSNR-HVS-M of one plane pair (vqa_psnr_hvs_submit / vqa_psnr_hvs_wait; the definition and the bounds of the
 * sums are stated there).  s_hvs and s_hvsm are the device's 2^-20 fixed-point integer totals divided by the coefficient
 * count, so the same pair gives the same bits at any place of any batch, from host or device memory; the two dB values are
 * formed from them in double on the host by vqa_psnr_hvs_wait.                                                              */
typedef struct vqa_psnr_hvs_metrics {
    double s_hvs;     /* mean over the coefficients of the whole 8x8 blocks of (|A - B| csf)^2                        */
    double s_hvsm;    /* likewise with the contrast-masking threshold taken off |A - B| first; s_hvsm <= s_hvs       */
    double psnr_hvs;  /* 10 log10((2^depth - 1)^2 / s_hvs), +infinity when s_hvs = 0                                  */
    double psnr_hvsm; /* 10 log10((2^depth - 1)^2 / s_hvsm), +infinity when s_hvsm = 0                                */
} vqa_psnr_hvs_metrics;

/* CIEDE2000 colour difference of one frame pair, the three planes of a pixel taken together (vqa_ciede_submit /
 * vqa_ciede_wait; the definition and the bound of the sum are stated there).  de_sum is the device's 2^-20 fixed-point integer
 * total, so the same pair gives the same bits at any place of any batch, from host or device memory; the mean and the score
 * are formed from it in double on the host by vqa_ciede_wait.                                                              */
typedef struct vqa_ciede_metrics {
    double de_sum;    /* sum over the luma grid of min(dE00, 4096), each pixel's value rounded to 2^-20              */
    double de_mean;   /* de_sum / (h w)                                                                               */
    double ciede2000; /* 45 - 20 log10(de_mean), libvmaf's score shape; +infinity when de_mean = 0                    */
} vqa_ciede_metrics;

/* GMSD of one plane pair (vqa_gmsd_submit / vqa_gmsd_wait; the definition and the bounds of the sums are stated there).  The
 * three words are the device's integer totals of u = rint(gms 2^24) and of u^2, so the same pair gives the same words at any
 * place of any batch, from host or device memory; the mean and the deviation are formed from them on the host by
 * vqa_gmsd_wait.                                                                                                            */
typedef struct vqa_gmsd_metrics {
    uint64_t sum_u;     /* sum of u over the N samples of the downsampled grid                                          */
    uint64_t sum_u2_lo; /* sum of u^2 = sum_u2_hi 2^32 + sum_u2_lo: the workgroups' totals, split into their low 32 bits  */
    uint64_t sum_u2_hi; /*   and the rest before they are added                                                         */
    int64_t count;      /* N = ceil(h / 2) ceil(w / 2)                                                                  */
    double gms_mean;    /* sum_u / (N 2^24): the paper's GMSM; exactly 1 for identical planes                           */
    double gmsd;        /* sqrt((N sum u^2 - (sum u)^2) / (N (N - 1))) / 2^24; exactly 0 for identical planes           */
} vqa_gmsd_metrics;

/* CAMBI of one plane (vqa_cambi_submit / vqa_cambi_wait; the definition is stated there).  top, k and masked are integers:
 * the same plane gives the same words at any place of any batch, from host or device memory.  pool and cambi are formed from
 * them on the host by vqa_cambi_wait.                                                                                        */
typedef struct vqa_cambi_metrics {
    uint64_t top[5];    /* top_s: the exact sum of the K_s largest u_s of scale s                                          */
    int64_t k[5];       /* K_s = max(1, 3 N_s / 10)                                                                        */
    int64_t masked[5];  /* the number of samples with m_s = 1                                                              */
    double pool[5];     /* top_s / (K_s 2^16)                                                                              */
    double cambi;       /* ((((16 pool_0 + 8 pool_1) + 4 pool_2) + 2 pool_3) + pool_4) / 31; exactly 0 without banding     */
} vqa_cambi_metrics;

/* XPSNR of one plane pair (vqa_xpsnr_submit / vqa_xpsnr_wait; the definition is stated there).  sse is the device's integer
 * total; wsse and xpsnr are formed on the host by vqa_xpsnr_wait from the per-block integer words, which the wait also hands
 * out on request: the same pair (with its predecessor) gives the same words at any place of any batch, from host or device
 * memory.                                                                                                                   */
typedef struct vqa_xpsnr_metrics {
    uint64_t sse;       /* sum (r - d)^2 over the plane: the plain total, the sum of the blocks' sse_k                     */
    double wsse;        /* avg sum_k sse_k / a_k: the activity-weighted squared error                                      */
    double xpsnr;       /* 10 log10(w h peak^2 / wsse) in dB; +infinity for identical planes                               */
    int32_t block;      /* B, the side of a luma block; this plane's blocks are B or B / 2 wide and high                   */
    int32_t nbx, nby;   /* the block grid, ceil(W / B) x ceil(H / B): the same for every plane of the frame               */
} vqa_xpsnr_metrics;

/* HaarPSI of one plane pair (vqa_haarpsi_submit / vqa_haarpsi_wait; the definition and the bounds of the sums are stated
 * there).  The three words are the device's integer totals, so the same pair gives the same words at any place of any batch,
 * from host or device memory; similarity and haarpsi are formed from them on the host by vqa_haarpsi_wait.                  */
typedef struct vqa_haarpsi_metrics {
    uint64_t den;       /* sum of the weights wI_o over both orientations and every sample of the downsampled grid        */
    uint64_t num_lo;    /* sum of u_o wI_o = num_hi 2^32 + num_lo: the threads' totals, split into their low 32 bits      */
    uint64_t num_hi;    /*   and the rest before they are added                                                           */
    double similarity;  /* num / (den 2^30): the weighted mean of the sigmoid; U1 / 2^30 for identical planes             */
    double haarpsi;     /* (logit(similarity) / alpha')^2; exactly 1 for identical planes                                  */
} vqa_haarpsi_metrics;

/* VCA texture features of one reference plane (vqa_vca_submit / vqa_vca_wait; the definition is stated there).  The three words
 * are the device's integer totals over the plane's 32 x 32 blocks, so the same frame (with its predecessor) gives the same
 * words at any place of any batch, from host or device memory; e, h and l are formed from them on the host by vqa_vca_wait. */
typedef struct vqa_vca_metrics {
    uint64_t e_sum;     /* sum_k qH_k: the blocks' weighted |DCT| sums in steps of 2^-(24 - depth)                         */
    uint64_t h_sum;     /* sum_k |qH_k(i) - qH_k(i - 1)|; 0 for a frame with no predecessor                                */
    uint64_t l_sum;     /* sum_k qL_k, qL_k = rint(sqrt(S_k) 2^24)                                                         */
    int32_t nbx, nby;   /* the block grid, floor(w / 32) x floor(h / 32)                                                   */
    double e;           /* spatial texture energy E on the 8-bit scale                                                     */
    double h;           /* temporal gradient of the energy, on the 8-bit scale; exactly 0 for a static pair                */
    double l;           /* brightness L on the 8-bit scale: 64 for a flat 8-bit plane of 128                               */
} vqa_vca_metrics;

/* No-reference blockiness, blur and noise of one plane (vqa_artifacts_submit / vqa_artifacts_wait; the definition is stated
 * there).  The 21 words are the device's integer sums, so the same plane gives the same words at any place of any batch, from
 * host or device memory; everything below them is formed on the host by vqa_artifacts_wait.                                 */
typedef struct vqa_artifacts_metrics {
    uint64_t edge_h[8]; /* per phase p: sum of |x(i, c) - x(i, c - 1)| over all rows and the boundaries c with c mod 8 == p    */
    uint64_t edge_v[8]; /* the same over rows: |x(r, j) - x(r - 1, j)|, r mod 8 == p                                           */
    uint64_t blur_f_h;  /* sum dF over the horizontal blur domain                                                              */
    uint64_t blur_v_h;  /* sum max(0, 9 dF - dB9) there                                                                        */
    uint64_t blur_f_v;  /* sum dF over the vertical blur domain                                                                */
    uint64_t blur_v_v;  /* sum max(0, 9 dF - dB9) there                                                                        */
    uint64_t lap;       /* sum |L| over the interior                                                                           */
    int32_t phase_h, phase_v;   /* argmax_p r_h[p], argmax_p r_v[p]; the lowest p on a tie                                     */
    double blockiness;      /* (r_h[0] + r_v[0]) / 2: the 8 x 8 grid anchored at the plane's origin, in [-1, 1]                */
    double blockiness_max;  /* (r_h[phase_h] + r_v[phase_v]) / 2: the grid of a cropped or shifted picture                     */
    double blur_h, blur_v;  /* (9 blur_f - blur_v) / (9 blur_f) per direction; exactly 0 where blur_f == 0                     */
    double blur;            /* max(blur_h, blur_v), in [0, 1]; larger = less sharp                                             */
    double noise;           /* Immerkaer's sigma on the 8-bit scale                                                            */
} vqa_artifacts_metrics;

/* BRISQUE's natural-scene statistics of one plane (vqa_brisque_submit / vqa_brisque_wait; the definition is stated there).  The
 * 60 words are the device's integer sums, so the same plane gives the same words at any place of any batch, from host or device
 * memory; flags and features are formed from them on the host by vqa_brisque_wait.  First index: the scale (0: the plane, 1: its
 * half); second index: the orientation H, V, D1, D2.                                                                        */
typedef struct vqa_brisque_metrics {
    uint64_t sum_abs_u[2];      /* sum |u| over the scale's samples, u = rint(m 2^16)                                          */
    uint64_t sum_u2[2];         /* sum u^2                                                                                     */
    uint64_t n_neg[2][4];       /* pairs whose exact product u_a u_b is negative                                               */
    uint64_t n_pos[2][4];       /* pairs whose exact product is positive (a zero product is in neither)                        */
    uint64_t sum_abs_p[2][4];   /* sum |p| over all pairs, |p| = (|u_a u_b| + 2^15) >> 16: the product's magnitude in 2^-16    */
    uint64_t sq_neg_lo[2][4];   /* sum of (|p|^2 mod 2^32) over the negative pairs                                             */
    uint64_t sq_neg_hi[2][4];   /* sum of (|p|^2 >> 32) over them: sum p^2 = sq_neg_hi 2^32 + sq_neg_lo, in 2^-32              */
    uint64_t sq_pos_lo[2][4];   /* the same over the positive pairs                                                            */
    uint64_t sq_pos_hi[2][4];
    uint32_t flags;             /* bit 5 s + k: at scale s the fit k (0: GGD, 1..4: the AGGD of H, V, D1, D2) met a zero
                                   denominator; its features are 0                                                            */
    uint32_t reserved;          /* 0                                                                                           */
    double features[36];        /* per scale 18: GGD alpha, sigma2; then per orientation alpha, mean, l^2, r^2                 */
} vqa_brisque_metrics;

/* MDSI of one frame pair, the planes of a pixel taken together (vqa_mdsi_submit / vqa_mdsi_wait; the definition and the bounds
 * of the words are stated there).  The four words are the device's integer totals, so the same pair gives the same words at any
 * place of any batch, from host or device memory; dev and mdsi are formed from them on the host by vqa_mdsi_wait.            */
typedef struct vqa_mdsi_metrics {
    uint64_t sum_pos; /* A: sum of zq = rint(|g 2^-24|^(1/4) 2^28) over the samples with g >= 0, g = rint(GCS 2^24)          */
    uint64_t sum_neg; /* B: likewise over the samples with g < 0                                                            */
    uint64_t n_neg;   /* the samples with g < 0                                                                             */
    uint64_t sum_dev; /* D: sum of rint(|z - mean z| 2^28), z the complex quarter root in 2^-28 units                        */
    int64_t count;    /* N = ceil(h / f) ceil(w / f)                                                                        */
    int32_t factor;   /* f = max(1, floor(min(h, w) / 256 + 0.5))                                                           */
    int32_t reserved; /* 0                                                                                                  */
    double dev;       /* D / (N 2^28): the mean absolute deviation; exactly 0 for identical frames                          */
    double mdsi;      /* dev^(1/4) as sqrt(sqrt(dev)); exactly 0 for identical frames                                       */
} vqa_mdsi_metrics;

/* dE_ITP (ITU-R BT.2124) of one frame pair, the three planes of a pixel taken together (vqa_itp_submit / vqa_itp_wait; the
 * definition and the bounds of the words are stated there).  The two words are the device's integer totals, so the same pair
 * gives the same words at any place of any batch, from host or device memory; the doubles are formed from them on the host by
 * vqa_itp_wait.                                                                                                             */
typedef struct vqa_itp_metrics {
    uint64_t sum_q;   /* the sum over the luma grid of q = rint(dE_ITP 2^20), a pixel's difference in 2^-20 units               */
    uint64_t max_q;   /* the largest q of the frame                                                                         */
    double de_sum;    /* sum_q 2^-20                                                                                        */
    double de_mean;   /* de_sum / (h w): the mean dE_ITP; exactly 0 for identical frames                                    */
    double de_max;    /* max_q 2^-20: the largest dE_ITP of a pixel                                                         */
} vqa_itp_metrics;

/* PU21-PSNR and PU21-SSIM of one frame pair, the three planes of a pixel taken together (vqa_pu21_submit / vqa_pu21_wait; the
 * definition and the bounds of the words are stated there).  The five words are the device's integer totals, so the same pair
 * gives the same words at any place of any batch, from host or device memory; windows and the doubles are formed on the host by
 * vqa_pu21_wait.                                                                                                            */
typedef struct vqa_pu21_metrics {
    uint64_t sse_y_lo;    /* the sum over the luma grid of the LOW 32 bits of (q_Y,ref - q_Y,dist)^2                            */
    uint64_t sse_y_hi;    /* the sum of the same terms >> 32: sse_y = (sse_y_hi << 32) + sse_y_lo, in 128-bit integers          */
    uint64_t sse_rgb_lo;  /* likewise over the three channels q_R, q_G, q_B                                                    */
    uint64_t sse_rgb_hi;
    int64_t ssim_q;       /* the signed sum over the valid windows of u = rint(ssim 2^24)                                      */
    int64_t windows;      /* (h - 10)(w - 10)                                                                                  */
    double mse_y;         /* sse_y / (2^32 h w): the mean squared error in PU units                                            */
    double mse_rgb;       /* sse_rgb / (2^32 3 h w)                                                                            */
    double pu_psnr;       /* 10 log10(256^2 / mse_y); inf for a zero sum                                                       */
    double pu_psnr_rgb;   /* 10 log10(256^2 / mse_rgb); inf for a zero sum                                                     */
    double pu_ssim;       /* ssim_q / (2^24 windows); exactly 1 for identical frames                                           */
} vqa_pu21_metrics;

/* FSIM and FSIMc of one frame pair, the planes of a pixel taken together (vqa_fsim_submit / vqa_fsim_wait; the definition and the
 * bounds of the words are stated there).  The three words are the device's integer totals, so the same pair gives the same
 * words at any place of any batch, from host or device memory; the doubles are formed from them on the host by vqa_fsim_wait. */
typedef struct vqa_fsim_metrics {
    uint64_t sum_pc;    /* P: the sum over the N samples of pm = max(p_r, p_d), p = rint(PC 2^24)                              */
    uint64_t sum_sim;   /* A: the sum of (g pm + 2^23) >> 24, g = rint(S_L 2^24)                                               */
    uint64_t sum_simc;  /* B: the sum of (gc pm + 2^23) >> 24, gc = rint(S_L C 2^24); gc may be negative: the word is the SIGNED
                           64-bit sum in two's complement                                                                    */
    int64_t count;      /* N = hd wd: the samples of the downsampled grid                                                      */
    int32_t factor;     /* f                                                                                                   */
    uint32_t flags;     /* bit 0: P == 0 - neither image has any phase congruency (flat against flat included); both scores
                           are then 1.0 by definition                                                                        */
    double fsim;        /* A / P; exactly 1 for identical frames                                                               */
    double fsimc;       /* (signed) B / P; exactly 1 for identical frames; equals fsim under VQA_FSIM_GRAY                     */
} vqa_fsim_metrics;

/* Signal statistics of one plane of one frame of ONE stream (vqa_sigstats_submit / vqa_sigstats_wait; the definition and the bounds
 * of the words are stated there).  Every word but the last three doubles and bits_used is an integer the device formed, so the
 * same frame (with its predecessor) gives the same record bytes at any place of any batch, from host or device memory;
 * vqa_sigstats_wait forms bits_used, mean, stdev and dif from them on the host. */
typedef struct vqa_sigstats_metrics {
    int64_t count;         /* N = h w                                                                                          */
    uint64_t sum;          /* sum x                                                                                            */
    uint64_t sum_sq;       /* sum x^2                                                                                          */
    uint32_t min, max;     /* the smallest and the largest sample                                                              */
    uint32_t low, median, high; /* the smallest v with C(v) >= (N + 9) / 10, (N + 1) / 2, (9 N + 9) / 10                      */
    uint32_t or_mask;      /* the bitwise OR of all samples                                                                    */
    uint32_t and_mask;     /* the bitwise AND of all samples                                                                   */
    int32_t bits_used;     /* depth - ctz(or_mask); 0 for an all-zero plane                                                    */
    uint64_t below_black;  /* #{x < black_level}                                                                               */
    uint64_t under;        /* #{x < 16 s}                                                                                      */
    uint64_t over_luma;    /* #{x > 235 s}                                                                                     */
    uint64_t over_chroma;  /* #{x > 240 s}                                                                                     */
    uint64_t above_peak;   /* #{x > 2^depth - 1}; always 0 for uint8 samples                                                   */
    uint64_t sad;          /* sum |x - x'|; 0 for a frame with no predecessor                                                  */
    uint64_t changed;      /* #{x != x'}; 0 for a frame with no predecessor                                                    */
    int32_t top, bottom;   /* the first and the last row that is not dark; h, -1 for an all-dark plane                         */
    int32_t left, right;   /* the first and the last column that is not dark; w, -1 for an all-dark plane                      */
    double mean;           /* sum / N, in sample units                                                                         */
    double stdev;          /* sqrt(max(sum_sq / N - mean^2, 0))                                                                */
    double dif;            /* sad / N                                                                                          */
} vqa_sigstats_metrics;

/* HDR light levels and gamut QC of one frame of ONE stream, the three planes of a pixel taken together (vqa_light_submit /
 * vqa_light_wait; the definition and the bounds of the words are stated there).  Every word up to pct_bin is an integer the
 * device formed, so the same frame gives the same words at any place of any batch, from host or device memory; vqa_light_wait
 * forms the doubles from them and the call's table T on the host: x nits = T[code] 2^-20. */
#define VQA_LIGHT_PERCENTILES 10
#define VQA_LIGHT_BINS 4096
typedef struct vqa_light_metrics {
    int64_t count;             /* N = h w                                                                                       */
    uint32_t max_code[3];      /* the largest code of R, G, B: the codes behind maxSCL                                          */
    uint32_t max_code_rgb;     /* the largest m = max(cR, cG, cB)                                                               */
    uint32_t min_code_rgb;     /* the smallest m                                                                                */
    uint32_t reserved;         /* 0                                                                                             */
    uint64_t sum_q;            /* sum T[m], in 2^-20 cd/m2                                                                      */
    uint64_t sum_y;            /* sum y, the BT.2020 luminance, in 2^-20 cd/m2                                                  */
    uint64_t max_y;            /* the largest y                                                                                 */
    uint64_t out_709;          /* pixels outside BT.709                                                                         */
    uint64_t out_p3;           /* pixels outside P3-D65                                                                         */
    uint64_t clamped;          /* pixels with R', G' or B' below 0 or above 1 before the clamp                                  */
    uint32_t pct_bin[VQA_LIGHT_PERCENTILES];  /* of the histogram of m >> 4: the smallest bin b with C(b) >= (p N + 9999) / 10000,
                                                 p = 100, 500, 1000, 2500, 5000, 7500, 9000, 9500, 9900, 9998 per ten thousand */
    double max_nits;           /* T[max_code_rgb] 2^-20: the frame's term of MaxCLL                                             */
    double min_nits;           /* T[min_code_rgb] 2^-20                                                                         */
    double avg_nits;           /* sum_q 2^-20 / N: the frame average light level, the frame's term of MaxFALL                   */
    double y_avg;              /* sum_y 2^-20 / N                                                                               */
    double y_max;              /* max_y 2^-20                                                                                   */
    double maxscl[3];          /* T[max_code[k]] 2^-20, k = R, G, B                                                             */
    double pct_nits[VQA_LIGHT_PERCENTILES];   /* T[pct_bin << 4] 2^-20: THE BIN'S LOWER EDGE                                   */
    double share_709;          /* out_709 / N                                                                                   */
    double share_p3;           /* out_p3 / N                                                                                    */
} vqa_light_metrics;

/* Colour registration of one frame pair, the planes of a pixel taken together on the luma grid (vqa_colorfit_submit /
 * vqa_colorfit_wait; the definition, the bounds and the host formulas are stated there).  r_i: the sample of plane i of the
 * reference, d_k: of plane k of the distorted frame; every sum runs over the h w luma positions and every word is an exact
 * integer below 2^60.  With one plane the words of planes 1 and 2 are 0. */
typedef struct vqa_colorfit_metrics {
    uint64_t count;            /* N = h w                                                                                       */
    uint64_t sum_r[3];         /* sum r_i                                                                                       */
    uint64_t sum_d[3];         /* sum d_k                                                                                       */
    uint64_t rr[6];            /* sum r_i r_i' for (i, i') = 00, 01, 02, 11, 12, 22                                             */
    uint64_t rd[9];            /* rd[3 i + k] = sum r_i d_k                                                                     */
    uint64_t dd[3];            /* sum d_k^2                                                                                     */
    uint64_t sse[3];           /* dd[k] - 2 rd[4 k] + rr(k, k), formed by the wait: the exact squared error of plane k on this
                                  grid; for plane 0 exactly vqa_plane_metrics.sse of the same pair                              */
} vqa_colorfit_metrics;

/* Field statistics of one plane of one frame against its predecessor (vqa_fields_submit / vqa_fields_wait; the definition is
 * stated there).  Index f is the row parity y & 1: 0 the top field, 1 the bottom field.  Every word is an exact integer. */
typedef struct vqa_fields_metrics {
    uint64_t comb[2];          /* sum |c[y-1][x] + c[y+1][x] - 2 c[y][x]|, 2 <= y < h - 2                                       */
    uint64_t fwd[2];           /* sum |c[y-1][x] + c[y+1][x] - 2 p[y][x]|, same rows                                            */
    uint64_t bwd[2];           /* sum |p[y-1][x] + p[y+1][x] - 2 c[y][x]|, same rows                                            */
    uint64_t sad[2];           /* sum |c[y][x] - p[y][x]|, all rows of the parity                                               */
    uint64_t changed[2];       /* the samples with c != p, all rows of the parity                                               */
    uint64_t count;            /* (h - 4) w: the positions of comb[0] + comb[1]                                                 */
    uint64_t has_prev;         /* 1: the frame had a predecessor; 0: it had none, and fwd, bwd, sad and changed are 0           */
} vqa_fields_metrics;

/* ---- lifecycle ------------------------------------------------------------ */
VQA_API int vqa_abi_version(void);
VQA_API const char *vqa_strerror(int status);
VQA_API int vqa_device_count(int *count);
VQA_API int vqa_create(int device, vqa_ctx **out);
VQA_API int vqa_destroy(vqa_ctx *ctx);
/* Gives back everything an idle ctx keeps between batches: every grow-only scratch buffer, the result staging and every
 * cached table (device and pinned host memory; the streams, events and options stay).  The next submit re-grows what it
 * needs.  VQA_ERR_STATE while a batch is pending (between a *_submit and its *_wait).                                    */
VQA_API int vqa_trim(vqa_ctx *ctx);
/* text of the last failing HIP call on this ctx ("" if none) */
VQA_API const char *vqa_last_hip_error(const vqa_ctx *ctx);
VQA_API void vqa_default_params(vqa_params *p);
/* 0 = the shipped library; bit 0 = built with the superseded A/B kernels, bit 1 = built with the test seams (lab build) */
VQA_API int vqa_build_flavour(void);

/* ---- per-ctx options (none of them changes a result) ------------------------ */
enum vqa_option {
    VQA_OPT_OVERLAP = 0,    /* 1 (default; initial value from VQA_OVERLAP if set): inside one complexity submit block-SAD,
                               the Canny chain and (VQA_DCT_FULL) the full-frame DCT run on side streams of the ctx next to
                               the 8x8 DCT / ORB / Farneback kernels and join before the results are copied (+3 % on the
                               full suite, +5 % with the reference's own definitions).  0: every kernel on the ctx stream
                               in program order - per-kernel event times (vqa_profile_*) are then free of overlap        */
    VQA_OPT_HYST_STATS = 1  /* 1: fill vqa_frame_metrics.hyst_steps (default 0)                                        */
};
/* VQA_ERR_STATE while a submit is pending on the ctx */
VQA_API int vqa_set_option(vqa_ctx *ctx, int option, int value);
VQA_API int vqa_get_option(const vqa_ctx *ctx, int option, int *value);

/* ---- memory --------------------------------------------------------------- */
VQA_API int vqa_alloc_pinned(vqa_ctx *ctx, size_t bytes, void **out);
VQA_API int vqa_free_pinned(vqa_ctx *ctx, void *p);
/* *out = 1 if the WHOLE range [p, p + bytes) is page-locked host memory HIP knows (vqa_alloc_pinned, hipHostMalloc,
 * hipHostRegister, a torch tensor with pin_memory=True; first and last byte are probed): a *_submit / vqa_copy_h2d from it is
 * a true asynchronous DMA.  0 for ordinary (pageable) host memory - the host side then stages through pinned buffers of
 * its own - for a range that leaves a registered region, and for device memory.                                          */
VQA_API int vqa_host_is_pinned(vqa_ctx *ctx, const void *p, size_t bytes, int *out);
VQA_API int vqa_alloc_device(vqa_ctx *ctx, size_t bytes, void **out);
VQA_API int vqa_free_device(vqa_ctx *ctx, void *p);
/* async on the ctx stream; host side should be pinned for true overlap */
VQA_API int vqa_copy_h2d(vqa_ctx *ctx, void *dst_device, const void *src_host, size_t bytes);
VQA_API int vqa_copy_d2h(vqa_ctx *ctx, void *dst_host, const void *src_device, size_t bytes);
VQA_API int vqa_sync(vqa_ctx *ctx);
/* Device-side ordering between two contexts of ONE device, no host wait: everything enqueued on `waiter`'s stream after this
 * call starts only after everything enqueued on `signaler`'s stream BEFORE this call has completed (hipEventRecord +
 * hipStreamWaitEvent).  What it is for: a host that feeds frames over PCIe keeps ONE context as its copy lane - all
 * vqa_copy_h2d calls go there, so uploads cross PCIe one after another, in chunk order - and lets the context that will
 * measure a chunk wait for it:  vqa_copy_h2d(copy_ctx, ...); vqa_stream_wait(work_ctx, copy_ctx); vqa_*_submit(work_ctx, ...).
 * The upload of chunk k+1 then runs under the kernels of chunk k (uploads enqueued on the work contexts' own streams all
 * start at once, share the link and finish together: the kernels wait for all of them - profiles/round6_api_trace_*.json).
 * Both contexts are the calling thread's.  VQA_ERR_INVALID for the same ctx twice or contexts of different devices.     */
VQA_API int vqa_stream_wait(vqa_ctx *waiter, vqa_ctx *signaler);
/* the ctx's hipStream_t, as an opaque pointer (for event timing by the caller) */
VQA_API void *vqa_stream(vqa_ctx *ctx);

/* ---- complexity kernels (replaces process_in_batches over process_*_frame) - */
/* frames: n packed BGR24 frames (what cv2.VideoCapture.read yields,
 * complexity_metrics.py:100), frame i at frames + i*frame_stride, rows of
 * 3*w bytes at row_stride (>= 3*w: padded rows, or a region of interest
 * inside larger frames; only the 3*w bytes of each row are ever read).
 * prev0: the frame preceding frames[0] (same geometry, row_stride and
 * mem_kind) or NULL; frame i's "previous" is frame i-1.
 * Asynchronous: returns once the work is enqueued.  Limits: h*w <= 2^28 pixels
 * (VQA_ERR_UNSUPPORTED beyond); n is bounded by memory only (batches above 32768
 * frames are enqueued as consecutive slices internally).
 * Failure: a submit that returns non-zero has left NOTHING in flight - whatever it had
 * already enqueued has completed on every stream of the ctx before the call returns,
 * no batch is pending, the caller's buffers are free again and the ctx stays usable
 * (the reference's convention: log, re-raise, nothing left running,
 * video_processing.py:295-297).  The same holds for vqa_quality_submit.          */
VQA_API int vqa_complexity_submit(vqa_ctx *ctx, const uint8_t *frames, const uint8_t *prev0, int mem_kind,
                          int n, int h, int w, int64_t frame_stride, int64_t row_stride,
                          uint32_t metric_mask, const vqa_params *params);
/* blocks until the submitted batch is done, then fills out[0..n) */
VQA_API int vqa_complexity_wait(vqa_ctx *ctx, vqa_frame_metrics *out, int n);

/* ---- quality kernels (replaces run_ffmpeg_metrics' psnr + ssim filters) ---- */
/* ref/dist: n frames each; every frame holds n_planes planes described by
 * planes[].  out of vqa_quality_wait: n*n_planes entries, frame-major.        */
VQA_API int vqa_quality_submit(vqa_ctx *ctx, const uint8_t *ref, const uint8_t *dist, int mem_kind, int n,
                       int64_t ref_frame_stride, int64_t dist_frame_stride,
                       const vqa_plane_desc *planes, int n_planes, int ssim_mode);
VQA_API int vqa_quality_wait(vqa_ctx *ctx, vqa_plane_metrics *out, int n_entries);
/* vqa_quality_wait that also fills scales[0..n_entries) with the per-scale means of a VQA_SSIM_MS submit (out[i].ssim is the
 * product formed from scales[i]).  scales may be NULL: then it is vqa_quality_wait.  VQA_ERR_STATE, the batch still pending,
 * when scales is given and the pending submit was not a VQA_SSIM_MS one.  (vqa_quality_wait serves an MS submit as well.) */
VQA_API int vqa_quality_wait_ms(vqa_ctx *ctx, vqa_plane_metrics *out, vqa_ms_scales *scales, int n_entries);

/* ---- VIF on four scales (the model-free part of the reference's libvmaf step, video_processing.py:270-297) ----
 * For one plane pair (ref R, dist D, `depth` bits, h x w), in fp32 on the device:
 *   samples   x = R / 2^(depth-8) - 128, y = D / 2^(depth-8) - 128 (exact at every depth; samples above 2^depth - 1 are read
 *             as they are).
 *   filter    of scale s = 0..3: n_s = 2^(4-s) + 1 taps (17, 9, 5, 3), t[k] = exp(-(k - n_s/2)^2 / (2 (n_s/5)^2)), n_s/2 the
 *             integer half width, normalised to sum 1; separable, columns (vertical) first, then rows.
 *   borders   an index i < 0 reads -i; an index i >= n reads 2n - i - 1.  Every level keeps its full size.
 *   levels    level 0 is (x, y); level s > 0 is level s-1 filtered with the filter OF SCALE s, kept at even rows and even
 *             columns: dims floor(dim / 2).
 *   per level with its filter F: mu1 = F(x), mu2 = F(y), s1 = max(F(xx) - mu1^2, 0), s2 = max(F(yy) - mu2^2, 0),
 *             s12 = F(xy) - mu1 mu2; then per sample, in this order, eps = 1e-10, nsq = 2, smi = 4 / 255^2:
 *               g = s12 / (s1 + eps); sv = s2 - g s12;
 *               if s1 < eps: g = 0, sv = s2, s1 = 0;  if s2 < eps: g = 0, sv = 0;  if g < 0: sv = s2, g = 0;
 *               sv = max(sv, eps); g = min(g, 100);
 *               num = log2(1 + g^2 s1 / (sv + nsq)), den = log2(1 + s1 / nsq);  if s12 < 0: num = 0;
 *               if s1 < nsq: num = 1 - s2 smi, den = 1.
 *   results   num_s = sum num, den_s = sum den, scale_s = num_s / den_s, vif = sum_s num_s / sum_s den_s.
 * This is libvmaf's float `vif` feature at its default options (vif_enhn_gain_limit 100, vif_kernelscale 1) as the project
 * states it; it is pinned against the float64 restatement in tests/vif_reference.py (1e-4 on every scale), not against
 * libvmaf's binary.
 * The contract of vqa_quality_submit: asynchronous, the same plane descriptors, depths (one per submit), alignment rules and
 * failure guarantee.  Every plane must be at least 16 x 16 (level 3 is then 2 x 2 and every reflection stays inside its
 * level): VQA_ERR_UNSUPPORTED below.  VQA_ERR_STATE while a VIF batch is pending.  A VIF batch is a batch of its own: it may
 * be in flight next to a quality and a complexity batch of the same ctx (one upload then serves PSNR / SSIM and VIF), and
 * each wait collects its own kind only - vqa_quality_wait with only a VIF batch pending, and vqa_vif_wait with only a
 * quality batch pending, are VQA_ERR_STATE and leave that batch pending.
 * Scratch on the device: 2.7 bytes per pixel of the largest group of same-geometry planes of a batch (levels 1..3 of both
 * images as fp32: 2 x 4 x (1/4 + 1/16 + 1/64)), kept by the ctx until vqa_trim / vqa_destroy.
 * out of vqa_vif_wait: n * n_planes entries, frame-major.                                                             */
VQA_API int vqa_vif_submit(vqa_ctx *ctx, const uint8_t *ref, const uint8_t *dist, int mem_kind, int n,
                           int64_t ref_frame_stride, int64_t dist_frame_stride,
                           const vqa_plane_desc *planes, int n_planes);
VQA_API int vqa_vif_wait(vqa_ctx *ctx, vqa_vif_metrics *out, int n_entries);

/* ---- ADM on four scales (the other model-free feature family of the reference's libvmaf step) ----
 * For one plane pair (ref R, dist D, `depth` bits, h x w), in fp32 on the device:
 *   samples   x = R / 2^(depth-8) - 128, y = D / 2^(depth-8) - 128 (samples above 2^depth - 1 are read as they are).
 *   DWT       of a level, H x W -> four bands of ceil(H/2) x ceil(W/2), with the db2 taps
 *               lo = ( 0.482962913144690,  0.836516303737469, 0.224143868041857, -0.129409522550921)
 *               hi = (-0.129409522550921, -0.224143868041857, 0.836516303737469, -0.482962913144690):
 *             output index i reads the input indices |2i-1|, 2i, 2i+1, 2i+2, paired with taps 0..3; an index k >= n reads
 *             2n - k - 1.  The vertical pass comes first and gives L = lo, Hh = hi; the horizontal pass then gives a = lo(L),
 *             v = hi(L), h = lo(Hh), d = hi(Hh).  Scale s + 1 is the DWT of the a band of scale s, for each image.
 *   decoupling per sample, (oh, ov, od) from ref and (th, tv, td) from dist: for each band k = clamp(t / (o + 1e-30), 0, 1),
 *             r = k o;  dp = oh th + ov tv;  flag = dp >= 0 && dp^2 >= cos^2(1 degree) (oh^2 + ov^2)(th^2 + tv^2);
 *             if flag && r > 0: r = min(100 r, t);  if flag && r < 0: r = max(100 r, t)  (h, v and d alike);
 *             a_band = t - r.
 *   CSF       rf_s[h] = rf_s[v] = 1 / Q(s, 1), rf_s[d] = 1 / Q(s, 2),
 *             Q(l, th) = 2 * 0.495 * 10^(0.466 log10(2^(l+1) * 0.401 * g[th] / rho)^2) / A[l][th], rho = 3 * 1080 * pi / 180,
 *             g = (1.501, 1, 0.534, 1), A (the 7/9 basis amplitudes), rows l = 0..3, columns th = 0..3:
 *               (0.62171, 0.67234, 0.72709, 0.67234) (0.34537, 0.41317, 0.49428, 0.41317)
 *               (0.18004, 0.22727, 0.28688, 0.22727) (0.091401, 0.11792, 0.15214, 0.11792);
 *             (rf[h], rf[d]) per scale: (0.0173815342, 0.0058906866) (0.0319848145, 0.0142990667) (0.0433726647, 0.0243969129)
 *             (0.0456734100, 0.0313127351).
 *   masking   per sample thr = sum_bands [ |rf a_band| / 15 at the sample + (sum over its 8 neighbours of |rf a_band|) / 30 ];
 *             neighbour index -1 reads 1 and index n reads n - 1 (VIF's border rule); one thr serves the three bands.
 *   region    band dims (bh, bw): left = (int)(bw * 0.1 - 0.5), top = (int)(bh * 0.1 - 0.5); rows [top, bh - top), columns
 *             [left, bw - left); area = their product.
 *   pooling   num_s = sum_bands [ cbrt(sum_region max(|rf r| - thr, 0)^3) + cbrt(area / 32) ],
 *             den_s = sum_bands [ cbrt(sum_region |rf o|^3) + cbrt(area / 32) ].
 *   results   scale_s = num_s / den_s;  adm2 = N / D with N = sum_s num_s, D = sum_s den_s, each set to 0 when below
 *             1e-10 h w / (1920 * 1080); adm2 = 1 when D = 0.  Enhancement counts: a sharpened image may score above 1.
 * This is libvmaf's float `adm` feature at its default options (adm_enhn_gain_limit 100, adm_norm_view_dist 3,
 * adm_ref_display_height 1080, adm_csf_mode 0) as the project states it; it is pinned against the float64 restatement in
 * tests/adm_reference.py (1e-4 on every scale and on adm2), not against libvmaf's binary.  The angle test of the decoupling
 * is a discontinuity: where fp32 rounding decides a sample's flag differently from float64, a small band moves by that
 * sample's whole contribution; the tests widen the bar for such a (case, scale) by the spread the reference reports when
 * the flags within 2^-20 of the boundary are forced either way (never beyond 2e-3; the precedent is Farneback's).
 * The contract of vqa_vif_submit: asynchronous, the same plane descriptors, depths (one per submit), alignment rules and
 * failure guarantee.  Every plane must be at least 16 x 16 (the bands of scale 3 are then 1 x 1): VQA_ERR_UNSUPPORTED below.
 * VQA_ERR_STATE while an ADM batch is pending.  An ADM batch is a batch of its own: it may be in flight next to a quality, a
 * VIF and a complexity batch of the same ctx (one upload then serves all), and each wait collects its own kind only -
 * vqa_adm_wait with only a quality or VIF batch pending, and vqa_quality_wait / vqa_vif_wait with only an ADM batch
 * pending, are VQA_ERR_STATE and leave that batch pending.
 * Scratch on the device: 2.7 bytes per pixel of the largest group of same-geometry planes of a batch (the a bands of scales
 * 0..2 of both images as fp32: 2 x 4 x (1/4 + 1/16 + 1/64)) plus 48 bytes per 32 x 16 band tile, kept by the ctx until
 * vqa_trim / vqa_destroy.  out of vqa_adm_wait: n * n_planes entries, frame-major.                                       */
VQA_API int vqa_adm_submit(vqa_ctx *ctx, const uint8_t *ref, const uint8_t *dist, int mem_kind, int n,
                           int64_t ref_frame_stride, int64_t dist_frame_stride,
                           const vqa_plane_desc *planes, int n_planes);
VQA_API int vqa_adm_wait(vqa_ctx *ctx, vqa_adm_metrics *out, int n_entries);

/* ---- VMAF's motion feature (the temporal feature of the reference's libvmaf step, video_processing.py:270-297) ----
 * For one plane of the REFERENCE stream (`depth` bits, h x w), frame i with its predecessor i - 1, in fp32 on the device; the
 * distorted stream is never looked at:
 *   samples   x = R / 2^(depth-8) - 128, as VIF states it (exact at every depth; samples above 2^depth - 1 are read as they are).
 *   blur      5 taps (0.054488685, 0.244201342, 0.402619947, 0.244201342, 0.054488685), each rounded once to fp32; separable,
 *             columns (vertical) first, then rows; every output sums its taps in ascending order (fused multiply-adds from 0).
 *   borders   VIF's rule: an index i < 0 reads -i; an index i >= n reads 2n - i - 1.
 *   motion[i] = sum |blur(x_i) - blur(x_{i-1})| / (h w); 0 for a frame with no predecessor.  Identical frames give exactly 0.
 *   motion2[i] = min(motion[i], motion[i+1]), motion2[last] = motion[last] (so motion2[0] = 0 whenever motion[0] = 0).  It needs
 *             the next frame, so it is NOT formed here: the host forms it over the whole clip (the Python binding's
 *             tails.motion2).
 * This is libvmaf's float `motion` feature at its default options (no motion_force_zero) as the project states it; where this
 * text and libvmaf differ in a detail, this text is what is built.  It is pinned against the float64 restatement in
 * tests/motion_reference.py, not against libvmaf's binary.
 * Error bound (in-range samples, |x| <= 128, against exact arithmetic on the decimal taps): a rounding of a value below 256 is at
 * most 2^-17.  Per blurred sample: 5 roundings in the vertical pass, carried through the horizontal pass with weight <= 1, 5 more
 * there, and the taps' own rounding to fp32 (2^-24 relative on a sum of at most 128: 2^-17 per pass) - 12 x 2^-17.  The
 * difference of two blurred samples adds one rounding, the fixed-point quantum 2^-17 more: 2 x 12 + 1 + 1 = 26 units of 2^-17,
 * 1.99e-4 per sample and therefore on motion (a mean of the per-sample terms).  The tests use that figure as their bar.
 * The contract of vqa_vif_submit: asynchronous, the same plane descriptors, depths (one per submit), alignment rules and
 * failure guarantee.  prev0: the frame preceding ref[0] (same layout and mem_kind) or NULL, exactly as in
 * vqa_complexity_submit; frame i's predecessor is frame i - 1 of the batch.  Every plane must be at least 16 x 16:
 * VQA_ERR_UNSUPPORTED below.  VQA_ERR_STATE while a motion batch is pending.  A motion batch is a batch of its own: it may be
 * in flight next to a quality, a VIF, an ADM and a complexity batch of the same ctx (one upload then serves all), and each wait
 * collects its own kind only - vqa_motion_wait with only another kind pending, and another kind's wait with only a motion
 * batch pending, are VQA_ERR_STATE and leave that batch pending.
 * One fused kernel: a tile and its apron of 2 samples of both frames go to shared memory, both are blurred there and only the
 * integer total leaves the kernel.  Scratch on the device: 8 bytes per entry; frames handed over in host memory (and prev0)
 * are staged in device buffers of the batch's size.  All of it is kept by the ctx until vqa_trim / vqa_destroy.
 * out of vqa_motion_wait: n * n_planes entries, frame-major.
 * The VMAF score itself is NOT in this ABI: the predictor (an RBF support-vector sum of a few thousand flops per frame over the
 * model file the caller names) runs on the host next to the other float tails - the Python binding's vmaf_model module; parsing
 * a JSON model in C would buy nothing.                                                                                  */
VQA_API int vqa_motion_submit(vqa_ctx *ctx, const uint8_t *ref, const uint8_t *prev0, int mem_kind, int n,
                              int64_t ref_frame_stride, const vqa_plane_desc *planes, int n_planes);
VQA_API int vqa_motion_wait(vqa_ctx *ctx, vqa_motion_metrics *out, int n_entries);

/* ---- ITU-T P.910 spatial and temporal information (SI / TI): the standard description of source content ----
 * For one plane of the REFERENCE stream (`depth` bits, h x w), frame i with its predecessor i - 1, on the raw integer samples R
 * (samples above 2^depth - 1 are read as they are, as elsewhere); the distorted stream is never looked at.  Where this text
 * differs from a tool's detail, this text is what is built.
 *   Sobel     gx = (R[y-1][x+1] + 2 R[y][x+1] + R[y+1][x+1]) - (R[y-1][x-1] + 2 R[y][x-1] + R[y+1][x-1]); gy is its transpose.
 *             Both on the interior only: rows 1 .. h-2, columns 1 .. w-2, n_i = (h-2)(w-2) samples.  There is no border rule:
 *             no sample outside the plane is ever needed.  q = gx^2 + gy^2 is an integer, below 2^21 for uint8 samples and
 *             below 2^37.01 for any uint16 samples.
 *   sums      of the frame, all integers:
 *             grad_sq  = sum q (uint64);
 *             grad_fix = sum rint(sqrt((double) q) 2^32), kept by the device in two uint64 words: every workgroup splits its
 *                        own 64-bit total into the low and the high 32 bits and adds them to lo and hi separately, grad_fix =
 *                        hi 2^32 + lo; neither word can overflow for a plane of 2^28 samples;
 *             diff_sum = sum (R_i - R_{i-1}) (int64) and diff_sq = sum (R_i - R_{i-1})^2 (uint64), both over ALL h w samples,
 *                        both 0 for a frame with no predecessor.
 *   results   in double on the host (vqa_siti_wait), sc = 2^-(depth-8):
 *             grad_sum = (double) hi + (double) lo 2^-32;  m = grad_sum / n_i;
 *             si = sc sqrt(max(grad_sq / n_i - m m, 0));
 *             md = diff_sum / (h w);  ti = sc sqrt(max(diff_sq / (h w) - md md, 0)); ti = 0 for a frame with no predecessor.
 *             Both are population standard deviations on the 8-bit scale, at every depth.
 *   clip      P.910's SI and TI of a clip are the MAXIMA over its frames; the host forms them (the Python binding's entry
 *             points).  The first frame's ti = 0 cannot win a maximum.
 * Limits: every plane at least 16 x 16 (the family's rule), h w <= 2^28 for uint8 samples and h w <= 2^26 at depths above 8 - so
 * that grad_sq stays below 2^64 for arbitrary 16-bit samples: VQA_ERR_UNSUPPORTED beyond either.
 * Why integers: the sums are associative.  A frame (with its predecessor) gives the same record bits at any place of any batch,
 * from host, pinned or device memory, for any tiling - the guarantee every other record of this header gives.
 * Why the quantum is 2^-32 and not motion's 2^-16: si is a difference of two nearly equal numbers on smooth content, and an
 * error e on m moves the variance by 2 m e.  On a plane whose gradient is the same everywhere (R = x + y: q = 128, true SI 0)
 * a 2^-16 quantum would report si near 0.013; with 2^-32 the figure is about 5e-5, and si's error stays below 6e-4 for any
 * 8-bit content (m <= 1020 sqrt 2: sqrt(2 m 2^-33) = 5.8e-4, the case of a true variance of 0).
 * The contract of vqa_motion_submit: asynchronous, prev0 (the frame preceding ref[0], same layout and mem_kind) or NULL, the
 * same plane descriptors, depths (one per submit), alignment rules and failure guarantee: a failed submit leaves nothing in
 * flight.  VQA_ERR_STATE while an SI/TI batch is pending.  An SI/TI batch is a batch of its own: it may be in flight next to a
 * quality, a VIF, an ADM, a motion and a complexity batch of the same ctx (one upload then serves all), and each wait collects
 * its own kind only - vqa_siti_wait with only another kind pending, and another kind's wait with only an SI/TI batch pending,
 * are VQA_ERR_STATE and leave that batch pending.
 * One fused kernel: a tile and its apron of one sample of frame i go to shared memory as raw integers, the predecessor's
 * samples are read straight from global memory, and only the five 64-bit words leave the kernel.  Scratch on the device: 40
 * bytes per entry; frames handed over in host memory (and prev0) are staged in device buffers of the batch's size.  All of it
 * is kept by the ctx until vqa_trim / vqa_destroy.  out of vqa_siti_wait: n * n_planes entries, frame-major.              */
VQA_API int vqa_siti_submit(vqa_ctx *ctx, const uint8_t *ref, const uint8_t *prev0, int mem_kind, int n,
                            int64_t ref_frame_stride, const vqa_plane_desc *planes, int n_planes);
VQA_API int vqa_siti_wait(vqa_ctx *ctx, vqa_siti_metrics *out, int n_entries);

/* ---- PSNR-HVS (Egiazarian et al. 2006) and PSNR-HVS-M (Ponomarenko et al. 2007): the perceptually weighted PSNRs ----
 * The published MATLAB definition (psnrhvsm.m, block step 8) applied per plane.  It is NOT Daala's / libvmaf's `psnr_hvs`
 * feature, which walks overlapping blocks at step 7, uses an integer DCT and has chroma CSF tables of its own.  Where this
 * text and a tool differ in a detail, this text is what is built.
 * For one plane pair (ref R, dist D, `depth` bits, h x w), on the RAW INTEGER SAMPLES (samples above 2^depth - 1 are read as
 * they are, as elsewhere):
 *   blocks    non-overlapping 8x8 blocks with top-left corners at (8 i, 8 j), i < floor(h / 8), j < floor(w / 8).  Rows and
 *             columns beyond the last whole block are not looked at.  n_c = 64 floor(h / 8) floor(w / 8).
 *   DCT       the orthonormal 2-D DCT-II of a block, A = C a C^T, C[k][n] = c_k cos((2 n + 1) k pi / 16), c_0 = sqrt(1 / 8) and
 *             c_k = sqrt(2 / 8) otherwise.
 *   tables    Q, the JPEG Annex K luminance quantisation table, rows
 *               (16 11 10 16 24 40 51 61) (12 12 14 19 26 58 60 55) (14 13 16 24 40 57 69 56) (14 17 22 29 51 87 80 62)
 *               (18 22 37 56 68 109 103 77) (24 35 55 64 81 104 113 92) (49 64 78 87 103 121 120 101) (72 92 95 98 112 100 103 99);
 *             csf[k][l] = 25.735088 / Q[k][l] and msk[k][l] = (10 / Q[k][l])^2, formed in double and rounded once to fp32 -
 *             the published CSFCof / MaskCof to six decimals.  The same tables serve every plane.
 *   masking   of a block z with DCT Z: E = sum over (k,l) != (0,0) of Z[k][l]^2 msk[k][l];
 *             vari(X) = (sum (x - mean)^2) n / (n - 1) (the factor is 64/63 for the block, 16/15 for a quadrant);
 *             pop = (vari of the four 4x4 quadrants, summed) / vari(z) when vari(z) > 0, else 0;
 *             m(z) = sqrt(E pop) / 32; for the pair m = max(m(a), m(b)).
 *   terms     u = |A[k][l] - B[k][l]|.  PSNR-HVS: (u csf)^2.  PSNR-HVS-M: u' = u at (0,0), elsewhere
 *             u' = max(u - m / msk[k][l], 0); the term is (u' csf)^2.
 *   results   S_hvs = sum of the terms / n_c, S_hvsm likewise; psnr_hvs = 10 log10(peak^2 / S_hvs), peak = 2^depth - 1, and
 *             +infinity when S = 0; psnr_hvsm likewise.  Identical planes give exactly S = 0.
 * How the device forms it (fp32 on the vector ALUs unless stated):
 *   variances from EXACT INTEGER SUMS: s1 = sum x and s2 = sum x^2 of a quadrant and of the block are integers (32 bits hold
 *             them at depth 8, 64 bits above); vari = (n s2 - s1^2) / (n - 1), whose numerator is an integer below 2^44, and
 *             pop are formed from them in double, once.  A float mean-and-subtract loses the ratio on near-flat content.
 *   u         as the DCT of the integer difference a - b (the DCT is linear; the difference is exact in fp32 at every depth),
 *             not as the difference of two rounded DCTs.  m / msk as m (Q / 10)^2, the table rounded once like the others.
 *   sums      BATCH-INVARIANT BITS: each block's two sums of 64 terms are rounded to a 2^-20 quantum and added as integers.
 *             The squared DCT differences of a block sum to the squared sample differences (Parseval), at most
 *             64 * 65535^2 < 2^38 for any uint16 input; times csf^2 <= 6.63 a block sum is below 2^41, its fixed-point value
 *             below 2^61.  Every block's value is split into its low and its high 32 bits and the halves are added to two
 *             64-bit words per sum - four words per entry.  A plane of 2^28 samples has 2^22 blocks: the low words stay below
 *             2^54 and the high words below 2^51, so no word can overflow, for any tiling.  The host joins them as
 *             hi 2^32 + lo, times 2^-20, over n_c, in double.  The rounding moves S by at most half a quantum per block over
 *             64 coefficients: |error on S| <= 2^-21 / 64 = 2^-27, under 7.5e-9, whatever the content.
 * Limits: every plane at least 16 x 16 and h w <= 2^28: VQA_ERR_UNSUPPORTED beyond either.
 * The contract of vqa_vif_submit: asynchronous, the same plane descriptors, depths (one per submit), alignment rules, memory
 * kinds and failure guarantee: a failed submit leaves nothing in flight.  VQA_ERR_STATE while a PSNR-HVS batch is pending.  A
 * PSNR-HVS batch is a batch of its own: it may be in flight next to a quality, a VIF, an ADM, a motion, an SI/TI and a
 * complexity batch of the same ctx (one upload then serves all), and each wait collects its own kind only -
 * vqa_psnr_hvs_wait with only another kind pending, and another kind's wait with only a PSNR-HVS batch pending, are
 * VQA_ERR_STATE and leave that batch pending.  The same pair gives the same record bits at any place of any batch, from host,
 * pinned or device memory.
 * One fused kernel: a thread owns a whole block of both images, reads every sample once and keeps all three DCTs in its
 * registers; only the four 64-bit words leave the kernel.  Scratch on the device: 32 bytes per entry; host frames are staged
 * in the buffers a quality, a VIF or an ADM submit uses.  All of it is kept by the ctx until vqa_trim / vqa_destroy.
 * out of vqa_psnr_hvs_wait: n * n_planes entries, frame-major.                                                             */
VQA_API int vqa_psnr_hvs_submit(vqa_ctx *ctx, const uint8_t *ref, const uint8_t *dist, int mem_kind, int n,
                                int64_t ref_frame_stride, int64_t dist_frame_stride, const vqa_plane_desc *planes, int n_planes);
VQA_API int vqa_psnr_hvs_wait(vqa_ctx *ctx, vqa_psnr_hvs_metrics *out, int n_entries);

/* ---- CIEDE2000 (CIE 142-2001; Sharma, Wu and Dalal 2005): the colour difference dE00, three planes jointly ----
 * Every other metric here looks at one plane at a time; this one turns the three samples of a pixel of either image into
 * CIELAB and takes the CIEDE2000 difference of the two colours.  Where this text and a tool differ in a detail, this text is
 * what is built.
 * A frame is THREE planes of one depth (8 bits, or 9..16 bits as uint16), the RAW INTEGER SAMPLES read as they are.
 * Colour model (`model`):
 *   VQA_CIEDE_YUV709   planes Y, U, V.  U and V share one geometry (width, height, row stride, pixel step): the luma's, or the
 *             ceil-halved one, in each direction independently ((w + 1) / 2, (h + 1) / 2: 4:4:4, 4:2:2, 4:2:0, odd sizes
 *             included).  With sh = 1 when the chroma width is halved (else 0) and sv likewise for the height, the chroma
 *             sample of luma (i, j) is (i >> sv, j >> sh): replication, no interpolation.  With s = 2^(depth - 8):
 *               y = (Y - 16 s) / (219 s), u = (U - 128 s) / (224 s), v = (V - 128 s) / (224 s)
 *               R' = y + 1.5748 v, G' = y - 0.1873 u - 0.4681 v, B' = y + 1.8556 u            (BT.709, limited range)
 *   VQA_CIEDE_BGR      planes B, G, R of a common geometry (any pixel step: packed bgr24 has step 3);
 *               R' = R / (2^depth - 1), G' and B' likewise.
 *   NO CLAMPING ANYWHERE: every piecewise function below is defined on all reals and takes its linear branch for negative
 *   arguments, so out-of-gamut triples give finite, smooth values.
 * R'G'B' -> linear, per channel:  c > 0.04045 ? ((c + 0.055) / 1.055)^2.4 : c / 12.92
 * linear -> XYZ:   X = 0.4124 R + 0.3576 G + 0.1805 B, Y = 0.2126 R + 0.7152 G + 0.0722 B, Z = 0.0193 R + 0.1192 G + 0.9505 B
 *             (IEC 61966-2-1), each divided by the white point taken as the matrix's ROW SUMS, (0.9505, 1.0000, 1.0890): a gray
 *             pixel has a = b = 0 up to rounding.
 * XYZ -> Lab:      f(t) = t > 0.008856 ? cbrt(t) : 7.787 t + 16 / 116;
 *             L = 116 f(Y) - 16, a = 500 (f(X) - f(Y)), b = 200 (f(Y) - f(Z)).
 * dE00 of (L1, a1, b1), (L2, a2, b2) with the parametric weights (kL, kC, kH); angles in degrees:
 *   C_i = sqrt(a_i^2 + b_i^2), Cm = (C1 + C2) / 2, G = 0.5 (1 - sqrt(Cm^7 / (Cm^7 + 25^7)))
 *   a'_i = (1 + G) a_i, C'_i = sqrt(a'_i^2 + b_i^2), h'_i = atan2(b_i, a'_i) brought into [0, 360), and 0 when a'_i = b_i = 0
 *   dL' = L2 - L1, dC' = C'2 - C'1
 *   dh' = 0 when C'1 C'2 = 0; else h'2 - h'1, less 360 when that is above 180, plus 360 when it is below -180   (eq. 10)
 *   dH' = 2 sqrt(C'1 C'2) sin(dh' / 2)
 *   Lm = (L1 + L2) / 2, C'm = (C'1 + C'2) / 2
 *   hm = h'1 + h'2 when C'1 C'2 = 0; else (h'1 + h'2) / 2 when |h'1 - h'2| <= 180; else (h'1 + h'2 + 360) / 2 when
 *        h'1 + h'2 < 360, and (h'1 + h'2 - 360) / 2 otherwise                                                    (eq. 14)
 *   T = 1 - 0.17 cos(hm - 30) + 0.24 cos(2 hm) + 0.32 cos(3 hm + 6) - 0.20 cos(4 hm - 63)
 *   dtheta = 30 exp(-((hm - 275) / 25)^2), R_C = 2 sqrt(C'm^7 / (C'm^7 + 25^7))
 *   S_L = 1 + 0.015 (Lm - 50)^2 / sqrt(20 + (Lm - 50)^2), S_C = 1 + 0.045 C'm, S_H = 1 + 0.015 C'm T
 *   R_T = -sin(2 dtheta) R_C
 *   dE00 = sqrt(tL^2 + tC^2 + tH^2 + R_T tC tH), tL = dL' / (kL S_L), tC = dC' / (kC S_C), tH = dH' / (kH S_H)
 *   A pair of triples with equal integer samples gives EXACTLY 0 (the kernel tests for it).
 * weights: kL, kC, kH as doubles, NULL = (1, 1, 1), the CIE standard.  Non-finite or non-positive: VQA_ERR_INVALID.
 * Results, ONE ENTRY PER FRAME (not per plane): de_mean = the mean of dE00 over the luma grid;
 *   ciede2000 = 45 - 20 log10(de_mean), libvmaf's score shape, +infinity when de_mean = 0.
 * How the device forms it:
 *   arithmetic per pixel is fp32; the powers of 7 are multiplications (as (25 / C)^7, which cannot overflow); the radicand
 *   of dE00 is raised to 0 when rounding left it below.
 *   sums      BATCH-INVARIANT BITS: each pixel's dE00 is rounded to a 2^-20 quantum and added as a 64-bit integer: one word
 *             per frame, whatever the tiling and the order in which workgroups retire.  In-range colours give dE00 < 2^8.
 *             For UNCLAMPED input (raw uint16 samples far above 2^depth - 1) two of the three terms stay bounded at weights
 *             (1, 1, 1): |dC'| <= 2 C'm gives |tC| < 2 / 0.045 < 45; |dH'| <= 2 sqrt(C'1 C'2) <= 2 C'm and
 *             T >= 1 - 0.17 - 0.24 - 0.32 - 0.20 = 0.07 give |tH| < 2 / (0.015 * 0.07) < 1905; |R_T| <= 2.  tL is NOT bounded:
 *             S_L = 1 at Lm = 50 whatever dL' is, and L is as wide as the input - a sample of 65535 read at depth 9 gives
 *             y near 150, R' near 380, a linear value near 1.4e6 and L near 1.3e4, and the linear branches reach L near -5e3
 *             - so dE00 can exceed 2^14, and weights below 1 divide all three terms further.
 *             THE PER-PIXEL VALUE IS THEREFORE SATURATED AT 2^12: min(dE00, 4096); a NaN, which no finite input has
 *             produced, would count as 4096 too.  In-range input never comes near it.  A pixel's fixed-point value is then at
 *             most 2^32 and a frame of 2^28 pixels gives a word of at most 2^60: it cannot overflow.  The rounding moves
 *             de_mean by at most half a quantum: 2^-21.
 *   host      the word -> double, times 2^-20 (de_sum), over h w (de_mean), and the logarithm: in vqa_ciede_wait, in double,
 *             with contraction off.
 * Limits: luma at least 16 x 16 and h w <= 2^28: VQA_ERR_UNSUPPORTED beyond either.  n_planes other than 3, U and V (or
 * B, G, R) geometries that differ, a chroma size that is neither the luma's nor its ceil-half, mixed depths, an unknown
 * model: VQA_ERR_INVALID.
 * The contract of vqa_psnr_hvs_submit: asynchronous, the same plane descriptors, depths (one per submit), alignment rules,
 * memory kinds and failure guarantee: a failed submit leaves nothing in flight.  VQA_ERR_STATE while a CIEDE2000 batch is
 * pending.  A CIEDE2000 batch is a batch of its own: it may be in flight next to a batch of every other kind of the same ctx
 * (one upload then serves all), and each wait collects its own kind only - vqa_ciede_wait with only another kind pending,
 * and another kind's wait with only a CIEDE2000 batch pending, are VQA_ERR_STATE and leave that batch pending.
 * One fused kernel per submit: a thread owns a 2 x 4 luma patch of both images (a 4:2:0 chroma sample is loaded once for four
 * luma samples), forms both Lab triples and dE00 in registers; only the one word per frame leaves the kernel.  Scratch on the
 * device: 8 bytes per frame; host frames are staged in the buffers a quality, a VIF, an ADM or a PSNR-HVS submit uses.  All
 * of it is kept by the ctx until vqa_trim / vqa_destroy.
 * out of vqa_ciede_wait: n entries (n_entries = n).                                                                      */
enum vqa_ciede_model { VQA_CIEDE_YUV709 = 0, VQA_CIEDE_BGR = 1 };
VQA_API int vqa_ciede_submit(vqa_ctx *ctx, const uint8_t *ref, const uint8_t *dist, int mem_kind, int n,
                             int64_t ref_frame_stride, int64_t dist_frame_stride, const vqa_plane_desc *planes, int n_planes,
                             int model, const double *weights);
VQA_API int vqa_ciede_wait(vqa_ctx *ctx, vqa_ciede_metrics *out, int n_entries);

/* ---- GMSD: gradient magnitude similarity deviation (Xue, Zhang, Mou, Bovik, IEEE TIP 2014) ----
 * The authors' published GMSD.m applied per plane, as read here; where this text and a tool differ in a detail, this text is
 * what is built.  For one plane pair (ref r, dist d, `depth` bits, h x w) on the RAW INTEGER SAMPLES, peak = 2^depth - 1:
 *   2x2 mean  D(i, j) = (x(2i, 2j) + x(2i+1, 2j) + x(2i, 2j+1) + x(2i+1, 2j+1)) / 4 for i < hd = ceil(h / 2) and
 *             j < wd = ceil(w / 2).  A sample outside the plane counts as 0: MATLAB's conv2(.., 'same') with a 2x2 box reads
 *             rows and columns i .. i+1, and (1:2:end, 1:2:end) keeps every other one.  The last row or column of an odd-sized
 *             plane is therefore a half-weight mean, not a dropped row.  S = 4 D is an exact integer.
 *   Prewitt   gx(i, j) = (D(i-1, j+1) + D(i, j+1) + D(i+1, j+1) - D(i-1, j-1) - D(i, j-1) - D(i+1, j-1)) / 3, gy its
 *             transpose, at EVERY sample of D with D = 0 outside (conv2 'same' again: a zero fill, not a clamp, so a flat
 *             non-zero field has gradient on its border ring).  q = (12 gx)^2 + (12 gy)^2 is an exact integer, sums and
 *             differences of S: |12 gx| <= 12 peak, so q <= 288 peak^2, below 2^25 for 8-bit and below 2^41 for 16-bit samples.
 *             m^2 = q / 144.
 *   gms       (2 m_r m_d + T) / (m_r^2 + m_d^2 + T) with T = 170 (peak / 255)^2 - the paper's c = 170 on the 8-bit scale, so a
 *             clip scores the same at any depth after exact upscaling.  0 < gms <= 1, and gms = 1 where q_r = q_d.
 *   pooling   gmsd = the standard deviation of gms over the N = hd wd samples with divisor N - 1 (MATLAB's std2);
 *             gms_mean = their mean (the paper's GMSM).
 * How the device forms it: S of both images as integers; q_r, q_d as integers (32 bits at depth 8, 64 above); then in double
 *             gms = (2 sqrt(q_r q_d) + c) / ((q_r + q_d) + c), c = 144 T = 144 (170 ((peak / 255) (peak / 255))), every step
 *             rounded to double once.  sqrt(x x) = x in IEEE arithmetic, so q_r = q_d gives gms = 1 EXACTLY.
 *   sums      BATCH-INVARIANT BITS: u = rint(gms 2^24), an integer, u <= 2^24.  Three integer words leave the device per
 *             entry: sum u, and sum u^2 as two words.  A workgroup's 2048 samples give a total of u^2 below 2^59, which is
 *             split into its low and its high 32 bits before it is added.  A plane of 2^28 samples has N <= 2^26: sum u < 2^50,
 *             the low word below 2^58 and the high word below 2^42 - nothing can overflow, for any tiling.
 *   host      sum u^2 = hi 2^32 + lo and N sum u^2 - (sum u)^2 (below 2^100) in 128-bit integer arithmetic; then
 *             gmsd = sqrt(that / (N (N - 1))) / 2^24 and gms_mean = sum u / (N 2^24) in double, contraction off.  Identical
 *             planes give gmsd = 0.0 and gms_mean = 1.0 exactly.  The rounding of u moves either result by less than 2^-24:
 *             the deviation is 1-Lipschitz in the root mean square of the per-sample changes (at most 2^-25) times
 *             sqrt(N / (N - 1)).
 * Limits: every plane at least 16 x 16 and h w <= 2^28: VQA_ERR_UNSUPPORTED beyond either.
 * The contract of vqa_psnr_hvs_submit: asynchronous, the same plane descriptors (one to four planes, each measured by itself;
 * packed layouts through pixel_step), depths (one per submit), alignment rules, memory kinds and failure guarantee: a failed
 * submit leaves nothing in flight.  VQA_ERR_STATE while a GMSD batch is pending.  A GMSD batch is a batch of its own: it may be
 * in flight next to a batch of every other kind of the same ctx (one upload then serves all), and each wait collects its own
 * kind only - vqa_gmsd_wait with only another kind pending, and another kind's wait with only a GMSD batch pending, are
 * VQA_ERR_STATE and leave that batch pending.
 * One fused kernel per group of same-geometry planes: a workgroup forms a 64 x 32 tile of S and its one-sample apron for both
 * images in LDS straight from the input quads; only the three words leave the kernel.  Scratch on the device: 24 bytes per
 * entry; host frames are staged in the buffers a quality, a VIF, an ADM, a PSNR-HVS or a CIEDE2000 submit uses.  All of it is
 * kept by the ctx until vqa_trim / vqa_destroy.
 * out of vqa_gmsd_wait: n * n_planes entries, frame-major.                                                                 */
VQA_API int vqa_gmsd_submit(vqa_ctx *ctx, const uint8_t *ref, const uint8_t *dist, int mem_kind, int n,
                            int64_t ref_frame_stride, int64_t dist_frame_stride, const vqa_plane_desc *planes, int n_planes);
VQA_API int vqa_gmsd_wait(vqa_ctx *ctx, vqa_gmsd_metrics *out, int n_entries);

/* ---- CAMBI: contrast-aware multiscale banding index (Tandon, Afonso, Sole, Krasula, PCS 2021) ----
 * The first metric here that scores ONE stream - the encoded one - without comparing it to another: it measures banding (false
 * contours), smooth gradients quantised into visible steps.  It is the paper's method applied per plane with the details fixed
 * as below; where this text and a tool differ in a detail, this text is what is built.  It is NOT pinned against libvmaf's
 * `cambi` feature, whose differences are left out: the upscale to the encode resolution, the 3 x 3 mode filter before
 * decimation, luminance-dependent visibility thresholds, a resolution-dependent mask threshold, a top-k share of its own and
 * its own score scale, and the full-reference variant.  The constants (window 65, mask 7 x 7 with more than 24 hits, contrasts
 * 1..4, top 30 %, scale weights 16, 8, 4, 2, 1) are the paper's as recalled, unverified.
 * All arithmetic is integer.  For one plane, h x w samples x of `depth` = b bits:
 *   1 to 10 bits  b < 10: t = min(1023, x << (10 - b)) (b = 8: x << 2).  b >= 10: t = min(1023, (x + r) >> (b - 10)) with
 *                 r = 1 << (b - 11) for b > 10 and r = 0 for b = 10.  A sample above 2^b - 1 is read as it is and clamped to
 *                 1023 by the same min, at every depth.
 *   2 anti-dither y0(i, j) = (t(i, j) + t(i, j+1) + t(i+1, j) + t(i+1, j+1) + 2) >> 2, row and column indices clamped to the
 *                 plane.
 *   3 mask        Z(i, j) = 1 when y0(i, j) == y0(i, j+1) and y0(i, j) == y0(i+1, j), otherwise 0; indices clamped, so the
 *                 comparison across the last row or column holds trivially.  S(i, j) = the sum of Z over the 7 x 7 window
 *                 centred on (i, j), with zeros outside the plane.  m0(i, j) = (S(i, j) > 24).  A border sample's window is
 *                 short (a corner sees 16 samples, its neighbours 20 and 24), so the outer ring is seldom in the mask and the
 *                 four corners never are: that is intended.
 *   4 scales      s = 0..4: y_{s+1}(i, j) = y_s(2i, 2j), m_{s+1}(i, j) = m_s(2i, 2j), h_{s+1} = ceil(h_s / 2), likewise w;
 *                 N_s = h_s w_s.
 *   5 contrast    for a sample with m_s(i, j) = 1 take the 65 x 65 window centred on it, clipped to the plane.  A = the number
 *                 of plane samples in the clipped window.  n_d, d = -4..4, = the number of window samples with m_s = 1 and
 *                 y_s = y_s(i, j) + d; n_0 >= 1, the sample counts itself.  For k = 1..4 and both signs the contrast is
 *                 c = k n_0 n_{+-k} / ((n_0 + n_{+-k}) A), in [0, 1], kept as u = (num 2^17 + den) / (2 den) in 64-bit integer
 *                 division with num = k n_0 n_{+-k} and den = (n_0 + n_{+-k}) A: round-to-nearest at a step of 2^-16, no
 *                 floating point anywhere; 0 <= u <= 65536.  u_s(i, j) = the largest of the eight; 0 where m_s = 0.
 *   6 pool        K_s = max(1, (3 N_s) / 10) in integer division; top_s = the exact sum of the K_s largest u_s of the scale,
 *                 unmasked samples counting as zeros; pool_s = top_s / (K_s 2^16).
 *   7 score       cambi = ((((16 pool_0 + 8 pool_1) + 4 pool_2) + 2 pool_3) + pool_4) / 31, in [0, 1]; 0 for a plane with no
 *                 masked sample or no neighbour level.  vqa_cambi_wait forms pool and cambi on the host in double, contraction
 *                 off, from the integer words.
 * Limits: every plane at least 16 x 16 and h w <= 2^28: VQA_ERR_UNSUPPORTED beyond either.  A 16 x 16 plane reaches 1 x 1 at
 * scale 4: that is legal.
 * The contract of vqa_siti_submit without a prev0: asynchronous, ONE stream, the same plane descriptors (one to four planes,
 * each measured by itself; packed layouts through pixel_step), depths (one per submit, 8..16), alignment rules, memory kinds and
 * failure guarantee: a failed submit leaves nothing in flight.  VQA_ERR_STATE while a CAMBI batch is pending.  A CAMBI batch is a
 * batch of its own: it may be in flight next to a batch of every other kind of the same ctx (one upload then serves all), and
 * each wait collects its own kind only - vqa_cambi_wait with only another kind pending, and another kind's wait with only a
 * CAMBI batch pending, are VQA_ERR_STATE and leave that batch pending.
 * Kernels, per group of same-geometry planes: k_cambi_mask (steps 1-3; one 16-bit word v0 = m0 ? y0 : 65535 per sample),
 * k_cambi_decimate (scales 1..4 of v in one launch), then per scale k_cambi_contrast (a 32 x 32 tile and its 32-sample apron
 * in LDS; every lane walks its window; a wave without a masked sample skips it; u > 0 goes into a 65537-bin integer histogram
 * per frame and plane) and k_cambi_topk (top_s from the histogram, walked from the top).  Scratch on the device: per frame and
 * plane about 2.7 bytes per sample for the five scales and 263 KB for the histogram, sized by the largest group; ten 64-bit
 * words per entry; host frames are staged in the buffer of the second stream of a quality submit.  All of it is kept by the
 * ctx until vqa_trim / vqa_destroy.
 * out of vqa_cambi_wait: n * n_planes entries, frame-major.                                                                 */
VQA_API int vqa_cambi_submit(vqa_ctx *ctx, const uint8_t *frames, int mem_kind, int n, int64_t frame_stride,
                             const vqa_plane_desc *planes, int n_planes);
VQA_API int vqa_cambi_wait(vqa_ctx *ctx, vqa_cambi_metrics *out, int n_entries);

/* ---- XPSNR: activity-weighted PSNR with block weights (Helmrich, Siekmann, Becker, Bosse, Marpe, Wiegand, ICASSP 2020;
 *      JVET-H0047) ----
 * Plain PSNR in which the squared error of every block is divided by the spatial and temporal activity of the REFERENCE's luma
 * at that block: error in busy or moving regions counts less, error in flat, static regions more.  It is the paper's method
 * with the details fixed here; where this text and a tool differ in a detail, this text is what is built.  FFmpeg's `xpsnr`
 * filter differs in three things that are left out on purpose: its second-order temporal activity above 32 fps (first order
 * only here), its extra smoothing of the weights for pictures of at most 640 x 480, and its 6 x 6 folded high-pass above HD
 * (plain 2 x 2 sums here).  It is NOT pinned against FFmpeg's binary.
 * Inputs   a planar layout whose plane 0 is the full-resolution luma, W x H at `depth` bits; planes 1.. are of the luma's
 *          size or ceil(W / 2) wide and / or ceil(H / 2) high (4:4:4, 4:2:2, 4:2:0; mono has plane 0 alone).  R, D: the RAW
 *          INTEGER SAMPLES of the reference and the distorted frame; P: the reference frame before it, or none.
 *          peak = 2^depth - 1.
 * Blocks   rho = W H / (3840 * 2160) in double; B = max(4, 4 floor(32 sqrt(rho) + 0.5)): 128 at 2160p, 64 at 1080p, 8 at
 *          135 x 241, 4 at 16 x 16.  Luma blocks tile the plane from (0, 0), nbx = ceil(W / B), nby = ceil(H / B), edge blocks
 *          truncated; block k = by nbx + bx.  A plane subsampled by 2 in a direction uses B / 2 there (B is a multiple of 4), so
 *          every plane has the same nbx x nby grid and block k of every plane is co-located.
 * Grid G   bv = 1 when W H <= 2048 * 1152, else 2; s = bv^2.  bv = 1: G = R (luma).  bv = 2: G[y][x] = R[2y][2x] + R[2y][2x+1] +
 *          R[2y+1][2x] + R[2y+1][2x+1] on floor(H / 2) x floor(W / 2) = Gh x Gw: the last row or column of an odd plane is not
 *          looked at.  Gp: the same grid of P.  Origins are the interior of G only, rows 1 .. Gh - 2 and columns 1 .. Gw - 2:
 *          no sample outside the plane is ever needed.  Block k owns the origins whose sample coordinate (bv x, bv y) lies in
 *          it; n_k is their number (0 is possible: a last block that holds only the ignored column).
 * Words    per (frame, luma block), uint64 sums over the owned origins:
 *            sa_k = sum |f|, f = 12 G[y][x] - 2 (G[y-1][x] + G[y+1][x] + G[y][x-1] + G[y][x+1])
 *                                - (G[y-1][x-1] + G[y-1][x+1] + G[y+1][x-1] + G[y+1][x+1])
 *            ta_k = sum |G[y][x] - Gp[y][x]|, 0 for a frame with no predecessor
 *          per (frame, plane, block): sse_k = sum (R - D)^2 over every sample of the plane's block.
 *          Bounds: |f| <= 12 s peak <= 48 peak < 2^22; B <= 728 at the size limit, so a block owns fewer than 2^20 origins and
 *          2^20 samples: sa_k + 2 ta_k < 2^43 and sse_k < 2^52 - every word stays below 2^53 and converts to double exactly.
 * Host     in double, contraction off, blocks in ascending k:
 *            a_min = 2^(depth - 6); a_k = (double)(sa_k + 2 ta_k) / (double)(s n_k), raised to a_min where lower, a_min
 *            where n_k = 0;  avg = sqrt(16 * 2^(2 depth - 9) / sqrt(max(1e-5, rho)));
 *            wsse_c = avg * sum_k (double) sse_{c,k} / a_k;  xpsnr_c = 10 log10(((double)(Wc Hc) (peak peak)) / wsse_c), and
 *            +infinity for wsse_c = 0.
 * Limits   VQA_ERR_UNSUPPORTED for a packed layout (pixel step beyond one sample: bgr24), a plane 1.. of any other ratio to
 *          plane 0, a plane below 16 x 16, and W H > 2^28 at 8 bits or > 2^26 above.
 * The contract of vqa_gmsd_submit for both streams - asynchronous, the same plane descriptors, depths (one per submit),
 * alignment rules, memory kinds and failure guarantee - and of vqa_siti_submit for prev0: the reference frame before frame 0,
 * one frame of the reference's layout, resident where the frames are, or NULL: frame 0 then has no predecessor (ta = 0).  A
 * batch of more than 32768 frames goes out in slices; a slice's first frame takes the previous slice's last frame as its
 * predecessor.  VQA_ERR_STATE while an XPSNR batch is pending.  An XPSNR batch is a batch of its own: it may be in flight next
 * to a batch of every other kind of the same ctx, and each wait collects its own kind only - vqa_xpsnr_wait with only another
 * kind pending, and another kind's wait with only an XPSNR batch pending, are VQA_ERR_STATE and leave that batch pending.
 * Kernels: k_xpsnr_act (a 64 x 32 tile of G and its one-sample apron in LDS as integers, the quad sums of bv = 2 formed on the
 * way in, Gp straight from global memory) and, per group of same-geometry planes, k_xpsnr_sse; both find the block of every
 * origin or sample by itself, add into block accumulators in LDS and send one 64-bit integer atomic per touched block and
 * word.  Integer adds only: tiling, retirement order, batch size and position cannot change a word.  Scratch on the device:
 * 8 (2 + n_planes) nbx nby bytes per frame (510 blocks at 1080p and at 2160p), zeroed on the stream before the launches,
 * and as much pinned host memory; host frames are staged in the buffers of a quality submit, prev0 in one of its own.  All of
 * it is kept by the ctx until vqa_trim / vqa_destroy.
 * out of vqa_xpsnr_wait: n * n_planes entries, frame-major.  blocks: NULL, or room for n_block_words =
 * n nbx nby (3 + n_planes) words - per frame nbx nby triples (sa_k, ta_k, n_k), then per plane nbx nby words sse_k: the weight
 * map, for callers who want it.  Any other n_block_words with blocks given is VQA_ERR_INVALID and leaves the batch pending. */
VQA_API int vqa_xpsnr_submit(vqa_ctx *ctx, const uint8_t *ref, const uint8_t *dist, const uint8_t *prev0, int mem_kind, int n,
                             int64_t ref_frame_stride, int64_t dist_frame_stride, const vqa_plane_desc *planes, int n_planes);
VQA_API int vqa_xpsnr_wait(vqa_ctx *ctx, vqa_xpsnr_metrics *out, int n_entries, uint64_t *blocks, int64_t n_block_words);

/* ---- HaarPSI: Haar wavelet-based perceptual similarity index (Reisenhofer, Bosse, Kutyniok, Wiegand, Signal Processing:
 *      Image Communication 61, 2018) ----
 * The authors' HaarPSI.m for grayscale input applied per plane, AS RECALLED: their code was not at hand when this was written
 * and nothing here is pinned against their MATLAB or Python files.  Where this text and a tool differ in a detail, this text
 * is what is built.  For one plane pair (ref r, dist d, `depth` bits, h x w) on the RAW INTEGER SAMPLES, peak = 2^depth - 1,
 * k = peak / 255:
 *   2x2 mean  vqa_gmsd_submit's stage exactly: S(i, j) = the integer sum of the input quad at (2i, 2j), a sample outside the
 *             plane counting 0, for i < hd = ceil(h / 2), j < wd = ceil(w / 2); D = S / 4 (MATLAB's conv2(.., ones(2) / 4,
 *             'same') and (1:2:end, 1:2:end): the last row or column of an odd plane is a half-weight mean).
 *   Haar      at EVERY sample of D, with D = 0 outside (conv2 'same': a zero fill, not a clamp).  For scale s = 1, 2, 3 and
 *             K = 2^s the horizontal-edge coefficient is
 *               H_s^0(i, j) = sum_{b = -K/2+1 .. K/2} (sum_{a = -K/2+1 .. 0} S(i+a, j+b) - sum_{a = 1 .. K/2} S(i+a, j+b))
 *             and H_s^1 is its transpose (a and b exchange their roles).  The window i - K/2 + 1 .. i + K/2 is MATLAB's
 *             centring of an even kernel.  The paper's coefficient is H / 2^(s+2); only |H| is used, so the sign is free.
 *             |H_1| <= 8 peak, |H_2| <= 32 peak, |H_3| <= 128 peak < 2^23 at 16 bits: 32-bit integers throughout.
 *   local     for orientation o and s = 1, 2:  sim_s = (2 |H_r H_d| + c_s) / ((H_r^2 + H_d^2) + c_s) with
 *             c_s = 4^(s+2) (30 (k k)) - the paper's C = 30 on the 8-bit scale, so a clip scores the same at any depth after
 *             exact upscaling.  In double, every step rounded once, contraction off; the integer products (below 2^45) and
 *             H_r^2 + H_d^2 are exact, so |H_r| = |H_d| gives sim_s = 1 EXACTLY.  ls_o = (sim_1 + sim_2) / 2.
 *   weight    wI_o = max(|H_3^o| of ref, |H_3^o| of dist), an integer (the paper's weight is wI / 32; the scale cancels).
 *   sums      BATCH-INVARIANT BITS: alpha = 4.2, FIX = 2^30, u_o = rint(FIX / (1 + exp(-alpha ls_o))), and u_o = U1 where
 *             ls_o = 1.0 exactly; U1 = rint(FIX / (1 + exp(-alpha))) is formed once on the host and handed to the kernel, so
 *             identical planes do not depend on the device's exp.  Three integer words leave the device per entry:
 *             den = sum_o sum_ij wI_o, and num = sum u_o wI_o as two words.  u <= 2^30 and wI < 2^23: a term is below 2^53.
 *             A thread's 16 terms total less than 2^57 and are split into their low and their high 32 bits THERE, before
 *             anything else is added.  hd wd <= 2^26 + 2^22 + 5 for h w <= 2^28, so there are fewer than 2^27.1 terms: den is
 *             below 2^51 (below 2^50 when h and w are even), num_lo below 2^60 and num_hi below 2^53 however the terms are
 *             grouped - nothing can overflow, for any tiling.  Integer adds only.
 *   host      in double, contraction off.  num = num_hi 2^32 + num_lo in 128-bit integers;
 *             similarity = (floor(num / den) + (num mod den) / den) / FIX - the quotient is below 2^30 and the remainder
 *             below 2^51, both exact in double, so this is num / (den FIX) with one rounding in the fraction and one in the
 *             sum; alpha' = logit(U1 / FIX), alpha's fixed-point image (within 8e-9 relative of 4.2);
 *             haarpsi = (logit(similarity) / alpha')^2, logit(x) = log(x / (1 - x)).  den = 0 happens only when both planes
 *             are all zero: similarity = U1 / FIX and haarpsi = 1.0.  Identical planes give num = U1 den, similarity =
 *             U1 / FIX and haarpsi = 1.0 exactly.
 *   error     against the same formula in plain float64 with the true alpha and no rounding of u: the rounding of u moves
 *             similarity by at most 2^-31 (a weighted mean of changes of at most 2^-31); similarity = x lies in [1/2, X],
 *             X = 1 / (1 + exp(-4.2)) = 0.98523, where |d haarpsi / d x| = 2 logit(x) / (alpha^2 x (1 - x)) <=
 *             2 / (alpha X (1 - X)) = 32.7: at most 1.53e-8.  alpha' for alpha scales haarpsi by (alpha / alpha')^2, within
 *             1.6e-8 of 1, and haarpsi <= 1.  Together below 3.2e-8; the tests hold the device to 4e-8.
 * Deliberate differences: the paper's colour variant (YIQ chroma similarity at one mean-filtered scale) is left out - each
 * plane is measured by itself, like every other metric here; and the authors' Python port uses SciPy's 'same', which centres
 * an even kernel one sample away from MATLAB's centring - MATLAB's is built.
 * Limits: every plane at least 16 x 16 and h w <= 2^28: VQA_ERR_UNSUPPORTED beyond either.
 * The contract of vqa_gmsd_submit: asynchronous, the same plane descriptors (one to four planes, each measured by itself;
 * packed layouts through pixel_step), depths (one per submit), alignment rules, memory kinds, slices of 32768 frames and
 * failure guarantee.  VQA_ERR_STATE while a HaarPSI batch is pending.  A HaarPSI batch is a batch of its own: it may be in
 * flight next to a batch of every other kind of the same ctx, and each wait collects its own kind only - vqa_haarpsi_wait
 * with only another kind pending, and another kind's wait with only a HaarPSI batch pending, are VQA_ERR_STATE and leave that
 * batch pending.
 * One fused kernel per group of same-geometry planes, k_haarpsi: a workgroup forms a 64 x 32 tile of S and its apron (3
 * samples before, 4 after) for both images in LDS straight from the input quads; only the three words leave the kernel.
 * Scratch on the device: 24 bytes per entry; host frames are staged in the buffers a quality submit uses.  All of it is kept
 * by the ctx until vqa_trim / vqa_destroy.
 * out of vqa_haarpsi_wait: n * n_planes entries, frame-major.                                                              */
VQA_API int vqa_haarpsi_submit(vqa_ctx *ctx, const uint8_t *ref, const uint8_t *dist, int mem_kind, int n,
                               int64_t ref_frame_stride, int64_t dist_frame_stride, const vqa_plane_desc *planes, int n_planes);
VQA_API int vqa_haarpsi_wait(vqa_ctx *ctx, vqa_haarpsi_metrics *out, int n_entries);

/* ---- VCA texture features: spatial energy E, its temporal gradient h and brightness L from a weighted 32 x 32 block DCT
 *      (Menon, Feldmann, Amirpour, Ghanbari, Timmerer: VCA, Video Complexity Analyzer, MMSys 2022) ----
 * The complexity side of a CRF-prediction row: what the per-title literature measures on the SOURCE.  It reads planes of the
 * REFERENCE stream only.  It is the paper's method with the details fixed here; where this text and the VCA tool differ, this
 * text is what is built: VCA uses an integer transform and its own normalisation of L, neither of which was at hand.  It is
 * NOT pinned against VCA's binary.
 * Inputs   one to four planes, each measured by itself; R: the RAW INTEGER SAMPLES of a plane, h x w at `depth` bits;
 *          sc = 2^-(depth - 8).
 * Blocks   nbx = floor(w / 32), nby = floor(h / 32), C = nbx nby; blocks tile from (0, 0) and the right and bottom remainder
 *          is not looked at (1080p: 60 x 33); block k = by nbx + bx.
 * Transform D = T X T^t, the orthonormal 2-D DCT-II of the block's samples X: T[u][x] = c_u cos(pi (2x + 1) u / 64),
 *          c_0 = sqrt(1 / 32), c_u = sqrt(2 / 32) otherwise.
 * Energy   H_k = sum over (u, v) != (0, 0) of w(u, v) |D(u, v)|, w(u, v) = exp(|(u v / 1024)^2 - 1|): the DC is left out.
 * Brightness S_k = the sum of the block's samples, an exact integer below 2^26; the DC coefficient is S_k / 32 and is taken
 *          from S_k, not from the product.
 * Words    qH_k = rint(H_k 2^(24 - depth)), below 2^37 at every depth (H_k <= e 32 sqrt(sum X^2) < 2784 2^depth);
 *          qL_k = rint(sqrt((double) S_k) 2^24), below 2^37.  Per frame and plane three uint64 sums over the blocks:
 *          e_sum = sum qH_k, h_sum = sum |qH_k(i) - qH_k(i - 1)| (0 for a frame with no predecessor), l_sum = sum qL_k; with
 *          C <= 2^18 blocks every sum stays below 2^55.
 * Host     in double: E = sc e_sum 2^-(24 - depth) / (1024 C), h = sc h_sum 2^-(24 - depth) / (1024 C),
 *          L = sqrt(sc / 32) l_sum 2^-24 / C: all three on the 8-bit scale at every depth.
 * Device   fp32: T and w rounded to fp32 once; the block's rounded mean (S_k + 512) >> 10 is taken off every sample first (the
 *          AC coefficients do not change and the DC's rounding stays out of them); both products are k-ordered fp32 fma chains
 *          of 32 terms on v_mfma_f32_32x32x2_f32 in an order that depends on the block alone; w |D| is summed in double in a
 *          fixed order.  DESIGN.md 4n derives the error against the formula in float64; the tests hold E, h, L and every
 *          block's H / 1024 to 1e-4 max(1, |value|) on the 8-bit scale.  l_sum is exact: integers and one double sqrt.
 * Limits   VQA_ERR_UNSUPPORTED for a plane below 32 x 32, a packed layout (pixel step beyond one sample: bgr24), and
 *          w h > 2^28 at 8 bits or > 2^26 above (the family's limits).
 * The contract of vqa_siti_submit for the stream and for prev0 - asynchronous, the same plane descriptors, depths (one per
 * submit), alignment rules, memory kinds and failure guarantee; prev0: the reference frame before frame 0, one frame of the
 * reference's layout, resident where the frames are, or NULL: frame 0 then has no predecessor (h_sum = 0).  A batch of more
 * than 32768 frames goes out in slices; a slice's first frame takes the previous slice's last frame as its predecessor.
 * VQA_ERR_STATE while a VCA batch is pending.  A VCA batch is a batch of its own: it may be in flight next to a batch of every
 * other kind of the same ctx, and each wait collects its own kind only - vqa_vca_wait with only another kind pending, and
 * another kind's wait with only a VCA batch pending, are VQA_ERR_STATE and leave that batch pending.
 * Kernels: per slice and group of same-geometry planes k_vca_blocks (a wave per block, every sample read once, both products
 * on the matrix cores, qH_k, S_k, qL_k into a block map with one slot more than frames: prev0's), then k_vca_sum (the map and
 * its |difference| to the slot before, integer adds only: no order can change a word).  A static clip gives h_sum == 0
 * exactly.  Scratch on the device: 24 bytes per block and slot, 24 per entry and 12 KiB of tables, and as much pinned host
 * memory; host frames and prev0 are staged in the buffers of an SI / TI submit.  All of it is kept by the ctx until vqa_trim /
 * vqa_destroy.
 * out of vqa_vca_wait: n * n_planes entries, frame-major.  blocks: NULL, or room for n_block_words = 2 n sum_p C_p words - per
 * frame and plane, in plane order, C_p pairs (qH_k, S_k): the block map, for callers who want it.  Any other n_block_words
 * with blocks given is VQA_ERR_INVALID and leaves the batch pending.                                                        */
VQA_API int vqa_vca_submit(vqa_ctx *ctx, const uint8_t *ref, const uint8_t *prev0, int mem_kind, int n, int64_t ref_frame_stride,
                           const vqa_plane_desc *planes, int n_planes);
VQA_API int vqa_vca_wait(vqa_ctx *ctx, vqa_vca_metrics *out, int n_entries, uint64_t *blocks, int64_t n_block_words);

/* ---- No-reference artefact measures of ONE stream: blockiness, blur and noise ----
 * The three artefacts an encode is screened for beside banding (CAMBI).  All three are neighbour-difference statistics of one
 * plane: integer work up to the last division, no frame before, no model file, no constants from a tool.  They are the three
 * papers' methods with the details fixed here; no tool is compared (FFmpeg's blockdetect and blurdetect measure other things).
 * Inputs   one to four planes, each measured by itself; x[H][W]: the RAW INTEGER SAMPLES of a plane at `depth` bits;
 *          s = 2^(depth - 8).  Packed bgr24 is measured per channel plane, as in SI/TI.
 * Blockiness  the boundary-difference measure of Wang, Sheikh and Bovik (ICIP 2002), resolved by grid phase; the normalisation
 *          is this project's own.  A horizontal boundary c lies between columns c - 1 and c, c = 1 .. W - 1; its step in row i
 *          is |x(i, c) - x(i, c - 1)|.  edge_h[p], p = 0 .. 7: the sum of the steps over all rows and all boundaries with
 *          c mod 8 == p; cnt_h[p]: the number of such terms, H times the number of c in 1 .. W - 1 with c mod 8 == p (it follows
 *          from H and W alone and is not a device word).  edge_v[p], cnt_v[p]: the same over rows, boundary r between rows r - 1
 *          and r.  Per direction and phase, in double:
 *              m_B = edge[p] / cnt[p],  m_O = (sum_q edge[q] - edge[p]) / (sum_q cnt[q] - cnt[p])   (integer differences),
 *              r[p] = (m_B - m_O) / (m_B + m_O), and exactly 0 when m_B + m_O == 0;  r[p] lies in [-1, 1].
 *          blockiness = (r_h[0] + r_v[0]) / 2: the 8 x 8 grid anchored at the plane's origin, where a codec puts it.
 *          phase_h = argmax_p r_h[p], the lowest p on a tie; phase_v likewise;
 *          blockiness_max = (r_h[phase_h] + r_v[phase_v]) / 2: the grid of a cropped or shifted picture.
 *          Constant 8 x 8 blocks read 1; the same blocks shifted by (3, 5) read phase_h 3, phase_v 5, blockiness_max 1 and
 *          blockiness -1; a flat plane reads 0.
 * Blur     Crete-Roffet, Dolmiere, Ladret and Nicolas (SPIE 2007), the paper's form: a 9-tap mean and plain neighbour
 *          differences (not scikit-image's blur_effect: Sobel, 11 taps).  Vertically dF(i, j) = |x(i, j) - x(i - 1, j)|; the
 *          neighbour difference of the 9-tap column mean telescopes, nine times it is dB9(i, j) = |x(i + 4, j) - x(i - 5, j)|,
 *          so no blur pass is made.  Domain: i = 5 .. H - 5 and every column j - where the whole window lies inside, H - 9 rows.
 *          blur_f_v = sum dF, blur_v_v = sum max(0, 9 dF - dB9); in double F9 = 9 blur_f_v,
 *          blur_v = (F9 - blur_v_v) / F9, and exactly 0 when blur_f_v == 0.  Horizontally the same over columns
 *          (j = 5 .. W - 5, every row): blur_f_h, blur_v_h, blur_h.  blur = max(blur_h, blur_v), in [0, 1]; larger = less
 *          sharp.  A 0 / peak checkerboard reads exactly 1/9; the ramp x(i, j) = j reads blur_h 1 and blur_v 0.
 * Noise    Immerkaer's fast noise estimate (CVIU 1996): L = x(i-1,j-1) - 2 x(i-1,j) + x(i-1,j+1) - 2 x(i,j-1) + 4 x(i,j)
 *          - 2 x(i,j+1) + x(i+1,j-1) - 2 x(i+1,j) + x(i+1,j+1) over the interior i = 1 .. H - 2, j = 1 .. W - 2;
 *          lap = sum |L|; in double noise = (c lap) / ((6 N) s) with N = (W - 2)(H - 2) and c = 1.2533141373155003, the
 *          double nearest sqrt(pi / 2): a standard deviation on the 8-bit scale at every depth.  A ramp reads exactly 0.
 * Ranges   the largest term per sample is 9 * 65535 (blur_v_*), so the largest word stays below 9 * 65535 H W: under 2^43 at
 *          2160p and, with H W <= 2^28, under 2^48 < 2^63 at any plane the library accepts.  No lane of the kernel sums more
 *          than 64 samples (below 2^26) in 32 bits; everything beyond a lane is 64-bit.
 * Limits   every plane at least 16 x 16 and H W <= 2^28 (the family's limits): VQA_ERR_UNSUPPORTED beyond either.  At 16 rows
 *          the vertical blur domain is 7 rows.
 * The contract of vqa_cambi_submit: asynchronous, ONE stream, the same plane descriptors (one to four planes, each measured by
 * itself; packed layouts through pixel_step), depths (one per submit, 8..16), alignment rules, memory kinds and failure
 * guarantee: a failed submit leaves nothing in flight.  A batch of more than 32768 frames goes out in slices.  VQA_ERR_STATE
 * while an artefacts batch is pending.  An artefacts batch is a batch of its own: it may be in flight next to a batch of every
 * other kind of the same ctx (one upload then serves all), and each wait collects its own kind only - vqa_artifacts_wait with
 * only another kind pending, and another kind's wait with only an artefacts batch pending, are VQA_ERR_STATE and leave that
 * batch pending.
 * Kernel: per slice and group of same-geometry planes one launch of k_artifacts: a 64 x 32 tile and its apron (5 samples up
 * and left, 4 down and right; 8 are loaded on the left, which keeps groups of four samples aligned) go to LDS as raw integers,
 * every sample read once apart from aprons, four samples per load where the layout allows; tile origins are multiples of 8, so a boundary's phase is a local index mod 8; every term belongs to one
 * sample - the right-hand or lower one of a boundary, the centre of a window - so tiles neither share nor drop a term; integer
 * adds only, 64-bit integer atomics: no order can change a word; no floating point on the device.  vqa_artifacts_wait forms
 * everything below the words on the host in double, contraction off, in the order written above.  Scratch on the device: the
 * 21 words per entry, and as much pinned host memory; host frames are staged in the buffer of the second stream of a quality
 * submit.  All of it is kept by the ctx until vqa_trim / vqa_destroy.
 * out of vqa_artifacts_wait: n * n_planes entries, frame-major.                                                             */
VQA_API int vqa_artifacts_submit(vqa_ctx *ctx, const uint8_t *frames, int mem_kind, int n, int64_t frame_stride,
                                 const vqa_plane_desc *planes, int n_planes);
VQA_API int vqa_artifacts_wait(vqa_ctx *ctx, vqa_artifacts_metrics *out, int n_entries);

/* ---- BRISQUE: the natural-scene statistics of ONE stream, 36 features per plane ----
 * Mittal, Moorthy and Bovik, "No-reference image quality assessment in the spatial domain" (IEEE TIP 2012): the features every
 * NR-IQA baseline is built on.  The definition follows the authors' brisque_feature.m, estimateggdparam.m and
 * estimateaggdparam.m AS RECALLED; it is not pinned against their MATLAB nor against OpenCV's QualityBRISQUE.  The score (an
 * epsilon-SVR over the rescaled features) is not part of this ABI; no model ships.
 * Inputs   one to four planes, each measured by itself; x[H][W]: the RAW INTEGER SAMPLES of a plane at `depth` bits;
 *          peak = 2^depth - 1, C = peak / 255 (the authors' constant 1 on the 8-bit scale: the field is the same at every depth).
 * Scales   scale 0 is x; scale 1 is half(x), of ceil(H / 2) x ceil(W / 2) samples: MATLAB's imresize(x, 0.5) - bicubic with
 *          antialiasing - of the SAMPLES.  Per axis output o takes the inputs 2 o - 3 .. 2 o + 4 with the weights
 *          [-3, -9, 29, 111, 111, 29, -9, -3] / 256; an index outside 0 .. n - 1 is mirrored: aux = [0 .. n - 1, n - 1 .. 0],
 *          index mod 2 n.  The filter is separable, so half(x) is an exact integer over 65536; it may be negative or above peak.
 * MSCN     window w = g g^t / sum, g_k = exp(-k^2 / (2 (7/6)^2)), k = -3 .. 3 (the library applies g / sum g along rows, then
 *          along columns).  mu = sum w x, s = sqrt(|sum w x^2 - mu^2|), ZERO outside the plane (filter2(.., 'same'));
 *          m = (x - mu) / (s + C), in double; u = rint(m 2^16), ties to even: the one rounding.  Everything below is integer.
 * Pairs    with wrap-around, as circshift does it (indices mod H, mod W):  H: m(i, j) m(i, j - 1);  V: m(i, j) m(i - 1, j);
 *          D1: m(i, j) m(i - 1, j - 1);  D2: m(i, j) m(i + 1, j - 1).  A pair is CLASSED by the sign of the exact integer
 *          product e = u_a u_b (negative, positive; e == 0 is in neither and adds nothing); its magnitude is then rounded to
 *          2^-16: |p| = (|e| + 2^15) >> 16.
 * Words    per scale: sum |u|, sum u^2; per orientation n_neg, n_pos, sum |p| over all pairs, and sum |p|^2 over the negative
 *          and over the positive pairs, each as the sum of the squares' low 32 bits and the sum of the rest.  30 words a scale.
 * GGD fit  N = the scale's sample count.  sigma2 = sum_u2 / 2^32 / N, E = sum_abs_u / 2^16 / N, rho = sigma2 / E^2;
 *          alpha = the gam of the grid gam_k = (200 + k) / 1000, k = 0 .. 9800, that minimises
 *          |rho - G(1/gam) G(3/gam) / G(2/gam)^2|, the first on a tie; the ratio is exp(lgamma(1/gam) + lgamma(3/gam) -
 *          2 lgamma(2/gam)).  Features: alpha, sigma2.
 * AGGD fit of an orientation: S- = sq_neg_hi 2^32 + sq_neg_lo and S+ likewise, exact integers rounded once to double;
 *          l = sqrt(S- / 2^32 / n_neg), r = sqrt(S+ / 2^32 / n_pos), gh = l / r;
 *          rhat = (sum_abs_p / 2^16 / N)^2 / ((S- + S+) / 2^32 / N);  rn = rhat (gh^3 + 1)(gh + 1) / (gh^2 + 1)^2;
 *          alpha = the gam of the same grid that minimises (G(2/gam)^2 / (G(1/gam) G(3/gam)) - rn)^2, the first on a tie;
 *          mean = (r - l) exp(lgamma(2/alpha) - lgamma(1/alpha)) exp((lgamma(1/alpha) - lgamma(3/alpha)) / 2).
 *          Features: alpha, mean, l^2, r^2.
 * Order    per scale GGD, H, V, D1, D2: 18 features, 36 in all.
 * Degenerate  GGD: sum_abs_u == 0 (no non-zero m).  AGGD: n_neg == 0, n_pos == 0 or S+ == 0 (then r == 0, the divisor of gh).
 *          The fit's features are 0 and bit 5 scale + fit of flags is set.  A plane of zeros gives 36 zeros and flags 0x3ff.
 *          No NaN ever leaves the library.
 * Ranges   |m| <= sqrt((1 - w0) / w0) = 2.742, w0 = 0.11740 the window's centre weight: with mu' the weighted mean of the
 *          other 48 samples (zeros outside included), x - mu = (1 - w0)(x - mu') and, by the law of total variance,
 *          sum w x^2 - mu^2 >= w0 (1 - w0)(x - mu')^2, so |x - mu| / s <= (1 - w0) / sqrt(w0 (1 - w0)); C > 0 only lowers it.
 *          So |u| <= 2.742 * 2^16 < 2^18, u^2 < 7.52 * 2^32, and with H W <= 2^28 sum_u2 < 7.52 * 2^60 < 2^63 and
 *          sum_abs_u < 2^46.  |p| <= 7.52 * 2^16 < 2^19, sum_abs_p < 2^47; |p|^2 < 2^38, whose sum could pass 2^63: its low
 *          32 bits sum to less than 2^60 and the rest (< 2^6 a pair) to less than 2^34.  half(x): |v 65536| <= 304^2 * 65535
 *          < 2^33, beyond 32 bits above 8-bit depth: the device holds it in a double, exactly.
 * Accuracy the one rounding moves m by at most d = 2^-17; rounding |p| adds 2^-17.  Per sample m^2 moves by 2 |m| d + d^2, per
 *          pair p by (|m_a| + |m_b|) d + d^2 + 2^-17 and p^2 by 2 |p| dp + dp^2.  Against the unrounded field, with E = mean |m|
 *          and A = mean |p|: mean |m| within d = 7.7e-6; mean m^2 within 2 E d + d^2 <= 2 * 2.742 d + d^2 = 4.2e-5; mean |p|
 *          within 2 E d + d^2 + 2^-17 <= 5.0e-5; sum p^2 / N of a class within 2 A 5.0e-5 + 2.5e-9 <= 7.5e-4.  A pair changes
 *          class only if one of its m is within d of zero; its |p| is then below 2.742 d.  The moments are formed in double on
 *          the device; what their own error moves m by is below 2e-9 at 16 bits (64 ulp of 65535^2 under (s + C)^2 >= 257^2).
 * Limits   every plane at least 16 x 16 and H W <= 2^28 (the family's limits): VQA_ERR_UNSUPPORTED beyond either.
 * The contract of vqa_cambi_submit: asynchronous, ONE stream, the same plane descriptors (one to four planes, each measured by
 * itself; packed layouts through pixel_step), depths (one per submit, 8..16), alignment rules, memory kinds and failure
 * guarantee: a failed submit leaves nothing in flight.  A batch of more than 32768 frames goes out in slices.  VQA_ERR_STATE
 * while a BRISQUE batch is pending.  A BRISQUE batch is a batch of its own: it may be in flight next to a batch of every other
 * kind of the same ctx (one upload then serves all), and each wait collects its own kind only - vqa_brisque_wait with only
 * another kind pending, and another kind's wait with only a BRISQUE batch pending, are VQA_ERR_STATE and leave that batch
 * pending.
 * Kernels: per slice and group of same-geometry planes k_brisque_half (the exact scale-1 planes into scratch), then per scale
 * k_brisque_mscn (a 64 x 16 tile and a 4 / 4 / 4 / 3 apron in LDS, both 7-tap moment passes in double, u, the pairs inside the
 * plane, 64-bit integer atomics; the u of the first and last row and column go to four strips) and k_brisque_seam (the pairs
 * that wrap around, corners included, from the strips).  Tiles start at the plane's origin, so u does not depend on the batch.
 * vqa_brisque_wait forms flags and features on the host in double, contraction off, in the order written above; the two Gamma
 * ratio tables (9801 entries) are built once from lgamma.  Scratch on the device: the 60 words per entry and as much pinned host
 * memory; per frame of a slice the scale-1 planes (8 bytes a sample) and strips of the largest plane group; host frames are
 * staged in the buffer of the second stream of a quality submit.  All of it is kept by the ctx until vqa_trim / vqa_destroy.
 * out of vqa_brisque_wait: n * n_planes entries, frame-major.                                                                */
VQA_API int vqa_brisque_submit(vqa_ctx *ctx, const uint8_t *frames, int mem_kind, int n, int64_t frame_stride,
                               const vqa_plane_desc *planes, int n_planes);
VQA_API int vqa_brisque_wait(vqa_ctx *ctx, vqa_brisque_metrics *out, int n_entries);

/* ---- MDSI (Nafchi, Shahkolaei, Hedjam and Cheriet, IEEE Access 2016): mean deviation similarity index ----
 * Gradient similarity of the luminance, with the paper's fused-image term, plus a chromaticity similarity of two opponent
 * channels, the three planes of a pixel taken together, pooled by a deviation.  0 means identical; larger is worse.  The metric
 * is NOT symmetric in (ref, dist).  This is the authors' MDSI.m with the "sum" combination AS RECALLED: it is NOT pinned against
 * their MATLAB nor against any Python port (neither was available).  Where this text and a tool differ, this text is what is
 * built.  The paper's multiplicative combination is not built.
 * A frame is THREE planes of one depth (8 bits, or 9..16 bits as uint16), or ONE plane; the RAW INTEGER SAMPLES are read as they
 * are and nothing is clamped anywhere.  With s = 2^(depth - 8) and peak = 2^depth - 1 the planes give R, G, B on the 0..255 scale:
 *   VQA_MDSI_YUV709  planes Y, U, V; the geometry rules and the chroma replication of vqa_ciede_submit exactly: the chroma sample
 *             of luma (i, j) is (i >> sv, j >> sh); 4:4:4, 4:2:2, 4:2:0, odd sizes.
 *               y = (Y - 16 s) / (219 s), u = (U - 128 s) / (224 s), v = (V - 128 s) / (224 s)
 *               R = 255 (y + 1.5748 v), G = 255 (y - 0.1873 u - 0.4681 v), B = 255 (y + 1.8556 u)
 *   VQA_MDSI_BGR     planes B, G, R of a common geometry (packed bgr24 through the pixel step); R = 255 R_int / peak, G, B likewise.
 *   VQA_MDSI_GRAY    one plane Y: the YUV709 model with u = v = 0.
 * Downsampling.  f = max(1, floor(min(h, w) / 256 + 0.5)) of plane 0 (MATLAB's round: 640 gives 3).  The grid is hd = ceil(h / f)
 *   by wd = ceil(w / f).  Sample (i, j) of a downsampled channel is the sum of the channel over rows i f + o .. i f + o + f - 1, o =
 *   floor(f / 2) - (f - 1), and the same columns, over f^2; a position outside the plane counts R = G = B = 0.  This is
 *   conv2(x, ones(f) / f^2, 'same') kept at 1:f:end; for f = 2 it is vqa_gmsd_submit's 2x2 stage.
 * Channels.  L = 0.2989 R + 0.5870 G + 0.1140 B, H = 0.30 R + 0.04 G - 0.35 B, M = 0.34 R - 0.60 G + 0.17 B.  All are affine in the
 *   samples, so the device box-sums the INTEGER samples of each plane, S0, S1, S2, counts the in-plane positions of the window,
 *   cnt (which carries the YUV offsets: the fill is a zero of R, G, B, not of Y, U, V), and applies one 3 x 4 double matrix:
 *     rgb[c][0..2] = the coefficient of plane 0, 1, 2 in colour c (R, G, B): with ky = 255 / (219 s), kc = 255 / (224 s)
 *       YUV709: R (ky, 0, 1.5748 kc), G (ky, -0.1873 kc, -0.4681 kc), B (ky, 1.8556 kc, 0); GRAY: (ky, 0, 0) for all three;
 *       BGR, k = 255 / peak: R (0, 0, k), G (0, k, 0), B (k, 0, 0);
 *     rgb[c][3] = -((o0 rgb[c][0] + o1 rgb[c][1]) + o1 rgb[c][2]), o0 = 16 s and o1 = 128 s (both 0 for BGR);
 *     mat[ch][j] = ((a_R rgb[0][j] + a_G rgb[1][j]) + a_B rgb[2][j]) / (f f), (a_R, a_G, a_B) the row of channel ch above;
 *     channel = ((mat[ch][0] S0 + mat[ch][1] S1) + mat[ch][2] S2) + mat[ch][3] cnt.
 * Gradients.  Prewitt over 3, divided by 3, at every downsampled sample, L counting 0 outside the grid (vqa_gmsd_submit's
 *   convention), with x(di, dj) = L(i + di, j + dj):
 *     gx = (((x(-1,1) + x(0,1)) + x(1,1)) - ((x(-1,-1) + x(0,-1)) + x(1,-1))) / 3
 *     gy = (((x(1,-1) + x(1,0)) + x(1,1)) - ((x(-1,-1) + x(-1,0)) + x(-1,1))) / 3
 *   for the reference (r) and the distorted image (d); the fused image F = 0.5 (L_r + L_d) has, by linearity, the gradient
 *   0.5 (g_r + g_d) per component, and that form is what is evaluated.  q_x = gx^2 + gy^2 (= m_x^2) for x in r, d, F.
 * Similarities, C1 = 140, C2 = 55, C3 = 550 on the 8-bit scale (R, G, B are on it at any depth):
 *     S(a, b, c) = (2 m_a m_b + c) / (m_a^2 + m_b^2 + c), evaluated as (2 sqrt(q_a q_b) + c) / ((q_a + q_b) + c)
 *     GS = (S(r, d, C1) + S(d, F, C2)) - S(r, F, C2)
 *     CS = (2 (H_r H_d + M_r M_d) + C3) / (((H_r^2 + H_d^2) + (M_r^2 + M_d^2)) + C3)
 *     GCS = 0.6 GS + 0.4 CS, in (-1, 1.6)
 *   Equal samples give S = CS = 1 and GCS = 1 exactly (sqrt(q q) = q, x + x = 2 x, 0.6 + 0.4 = 1 in IEEE double).
 * Pooling.  z = GCS^(1/4), the principal complex root: |GCS|^(1/4) times 1 for GCS >= 0 and times (1 + i) / sqrt(2) for GCS < 0;
 *   dev = mean |z - mean z| over the N = hd wd samples; mdsi = dev^(1/4).
 * How the device forms it: everything up to GCS in double, contraction off, every step rounded once in the order written.
 *   g = rint(GCS 2^24), a signed 32-bit integer, rounded ONCE; from here on everything is a function of g.
 *   k_mdsi_map writes g to a scratch map and adds, as 64-bit integers, zq = rint(sqrt(sqrt(|g| 2^-24)) 2^28) into word A where
 *   g >= 0 and into word B where g < 0, and the count n_neg.  k_mdsi_dev reads the map and the frame's A, B, forms the mean
 *   (m_re, m_im) = (((double)A + (double)B r) / N, ((double)B r) / N), r = sqrt(0.5) as a double, in 2^-28 units and identically
 *   in every thread, takes (re, im) = (zq, 0) for g >= 0 and (zq r, zq r) for g < 0, and adds
 *   rint(sqrt((re - m_re)^2 + (im - m_im)^2)) into word D.  zq < 2^29 and N <= 2^28: no word can overflow.  Integer addition
 *   is associative: the four words do not depend on the tiling, the batch or the order in which workgroups retire.
 *   vqa_mdsi_wait forms dev = D / (N 2^28) and mdsi = sqrt(sqrt(dev)) in double, contraction off.  Identical inputs give g = 2^24
 *   everywhere, so B = n_neg = D = 0 and dev = mdsi = 0.0 EXACTLY (a plain float64 evaluation leaves dev near 1e-16, which the
 *   quarter power would turn into 1e-4: this is why the record carries dev).
 * Limits: plane 0 at least 16 x 16 and h w <= 2^28: VQA_ERR_UNSUPPORTED beyond either.  n_planes other than 1 or 3, one plane
 *   with a model other than VQA_MDSI_GRAY (or three with it), mixed depths, chroma geometries vqa_ciede_submit would refuse, an
 *   unknown model: VQA_ERR_INVALID.
 * The contract of vqa_ciede_submit: asynchronous, ONE ENTRY PER FRAME, the same plane descriptors, depths, alignment rules,
 * memory kinds and failure guarantee: a failed submit leaves nothing in flight.  VQA_ERR_STATE while an MDSI batch is pending.
 * An MDSI batch is a batch of its own: it may be in flight next to a batch of every other kind of the same ctx, and each wait
 * collects its own kind only - vqa_mdsi_wait with only another kind pending, and another kind's wait with only an MDSI batch
 * pending, are VQA_ERR_STATE and leave that batch pending.  A batch of more than 32768 frames goes out in slices.
 * Kernels, one launch each per slice: k_mdsi_map (a workgroup owns a 64 x 32 tile of the downsampled grid and its apron of one
 * sample; input rows are read coalesced and box-summed in LDS, one loop for every f; L_r, L_d of tile and apron in LDS as
 * doubles, H and M in registers) and k_mdsi_dev.  Scratch on the device: 32 bytes per frame and the map, 4 bytes per
 * downsampled sample per frame of a slice; host frames are staged in the buffers a quality submit uses.  All of it is kept by
 * the ctx until vqa_trim / vqa_destroy.
 * out of vqa_mdsi_wait: n entries (n_entries = n).                                                                         */
enum vqa_mdsi_model { VQA_MDSI_YUV709 = 0, VQA_MDSI_BGR = 1, VQA_MDSI_GRAY = 2 };
VQA_API int vqa_mdsi_submit(vqa_ctx *ctx, const uint8_t *ref, const uint8_t *dist, int mem_kind, int n,
                            int64_t ref_frame_stride, int64_t dist_frame_stride, const vqa_plane_desc *planes, int n_planes,
                            int model);
VQA_API int vqa_mdsi_wait(vqa_ctx *ctx, vqa_mdsi_metrics *out, int n_entries);
/* the downsampling factor f of an h x w plane 0, as stated above; needs no ctx and no device (0 when h or w is not positive) */
VQA_API int vqa_mdsi_factor(int height, int width);

/* ---- dE_ITP (Recommendation ITU-R BT.2124-0, 2019): the colour difference for HDR and wide-gamut video, three planes jointly ----
 * CIEDE2000 above reads every input as BT.709 / sRGB against a 100 cd/m2 white.  This one reads a BT.2020 signal with the PQ or
 * the HLG transfer function of BT.2100, turns the three samples of a pixel of either image into display light and then into
 * ICtCp, and takes the Euclidean distance of the two colours, scaled so that 1 is about one just-noticeable difference.
 * Everything below is the Recommendations' text, constant for constant.  A transfer function and a range travel with the call.
 * A frame is THREE planes of one depth (8 bits, or 9..16 bits as uint16), the RAW INTEGER SAMPLES read as they are.  With
 * s = 2^(depth - 8) and P = 2^depth - 1:
 * Colour model (`model`):
 *   VQA_ITP_YUV2020   planes Y, Cb, Cr; the geometry rules and the chroma replication of vqa_ciede_submit exactly: Cb and Cr
 *             share one geometry, the luma's or its ceil-half in each direction independently (4:4:4, 4:2:2, 4:2:0, odd sizes),
 *             and the chroma sample of luma (i, j) is (i >> sv, j >> sh).
 *               full_range = 0 (limited):  y = (Y - 16 s) / (219 s), cb = (Cb - 128 s) / (224 s), cr = (Cr - 128 s) / (224 s)
 *               full_range = 1:            y = Y / P, cb = (Cb - 2^(depth - 1)) / P, cr = (Cr - 2^(depth - 1)) / P
 *             BT.2020 non-constant luminance, Kr = 0.2627, Kb = 0.0593, Kg = 0.6780:
 *               R' = y + 1.4746 cr, B' = y + 1.8814 cb, G' = ((y - Kr R') - Kb B') / Kg
 *   VQA_ITP_BGR       planes B, G, R of a common geometry (any pixel step: packed bgr24 has step 3); R' = R / P, G' and B'
 *             likewise; full_range is ignored (but must be 0 or 1).
 * Clamp.  R', G', B' are CLAMPED to [0, 1].  This is deliberate and differs from CIEDE2000's "no clamping anywhere": the PQ
 *   EOTF has a pole at E'^(1/m2) = c2 / c3, which is E' near 1.99, unclamped limited-range input reaches R' near 1.94, and a
 *   display shows nothing outside [0, 1].
 * Transfer (`transfer`): the signal E' of a channel -> display light Fd in cd/m2.
 *   VQA_ITP_PQ    Fd = 10000 (max(E'^(1/m2) - c1, 0) / (c2 - c3 E'^(1/m2)))^(1/m1),
 *             m1 = 2610 / 16384, m2 = 2523 / 4096 * 128, c1 = 3424 / 4096, c2 = 2413 / 4096 * 32, c3 = 2392 / 4096 * 32.
 *   VQA_ITP_HLG   scene light E = E'^2 / 3 for E' <= 1 / 2, otherwise (exp((E' - c) / a) + b) / 12,
 *             a = 0.17883277, b = 0.28466892, c = 0.55991073; then the BT.2100 OOTF of a 1000 cd/m2 display (gamma 1.2, black
 *             level 0): Ys = (0.2627 E_R + 0.6780 E_G) + 0.0593 E_B, Fd_ch = (1000 Ys^0.2) E_ch; Ys = 0 gives 0.
 * ICtCp (BT.2100, the PQ form, for both transfers), on Fd:
 *   L = ((1688 R + 2146 G) + 262 B) / 4096, M = ((683 R + 2951 G) + 462 B) / 4096, S = ((99 R + 309 G) + 3688 B) / 4096
 *   X' = ((c1 + c2 Yn^m1) / (1 + c3 Yn^m1))^m2 with Yn = X / 10000, for X = L, M, S
 *   I = 0.5 (L' + M'), Ct = ((6610 L' - 13613 M') + 7003 S') / 4096, Cp = ((17933 L' - 17390 M') - 543 S') / 4096
 * BT.2124: T = 0.5 Ct and dE_ITP = 720 sqrt((dI^2 + dT^2) + dCp^2), the differences taken between the two images.
 *   A pair of triples with equal integer samples gives EXACTLY 0 (the kernel tests for it).
 * Bound.  L', M', S' lie in [0, 1] (Fd in [0, 10000] by the clamp, and the inverse EOTF maps that onto [c1^m2, 1] within [0, 1]), so
 *   |dI| <= 1; Ct lies between -13613 / 4096 and (6610 + 7003) / 4096 = 13613 / 4096, so |dT| = |dCt| / 2 <= 13613 / 4096 < 3.3236;
 *   Cp lies between -(17390 + 543) / 4096 and 17933 / 4096, so |dCp| <= 2 * 17933 / 4096 < 8.7564.  Hence
 *   dE <= 720 sqrt(1 + 3.3236^2 + 8.7564^2) < 720 * 9.42 < 6800 < 2^13.  A pixel's q = rint(dE 2^20) stays below 2^33 and a frame
 *   of h w <= 2^28 pixels below 2^61: no word can overflow and NO SATURATION CONSTANT is needed.
 * Results, ONE ENTRY PER FRAME (not per plane): sum_q, the sum of q over the luma grid, and max_q, the largest q;
 *   de_sum = sum_q 2^-20, de_mean = de_sum / (h w), de_max = max_q 2^-20.
 * How the device forms it:
 *   arithmetic per pixel is DOUBLE with contraction off, every step rounded once in the order written above; the powers and the
 *   exponential are the accurate library functions.  (fp32 is not enough: E'^(1/m2) - c1 cancels on dark pixels and the 6.28th
 *   power multiplies what is left - up to 0.1 per pixel and 7e-4 on a frame's mean.)
 *   sums      BATCH-INVARIANT BITS: q is added as a 64-bit integer and the maximum taken as one: two words per frame, whatever
 *             the tiling and the order in which workgroups retire.  The rounding moves de_mean and de_max by at most half a
 *             quantum: 2^-21.
 *   host      the words -> double, times 2^-20, over h w: in vqa_itp_wait, in double, with contraction off.
 * Limits: luma at least 16 x 16 and h w <= 2^28: VQA_ERR_UNSUPPORTED beyond either.  n_planes other than 3, Cb and Cr (or
 * B, G, R) geometries that differ, a chroma size that is neither the luma's nor its ceil-half, mixed depths, an unknown
 * model or transfer, a full_range other than 0 or 1: VQA_ERR_INVALID.
 * The contract of vqa_ciede_submit: asynchronous, ONE ENTRY PER FRAME, the same plane descriptors, depths, alignment rules,
 * memory kinds and failure guarantee: a failed submit leaves nothing in flight.  VQA_ERR_STATE while a dE_ITP batch is pending.
 * A dE_ITP batch is a batch of its own: it may be in flight next to a batch of every other kind of the same ctx, and each wait
 * collects its own kind only - vqa_itp_wait with only another kind pending, and another kind's wait with only a dE_ITP batch
 * pending, are VQA_ERR_STATE and leave that batch pending.  A batch of more than 32768 frames goes out in slices.
 * One fused kernel per slice, k_itp: a thread owns a 2 x 4 luma patch of both images, as in k_ciede; only the two words per
 * frame leave the kernel.  Scratch on the device: 16 bytes per frame; host frames are staged in the buffers vqa_ciede_submit
 * uses.  All of it is kept by the ctx until vqa_trim / vqa_destroy.
 * Not built: ICtCp-coded input planes, constant-luminance BT.2020, HLG display peaks other than 1000 cd/m2, chroma
 * interpolation other than replication.
 * out of vqa_itp_wait: n entries (n_entries = n).                                                                          */
enum vqa_itp_model { VQA_ITP_YUV2020 = 0, VQA_ITP_BGR = 1 };
enum vqa_itp_transfer { VQA_ITP_PQ = 0, VQA_ITP_HLG = 1 };
VQA_API int vqa_itp_submit(vqa_ctx *ctx, const uint8_t *ref, const uint8_t *dist, int mem_kind, int n,
                           int64_t ref_frame_stride, int64_t dist_frame_stride, const vqa_plane_desc *planes, int n_planes,
                           int model, int transfer, int full_range);
VQA_API int vqa_itp_wait(vqa_ctx *ctx, vqa_itp_metrics *out, int n_entries);

/* ---- PU21 HDR quality: PU21-PSNR and PU21-SSIM (Mantiuk and Azimi, "PU21: A novel perceptually uniform encoding for adapting
 * existing quality metrics for HDR", PCS 2021), three planes jointly ----
 * dE_ITP above is a pointwise colour difference.  Every structural or error figure of the other kinds reads a code value as a
 * linear SDR-like scale, which on a PQ stream weighs an error at 2 cd/m2 like one at 2000 cd/m2.  PU21 maps ABSOLUTE luminance to
 * perceptually uniform units; the ordinary PSNR and the ordinary Gaussian SSIM then run on those units.
 * Input.  Exactly vqa_itp_submit's: THREE planes of one depth (8 bits, or 9..16 bits as uint16), the colour models
 *   VQA_ITP_YUV2020 (Y, Cb, Cr, BT.2020 non-constant luminance, limited or full range, chroma replicated: 4:4:4, 4:2:2, 4:2:0, odd
 *   sizes) or VQA_ITP_BGR, the transfers VQA_ITP_PQ or VQA_ITP_HLG - the same enums, the same geometry rules.
 * Display light.  R', G', B' CLAMPED to [0, 1], then per channel the display light Fd in cd/m2 through the PQ EOTF, or through
 *   HLG's inverse OETF and the OOTF of a 1000 cd/m2 display: word for word the chain vqa_itp_submit states up to "display light",
 *   in double with contraction off, each step rounded once in the order written there.
 * Luminance.  Y = (0.2627 R + 0.6780 G) + 0.0593 B on the display-light R, G, B.
 * PU21 encoding (the authors' banding_glare fit, their default), with L CLAMPED to [0.005, 10000] first:
 *   V(L) = max(p7 (((p1 + p2 L^p4) / (1 + p3 L^p4))^p5 - p6), 0)
 *   p1 = 0.353487901, p2 = 0.3734658629, p3 = 8.277049286e-05, p4 = 0.9062562627, p5 = 0.09150303166, p6 = 0.9099517204,
 *   p7 = 596.3148142.
 *   In double with these constants V(0.005) = 5.47e-10, V(100) = 256.3838973127, V(10000) = 595.3939200201, and V is strictly
 *   increasing over the whole range.  The constants are the authors' AS RECALLED, cross-checked only by those design properties
 *   (zero at the floor, 256 at 100 cd/m2); they are NOT pinned against the authors' MATLAB.  vqa_pu21_encode is V on the host.
 * Quantisation, ONCE.  q = rint(V 2^16), below 2^26, for four channels of each image: q_Y from V(Y), and q_R, q_G, q_B from V of
 *   each display-light channel.  Everything below is a function of these integers.
 * PU21-PSNR.  sse_y = the sum over the luma grid of (q_Y,ref - q_Y,dist)^2, sse_rgb the same sum over the three channels.  A term
 *   is below 2^52 and a frame of h w <= 2^28 pixels has up to 3 * 2^28 of them, so each sum leaves the device as TWO 64-bit words:
 *   the sum of the terms' low 32 bits and the sum of the terms >> 32 (each below 2^62: no word can overflow).  The wait joins them
 *   in 128-bit integers, sse = (hi << 32) + lo, converts that integer to double (round to nearest) and divides:
 *     mse_y = sse_y / (2^32 h w), mse_rgb = sse_rgb / (2^32 (3 h w))      (both divisors are exact doubles)
 *     pu_psnr = 10 log10(256^2 / mse_y), pu_psnr_rgb = 10 log10(256^2 / mse_rgb); both are inf for a zero sum.
 *   The peak of 256 is this project's choice: PU21 puts 100 cd/m2 at 256, so SDR-range content scores near its ordinary PSNR;
 *   mse_y and mse_rgb are in the record for callers who want another peak.
 * PU21-SSIM on x = q_Y / 2^16 (exact in double):
 *   window    11 x 11 Gaussian, g_i = exp(-(i - 5)^2 / 4.5) normalised to sum 1 in double (the sum taken for i = 0 .. 10 in
 *             order), separable: horizontal first, s(y, x) = the sum over j = 0 .. 10 in order of g_j v(y, x + j), then vertical,
 *             the sum over i = 0 .. 10 in order of g_i s(y + i, x); v is x_r, x_d, x_r x_r, x_d x_d or x_r x_d (products of two
 *             26-bit values: exact).  Valid windows only: (h - 10)(w - 10) of them.
 *   moments   mu = sum w x, var = sum w x^2 - mu^2, cov = sum w x_r x_d - mu_r mu_d
 *   value     ssim = ((2 (mu_r mu_d) + C1)(2 cov + C2)) / (((mu_r^2 + mu_d^2) + C1)((var_r + var_d) + C2)),
 *             C1 = (0.01 * 256)^2, C2 = (0.03 * 256)^2 (each as the double product t t of t = 0.01 * 256, t = 0.03 * 256)
 *   all in double, contraction off.  u = rint(ssim 2^24) is a SIGNED integer (ssim may be negative), ssim_q = the sum of u over
 *   the valid windows, one signed 64-bit word (|u| <= 2^24 + 1 and at most 2^28 windows: below 2^53);
 *   pu_ssim = ssim_q / (2^24 windows).  The quantum is 2^-24 and not finer: the cancellation in sum w x^2 - mu^2 at x near 596
 *   leaves about 1e-10 on a window's value, which must stay far below the quantum.
 * Consequences.  Identical frames give all-zero SSE words, inf PSNRs, ssim_q == windows << 24 and pu_ssim == 1.0 EXACTLY
 *   (2 (mu mu) and mu^2 + mu^2 are the same double, and cov is var when computed from the same values).  A frame gives the same
 *   five words in any batch, from any memory, alone or next to other kinds: a window's value is a fixed-order sum of the same
 *   doubles whichever tile or thread computes it, and all that is added across threads is integers.
 * How the device forms it.  Per sub-slice of frames two kernels: k_pu21_encode (a thread owns a 2 x 4 luma patch of both images
 *   as in k_itp; it writes q_Y of both images as uint32 into a scratch map and adds the four SSE half-words in the thread,
 *   across the wave, then with one 64-bit atomic add per word per workgroup; a pixel whose two triples are equal skips the second
 *   chain and still writes both map entries) and k_pu21_ssim (a workgroup owns a 16 x 16 tile of the valid-window grid with a
 *   5-sample apron of both maps in LDS, the five horizontally filtered moments in LDS, one thread per window, one 64-bit atomic
 *   add per workgroup).  Scratch on the device: 40 bytes per frame for the words, and the two maps at 8 bytes per luma sample;
 *   the submit runs the two kernels over sub-slices of at most max(1, 2^28 / (8 h w)) frames, so the maps stay at or below
 *   256 MiB whatever n is.  Host frames are staged in the buffers vqa_ciede_submit uses.  All of it is kept by the ctx until
 *   vqa_trim / vqa_destroy.
 * Limits: luma at least 16 x 16 and h w <= 2^28: VQA_ERR_UNSUPPORTED beyond either.  n_planes other than 3 (one-plane layouts
 * are an error), Cb and Cr (or B, G, R) geometries that differ, a chroma size that is neither the luma's nor its ceil-half, mixed
 * depths, an unknown model or transfer, a full_range other than 0 or 1: VQA_ERR_INVALID.
 * The contract of vqa_itp_submit: asynchronous, ONE ENTRY PER FRAME, the same plane descriptors, depths, alignment rules,
 * memory kinds and failure guarantee: a failed submit leaves nothing in flight.  VQA_ERR_STATE while a PU21 batch is pending.
 * A PU21 batch is a batch of its own: it may be in flight next to a batch of every other kind of the same ctx, and each wait
 * collects its own kind only.  A batch of more than 32768 frames goes out in slices, each slice in sub-slices as above.
 * Not built: an SDR display model (PU21 on gamma-coded input), the other three PU21 fits, PU21-MS-SSIM / VIF / FSIM, and
 * luminance from anything but the three planes.
 * out of vqa_pu21_wait: n entries (n_entries = n).                                                                         */
VQA_API int vqa_pu21_submit(vqa_ctx *ctx, const uint8_t *ref, const uint8_t *dist, int mem_kind, int n,
                            int64_t ref_frame_stride, int64_t dist_frame_stride, const vqa_plane_desc *planes, int n_planes,
                            int model, int transfer, int full_range);
VQA_API int vqa_pu21_wait(vqa_ctx *ctx, vqa_pu21_metrics *out, int n_entries);
/* V(cd_m2) as stated above, in double on the host; needs no ctx and no device                                               */
VQA_API double vqa_pu21_encode(double cd_m2);
/* LAB BUILD ONLY (vqa_build_flavour() & 2; the shipped library does not export it, and this header declares it only when
 * VQA_TEST_SEAMS is defined): the two q_Y maps of the LAST vqa_pu21_submit of the ctx, [n][2][h][w] uint32 (ref, then dist), after
 * its wait; n_values = n 2 h w.  There, too, the environment may shorten a sub-slice to a given number of frames, so that a
 * small batch spans several.                                                                                                */
#ifdef VQA_TEST_SEAMS
    VQA_API int vqa_pu21_lab_read_maps(vqa_ctx *ctx, uint32_t *dst, int64_t n_values);
#endif

/* ---- FSIM / FSIMc (Zhang, Zhang, Mou and Zhang, "FSIM: a feature similarity index for image quality assessment", IEEE TIP
 * 2011): phase congruency and gradient similarity, with a chromaticity term in the colour form ----
 * The reference point GMSD, HaarPSI and MDSI were each published against.  1 means identical; smaller is worse.  This is the
 * authors' FeatureSIM.m and its embedded phasecong2 (Kovesi) AS RECALLED: it is NOT pinned against their MATLAB nor against any
 * port (neither was available).  Where this text and a tool differ, this text is what is built.
 * Input, models, box stage.  Exactly vqa_mdsi_submit's: THREE planes of one depth (8 bits, or 9..16 bits as uint16), or ONE plane;
 *   VQA_FSIM_YUV709, VQA_FSIM_BGR, VQA_FSIM_GRAY give the same R, G, B on the 0..255 scale by the same formulas, the same chroma
 *   replication and geometry rules, the same f = max(1, floor(min(h, w) / 256 + 0.5)), hd = ceil(h / f), wd = ceil(w / f), window
 *   offset o = floor(f / 2) - (f - 1) and zero fill, and the same "box-sum the integer samples S0, S1, S2 and the count cnt, then
 *   ONE 3 x 4 double matrix" with rgb[c][0..3] as stated there and the channel rows
 *     Y = 0.299 R + 0.587 G + 0.114 B,  I = 0.596 R - 0.274 G - 0.322 B,  Q = 0.211 R - 0.523 G + 0.312 B
 *     mat[ch][j] = ((a_R rgb[0][j] + a_G rgb[1][j]) + a_B rgb[2][j]) / (f f);  channel = ((mat[ch][0] S0 + mat[ch][1] S1) + mat[ch][2] S2)
 *     + mat[ch][3] cnt.  VQA_FSIM_GRAY gives I = Q = 0: both rows of the matrix are zero.
 * Phase congruency of Y, per image, on the hd x wd grid (rows = hd, cols = wd, N = hd wd).
 *   Centring.  X = Y - Y(0, 0).  The filters have no DC term, so this does not change the definition; it makes a flat grid exactly
 *     X = 0, every response exactly 0 and PC = 0 (a dense DFT of a constant would leave rounding noise, and noise over noise).
 *   Frequency grids.  For a length n, range(n) = (-(n-1)/2 .. (n-1)/2) / (n-1) if n is odd, else (-n/2 .. n/2-1) / n; x over cols, y
 *     over rows; radius = ifftshift(sqrt(x^2 + y^2)), theta = ifftshift(atan2(-y, x)); lp = 1 / (1 + (radius / 0.45)^30), taken
 *     BEFORE radius(0,0) is set to 1.
 *   Scales s = 0..3.  fo = 1 / (6 2^s); logGabor_s = exp(-(ln(radius / fo))^2 / (2 (ln 0.55)^2)) lp, and logGabor_s(0,0) = 0.
 *   Orientations o = 0..3.  a = o pi / 4; ds = sin(theta) cos a - cos(theta) sin a, dc = cos(theta) cos a + sin(theta) sin a,
 *     dtheta = |atan2(ds, dc)|, spread_o = exp(-dtheta^2 / (2 sigma^2)), sigma = (pi / 4) / 1.2; filt_{s,o} = logGabor_s spread_o.
 *     vqa_fsim_filter writes one table, formed in double on the host; the device uses the same tables.
 *   Responses.  F = fft2(X), EO_{s,o} = ifft2(F filt_{s,o}) (complex).  Per orientation, sums over s = 0..3 in order:
 *     An = sum |EO_s| (|z| = sqrt(Re^2 + Im^2)), sE = sum Re, sO = sum Im; XE = sqrt(sE^2 + sO^2) + 1e-4, mE = sE / XE, mO = sO / XE;
 *     Energy_o = sum ((Re_s mE + Im_s mO) - |Re_s mO - Im_s mE|).
 *   Noise threshold.  med_o = MATLAB's median of |EO_{0,o}|^2 = Re^2 + Im^2 over the N samples (even N: 0.5 (a + b) of the two middle
 *     values); T_o = c_o sqrt(med_o); c_o = sqrt(S_o / (ln 2 EM_o)) (sqrt(pi / 2) + 2 sqrt(2 - pi / 2)) / 1.7, EM_o = sum filt_{0,o}^2,
 *     S_o = sum_x (sum_s real(ifft2(filt_{s,o})) sqrt(N))^2 - the file's EstSumAn2 + 2 EstSumAiAj, tau, k = 2 and T / 1.7 folded
 *     into one geometry constant.  By Parseval S_o = sum_k (sum_s fe_{s,o}(k))^2, fe(k) = (filt(k) + filt(-k mod (hd, wd))) / 2, which is
 *     how the host forms it; vqa_fsim_noise_factor returns c_o.
 *   Result.  PC = (sum_o max(Energy_o - T_o, 0)) / (sum_o An_o), sums over o = 0..3 in order, and 0 where the denominator is 0.
 * Similarity and pooling.
 *   Scharr gradient of the UNCENTRED Y, zeros outside the grid (vqa_gmsd_submit's convention), with x(di, dj) = Y(i + di, j + dj):
 *     gx = (((3 x(-1,1) + 10 x(0,1)) + 3 x(1,1)) - ((3 x(-1,-1) + 10 x(0,-1)) + 3 x(1,-1))) / 16
 *     gy = (((3 x(1,-1) + 10 x(1,0)) + 3 x(1,1)) - ((3 x(-1,-1) + 10 x(-1,0)) + 3 x(-1,1))) / 16
 *     (conv2(Y, [3 0 -3; 10 0 -10; 3 0 -3] / 16, 'same') and its transpose);  q = gx^2 + gy^2
 *     S_G = (2 sqrt(q_r q_d) + 160) / ((q_r + q_d) + 160)   (vqa_mdsi_submit's form: equal inputs give exactly 1)
 *   S_PC = (2 (PC_r PC_d) + 0.85) / ((PC_r^2 + PC_d^2) + 0.85), PC_m = max(PC_r, PC_d), S_L = S_G S_PC.
 *   Chroma.  S_I = (2 (I_r I_d) + 200) / ((I_r^2 + I_d^2) + 200), S_Q likewise; x = S_I S_Q; C = |x|^0.03 for x >= 0 and
 *     |x|^0.03 cos(0.03 pi) for x < 0 (the real part of the complex power the file takes).
 *   FSIM = sum S_L PC_m / sum PC_m;  FSIMc = sum S_L C PC_m / sum PC_m.  (fsim of a colour input is the authors' FSIM on Y.)
 * How the device rounds.  Everything in double, contraction off, in the order written.  The transforms are dense DFTs, complex
 *   matrix products on the fp64 matrix cores with the twiddle matrices W_n[j][k] = exp(-2 pi i (j k mod n) / n) formed in double on
 *   the host: F = W_h (X W_w), EO = (conj(W_h) (F filt)) conj(W_w) / N, every output a sum over k IN ORDER (a matrix instruction
 *   adds four k at a time), so it does not depend on the batch.  Then TWO roundings:
 *     p = rint(PC 2^24) ONCE, a uint32 map per image; from there on everything is a function of the two maps and of the input;
 *     with PC = p 2^-24: g = rint(S_L 2^24), gc = rint((S_L C) 2^24) (signed), pm = max(p_r, p_d).
 *   The three 64-bit words P = sum pm, A = sum (g pm + 2^23) >> 24, B = sum (gc pm + 2^23) >> 24 (an arithmetic shift) are added
 *   as integers: no overflow for N <= 2^28, and no dependence on tiling, batch or the order in which workgroups retire.
 *   vqa_fsim_wait forms fsim = A / P and fsimc = B / P in double.  Identical frames give g = gc = 2^24 (2 (p p) = p p + p p,
 *   sqrt(q q) = q, 1^0.03 = 1), so A = B = P and both scores are exactly 1.0.  P = 0 (structureless frames, flat against flat
 *   included) gives 1.0, 1.0 and bit 0 of flags; never a NaN.
 * Kernels, per sub-slice of frames: k_fsim_luma (MDSI's box stage: Y, I, Q as doubles), k_fsim_dft (the matrix product, 2 + 8
 *   launches), k_fsim_energy (4), k_fsim_median (the exact median by radix selection on the bit patterns), k_fsim_pc, k_fsim_pool.
 *   Scratch on the device: 24 bytes per frame for the words, the maps at 8 bytes and the intermediates at 560 bytes per downsampled
 *   sample per frame; a batch goes out in sub-slices of frames that keep the intermediates within 256 MiB.  The tables of a
 *   geometry (16 N + 2 hd^2 + 2 wd^2 doubles) are cached by the ctx.  All of it is kept until vqa_trim / vqa_destroy.  The dense
 *   DFT is a first version: FFT passes for 2-3-5-smooth grids are the next step.
 * Limits: plane 0 at least 16 x 16, h w <= 2^28 and max(hd, wd) <= 1024: VQA_ERR_UNSUPPORTED beyond any of these.  Every
 *   VQA_ERR_INVALID / VQA_ERR_STATE rule of vqa_mdsi_submit applies, and its contract: asynchronous, ONE ENTRY PER FRAME, the same
 *   descriptors, memory kinds and failure guarantee.  An FSIM batch is a batch of its own, next to every other kind; a batch of
 *   more than 32768 frames goes out in slices.
 * Not built: PU21-FSIM, a per-plane FSIM, FFT passes, any fp32 or bf16 transform.
 * out of vqa_fsim_wait: n entries (n_entries = n).                                                                         */
enum vqa_fsim_model { VQA_FSIM_YUV709 = 0, VQA_FSIM_BGR = 1, VQA_FSIM_GRAY = 2 };
VQA_API int vqa_fsim_submit(vqa_ctx *ctx, const uint8_t *ref, const uint8_t *dist, int mem_kind, int n,
                            int64_t ref_frame_stride, int64_t dist_frame_stride, const vqa_plane_desc *planes, int n_planes,
                            int model);
VQA_API int vqa_fsim_wait(vqa_ctx *ctx, vqa_fsim_metrics *out, int n_entries);
/* c_o of an hd x wd grid as stated above, in double on the host; needs no ctx and no device (NaN for hd or wd outside 2..1024 or
 * orient outside 0..3)                                                                                                      */
VQA_API double vqa_fsim_noise_factor(int hd, int wd, int orient);
/* filt_{scale,orient} of an hd x wd grid into dst[hd wd], row-major, in double on the host; VQA_ERR_INVALID for the same
 * arguments or a null dst                                                                                                   */
VQA_API int vqa_fsim_filter(int hd, int wd, int scale, int orient, double *dst);
/* LAB BUILD ONLY (vqa_build_flavour() & 2; declared only when VQA_TEST_SEAMS is defined): the p maps of the LAST vqa_fsim_submit of
 * the ctx, [n][2][hd][wd] uint32 (ref, then dist), after its wait; n_values = n 2 hd wd.  There, too, VQA_FSIM_SUBSLICE in the
 * environment shortens a sub-slice to a given number of frames, so that a small batch spans several.                        */
#ifdef VQA_TEST_SEAMS
    VQA_API int vqa_fsim_lab_read_maps(vqa_ctx *ctx, uint32_t *dst, int64_t n_values);
#endif

/* ---- Signal statistics and the words QC events are made of: what FFmpeg's signalstats, blackframe, freezedetect, scdet and
 * cropdetect answer - is the frame black, is the picture frozen, where are the cuts, is it letterboxed, are the levels legal, is
 * this "10-bit" stream 8-bit content shifted left ----
 * ONE stream, every plane by itself, frame i with its predecessor i - 1 as halo, like vqa_siti_submit; packed bgr24 planes work as
 * they do there.  Every word is an integer function of the samples.  Where this text differs from a tool's detail, this text is
 * what is built.
 * For one plane of h x w samples, N = h w:  x are the raw integer samples, d = depth, s = 2^(d-8).  The histogram covers the SAMPLE
 *   TYPE, not the depth: 256 bins for uint8 planes, 65536 for uint16 planes; a uint16 sample above 2^d - 1 is read as it is, as
 *   elsewhere in this header.  C(v) = #{x <= v}.  x' is the same plane of the frame before: frame i - 1 of the batch, prev0 for
 *   frame 0, the previous slice's last frame past 32768 frames.
 *   count        N
 *   sum, sum_sq  sum x, sum x^2 (uint64)
 *   min, max     the smallest and the largest sample
 *   low, median, high   the smallest v with C(v) >= k, k = (N + 9) / 10, (N + 1) / 2, (9 N + 9) / 10 in integer division: exact
 *                order statistics (FFmpeg's lrint ranks differ by rounding)
 *   below_black  #{x < black_level}; default black_level = 32 s, blackframe's threshold
 *   under, over_luma, over_chroma   #{x < 16 s}, #{x > 235 s}, #{x > 240 s}: all three for every plane; the host picks the ones
 *                that apply to the plane's role
 *   above_peak   #{x > 2^d - 1}; always 0 for uint8
 *   or_mask, and_mask   the bitwise OR and AND of all samples; bits_used = d - ctz(or_mask), 0 for an all-zero plane (the host)
 *   sad, changed sum |x - x'|, #{x != x'}; both 0 for a frame with no predecessor
 *   top, bottom, left, right (int32)   row r is dark iff sum_x x[r][.] <= crop_level w, column c is dark iff sum_y x[.][c] <=
 *                crop_level h: integer compares; default crop_level = 24 s, cropdetect's limit.  top and bottom are the first and
 *                the last row that is not dark, left and right likewise for columns; an all-dark plane gives top = h, bottom = -1,
 *                left = w, right = -1.
 *   vqa_sigstats_wait forms three doubles on the host, in sample units, in the order written and without contraction:
 *   mean = sum / N;  stdev = sqrt(max(sum_sq / N - mean mean, 0));  dif = sad / N.
 * Limits: every plane at least 16 x 16; N <= 2^28 for uint8 and N <= 2^26 for uint16 planes (vqa_siti_submit's rule):
 *   VQA_ERR_UNSUPPORTED beyond either.  0 <= black_level, crop_level <= 65535, a NEGATIVE level means the default; a level above
 *   65535 is VQA_ERR_INVALID.
 * Why no word can overflow inside the limits.  Every histogram counter is 32 bits and holds at most N <= 2^28 - a flat plane puts
 *   all N samples into ONE bin, so a packed 16-bit counter would be wrong from 65536 samples on.  sum <= 2^28 255 < 2^36 (uint8) and
 *   <= 2^26 65535 < 2^42 (uint16); sum_sq <= 2^28 255^2 < 2^44 and <= 2^26 65535^2 < 2^58; sad <= sum's bound; a row or a column sum
 *   is at most 2^24 65535 < 2^40 (a side is at most N / 16), and so is crop_level w or crop_level h: all inside 64 bits.  The counts
 *   are at most N.
 * The usual guarantee: a frame with its predecessor gives the same record bytes at any place of any batch, from host, pinned or
 *   device memory, alone or next to other kinds.  The kernels do integer adds, min, max, or and compares only - no floating point
 *   on the device - and all of these are associative and commutative, so neither the tiling nor the order in which workgroups
 *   retire can change a bit.
 * Kernels, per sub-slice of frames: k_sigstats_accum, tiled, reads every sample of the frame and of its predecessor once, builds
 *   the entry's histogram (uint8: in shared memory, then 32-bit global atomics per non-empty bin; uint16: 32-bit global vector
 *   atomics into the entry's 65536 bins in scratch), adds sad and changed, ORs the masks and adds the row and column sums into a
 *   profile of h + w uint64 words per entry; k_sigstats_scan, one workgroup per (frame, plane), walks the histogram once for every
 *   other word and reads the box off the profile.
 *   Scratch on the device: 168 bytes of words and 8 (h + w) bytes of profile per entry for the whole batch, and the histograms of
 *   one sub-slice: 1 KiB (uint8) or 256 KiB (uint16) per entry; a batch goes out in sub-slices of frames that keep the histograms
 *   within 256 MiB.  Frames handed over in host memory (and prev0) are staged in the device buffers an SI/TI batch uses.  All of
 *   it is kept by the ctx until vqa_trim / vqa_destroy.
 * The contract of vqa_siti_submit for the stream and prev0, for memory kinds, depths (one per submit) and alignment, and its
 *   failure guarantee: a failed submit leaves nothing in flight.  VQA_ERR_STATE while a sigstats batch is pending.  A sigstats
 *   batch is a batch of its own: it may be in flight next to every other kind of the same ctx, and each wait collects its own kind
 *   only.  A batch of more than 32768 frames goes out in slices.
 * vqa_sigstats_wait: out holds n * n_planes entries, frame-major.  With profiles != 0, profile_words receives the profiles: for
 *   every frame, for every plane in order, its h row sums and then its w column sums (n_profile_words = n sum_p (h_p + w_p)); a
 *   wrong word count or a null pointer is VQA_ERR_INVALID and the batch stays pending.  With profiles == 0 both are ignored.
 * Not built: signalstats' TOUT, VREP, saturation and hue; durations in seconds; cropdetect's rounding of the box; a joint-pixel
 *   BRNG.                                                                                                                     */
VQA_API int vqa_sigstats_submit(vqa_ctx *ctx, const uint8_t *frames, const uint8_t *prev0, int mem_kind, int n,
                                int64_t frame_stride, const vqa_plane_desc *planes, int n_planes, int black_level,
                                int crop_level);
VQA_API int vqa_sigstats_wait(vqa_ctx *ctx, vqa_sigstats_metrics *out, int n_entries, int profiles, uint64_t *profile_words,
                              int64_t n_profile_words);

/* ---- The resampler: the distorted stream of a ladder rung brought to the reference's size on the device, what
 * `[dist]scale=1920:1080:flags=bicubic` does before libvmaf in an FFmpeg graph - so a 360p, 540p or 720p encode is uploaded at its
 * own size and every kind above measures it at the source's ----
 * It is Pillow's Image.resize for 8-bit images, an exact fixed-point algorithm, carried unchanged to 9..16 bits.  Where this text
 * differs from a tool's detail, this text is what is built.
 * Plane i of src_planes is resampled into plane i of dst_planes, each plane by itself, the horizontal pass first and the vertical
 * pass second.
 * Tables, per axis, with `in` source samples, `out` destination samples, scale = in / out, fs = max(scale, 1), S the filter's
 *   support: support = S fs; ksize = 2 ceil(support) + 1; for output x the centre is c = (x + 0.5) scale,
 *   xmin = max(0, (int)(c - support + 0.5)), xmax = min(in, (int)(c + support + 0.5)), count = xmax - xmin; the weights are
 *   w_j = f((j + xmin - c + 0.5) / fs), j = 0 .. count - 1, added in index order and each divided by that sum (a window that runs
 *   off the plane is cut and renormalised: nothing is mirrored or padded); each weight is quantised ONCE,
 *   k_j = (int)(w_j 2^22 + 0.5), or - 0.5 for a negative weight, the conversion truncating towards zero (Pillow's
 *   normalize_coeffs_8bpc).  All of it in double, in the order written, without contraction.  vqa_scale_tables builds them.
 * Filters: VQA_SCALE_BILINEAR, S = 1, the triangle 1 - |x|; VQA_SCALE_BICUBIC, S = 2, Keys' cubic with a = -0.5 written as Pillow
 *   writes it, ((a + 2) x - (a + 3)) x x + 1 for |x| < 1 and (((x - 5) x + 8) x - 4) a for |x| < 2; VQA_SCALE_LANCZOS, S = 3,
 *   sinc(x) sinc(x / 3) on [-3, 3) with sinc(x) = sin(pi x) / (pi x), sinc(0) = 1.
 * Passes: out = clip((2^21 + sum_j k_j in[xmin + j]) >> 22, 0, peak), an arithmetic shift, peak = 2^depth - 1.  The horizontal
 *   pass is clipped and stored at the sample type before the vertical pass reads it, as Pillow does at 8 bits.  For uint8
 *   samples the sums fit 32 bits (255 sum |k| < 2^31); for uint16 samples they are 64-bit.  An axis whose size does not change is
 *   copied, not filtered (its tables are the identity in any case): a copied horizontal axis hands the samples to the vertical
 *   pass as they are, above peak included; what leaves the vertical pass, copied or filtered, is clipped to peak.
 * Consequences: a flat plane stays flat at every level, 0 and peak included (a row of k misses 2^22 by at most ksize / 2 units,
 *   far below what moves the floor of (2^21 + v sum k) 2^-22); the output at depth d never exceeds 2^d - 1, even where the input
 *   did.  Against Pillow: equal at every sample in mode L; in mode I;16 Pillow filters in double, so the two differ by at most
 *   one unit a pass where no pass leaves 0 .. 65535 - where one does, Pillow saturates the high byte only and this text clips.
 * Chroma is resampled over its own grid with the same centres, i.e. it is centre-sited.
 * Limits: 1 .. 4 planes, the same count and one depth (8, or 9 .. 16) in both lists; every plane of both lists at least 16 x 16
 *   with h w <= 2^28; per axis 1/4 <= out / in <= 8, so ksize <= 25: VQA_ERR_UNSUPPORTED beyond any of these (and for 8-bit planes
 *   whose tables had a row with 255 sum |k| + 2^21 >= 2^31: none is known, the submit checks the tables it builds).  pixel_step > 1
 *   works on either side (packed bgr24 is three planes).  An unknown filter, a dst that is not device memory of the ctx's
 *   device, and a destination range [dst, dst + (n - 1) dst_frame_stride + the span of dst_planes) that overlaps the source
 *   frames are VQA_ERR_INVALID.  The bytes of dst that no destination sample covers (row and frame padding) are not written.
 * frames: host, pinned or device memory, like vqa_cambi_submit; host frames are staged in a buffer of this kind's own.
 * A scale batch is a batch of its own (no result words): asynchronous on the ctx's stream, VQA_ERR_STATE while one is pending,
 *   in flight next to every other kind; a failed submit leaves nothing in flight; more than 32768 frames go out in slices.
 *   Every submit of any kind on the SAME ctx that follows reads dst after the resampler has written it - the stream orders them;
 *   no wait is needed in between.  vqa_scale_wait returns when dst is complete (another ctx, or the host, may then read it).
 * The kernel has no atomics and no reduction: the same frame gives the same bytes at any place of any batch, from any memory.
 * Kernel: k_scale, one fused launch per group of planes alike on both sides; the intermediate of the horizontal pass lives in
 *   shared memory only.  The tables sit in device memory per (filter, in, out), cached like the other per-geometry tables.
 * Not built: swscale's bicubic (a = -0.6) and its other flags; left-sited (MPEG-2) chroma; scaling the reference; ratios beyond
 *   1/4 .. 8.  Conversion between chroma layouts or depths is vqa_convert_submit's.                                          */
enum vqa_scale_filter {
    VQA_SCALE_BILINEAR = 0,
    VQA_SCALE_BICUBIC = 1,
    VQA_SCALE_LANCZOS = 2
};
VQA_API int vqa_scale_submit(vqa_ctx *ctx, const uint8_t *frames, int mem_kind, int n, int64_t frame_stride,
                             const vqa_plane_desc *src_planes, uint8_t *dst, int64_t dst_frame_stride,
                             const vqa_plane_desc *dst_planes, int n_planes, int filter);
VQA_API int vqa_scale_wait(vqa_ctx *ctx);
/* One axis' tables on the host.  *ksize receives the row length of k (at most 25); with k, xmin and count all non-NULL they
 * receive k[out][ksize] (0 past count), xmin[out] and count[out]; all three NULL asks for ksize alone.  An unknown filter, a
 * non-positive size, ksize == NULL or some but not all of the arrays: VQA_ERR_INVALID; a ratio beyond 1/4 .. 8:
 * VQA_ERR_UNSUPPORTED.  in == out gives the formula's tables, which are the identity.                                         */
VQA_API int vqa_scale_tables(int filter, int in, int out, int32_t *k, int32_t *xmin, int32_t *count, int *ksize);

/* ---- Conform: the registration that align, sync, shift and colorfit FIND, applied on the device ----
 * One input stream, one output stream: out[j][p][y][x] is a function of in[index[j]][p][y0_p + y][x0_p + x].  A pair is conformed
 * by two submits.  Everything is integer arithmetic; where this text differs from a tool's detail, this text is what is built.
 * frames: n_in frames described by src_planes, one to four planes of one depth (8, or 9 .. 16), any offset, row stride and pixel
 *   step (packed bgr24 is three planes); host, pinned or device memory, what vqa_scale_submit takes on its input side.
 * dst_planes: the same plane count and depth, sizes (oh_p, ow_p), strides and pads of their own: plane 0 at least 16 x 16, the
 *   others at least 8 x 8 (the chroma of a 16 x 16 4:2:0 frame), h w <= 2^28: VQA_ERR_UNSUPPORTED beyond.
 * origin: NULL (all zero) or [n_planes][2] = (y0_p, x0_p), the window's corner in source plane p; y0_p + oh_p <= h_p and
 *   x0_p + ow_p <= w_p, else VQA_ERR_INVALID.
 * index: NULL (identity, n_out is taken as n_in) or n_out source frames, 0 <= index[j] < n_in, in any order, repeats allowed: a
 *   constant offset, a drop, a repeat, or vqa_align's path.  n_out <= 32768, VQA_ERR_UNSUPPORTED beyond.
 * lut: NULL or [n_planes][2^depth] entries of the sample type, each at most peak = 2^depth - 1 (else VQA_ERR_INVALID), applied
 *   first: s_p = lut[p][min(sample, peak)] (a sample above the peak is no code of the depth; it reads the peak's entry).
 * matrix: NULL or int64 [3][4] in 2^-16 fixed point, three planes only; |M[k][i]| <= 2^20 for i < 3, |M[k][3]| <= 2^33, else
 *   VQA_ERR_INVALID.  The source planes follow the joint rule of vqa_ciede_submit (planes 1 and 2 alike; the size of plane 0 or
 *   its ceil-half per axis), sy, sx the chroma shifts that gives.  Stated in SOURCE coordinates:
 *     plane 0 at (Y, X):   t_0 = clip((M00 s_0(Y, X) + M01 s_1(cy, cx) + M02 s_2(cy, cx) + M03 + 2^15) >> 16, 0, peak) with
 *       cy = min(Y >> sy, h_c - 1), cx = min(X >> sx, w_c - 1): chroma replicated, the convention of colorfit, ciede and itp;
 *     planes k = 1, 2 at (Cy, Cx): t_k = clip((Mk0 Ybar + Mk1 s_1(Cy, Cx) + Mk2 s_2(Cy, Cx) + Mk3 + 2^15) >> 16, 0, peak), Ybar
 *       the rounded mean (sum + cnt / 2) / cnt of the luma samples s_0 of the source cell rows (Cy << sy) .., columns
 *       (Cx << sx) .. that exist, so cnt is 1, 2 or 4; in 4:4:4 and bgr24 the cell is one sample.
 *   >> is an arithmetic shift on 64-bit values.  Without a matrix t_p = s_p.
 * Output: out[j][p][y][x] = t_p at source sample (y0_p + y, x0_p + x) of frame index[j].  The bytes of dst that no destination
 *   sample covers (row and frame padding) are never written.  dst must be device memory of the ctx's device and must not
 *   overlap the source frames (VQA_ERR_INVALID).
 * A conform batch is a batch of its own (no result words) with the resampler's slot semantics: VQA_ERR_STATE while one is
 *   pending, in flight next to every other kind; every submit of any kind on the SAME ctx that follows reads dst after it has
 *   been written - the stream orders them; vqa_conform_wait is needed only before another ctx or the host reads dst.  The
 *   caller's origin, index, lut and matrix are free when the submit returns.
 * No atomics: the same input gives the same bytes in any batch, from any memory.  It takes no kernel id (like
 *   vqa_colorfit_submit): an added entry point, not a layout change, VQA_ABI_VERSION stays.
 * Kernels (k_conform.hip): k_conform_copy - a lane a 16-byte granule of the destination, the source loaded as aligned 16-byte
 *   words and realigned in registers, the tables in LDS up to 12 bits; k_conform_gather - a lane a sample, for a pixel step that
 *   is neither contiguous nor interleaved alike on both sides; k_conform_matrix - a lane a 2 x 4 patch of source cells.
 * Not built: interpolation (sub-pixel shifts, chroma of an odd shift on a subsampled axis); a matrix for other than three
 *   planes.  Conversion between layouts or depths is vqa_convert_submit's.                                                   */
VQA_API int vqa_conform_submit(vqa_ctx *ctx, const uint8_t *frames, int mem_kind, int n_in, int64_t frame_stride,
                               const vqa_plane_desc *src_planes, uint8_t *dst, int64_t dst_frame_stride,
                               const vqa_plane_desc *dst_planes, int n_planes, const int32_t *origin, const int32_t *index,
                               int n_out, const void *lut, const int64_t *matrix);
VQA_API int vqa_conform_wait(vqa_ctx *ctx);

/* ---- Convert: one stream written at another sample depth and / or chroma layout on the device - what an auto-inserted
 * `format=` does in an FFmpeg graph, so a 10-bit 4:2:2 mezzanine is measured against its 8-bit 4:2:0 encode (or an 8-bit rung
 * against a 10-bit master) with the distorted stream uploaded as it is ----
 * Plane i of src_planes goes into plane i of dst_planes, each plane by itself.  Everything is integer arithmetic with ONE
 * rounding per output sample.  Where this text differs from a tool's detail, this text is what is built.
 * Planes: 1 to 4, the same count on both sides; one depth per list (8, or 9 .. 16 as little-endian uint16): ds on the source
 *   side, dd on the destination side.  On both sides plane 0 is at least 16 x 16, the others at least 8 x 8, and h w <= 2^28:
 *   VQA_ERR_UNSUPPORTED beyond.  Per plane and per axis, with n_s source and n_d destination samples, the relation is one of
 *     same: n_d == n_s;    up: n_s == (n_d + 1) >> 1 (a 2x upsample: n_d is 2 n_s or 2 n_s - 1);    down: n_d == (n_s + 1) >> 1;
 *   any other relation is VQA_ERR_UNSUPPORTED.  Plane 0 of the layouts this project builds is always `same`; the rule is per
 *   plane, not per role.
 * Taps, per axis; the weights sum to 4 and c(i) = min(max(i, 0), n_s - 1) replicates the edge:
 *     relation     VQA_CHROMA_BOX                VQA_CHROMA_LINEAR, centre-sited    VQA_CHROMA_LINEAR, left-sited (horizontal only)
 *     same         4 s[x]                        4 s[x]                             4 s[x]
 *     up, x even   4 s[x>>1]                     3 s[x>>1] + s[c((x>>1) - 1)]       4 s[x>>1]
 *     up, x odd    4 s[x>>1]                     3 s[x>>1] + s[c((x>>1) + 1)]       2 s[x>>1] + 2 s[c((x>>1) + 1)]
 *     down         2 s[2x] + 2 s[c(2x + 1)]      the same                           s[c(2x - 1)] + 2 s[2x] + s[c(2x + 1)]
 *   The vertical axis is always centre-sited (the MPEG-2 / H.264 default for 4:2:0); siting (VQA_SITING_CENTER,
 *   VQA_SITING_LEFT) changes the horizontal axis of VQA_CHROMA_LINEAR only.  VQA_CHROMA_BOX is the convention the joint kinds
 *   already use: chroma replicated on the way up, the mean of the cell's existing samples on the way down (conform's Ybar
 *   rule).  The horizontal taps are applied first, then the vertical ones, with NO rounding in between: v is the exact integer
 *   with denominator 16, v <= 16 * 65535.
 * Depth and range, then the one rounding, in 64-bit arithmetic with Ps = 2^ds - 1, Pd = 2^dd - 1:
 *   VQA_RANGE_LIMITED keeps the code's meaning by a power of two (16 becomes 64, 235 becomes 940):
 *     dd >= ds: out = ((v << (dd - ds)) + 8) >> 4;      dd < ds: out = (v + (1 << (3 + ds - dd))) >> (4 + ds - dd);
 *   VQA_RANGE_FULL rescales by the peaks: out = (2 v Pd + 16 Ps) / (32 Ps), an integer division: v Pd / (16 Ps) rounded half up.
 *   Both are then clipped to Pd.  A source sample above Ps is read as it is; only the output is clipped.
 * Consequences: equal formats give the identity; a flat plane stays flat at every level, 0 and the peak included; at an
 *   unchanged layout ds -> dd -> ds with dd >= ds returns every code of the depth under both ranges; VQA_RANGE_FULL maps 0 to 0
 *   and Ps to Pd.
 * Pinned: the centre-sited linear taps equal torch's bilinear interpolation (scale 2, align_corners false) and the down taps
 *   equal its 2 x 2 average pooling, both times 16, exactly; the rest by hand-computed answers and a NumPy restatement of this
 *   text.  NOT pinned: FFmpeg's swscale is not matched - it dithers on the way down and uses other chroma filters - and no
 *   FFmpeg binary was at hand to compare with.
 * frames: host, pinned or device memory, what vqa_scale_submit takes; host frames are staged in a buffer of this kind's own.
 *   n <= 32768, VQA_ERR_UNSUPPORTED beyond.  dst is device memory of the ctx's device and does not overlap the source frames,
 *   else VQA_ERR_INVALID; an unknown chroma filter, siting or range is VQA_ERR_INVALID.  The bytes of dst that no destination
 *   sample covers (row, plane and frame padding) are never written.
 * A convert batch has conform's slot semantics exactly: a batch of its own with no result words, asynchronous on the ctx's
 *   stream, VQA_ERR_STATE while one is pending, in flight next to every other kind; a failed submit leaves nothing in flight;
 *   every later submit of any kind on the SAME ctx reads dst after it is written - no wait is needed in between;
 *   vqa_convert_wait is needed only before another ctx or the host reads dst.
 * No atomics, no reduction: a frame gives the same bytes at any place of any batch, from any memory.  It takes no kernel id
 *   (like vqa_conform_submit): an added entry point, not a layout change, VQA_ABI_VERSION stays.
 * Kernels (k_convert.hip): k_convert_rows - a pixel step equal to the sample size on both sides: a lane owns a 16-byte granule of
 *   the destination's address (in both destination rows fed by the same source rows where the vertical relation is up and the
 *   rows share a phase), the source loaded as aligned 16-byte words and realigned in registers, the ends of a row written
 *   sample by sample; k_convert_gather - the same function, a lane a sample, for any other pixel step.
 * Not built: packed bgr24 to or from planar YUV (a colour-matrix question); mono to or from three planes; dither; swscale's
 *   filters; chroma ratios other than 1 and 2; converting the reference of a pass; the pair-reading pre-passes on a mixed pair. */
enum vqa_convert_chroma {
    VQA_CHROMA_BOX = 0,
    VQA_CHROMA_LINEAR = 1
};
enum vqa_convert_siting {
    VQA_SITING_CENTER = 0,
    VQA_SITING_LEFT = 1
};
enum vqa_convert_range {
    VQA_RANGE_LIMITED = 0,
    VQA_RANGE_FULL = 1
};
VQA_API int vqa_convert_submit(vqa_ctx *ctx, const uint8_t *frames, int mem_kind, int n, int64_t frame_stride,
                               const vqa_plane_desc *src_planes, uint8_t *dst, int64_t dst_frame_stride,
                               const vqa_plane_desc *dst_planes, int n_planes, int chroma, int siting, int range);
VQA_API int vqa_convert_wait(vqa_ctx *ctx);

/* ---- Fields: is this stream interlaced, in which field order, and which fields repeat?  And weave: frames out of fields ----
 * Every kind above takes both streams as progressive pictures at one cadence.  This kind measures that for ONE stream - the
 * question FFmpeg's idet filter answers - and vqa_weave_submit builds frames out of the fields of other frames, which is what
 * inverse telecine, forward telecine of a reference and the test clips need.
 * Input: ONE plane descriptor (the luma of planar YUV, the gray plane, G of packed bgr24 through pixel_step 3, or whatever single
 *   plane the caller describes).  bit_depth 8 (0), or 9 .. 16 as little-endian uint16; samples are read as they are.  Any
 *   offset, row_stride and pixel_step the other kinds accept; a plane whose pixel_step is not its sample size takes a gather,
 *   THE SLOW PATH, which gives the same words, as in vqa_sig_submit.  Host, pinned or device memory.
 * Definition: frame i has samples c; its predecessor p is frame i - 1 of the submit, or prev0 for frame 0.  With f = y & 1 (0: the
 *   top field's rows, 1: the bottom field's):
 *     comb[f]    = sum |c[y-1][x] + c[y+1][x] - 2 c[y][x]|   over 2 <= y < h - 2 with y & 1 == f, all x
 *     fwd[f]     = sum |c[y-1][x] + c[y+1][x] - 2 p[y][x]|   over the same rows
 *     bwd[f]     = sum |p[y-1][x] + p[y+1][x] - 2 c[y][x]|   over the same rows
 *     sad[f]     = sum |c[y][x] - p[y][x]|                   over ALL rows with y & 1 == f
 *     changed[f] = the number of samples with c != p         over ALL rows with y & 1 == f
 *     count      = (h - 4) w;  has_prev = 1 with a predecessor, else 0
 *   Without a predecessor (frame 0 with prev0 == NULL) fwd, bwd, sad and changed are 0 and has_prev is 0.  fwd of frame t and
 *   bwd of frame t + 1 are together the two temporal terms idet forms at frame t from its `prev` and `next`; split this way the
 *   kind needs one frame of halo, which every windowed walk here already carries.
 * What follows: every word is an exact integer function of the samples of the frame and its predecessor alone: the same frame
 *   gives the same words in any batch, in any window, from any memory.  A frame equal to its predecessor has sad = changed = 0
 *   and fwd = bwd = comb.  Bounds: a term is at most 4 * 65535, so a sum over h w <= 2^28 samples stays below 2^46.
 * The classification (rtvqa_amd/fields.py, pure host, integers and exact fractions) applies idet's rule with its default
 *   thresholds 1.04 and 1.5 AS RECALLED: it is NOT pinned against FFmpeg, no binary being at hand.  Pinned: hand-computed
 *   answers and a NumPy restatement of this text.
 * Limits: the plane at least 16 x 16 with h w <= 2^28, VQA_ERR_UNSUPPORTED otherwise; n <= 32768 per submit.  The descriptor
 *   rules, memory kinds and the failure guarantee are vqa_sig_submit's.  A fields batch is a batch of its own: VQA_ERR_STATE
 *   for a second submit while one is pending and for a wait without a submit or with another n; in flight next to every other
 *   kind.  Host frames and prev0 are staged in buffers of this kind's own.
 * Kernel (k_fields.hip): k_fields_accum - a lane owns a 16-byte column chunk of a band of 32 rows, marches down it with rows
 *   y - 1, y, y + 1 of both frames in registers (two reads per sample), aligned 16-byte loads realigned in registers, row ends
 *   and the gather sample by sample; 64-bit partials, a wave reduction, one 64-bit atomic add per word and workgroup.  No
 *   kernel id (like vqa_convert_submit): an added entry point, not a layout change, VQA_ABI_VERSION stays.
 * Not built: idet's multi-frame history verdict; more than one plane in the measurement. */
VQA_API int vqa_fields_submit(vqa_ctx *ctx, const uint8_t *frames, const uint8_t *prev0, int mem_kind, int n, int64_t frame_stride,
                              const vqa_plane_desc *plane);
VQA_API int vqa_fields_wait(vqa_ctx *ctx, vqa_fields_metrics *out, int n);

/* Weave: out[j][p][y][x] = in[(y & 1 ? bottom_index : top_index)[j]][p][y][x] for every plane p of the list: the even rows of
 * output frame j come from source frame top_index[j], the odd rows from source frame bottom_index[j].  src_planes and dst_planes
 * describe the same planes (count, depth, widths and heights) with their own offsets, strides and pads; one to four planes, 8 or
 * 9 .. 16 bits, 4:2:0 / 4:2:2 / 4:4:4 / mono / packed bgr24 (whose three planes go out as one).  The row parity is the plane's
 * own: chroma row y of 4:2:0 belongs to field y & 1 of the chroma plane, as in an interlaced 4:2:0 frame.
 * frames: n_in frames in host, pinned or device memory; host frames are staged in a buffer of this kind's own.  dst: device
 *   memory of the ctx's device that does not overlap the source frames, else VQA_ERR_INVALID; an index outside 0 .. n_in - 1
 *   is VQA_ERR_INVALID; both are checked before anything is launched.  Plane 0 at least 16 x 16, the others 8 x 8, else
 *   VQA_ERR_UNSUPPORTED; n_out <= 32768.  The bytes of dst that no sample covers are never written.  The two index arrays are
 *   the caller's again when the submit returns.
 * A weave batch has conform's slot semantics exactly: no result words, VQA_ERR_STATE while one is pending, every later submit
 *   of any kind on the SAME ctx reads dst after it is written; vqa_weave_wait is needed only before another ctx or the host
 *   reads dst.  No atomics: a frame gives the same bytes at any place of any batch.  No kernel id.
 * Kernels (k_fields.hip): k_fields_weave on k_conform_copy's plan (aligned 16-byte destination granules, aligned source words
 *   realigned in registers, row ends sample by sample); k_fields_weave_gather, a lane a sample, for other pixel steps.
 * Not built: deinterlacing (bob, yadif); cadences other than 3:2 in the host's plans. */
VQA_API int vqa_weave_submit(vqa_ctx *ctx, const uint8_t *frames, int mem_kind, int n_in, int64_t frame_stride,
                             const vqa_plane_desc *src_planes, uint8_t *dst, int64_t dst_frame_stride,
                             const vqa_plane_desc *dst_planes, int n_planes, const int32_t *top_index, const int32_t *bottom_index,
                             int n_out);
VQA_API int vqa_weave_wait(vqa_ctx *ctx);

/* ---- Temporal alignment: is the distorted stream the same frames as the reference, in the same places? ----
 * Every full-reference kind above compares reference frame i with distorted frame i and trusts the caller that they belong
 * together.  This kind measures that: the squared error between distorted frame j and reference frame j + offset + k for every
 * k of a band -R .. R.  A dropped first frame, a repeated frame or a late start are read off the band by the host.
 * Input: ONE plane descriptor, applied to both streams - plane 0 of a layout: the luma of planar YUV, the gray plane, or whatever
 *   single plane the caller describes.  bit_depth 8 (0), or 9 .. 16 as little-endian uint16; samples above 2^depth - 1 are read
 *   as they are.  Any offset, row_stride and pixel_step the other kinds accept: rows that start at odd addresses, padded rows, a
 *   frame whose last row ends its allocation, and non-contiguous planes (pixel_step = 3: one channel of packed BGR) - the last
 *   through a gather, THE SLOW PATH, which gives the same words.  No byte beyond offset + (h - 1) row_stride + w pixel_step of a
 *   frame is read.  The streams have their own frame counts n_ref and n_dist and their own frame strides, and one mem_kind.
 * Parameters: radius R, 0 <= R <= VQA_ALIGN_MAX_RADIUS, and an integer offset (any value).
 * Output: sse[j][c], uint64, j = 0 .. n_dist - 1, c = 0 .. 2R, row-major, n_dist (2R + 1) words.  With k = c - R and
 *   i = j + offset + k: sse[j][c] = sum over the plane of (d_j - r_i)^2, exact, if 0 <= i < n_ref; VQA_ALIGN_NONE otherwise.
 * What follows: every word is an integer function of the samples of its two frames alone.  The same pair of frames gives the
 *   same word whatever else is in the submit, from host, pinned or device memory, for any offset / radius / windowing that covers
 *   it, alone or next to other kinds pending on the ctx.  Identical frames give exactly 0.
 * How: with X = x - s (s = 128 for uint8, 32896 for uint16: the same shift on both sides, so it cancels in the difference),
 *   sse = E_d[j] + E_r[i] - 2 C[j][i], E = sum X^2 per frame and C[j][i] = sum X_d,j X_r,i, a Gram matrix of frames over pixels on
 *   the int8 matrix cores; a uint16 X is 256 (hi - 128) + (lo - 128) and its products are four int8 products.  32-bit
 *   accumulators are added into 64-bit words before they can overflow (a product is at most 2^14; at most 2^16 of them are
 *   added between two flushes); |C| <= E <= 2^28 32896^2 < 2^59 and sse <= 2^28 65535^2 < 2^60.  Integer adds only: neither the
 *   tiling nor the order in which waves retire can change a bit.  vqa_align_wait forms sse and the VQA_ALIGN_NONE entries on
 *   the host; the caller gets finished words.
 * Limits: the plane at least 1 x 1 (this kind has no 16 x 16 floor) with h w <= 2^28; n_dist >= 1, n_ref >= 1; n_dist <= 32768
 *   and n_ref <= 32768 + 64 per submit, VQA_ERR_UNSUPPORTED beyond (a longer clip is measured in windows: distorted frames
 *   a .. b - 1 against reference frames max(a - R, 0) .. min(b + R, n) - 1 with offset = a - max(a - R, 0) give rows a .. b - 1 of
 *   the whole clip's array).  R outside 0 .. 32 is VQA_ERR_INVALID.  The descriptor rules, memory kinds and the failure
 *   guarantee are vqa_gmsd_submit's: a failed submit leaves nothing in flight; a frame stride smaller than the plane's span is
 *   VQA_ERR_INVALID for a stream of more than one frame.
 * An alignment batch is a batch of its own: VQA_ERR_STATE for a second submit while one is pending and for a wait without a
 *   submit or with a word count that is not n_dist (2R + 1) (the batch stays pending); in flight next to every other kind.
 *   Host frames are staged in the buffers the pair kinds share.  Scratch: 8 (n_dist (2R + 2) + n_ref) bytes on the device and
 *   pinned, kept by the ctx until vqa_trim / vqa_destroy.
 * Kernel: k_align_cross, ONE launch per submit.  Only 16 x 16 tiles of (distorted, reference) frames that meet the band are
 *   computed; the frames that pad a tile to 16 are not read.
 * Not built: a crop search (a spatial shift is vqa_shift_submit's); radii above 32; more than one plane; timestamps, frame-rate
 *   conversion; pulldown is not modelled here (vqa_fields_submit detects it, vqa_weave_submit undoes it). */
#define VQA_ALIGN_NONE UINT64_MAX
#define VQA_ALIGN_MAX_RADIUS 32
VQA_API int vqa_align_submit(vqa_ctx *ctx, const uint8_t *ref, int n_ref, const uint8_t *dist, int n_dist, int mem_kind,
                             int64_t ref_frame_stride, int64_t dist_frame_stride, const vqa_plane_desc *plane, int offset,
                             int radius);
VQA_API int vqa_align_wait(vqa_ctx *ctx, uint64_t *sse, int64_t n_words);   /* n_words == n_dist * (2 radius + 1) */

/* ---- Spatial registration: does the distorted picture sit where the reference picture sits? ----
 * Every full-reference kind above compares sample (y, x) of the reference with sample (y, x) of the distorted frame and trusts
 * the caller that the two pictures sit in the same place.  This kind measures that: the squared error between each distorted
 * frame and its reference frame for every integer shift (dy, dx) of a square band -R .. R.  A scaler with another siting, a crop
 * that is off by two or a capture with a one-line offset are read off the grid by the host.
 * Input: ONE plane descriptor, applied to both streams - plane 0 of a layout, or whatever single plane the caller describes.
 *   bit_depth 8 (0), or 9 .. 16 as little-endian uint16; samples above 2^depth - 1 are read as they are.  Any offset,
 *   row_stride and pixel_step vqa_align_submit accepts: rows that start at odd addresses, padded rows, a frame whose last row
 *   ends its allocation, and non-contiguous planes (pixel_step = 3: one channel of packed BGR) - the last through a gather,
 *   THE SLOW PATH, which gives the same words.  No byte beyond offset + (h - 1) row_stride + w pixel_step of a frame is read
 *   on either stream.  n frames per stream, frame j against frame j; each stream has its own frame stride; one mem_kind.
 * Parameters: radius R, 1 <= R <= VQA_SHIFT_MAX_RADIUS, and margin M >= R.
 * Output: sse[j][a][b], uint64, a = dy + R, b = dx + R, row-major, n (2R + 1)^2 words:
 *   sse[j][a][b] = sum over M <= y < h - M, M <= x < w - M of (d_j(y, x) - r_j(y + dy, x + dx))^2, exact.
 *   Every shift is summed over the SAME core of (h - 2M)(w - 2M) distorted samples: the entries of a grid are comparable
 *   without normalisation, and no sample outside the reference plane is ever needed, because M >= R.
 * The sign: a minimum at (dy, dx) says that the distorted picture shows at (y, x) what the reference shows at (y + dy, x + dx) -
 *   the picture has moved up by dy rows and left by dx samples on its way through the chain (down and right where they are
 *   negative), and the reference read at (y + dy, x + dx) is the frame to compare with.
 * What follows: every word is an integer function of the samples of its two frames, M and (dy, dx) alone.  The same pair gives
 *   the same word under any R that contains the shift at the same M, in any batch and at any position in it, from host, pinned
 *   or device memory, alone or next to other kinds pending on the ctx.  Identical frames give exactly 0 at (0, 0); a distorted
 *   frame that is the reference translated by (dy, dx) inside the core gives exactly 0 at that entry.
 * How: with X = x - s (s = 128 for uint8, 32896 for uint16: the same shift on both sides, so it cancels),
 *   sse(dy, dx) = E_d + E_r(dy, dx) - 2 C(dy, dx): E_d the core's sum of X_d^2, E_r(dy, dx) the sum of X_r^2 over the core moved
 *   by the shift, and C(dy, dx) = sum X_d(y, x) X_r(y + dy, x + dx), a cross-correlation taken as a Toeplitz product on the int8
 *   matrix cores: for a reference row y' and 64 core columns from x0 on, A[m][k] = X_d(y' - dy_m, x0 + k) (zero outside the core)
 *   and B[k][n] = X_r(y', x0 + k + dx_n), so one instruction adds 64 samples into a 16 (dy) x 16 (dx) tile of C; R <= 7 is one
 *   tile, R = 8 .. 15 four, R = 16 nine.  A uint16 X is 256 (hi - 128) + (lo - 128) and its products are four int8 products.
 *   E_r comes from the B operand cut to the core's columns, squared with the dot-product instruction, per reference row and dx,
 *   and added to the dy whose core holds that row: no second read of the plane.  32-bit accumulators are added into 64-bit words
 *   before they can overflow (a product is at most 2^14; at most 2^16 of them are added between two flushes); |C| <= E <=
 *   2^28 32896^2 < 2^59 and sse <= 2^28 65535^2 < 2^60.  Integer adds only: neither the tiling nor the order in which waves
 *   retire can change a bit.  vqa_shift_wait adds E_d on the host; the caller gets finished words.
 * Limits: h >= 2M + 1 and w >= 2M + 1 (a core of at least one sample), else VQA_ERR_UNSUPPORTED; h w <= 2^28; 1 <= n <= 32768
 *   per submit, VQA_ERR_UNSUPPORTED beyond (a longer clip is measured in windows).  R outside 1 .. 16 or M < R is
 *   VQA_ERR_INVALID.  The descriptor rules, memory kinds and the failure guarantee are vqa_align_submit's: a failed submit
 *   leaves nothing in flight; a frame stride smaller than the plane's span is VQA_ERR_INVALID for a stream of more than one
 *   frame.
 * A registration batch is a batch of its own: VQA_ERR_STATE for a second submit while one is pending and for a wait without a
 *   submit or with a word count that is not n (2R + 1)^2 (the batch stays pending); in flight next to every other kind.  Host
 *   frames are staged in the buffers the pair kinds share.  Scratch: 8 n ((2R + 1)^2 + 1) bytes on the device and pinned, kept
 *   by the ctx until vqa_trim / vqa_destroy.
 * Kernel: k_shift, ONE launch per submit.  Rows and columns that pad a tile beyond 2R + 1 are not read.
 * Not built: moving the pass by the found shift; a sub-pixel search on the GPU (the host fits a parabola to the integer grid);
 *   a per-plane or chroma-siting search; scale or rotation; a shift search combined with the temporal band; radii above 16. */
#define VQA_SHIFT_MAX_RADIUS 16
VQA_API int vqa_shift_submit(vqa_ctx *ctx, const uint8_t *ref, const uint8_t *dist, int n, int mem_kind, int64_t ref_frame_stride,
                             int64_t dist_frame_stride, const vqa_plane_desc *plane, int radius, int margin);
VQA_API int vqa_shift_wait(vqa_ctx *ctx, uint64_t *sse, int64_t n_words);   /* n_words == n * (2 radius + 1)^2 */

/* ---- HDR light levels and gamut QC: MaxCLL / MaxFALL (CTA-861.3), per-frame light statistics, and "is this BT.2020 container
 * wider than BT.709 or P3?", ONE stream, three planes jointly ----
 * dE_ITP and PU21 score an HDR encode against its source; sigstats answers the QC questions of an SDR signal.  This kind answers
 * the two every HDR10 delivery answers before it ships: the largest max(R, G, B) of any pixel and the largest frame average of
 * it, in cd/m2 (CTA-861.3's MaxCLL and MaxFALL, the static metadata of an encode), and whether any pixel of a BT.2020 stream lies
 * outside a smaller gamut - the HDR twin of sigstats' bits_used.  The same pass gives the per-frame statistics dynamic metadata is
 * made from (in the manner of ST 2094-40 / Dolby Vision L1): min / average / max of maxRGB, the per-channel maxima, a percentile
 * distribution and the frame's luminance.  This is CTA-861.3's definition AS STATED HERE; it is not compared with any tool.
 * Input.  Exactly vqa_itp_submit's, but ONE stream: THREE planes of one depth (8 bits, or 9..16 bits as uint16), the colour models
 *   VQA_ITP_YUV2020 (Y, Cb, Cr, BT.2020 non-constant luminance, limited or full range, chroma replicated: 4:4:4, 4:2:2, 4:2:0, odd
 *   sizes) or VQA_ITP_BGR; the same geometry rules, the same errors.  R', G', B' are formed word for word as vqa_itp_submit states
 *   them, in double with contraction off.
 * One rounding.  Per channel c = rint(min(max(E', 0), 1) 65535), a 16-bit code: THE ONLY ROUNDING; everything after it is integer.
 *   A pixel with any of R', G', B' below 0 or above 1 BEFORE the clamp is counted in `clamped`: illegal Y'CbCr combinations and
 *   uint16 samples above 2^depth - 1, a QC figure by itself.
 * Table.  T[65536] of uint64: the display light of code c in units of 2^-20 cd/m2.  It TRAVELS WITH THE CALL and must be
 *   non-decreasing with T[65535] < 2^34, else VQA_ERR_INVALID (checked on the host in the submit).  vqa_light_table(transfer, T)
 *   fills it on the host, with no ctx and no GPU: VQA_ITP_PQ gives T[c] = rint(2^20 EOTF_PQ(c / 65535)) with the PQ constants
 *   above (T[0] = 0, the first non-zero entry is code 6, T[65535] = 10485760000 = 10000 2^20); VQA_ITP_HLG is VQA_ERR_UNSUPPORTED -
 *   HLG's display light is not a per-channel function (the OOTF needs Ys), and CTA-861.3's figures are HDR10's.  A caller may pass
 *   any monotone table of their own, e.g. BT.1886 at 100 cd/m2 for SDR.
 * Per pixel.  qR, qG, qB = T[cR], T[cG], T[cB]; m = max(cR, cG, cB) and qm = T[m] - T is monotone, so this is the pixel's maxRGB;
 *   y = (2627 qR + 6780 qG + 593 qB + 5000) / 10000 in integer division, the BT.2020 luminance.
 * Gamut test.  For G in {BT.709, P3-D65} an integer matrix M_G = rint(2^16 A_G), A_G the linear BT.2020 -> G matrix, derived in
 *   double on the host from the published chromaticities and D65 (0.3127, 0.3290) by the usual primaries-to-XYZ construction -
 *   BT.2020: R (0.708, 0.292), G (0.170, 0.797), B (0.131, 0.046); BT.709: R (0.64, 0.33), G (0.30, 0.60), B (0.15, 0.06); P3: R (0.680,
 *   0.320), G (0.265, 0.690), B (0.150, 0.060) - not typed in; vqa_light_gamut returns it (the 709 matrix is BT.2087's to four
 *   decimals).  With S_k = sum_j M_G[k][j] q_j in int64, the pixel is OUTSIDE G iff
 *     min_k S_k < -((max(qR, qG, qB) << 16) >> VQA_LIGHT_GAMUT_REL_SHIFT) - VQA_LIGHT_GAMUT_FLOOR:
 *   a negative component larger than 2^-6 of the pixel's largest component plus 2^-4 cd/m2 (S is in units of 2^-36 cd/m2).  Both
 *   constants are this project's own.  Why these: 400 000 random in-gamut colours per gamut, saturated primaries included, at
 *   1e-4 .. 1 of 1000 cd/m2, encoded to limited-range BT.2020 PQ Y'CbCr 4:4:4 and decoded by this chain, flag 0 at 10 and 12 bits
 *   (2^-7 and a floor of 2^28 units, 2^-8 cd/m2, already flag 3216 at 10 bits); AT 8 BITS QUANTISATION ALONE CROSSES IT (8074 flagged): THE COUNTS MEAN
 *   SOMETHING FROM 10 BITS ON.  Pure BT.2020 red and green at 5, 100 and 1000 cd/m2 are outside both gamuts; red at 0.5 cd/m2 is
 *   not: the floor hides saturated colours below about half a cd/m2.
 * Overflow.  q < 2^34 and |M| < 2^17, so |S_k| < 3 2^51; every per-frame sum is below 2^34 2^28 = 2^62.
 * Record, ONE ENTRY PER FRAME (vqa_light_metrics): count; max_code[3] (R, G, B), max_code_rgb and min_code_rgb (the largest and
 *   smallest m); sum_q = sum qm, sum_y, max_y; out_709, out_p3, clamped (pixel counts); pct_bin[10]: over the 4096-bin histogram
 *   of m >> 4, the smallest bin b with C(b) >= (p N + 9999) / 10000 for p = 100, 500, 1000, 2500, 5000, 7500, 9000, 9500, 9900,
 *   9998 - sigstats' exact-rank rule, per ten thousand.  The wait forms max_nits = T[max_code_rgb] 2^-20, min_nits, avg_nits =
 *   sum_q 2^-20 / count, y_avg, y_max, maxscl[3], pct_nits[10] = T[pct_bin << 4] 2^-20 (the bin's LOWER EDGE) and the two shares.
 *   With want_histogram the wait also returns the [n, 4096] uint32 histograms.
 * What follows: integer sums, maxima and minima are order-free, so a frame gives the same words in any batch, from any memory,
 *   alone or next to other kinds.  MaxCLL is the largest max_nits of a clip, MaxFALL the largest avg_nits (rtvqa_amd/light.py).
 * Limits: luma at least 16 x 16 and h w <= 2^28: VQA_ERR_UNSUPPORTED beyond either.  n_planes other than 3, Cb and Cr (or B, G, R)
 *   geometries that differ, a chroma size that is neither the luma's nor its ceil-half, mixed depths, an unknown model, a
 *   full_range other than 0 or 1, a null or a bad table: VQA_ERR_INVALID.
 * The contract of vqa_itp_submit: asynchronous, the same plane descriptors, depths, alignment rules, memory kinds and failure
 *   guarantee: a failed submit leaves nothing in flight.  A light batch is a batch of its own: VQA_ERR_STATE while one is pending,
 *   in flight next to a batch of every other kind, and each wait collects its own kind only.  vqa_light_wait: hist must be NULL
 *   unless the submit asked for histograms (VQA_ERR_INVALID, the batch stays pending); NULL is always accepted.
 * Kernels: k_light_accum (a thread owns a 2 x 4 luma patch as in k_itp; no transcendental: three 8-byte gathers per pixel from
 *   the table, which the submit copies to the device and the ctx keeps; the histogram in 16 KB of LDS, a workgroup walks 16384
 *   pixels of one frame before it flushes) and k_light_scan (one workgroup per frame).  Scratch on the device: 168 bytes and a
 *   16 KB histogram per frame; batches go out in sub-slices that keep the histograms within 256 MiB (16384 frames), and beyond
 *   32768 frames in slices; the 512 KB table; host frames are staged in the buffer a one-stream submit uses.  All of it is kept
 *   by the ctx until vqa_trim / vqa_destroy.
 * Not built: HLG; a conformant ST 2094-40 / Dolby Vision metadata writer; automatic cropping to the active picture (a letterbox
 *   lowers MaxFALL: pass a region of interest); chroma interpolation other than replication; measuring inside another kind's pass.
 * out of vqa_light_wait: n entries (n_entries = n); hist: n * 4096 words or NULL.                                             */
enum vqa_light_gamut_id { VQA_LIGHT_GAMUT_709 = 0, VQA_LIGHT_GAMUT_P3 = 1 };
#define VQA_LIGHT_GAMUT_REL_SHIFT 6                /* outside: beyond 2^-6 of the pixel's largest component ...               */
#define VQA_LIGHT_GAMUT_FLOOR 4294967296LL         /* ... plus 2^32 units of 2^-36 cd/m2 = 2^-4 cd/m2                          */
#define VQA_LIGHT_TABLE_LIMIT 17179869184ULL       /* 2^34: every table entry is below it                                     */
VQA_API int vqa_light_submit(vqa_ctx *ctx, const uint8_t *frames, int mem_kind, int n, int64_t frame_stride,
                             const vqa_plane_desc *planes, int n_planes, int model, int full_range, const uint64_t *table,
                             int want_histogram);
VQA_API int vqa_light_wait(vqa_ctx *ctx, vqa_light_metrics *out, int n_entries, uint32_t *hist);
/* T[65536] of `transfer` on the host: no ctx, no device.  VQA_ITP_HLG: VQA_ERR_UNSUPPORTED; anything else but VQA_ITP_PQ, or a
 * null table: VQA_ERR_INVALID. */
VQA_API int vqa_light_table(int transfer, uint64_t *table);
/* M_G = rint(2^16 A_G), row-major, rows R, G, B of G, columns R, G, B of BT.2020: no ctx, no device */
VQA_API int vqa_light_gamut(int gamut, int64_t m[9]);

/* ---- Clip-wide sync: a signature per frame, and every pairing of two clips' signatures at once ----
 * vqa_align_submit answers inside a band of at most +-32 frames around the pairing the caller supplied.  An encode with a long
 * leader, a trimmed head or an excerpt of a long source lies outside every band.  This kind finds the pairing anywhere in the
 * clip: a signature of VQA_SIG_BYTES bytes per frame, read in one pass over one plane, and the squared distance between every
 * distorted and every reference signature, from which the host reads the best constant offset and every frame's best partner.
 * The signature is a fixed grid whatever the frame size: a ladder rung and its source are synchronised without scaling either.
 *
 * Signature (vqa_sig_submit / vqa_sig_wait).  Input: ONE stream and ONE plane descriptor under vqa_align_submit's rules:
 *   bit_depth 8 (0), or 9 .. 16 as little-endian uint16; any offset, row_stride and pixel_step the other kinds accept (rows at
 *   odd addresses, padded rows, pixel_step = 3: one channel of packed BGR - the last through a gather, THE SLOW PATH, which
 *   gives the same bytes); host (pinned or not) and device memory.  No byte beyond offset + (h - 1) row_stride + w pixel_step of
 *   a frame is read.
 * Definition: G = VQA_SIG_GRID = 16.  Cell (a, b) covers rows floor(a h / 16) .. floor((a + 1) h / 16) - 1 and columns
 *   floor(b w / 16) .. floor((b + 1) w / 16) - 1.  With S the exact sum of the cell's samples and c its sample count,
 *   sig[16 a + b] = min(255, floor(S / (c << (depth - 8)))), an exact unsigned 64-bit integer division.  Samples above
 *   2^depth - 1 are read as they are; the min is what bounds them.
 * Output: uint8 [n][256].  A frame gives the same 256 bytes at any place of any batch and from any memory.
 * Limits: the plane at least 16 x 16 (no cell is empty) with h w <= 2^28, VQA_ERR_UNSUPPORTED otherwise; 1 <= n <= 32768 per
 *   submit, VQA_ERR_UNSUPPORTED beyond (a longer clip goes in windows).  The descriptor rules and the failure guarantee are
 *   vqa_gmsd_submit's: a failed submit leaves nothing in flight.  Host frames are staged in the buffer the one-stream kinds share.
 * Kernel: k_sig, ONE launch per submit; a workgroup owns one (frame, cell row), sums in 64-bit integers, divides and writes its 16
 *   bytes.  No global atomics.
 *
 * Cross (vqa_sig_cross_submit / vqa_sig_cross_wait).  Input: two HOST arrays of signatures, dist_sig [n_dist][256] and ref_sig
 *   [n_ref][256], 1 <= n_dist, n_ref <= VQA_SIG_MAX_FRAMES (VQA_ERR_UNSUPPORTED beyond; below 1 is VQA_ERR_INVALID).
 * Definition: D[j][i] = sum_k (dist_sig[j][k] - ref_sig[i][k])^2 <= 256 * 255^2 < 2^24.
 *   diag[k + n_dist - 1], uint64, k = -(n_dist - 1) .. n_ref - 1: the sum of D[j][j + k] over every j with 0 <= j < n_dist and
 *     0 <= j + k < n_ref; n_dist + n_ref - 1 words.  k has vqa_align_submit's sign: distorted frame j belongs to reference
 *     frame j + k.
 *   best[j], uint64, j = 0 .. n_dist - 1: min over i of ((D[j][i] << 32) | i): the smallest distance, ties to the smallest i.
 *   Everything is an integer function of the signatures.
 * How: with X = x - 128 (`x ^ 0x80` read as a signed byte; the shift cancels in the difference), D = E_d[j] + E_r[i] - 2 C[j][i],
 *   C a Gram matrix on the int8 matrix cores, four steps of K = 64 per 16 x 16 tile; |C| <= 2^22 and E <= 2^22, one 32-bit
 *   accumulator.  Kernels: k_sig_diag (a wave walks one diagonal of tiles and keeps its 31 diagonal sums in registers; global
 *   64-bit atomics: 31 per tile diagonal, so their number grows with n_dist + n_ref, not with the product) and k_sig_best (a
 *   wave walks one strip of 16 distorted frames over all reference tiles and keeps the running minimum; no atomics).  Frames
 *   that pad a tile to 16 contribute to neither.
 * Scratch: 256 (n_dist + n_ref) bytes of staged signatures and 8 (2 n_dist + n_ref - 1) bytes of words on the device, the words
 *   also pinned, kept by the ctx until vqa_trim / vqa_destroy.
 *
 * Each of the two is a batch of its own: VQA_ERR_STATE for a second submit while one is pending and for a wait without a submit
 *   or with counts that are not the submit's (the batch stays pending); in flight next to a batch of every other kind.
 * Not built: re-pairing by a per-frame path; an FFT-based offset search; signatures of more than one plane or another grid;
 *   signatures kept on the device between the two calls; timestamps and frame-rate conversion. */
#define VQA_SIG_GRID 16
#define VQA_SIG_BYTES 256
#define VQA_SIG_MAX_BATCH 32768
#define VQA_SIG_MAX_FRAMES 262144
VQA_API int vqa_sig_submit(vqa_ctx *ctx, const uint8_t *frames, int mem_kind, int n, int64_t frame_stride,
                           const vqa_plane_desc *plane);
VQA_API int vqa_sig_wait(vqa_ctx *ctx, uint8_t *sig, int n);   /* n == the submit's n; sig: n * 256 bytes */
VQA_API int vqa_sig_cross_submit(vqa_ctx *ctx, const uint8_t *dist_sig, int n_dist, const uint8_t *ref_sig, int n_ref);
/* n_diag == n_dist + n_ref - 1 and n_best == n_dist */
VQA_API int vqa_sig_cross_wait(vqa_ctx *ctx, uint64_t *diag, int64_t n_diag, uint64_t *best, int64_t n_best);

/* ---- Colour registration: does a code value mean the same in both streams? ----
 * vqa_align_submit and vqa_sig_submit find which frame pairs with which, vqa_shift_submit where the picture sits, vqa_light_submit
 * checks the container.  This kind measures what is still taken on trust: a limited / full range mix-up, a BT.601 matrix applied
 * to BT.709 material and a gamma or transfer mismatch do to every full-reference figure what a dropped frame does.  Per frame
 * pair it returns the joint first and second moments of the planes of both streams and, per reference code, the count, sum and
 * sum of squares of the distorted samples; from those the host derives, in exact rational arithmetic, the per-plane gain and
 * offset, the best 3 x 3 matrix plus offset, the best per-code tone curve and the error each would leave.  It reports and never
 * corrects.
 * Input.  Two streams of n frames, frame j against frame j; n_planes is 1 or 3, one depth per submit: 8 bits (bit_depth 0 or 8), or
 *   9 .. 16 bits as little-endian uint16; samples above 2^depth - 1 are read as they are.  The geometry rules and errors are
 *   vqa_ciede_submit's / vqa_itp_submit's: luma at least 16 x 16 and h w <= 2^28 (VQA_ERR_UNSUPPORTED beyond either); planes 1
 *   and 2 of equal geometry, each side either the luma's or its ceil-half; any offset, row stride and pixel step those kinds
 *   accept, packed bgr24 included; host, pinned or device memory.  1 <= n <= VQA_COLORFIT_MAX_FRAMES per submit,
 *   VQA_ERR_UNSUPPORTED beyond: a longer clip goes in windows, so this kind has no slice seam.  The device needs no colour model:
 *   it forms integer moments only.
 * Grid.  The luma grid, chroma replicated, as in vqa_ciede_submit: plane p at luma position (y, x) is its sample at
 *   (y >> sy, x >> sx), sx / sy = 1 where the plane is halved in that direction.  Every sum runs over the h w luma positions.
 * Record, ONE ENTRY PER FRAME (vqa_colorfit_metrics): count = h w; sum_r[3], sum_d[3]; rr[6] = sum r_i r_i' for (i, i') = 00, 01,
 *   02, 11, 12, 22; rd[3 i + k] = sum r_i d_k; dd[3] = sum d_k^2; sse[k] = dd[k] - 2 rd[4 k] + rr(k, k), formed by the wait.
 *   Bound: 65535^2 2^28 < 2^60.
 * Transfer tables.  Optional (want_tables) and ONE set per submit, not per frame.  bins = 1 << min(depth, 10) and
 *   bin = min(r_p >> max(depth - 10, 0), bins - 1).  Per plane and bin three uint64 words, summed over all frames and luma
 *   positions of the submit: count, sum_d (of d_p of the same plane) and sum_dd.  Layout [n_planes][bins][3].  With tables
 *   n h w <= VQA_COLORFIT_TABLE_POSITIONS = 2^31 is required (then sum_dd < 2^63): VQA_ERR_UNSUPPORTED beyond, checked before any
 *   byte is read.  Without want_tables no table work is done at all.
 * What follows: every word is an integer sum.  A frame pair gives the same record in any batch at any position, from any memory,
 *   alone or next to other kinds pending on the ctx.  The tables of a submit equal the sum of the tables of its frames submitted
 *   one by one.  Identical streams give sse == 0, rd[4 k] == rr(k, k) == dd[k], and every bin has sum_d == the sum over the bin
 *   of r.
 * Host formulas (rtvqa_amd/colorfit.py forms them in exact fractions; a C caller can do the same from the record).  Sum the
 *   records of a clip.  With n = count, A = [[n, sum_r^T], [sum_r, rr]] (4 x 4, rr as the symmetric matrix) and
 *   c_k = (sum_d[k], rd[., k]), a map d_k ~ b_k + sum_i M[k][i] r_i with x = (b_k, M[k][.]) leaves
 *     sse_k(x) = dd[k] - 2 x . c_k + x^T A x.
 *   Given: sse_given[k] = sse[k].
 *   Levels: var = n rr(k, k) - sum_r[k]^2, cov = n rd[4 k] - sum_r[k] sum_d[k]; gain = cov / var,
 *     offset = (sum_d[k] - gain sum_r[k]) / n, sse_affine[k] = dd[k] - sum_d[k]^2 / n - cov^2 / (n var).  A flat reference plane
 *     (var == 0): gain = 1, offset = (sum_d[k] - sum_r[k]) / n, sse_affine[k] = dd[k] - sum_d[k]^2 / n.
 *   Matrix: V[i][i'] = n rr(i, i') - sum_r[i] sum_r[i'], W[i][k] = n rd[3 i + k] - sum_r[i] sum_d[k]; solve V m_k = W[., k] by
 *     elimination in the order 0, 1, 2 without exchanges (V is positive semidefinite: the pivots are Schur complements >= 0; a
 *     zero pivot drops that reference plane, its coefficient is 0 in all three fits); b_k from the means;
 *     sse_matrix[k] = dd[k] - sum_d[k]^2 / n - sum_i m_ki W[i][k] / n.
 *   Tone (tables): curve[p][bin] = sum_d / count; sse_lut[p] = the sum over non-empty bins of (sum_dd - sum_d^2 / count);
 *     dB(sse_affine, sse_lut) is what a per-code curve explains beyond gain and offset: a gamma or transfer mismatch.
 *   Catalogue of known mishaps, exact rational maps in code space scored by sse_k(x), s = 2^(depth - 8), P = 2^depth - 1:
 *     limited_to_full: d_Y = (r_Y - 16 s) P / (219 s), d_C = (r_C - 128 s) P / (224 s) + 128 s; full_to_limited: its inverse;
 *     bt601_to_bt709 (Y'CbCr, three planes): S F709 F601^-1 S^-1 about the centre (16 s, 128 s, 128 s), F the R'G'B' -> Y'PbPr
 *     matrix of (Kr, Kb) = (0.299, 0.114) and (0.2126, 0.0722), S = diag(219, 224, 224); bt709_to_bt601: the reverse.  B, G, R
 *     and one plane take the two range maps with the luma constants on every plane.  The candidate with the smallest total
 *     error (ties: this order) is NAMED when 2 sse_candidate <= sse_given and sse_given > 0 - it accounts for at least as much
 *     error as everything else together; the factor 2 is the rule's definition.  dB(a, b) = 0 if a == 0, infinite if b == 0 < a,
 *     else 10 log10(a / b).
 *   No clipping is modelled anywhere: clipped samples stay in the residual.
 * Limits and errors: n_planes other than 1 or 3, mixed depths, chroma geometries that differ or are neither the luma's nor its
 *   ceil-half, a want_tables other than 0 or 1: VQA_ERR_INVALID.  The contract of vqa_ciede_submit otherwise: asynchronous, the
 *   same descriptors, alignment rules, memory kinds and failure guarantee - a failed submit leaves nothing in flight; a frame
 *   stride smaller than the planes' span is VQA_ERR_INVALID for a stream of more than one frame.
 * A colour-fit batch is a batch of its own: VQA_ERR_STATE for a second submit while one is pending and for a wait without a
 *   submit or with n_entries != n (the batch stays pending); in flight next to a batch of every other kind.  vqa_colorfit_wait:
 *   tables must be NULL unless the submit asked for them (VQA_ERR_INVALID), and n_table_words must then be n_planes bins 3
 *   (VQA_ERR_STATE); either refusal leaves the batch pending; NULL is always accepted.  Host frames are staged in the buffers the
 *   pair kinds share.  Scratch: 192 bytes per frame and 24 n_planes bins bytes of tables, on the device and pinned, kept by the
 *   ctx until vqa_trim / vqa_destroy.
 * Kernel: k_colorfit, ONE launch per submit, tables fused: a thread owns a 2 x 4 luma patch of both images as in k_ciede, so every
 *   sample of both streams is read once; a workgroup walks 16384 positions of one frame, then one 64-bit atomic add per word.  The
 *   tables live in LDS (at most 48 KB: count and sum_d in 32 bits, sum_dd in 64; 16384 positions keep them below 2^14, 2^30 and
 *   2^46); equal adjacent bins of a thread, and a wave whose entries all name one bin, are joined before they reach LDS, so a
 *   chroma sample enters once with its weight and flat content does not serialise.  The kernel has no profiling id
 *   (enum vqa_kernel_id is closed): time it from outside.
 * Not built: applying the fit (vqa_conform_submit does); clipping-aware fits; per-frame tables; chroma interpolation other than replication; a fit after
 *   vqa_scale_submit; running inside another kind's pass.
 * out of vqa_colorfit_wait: n entries (n_entries = n); tables: n_table_words = n_planes * bins * 3 words, or NULL.            */
#define VQA_COLORFIT_MAX_FRAMES 32768
#define VQA_COLORFIT_MAX_BINS 1024
#define VQA_COLORFIT_TABLE_POSITIONS 2147483648LL   /* 2^31: n h w of a submit with tables                                   */
VQA_API int vqa_colorfit_submit(vqa_ctx *ctx, const uint8_t *ref, const uint8_t *dist, int mem_kind, int n,
                                int64_t ref_frame_stride, int64_t dist_frame_stride, const vqa_plane_desc *planes, int n_planes,
                                int want_tables);
VQA_API int vqa_colorfit_wait(vqa_ctx *ctx, vqa_colorfit_metrics *out, int n_entries, uint64_t *tables, int64_t n_table_words);

/* ---- per-kernel timing (HIP events on the ctx stream) -----------------------
 * The named kernel ids are exactly the ids for which vqa_kernel_name does not return "?"; vqa_profile_read accepts those and
 * no others.  The other names of the enum (VQA_K_COUNT, VQA_K_COUNT_ALL, ... VQA_K_EAVE) are frozen markers: each records
 * where the id list ended when one feature shipped, and is kept, name and value, for source compatibility.  The ids equal to
 * those markers, and the gap 15, are permanently unknown to both functions - with one exception from before the rule:
 * VQA_K_COUNT = 12 is also VQA_K_VIF's id, which is named.  A new kernel takes the next free id above the current last one
 * (a marker's value is not free) and needs no new marker. */
enum vqa_kernel_id {
    VQA_K_GRAY_HIST = 0, /* BGR->gray + histograms, native resolution   */
    VQA_K_RESIZE = 1,    /* cv2.resize gather + gray + histograms       */
    VQA_K_DCT8 = 2,      /* 8x8 DCT energy + temporal L1                */
    VQA_K_DCT_FULL = 3,  /* full-frame DCT: FFT row + column passes, or (sizes that do not factor into 2,3,5) 4 dense products */
    VQA_K_CANNY_NMS = 4,
    VQA_K_CANNY_HYST = 5,
    VQA_K_SAD = 6,
    VQA_K_SSIM_GAUSS = 7, /* VQA_SSIM_MS: one entry per level (five per group of same-geometry planes) */
    VQA_K_SSIM_FFMPEG = 8,
    VQA_K_ORB = 9,       /* FAST-9/16 + NMS on the 64x64 thumbnail's centre */
    VQA_K_FARNEBACK = 10, /* the whole Farneback pyramid (about 30 launches per chunk of pairs) */
    VQA_K_MS_PYRAMID = 11, /* VQA_SSIM_MS: levels 1..4 of both images from one read of level 0 */
    VQA_K_COUNT = 12,        /* frozen marker (= 12): the list as ABI 8 first shipped it                                  */
    VQA_K_VIF = 12,          /* vqa_vif_submit: the per-level statistic (four entries per group of same-geometry planes) */
    VQA_K_VIF_DECIMATE = 13, /* vqa_vif_submit: level s from level s - 1 (three entries per group)                    */
    VQA_K_COUNT_ALL = 14,    /* frozen marker (= 14)                                                                     */
    VQA_K_ADM = 16,          /* vqa_adm_submit: one scale - DWT, decoupling, masking, cube sums (four entries per group)  */
    VQA_K_ADM_REDUCE = 17,   /* vqa_adm_submit: the tile partials of a scale, added in a fixed order (four per group)     */
    VQA_K_COUNT_EXT = 18,    /* frozen marker (= 18)                                                                     */
    VQA_K_MOTION = 19,       /* vqa_motion_submit: blur of both frames and the sum of |difference| (one entry per group of
                                same-geometry planes)                                                                   */
    VQA_K_END = 20,          /* frozen marker (= 20)                                                                     */
    VQA_K_SITI = 21,         /* vqa_siti_submit: Sobel, frame difference and their integer sums (one entry per group of
                                same-geometry planes)                                                                   */
    VQA_K_LAST = 22,         /* frozen marker (= 22)                                                                     */
    VQA_K_PSNR_HVS = 23,     /* vqa_psnr_hvs_submit: the 8x8 DCTs, the masks and the two weighted sums (one entry per group of
                                same-geometry planes)                                                                    */
    VQA_K_PAST = 24,         /* frozen marker (= 24)                                                                     */
    VQA_K_CIEDE = 25,        /* vqa_ciede_submit: both Lab conversions, dE00 and the fixed-point sum (one entry per submit) */
    VQA_K_BEYOND = 26,       /* frozen marker (= 26)                                                                     */
    VQA_K_GMSD = 27,         /* vqa_gmsd_submit: the 2x2 sums, Prewitt, the similarity and its integer sums (one entry per
                                group of same-geometry planes)                                                           */
    VQA_K_LIMIT = 28,        /* frozen marker (= 28)                                                                     */
    VQA_K_CAMBI_MASK = 29,     /* vqa_cambi_submit: 10 bits, anti-dither, mask (one entry per group of same-geometry planes) */
    VQA_K_CAMBI_DECIMATE = 30, /* vqa_cambi_submit: scales 1..4 (one entry per group)                                      */
    VQA_K_CAMBI_CONTRAST = 31, /* vqa_cambi_submit: the 65 x 65 counts and u of one scale (five entries per group)         */
    VQA_K_CAMBI_TOPK = 32,     /* vqa_cambi_submit: a scale's histogram cleared, and its top-K sum (ten entries per group) */
    VQA_K_TERMINUS = 33,     /* frozen marker (= 33)                                                                     */
    VQA_K_XPSNR_ACT = 34,    /* vqa_xpsnr_submit: the luma activity words sa, ta per block (one entry per slice)          */
    VQA_K_XPSNR_SSE = 35,    /* vqa_xpsnr_submit: the squared error per block (one entry per group of same-geometry planes) */
    VQA_K_BOUND = 36,        /* frozen marker (= 36)                                                                     */
    VQA_K_HAARPSI = 37,      /* vqa_haarpsi_submit: the 2x2 sums, the Haar coefficients, the similarities and the integer sums
                                (one entry per group of same-geometry planes)                                            */
    VQA_K_FINIS = 38,        /* frozen marker (= 38)                                                                     */
    VQA_K_VCA_BLOCKS = 39,   /* vqa_vca_submit: the 32 x 32 block DCTs, qH_k, S_k, qL_k (one entry per group of same-geometry
                                planes)                                                                                  */
    VQA_K_VCA_SUM = 40,      /* vqa_vca_submit: the block map and its difference to the frame before, summed (one per slice) */
    VQA_K_CLOSE = 41,        /* frozen marker (= 41)                                                                     */
    VQA_K_ARTIFACTS = 42,    /* vqa_artifacts_submit: the boundary steps by phase, both blur sums and the Laplacian sum (one
                                entry per group of same-geometry planes)                                                 */
    VQA_K_STOP = 43,         /* frozen marker (= 43)                                                                     */
    VQA_K_BRISQUE_HALF = 44, /* vqa_brisque_submit: the exact scale-1 planes (one entry per group of same-geometry planes)   */
    VQA_K_BRISQUE_MSCN = 45, /* vqa_brisque_submit: the moments, u and the pairs inside the plane (two per group: the scales) */
    VQA_K_BRISQUE_SEAM = 46, /* vqa_brisque_submit: the pairs that wrap around (two per group)                                */
    VQA_K_EDGE = 47,         /* frozen marker (= 47)                                                                     */
    VQA_K_MDSI_MAP = 48,     /* vqa_mdsi_submit: the box sums, the channels, Prewitt, GCS, the map of g and the words A, B, n_neg
                                (one entry per slice)                                                                    */
    VQA_K_MDSI_DEV = 49,     /* vqa_mdsi_submit: the deviation word D from the map and the frame's A, B (one entry per slice) */
    VQA_K_BRINK = 50,        /* frozen marker (= 50)                                                                     */
    VQA_K_ITP = 51,          /* vqa_itp_submit: both ICtCp conversions, dE_ITP, the fixed-point sum and maximum (one entry per
                                slice)                                                                                   */
    VQA_K_VERGE = 52,        /* frozen marker (= 52)                                                                     */
    VQA_K_PU21_ENCODE = 53,  /* vqa_pu21_submit: display light, the PU21 encodings, the q_Y maps and the four SSE half-words (one
                                entry per sub-slice)                                                                     */
    VQA_K_PU21_SSIM = 54,    /* vqa_pu21_submit: the Gaussian SSIM over the maps (one entry per sub-slice)                     */
    VQA_K_RIM = 55,          /* frozen marker (= 55)                                                                     */
    VQA_K_FSIM_LUMA = 56,    /* vqa_fsim_submit: the box sums and Y, I, Q of both images (one entry per sub-slice)             */
    VQA_K_FSIM_DFT = 57,     /* vqa_fsim_submit: the dense DFTs on the fp64 matrix cores (five entries per sub-slice: the forward
                                pair and one inverse pair per orientation)                                               */
    VQA_K_FSIM_ENERGY = 58,  /* vqa_fsim_submit: Energy, An and |EO_0|^2 of an orientation (four entries per sub-slice)       */
    VQA_K_FSIM_MEDIAN = 59,  /* vqa_fsim_submit: the exact medians and the thresholds T_o (one entry per sub-slice)           */
    VQA_K_FSIM_PC = 60,      /* vqa_fsim_submit: PC and the p maps (one entry per sub-slice)                                  */
    VQA_K_FSIM_POOL = 61,    /* vqa_fsim_submit: Scharr, the similarities and the three words (one entry per sub-slice)       */
    VQA_K_HEM = 62,          /* frozen marker (= 62)                                                                     */
    VQA_K_SIGSTATS_ACCUM = 63, /* vqa_sigstats_submit: the histograms, sad, changed, the masks and the profiles (one entry per
                                  group of same-geometry planes and sub-slice)                                           */
    VQA_K_SIGSTATS_SCAN = 64,  /* vqa_sigstats_submit: every other word from the histograms and the profiles (one entry per
                                  sub-slice)                                                                             */
    VQA_K_FRINGE = 65,       /* frozen marker (= 65)                                                                     */
    VQA_K_SCALE = 66,        /* vqa_scale_submit: both passes of the resampler, fused (one entry per group of planes alike on
                                both sides)                                                                              */
    VQA_K_MARGIN = 67,       /* frozen marker (= 67)                                                                     */
    VQA_K_ALIGN_CROSS = 68,  /* vqa_align_submit: the Gram tiles of the band and E of every frame (one entry per submit)  */
    VQA_K_LEDGE = 69,        /* frozen marker (= 69)                                                                     */
    VQA_K_SHIFT = 70,        /* vqa_shift_submit: the tiles of the grid of shifts, E_r and E_d (one entry per submit)     */
    VQA_K_SILL = 71,         /* frozen marker (= 71)                                                                     */
    VQA_K_LIGHT_ACCUM = 72,  /* vqa_light_submit: the decode, the table gathers, the histogram and the per-frame words (one entry
                                per sub-slice)                                                                           */
    VQA_K_LIGHT_SCAN = 73,   /* vqa_light_submit: the percentile bins off the histograms (one entry per sub-slice)        */
    VQA_K_LINTEL = 74,       /* frozen marker (= 74)                                                                     */
    VQA_K_SIG = 75,          /* vqa_sig_submit: the cell sums and the signature bytes (one entry per submit)              */
    VQA_K_SIG_DIAG = 76,     /* vqa_sig_cross_submit: the walk along the tile diagonals, diag (one entry per submit)       */
    VQA_K_SIG_BEST = 77,     /* vqa_sig_cross_submit: the walk along the row strips, best (one entry per submit)           */
    VQA_K_EAVE = 78          /* frozen marker (= 78): one past the last id                                               */
};
/* When enabled, every kernel launch made by a submit call is bracketed by a
 * hipEvent pair recorded on the ctx stream; the elapsed times are accumulated
 * per kernel id when the batch is waited for.                                 */
VQA_API int vqa_profile_enable(vqa_ctx *ctx, int on);
VQA_API int vqa_profile_read(vqa_ctx *ctx, int kernel_id, double *total_ms, int64_t *launches, int reset);
VQA_API const char *vqa_kernel_name(int kernel_id);

/* ---- the path's one collective: SUM all-reduce of pooled scalars (RCCL over xGMI) ---
 * The reference has no communication layer (its parallelism is a process pool over
 * frames, complexity_metrics.py:143-147); frame batches shard one stream per GPU and
 * only a handful of pooled float64 scalars ever cross devices.
 * RCCL is loaded on first use (dlopen librccl.so.1): VQA_ERR_UNSUPPORTED without it.   */
typedef struct vqa_comm vqa_comm;
#define VQA_COMM_ID_BYTES 128
/* single process, several devices: one ctx per device (ncclCommInitAll)                */
VQA_API int vqa_comm_create(vqa_ctx *const *ctxs, int n_ctx, vqa_comm **out);
/* one process per device: rank 0 makes an id, the host program ships its
 * VQA_COMM_ID_BYTES bytes to the other ranks by its own means, every rank joins        */
VQA_API int vqa_comm_unique_id(void *id, size_t id_bytes);
VQA_API int vqa_comm_create_rank(vqa_ctx *ctx, const void *id, size_t id_bytes, int n_ranks, int rank, vqa_comm **out);
VQA_API int vqa_comm_destroy(vqa_comm *comm);
VQA_API int vqa_comm_size(const vqa_comm *comm);           /* ranks in the communicator */
VQA_API const char *vqa_comm_last_error(const vqa_comm *comm); /* comm == NULL: why this thread's last creation failed */
/* Test seam, LAB BUILD ONLY (vqa_build_flavour() & 2).  There, with VQA_COMM_FAKE_RCCL=1 in the environment when the
 * first communicator is made, an in-library stand-in takes the place of the RCCL entry points (it checks the group
 * bracketing and sums on the host), which lets the single-process multi-context path run on a one-GPU box; this returns
 * the stand-in's call trace.  The shipped library has no stand-in: it always returns "".  Multi-device use over real
 * RCCL has not run on hardware yet (no multi-GPU box was available to the builder).                                  */
VQA_API const char *vqa_comm_debug_trace(void);
/* In place: vals is [local contexts][count] doubles, row i belongs to the i-th local
 * context (one row with vqa_comm_create_rank); on return every row holds the sum over
 * ALL ranks.  count <= 64.  Blocking; runs on the contexts' streams.                   */
VQA_API int vqa_allreduce(vqa_comm *comm, double *vals, int count);

/* ---- introspection for tests (device-side intermediates) ------------------ */
/* Copies intermediate planes of the LAST complexity batch to host memory:
 * which = 0: DCT input plane  (resize(gray(frame)))   [n][ph][pw]
 * which = 1: hist/edge plane  (gray(resize(frame)))   [n][ph][pw]
 * which = 2: Canny edge map, 0/255                    [n][ph][pw]
 * which = 3: full-resolution gray (motion input)      [n][h][w]              */
VQA_API int vqa_debug_read_plane(vqa_ctx *ctx, int which, int frame, uint8_t *dst, int dst_h, int dst_w);
/* Copies float intermediates of the LAST CHUNK of the last VQA_MOTION_FARNEBACK submit to host memory (a submit is cut into
 * chunks of pairs only when its scratch would pass ~12 GiB: a small batch is one chunk).  Pair i of a submit is
 * (frame i - 1, frame i), pair 0 = (prev0, frame 0); gray plane q is prev0 for q = 0 and frame q - 1 otherwise.
 * which = 0: the final flow field of pair `index`; level must be 0; dst is [h][w][2] (dx, dy), dst_h x dst_w = h x w.
 * which = 1: the polynomial expansion of gray plane `index` at pyramid level `level` (0 = finest .. the coarsest the
 *            frame size allows, at most 3); dst is [5][lh][lw], FIVE PLANES as the device keeps them, dst_h x dst_w =
 *            lh x lw = lrint(h / 2^level) x lrint(w / 2^level).  Plane c holds coefficient c of OpenCV's [lh][lw][5]
 *            layout (FarnebackPolyExp: 0, 1 = the linear terms in y and x, 2, 3 = the quadratic ones, 4 = the mixed one).
 * VQA_ERR_STATE: no Farneback submit has completed its launches on this ctx, or its buffers were released since
 * (vqa_trim).  VQA_ERR_INVALID: a pair or plane outside the last chunk (pair 0 and plane 0 of a submit without prev0
 * among them), a level the pyramid does not have, dimensions that are not the level's.  Copy only; waits for the
 * streams of the ctx first.  An added entry point, not a layout change: VQA_ABI_VERSION stays.                          */
VQA_API int vqa_debug_read_farneback(vqa_ctx *ctx, int which, int index, int level, float *dst, int dst_h, int dst_w);

#ifdef __cplusplus
}
#endif
#endif /* VQA_H */
