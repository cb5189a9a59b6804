// vqa_kernels.hpp — host-side launchers of the gfx950 kernels (internal).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vqa.h"

// Build flavours (csrc/Makefile):
//   default            the product: one kernel per stage, no environment variable selects an arithmetic path.
//   -DVQA_AB_VARIANTS  (make lab) additionally compiles the superseded kernels of earlier rounds and their VQA_*_VARIANT /
//                      tuning selectors, for re-measurement (LAB_NOTES.md); results stay parity-tested.
//   -DVQA_TEST_SEAMS   (make lab) additionally compiles the fault-injection / stand-in hooks the tests use:
//                      VQA_COMM_FAKE_RCCL, VQA_HYST_MAX_ROUNDS, VQA_HYST_RESCUE_MAX_ROUNDS, VQA_FAIL_ENSURE_AT, VQA_FB_CHUNK_BYTES, VQA_QSLICE.
#ifdef VQA_AB_VARIANTS
#include <cstdlib>
#endif

namespace vqa {

// value of an A/B selector: the environment in the lab build, the shipped default otherwise (callers cache it)
inline int ab_knob(const char *name, int dflt)
{
#ifdef VQA_AB_VARIANTS
    const char *e = getenv(name);
    return e ? atoi(e) : dflt;
#else
    (void)name;
    return dflt;
#endif
}

// k_gray_hist.hip
void launch_bgr2gray_hist(hipStream_t st, const uint8_t *bgr, int n, int h, int w, int64_t frame_stride,
                          int64_t row_stride, uint8_t *gray, int gp, int64_t plane_stride, vqa_frame_metrics *res,
                          bool gray_hist, bool color_hist, bool sum2);
void launch_resize_planes(hipStream_t st, const uint8_t *bgr, int n, int h, int w, int64_t frame_stride,
                          int64_t row_stride, int rw, int rh, const int32_t *xofs, const int32_t *xa,
                          const int32_t *yofs, const int32_t *yb, int mode, uint8_t *planeA, uint8_t *planeB, int pp,
                          int64_t plane_stride, vqa_frame_metrics *res, bool gray_hist, bool color_hist, bool sum2);

// k_orb.hip
void launch_orb64(hipStream_t st, const uint8_t *bgr, int n, int h, int w, int64_t frame_stride, int64_t row_stride,
                  const int32_t *xofs, const int32_t *xa, const int32_t *yofs, const int32_t *yb, int mode,
                  vqa_frame_metrics *res);

// k_dct8.hip
int dct8_blocks_per_frame(int h, int w);
// wave slots of the CURRENT device for the marching kernel (CUs x resident workgroups x 4): queried once per ctx in
// vqa_create and handed to every launch - no process-wide cache of a per-device quantity
int dct8_wave_slots();
void launch_dct8(hipStream_t st, const uint8_t *planes, int pitch, int64_t plane_stride, int n, int h, int w,
                 bool energy, bool temporal, bool first_has_prev, double *partials, vqa_frame_metrics *res, int wave_slots);

// k_dct_full.hip
void launch_dct_full(hipStream_t st, const uint8_t *planes, int pitch, int64_t plane_stride, int n, int h, int w,
                     const float *cw, const float *ch, float *scratch, double *pe, double *pt, bool energy,
                     bool temporal, bool first_has_prev, vqa_frame_metrics *res);

void launch_dct_full_finalize(hipStream_t st, const double *pe, const double *pt, int tiles, int n, vqa_frame_metrics *res,
                              bool energy, bool temporal, bool first_has_prev);

// k_dct_fft.hip: the same full-frame metrics through FFT-based row / column passes (lengths that factor into 2, 3, 5)
constexpr int DCT_FFT_MAX_PASSES = 12;
struct dct_fft_plan {            // one per transform length
    int n, npass;
    int radix[DCT_FFT_MAX_PASSES];
    int m[DCT_FFT_MAX_PASSES], tstep[DCT_FFT_MAX_PASSES];   // per pass: n / radix, n / (Ns radix)   (Ns = product of the radices before it)
    uint32_t ns_magic[DCT_FFT_MAX_PASSES];                 // per pass: ceil(2^32 / Ns): j / Ns = mulhi(j, magic) for j Ns < 2^32 (Ns = 1: 0, see k_dct_fft.hip)
    const float2 *tw;            // device: tw[m] = e^{-2 pi i m / n}, m < n
    const float2 *post;          // device: post[k] = s_k (cos, sin)(pi k / 2n), s_0 = sqrt(1/n), s_k = sqrt(2/n)
};
bool dct_fft_factor(int n, int radix[DCT_FFT_MAX_PASSES], int *npass);
bool dct_fft_supported(int h, int w); // the plane takes the FFT passes (else k_dct_full.hip's dense products)
int dct_fft_tiles(int h, int w); // partial sums per frame the column pass writes (sizes pe / pt)
void launch_dct_full_fft(hipStream_t st, const uint8_t *planes, int pitch, int64_t plane_stride, int n, int h, int w,
                         const dct_fft_plan &plan_w, const dct_fft_plan &plan_h, float *scratch, double *pe, double *pt,
                         bool energy, bool temporal, bool first_has_prev, vqa_frame_metrics *res);

// k_canny.hip
struct canny_geom {
    int tiles_x, tiles_y;
};
canny_geom canny_tiles(int h, int w); // tiles of the bit-planes, which hold the TRANSPOSED frame (k_canny.hip)
// word (inside one frame's plane) that holds pixel (y, x) of an h x w frame; the pixel is bit y & 63 of it
int64_t canny_plane_word(int h, int w, int y, int x);
void launch_canny_nms(hipStream_t st, const uint8_t *gray, int pitch, int64_t plane_stride, int n, int h, int w,
                      int low, int high, unsigned long long *strong, unsigned long long *weak,
                      vqa_frame_metrics *res);
// hysteresis on the strong/weak bit-planes: round 0 visits every 64x64 tile, later rounds the
// tiles a neighbour enqueued (compact list + dedup flags); *out_count must be 0 at launch.
unsigned canny_hyst_tiles(int n, int h, int w);
constexpr int CANNY_HYST_SEGMENTS = 16; // work-list segments per frame (k_canny.hip: HSEG)
// stats != 0: every tile visit adds its relaxation steps to res[f].hyst_steps (VQA_OPT_HYST_STATS; one atomic per visit)
void launch_canny_hyst_all(hipStream_t st, unsigned long long *strong, const unsigned long long *weak, int n, int h,
                           int w, unsigned *queued, unsigned *out_list, unsigned *out_count, vqa_frame_metrics *res,
                           int stats);
void launch_canny_hyst_list(hipStream_t st, unsigned long long *strong, const unsigned long long *weak, int n, int h,
                            int w, unsigned *in_queued, const unsigned *in_list, const unsigned *in_count,
                            unsigned *out_queued, unsigned *out_list, unsigned *out_count, unsigned *zero_count,
                            vqa_frame_metrics *res, int stats);
void launch_canny_hyst_tail(hipStream_t st, unsigned long long *strong, const unsigned long long *weak, int n, int h,
                            int w, unsigned *list0, unsigned *cnt0, unsigned *q0, unsigned *list1, unsigned *cnt1,
                            unsigned *q1, int first_in, vqa_frame_metrics *res, int stats, int max_rounds, int rescue_max_rounds);
constexpr int CANNY_HYST_MAX_ROUNDS = 1 << 16; // the tail's drain bound (a 64x64-tile fixpoint over any frame ends far below); a frame
                                               // that hits it is finished by the rescue pass under the proof's bound (k_canny.hip)
void launch_canny_finish(hipStream_t st, const unsigned long long *strong, int n, int h, int w, vqa_frame_metrics *res);

// k_sad.hip
void launch_block_sad(hipStream_t st, const uint8_t *planes, int pitch, int64_t plane_stride, int n, int h, int w,
                      int range, bool first_has_prev, vqa_frame_metrics *res);

// k_farneback.hip
struct fb_taps {       // one Gaussian blur kernel (getGaussianKernel, CV_32F), ksize <= 31
    float k[32];
    int ksize;
};
struct fb_poly {       // FarnebackPrepareGaussian(n = 5, sigma = 1.2)
    float g[11], xg[11], xxg[11];
    double ig11, ig03, ig33, ig55;
};
struct fb_resize_tabs { // cv2.resize INTER_LINEAR tables for float data (device pointers)
    int32_t *xofs = nullptr, *yofs = nullptr;
    float *xa = nullptr, *yb = nullptr;
    int mode = 0;      // 1 = exact 2x decimation
    // the source columns / rows a bilinear downscale actually samples (sorted, unique); null = all of them
    int32_t *cols = nullptr, *rows = nullptr;
    int nc = 0, nr = 0;
    // the fused level kernel's view of a downscale: the two source columns / rows each level column / row samples
    // (clamps applied; 2 * dsize entries) and the widest extent of them over any 32 consecutive columns, 8 and 32 rows
    int32_t *sx = nullptr, *sy = nullptr;
    int span_x32 = 0, span_y8 = 0, span_y32 = 0;
};
// blurred values are produced only at the columns / rows listed (all when null): the level's resize reads nothing else
void launch_fb_blur(hipStream_t st, const uint8_t *gray, int pitch, int64_t plane_stride, int planes, int h, int w,
                    const fb_taps &T, const int32_t *cols, int nc, const int32_t *rows, int nr, float *tmp, float *out);
// Gaussian blur of the u8 planes + resize to the level in one kernel; T = nullptr: finest level (no resize).  false: the
// level does not fit its LDS budget - use launch_fb_blur (+ launch_fb_resize)
bool launch_fb_level(hipStream_t st, const uint8_t *gray, int pitch, int64_t plane_stride, int planes, int h, int w,
                     const fb_taps &K, const fb_resize_tabs *T, float *out, int lh, int lw);
void launch_fb_resize(hipStream_t st, const float *src, int sh, int sw, int cn, float *dst, int dh, int dw, int images,
                      const fb_resize_tabs &T, float mul, bool apply_mul);
void launch_fb_polyexp(hipStream_t st, const float *in, int planes, int h, int w, const fb_poly &C, float *out);
// one flow iteration (products + 15x15 box sums + solve, fused; the products never reach HBM).  flow == nullptr: zero
// flow (coarsest level); flow_out must not alias the input
void launch_fb_iter(hipStream_t st, const float *R, const float *flow, int pairs, int h, int w, float *flow_out,
                    double *mag_partials = nullptr);
// workgroups (= magnitude partials) per pair of that launch, and the mean |flow| from them
int fb_iter_blocks(int pairs, int h, int w);
int fb_iter_max_blocks(int h, int w); // >= fb_iter_blocks for every pair count
void launch_fb_mag_finalize(hipStream_t st, const double *partials, int nblk, int pairs, int h, int w, bool first_valid,
                            vqa_frame_metrics *res);
#ifdef VQA_AB_VARIANTS // the two-kernel form of rounds 2-3 (VQA_FB_VARIANT=1 in the lab build)
void launch_fb_update(hipStream_t st, const float *R, const float *flow, int pairs, int h, int w, float *M);
void launch_fb_update_first(hipStream_t st, const float *R, const float *coarse, int ch, int cw, const fb_resize_tabs &T,
                            float mul, int pairs, int h, int w, float *M);
void launch_fb_blur_solve(hipStream_t st, const float *M, int pairs, int h, int w, float *flow);
#endif
#ifdef VQA_AB_VARIANTS // the separate magnitude pass of rounds 2-3 (with the two-kernel iteration)
int fb_mag_blocks();
void launch_fb_mag(hipStream_t st, const float *flow, int pairs, int h, int w, double *partials, bool first_valid,
                   vqa_frame_metrics *res);
#endif

// One group of same-geometry planes of a submit, planes[idx[0 .. count)], as a kernel's four slots: each plane's byte offset
// inside a frame and / or its index in the submit (either may be null).  The slots beyond `count` repeat the first plane's.
inline void group_slots(const vqa_plane_desc *planes, const int *idx, int count, int64_t offset[4], int plane_index[4])
{
    for (int i = 0; i < 4; i++) {
        const int p = idx[i < count ? i : 0];
        if (offset) offset[i] = planes[p].offset;
        if (plane_index) plane_index[i] = p;
    }
}

// k_quality.hip
int ssim_gauss_blocks(int h, int w);
void launch_quality_gauss(hipStream_t st, const uint8_t *ref, const uint8_t *dist, int n, int64_t ref_frame_stride,
                          int64_t dist_frame_stride, const vqa_plane_desc *planes, const int *idx, int count,
                          int n_planes, double *partials, int64_t partial_plane_stride, vqa_plane_metrics *res, int depth);
void launch_quality_ffmpeg(hipStream_t st, const uint8_t *ref, const uint8_t *dist, int n, int64_t ref_frame_stride,
                           int64_t dist_frame_stride, const vqa_plane_desc *planes, const int *idx, int count,
                           int n_planes, double *partials, int64_t partial_plane_stride, vqa_plane_metrics *res, int depth);
int ssim_ffmpeg_blocks(int h, int w);

// multi-scale SSIM (VQA_SSIM_MS): k_msssim.hip holds the pyramid, k_quality.hip the per-scale Gaussian launches
constexpr int MS_LEVELS = 5;
constexpr int MS_MIN_DIM = 161;   // level 4 must hold an 11x11 window: 161 -> 81 -> 41 -> 21 -> 11
// Levels 1..4 of one group of same-geometry planes, as k_ms_pyramid writes them: fp32 planes holding the EXACT sum of the
// 4^s level-0 samples behind each level-s sample (the 2x2 mean times 4^s; < 2^24 for 16-bit planes at level 4).  Level s
// starts off[s] floats into the scratch and is laid out [image: ref, dist][frame][plane of the group][h[s]][w[s]].
struct ms_layout {
    int w[MS_LEVELS], h[MS_LEVELS];
    int64_t off[MS_LEVELS];   // off[0] unused (level 0 is the caller's memory)
    int64_t total;            // floats
};
inline ms_layout ms_levels(int n, int count, int h, int w)
{
    ms_layout L;
    L.w[0] = w; L.h[0] = h; L.off[0] = 0;
    int64_t at = 0;
    for (int s = 1; s < MS_LEVELS; s++) {
        L.w[s] = (L.w[s - 1] + 1) / 2;
        L.h[s] = (L.h[s - 1] + 1) / 2;
        L.off[s] = at;
        at += 2 * (int64_t)n * count * L.h[s] * L.w[s];
    }
    L.total = at;
    return L;
}
// levels 1..4 of ref and dist from ONE read of level 0 (uint8, or uint16 when depth > 8)
void launch_ms_pyramid(hipStream_t st, const uint8_t *ref, const uint8_t *dist, int n, int64_t ref_frame_stride,
                       int64_t dist_frame_stride, const vqa_plane_desc *planes, const int *idx, int count, int depth,
                       float *scratch);
void launch_quality_ms_level(hipStream_t st, const uint8_t *ref, const uint8_t *dist, int n, int64_t ref_frame_stride,
                             int64_t dist_frame_stride, const vqa_plane_desc *planes, const int *idx, int count, int n_planes,
                             double *partials, int64_t partial_plane_stride, vqa_plane_metrics *res, int depth, int level,
                             const float *scratch, vqa_ms_scales *ms);
// a level's fixed-point totals (ssim at `partials`, cs `cs_offset` slots behind) -> ms[frame * n_planes + plane].ssim / cs[level]
void launch_ms_finalize(hipStream_t st, const double *partials, int64_t cs_offset, int bpp, int n, double count,
                        int plane_index, int n_planes, int level, vqa_ms_scales *ms);
// res[e].ssim = prod_{s<4} max(cs_s, 0)^w_s * max(ssim_4, 0)^w_4 for e < n_entries
void launch_ms_combine(hipStream_t st, const vqa_ms_scales *ms, int n_entries, vqa_plane_metrics *res);

// VIF on four scales (vqa_vif_submit): k_vif.hip
constexpr int VIF_LEVELS = 4;
constexpr int VIF_MIN_DIM = 16;   // level 3 of a 16 x 16 plane is 2 x 2: every reflection stays inside its level
// Levels 1..3 of one group of same-geometry planes, as k_vif_decimate writes them: centred fp32 samples, dims floor(dim / 2)
// per level.  Level s starts off[s] floats into the scratch and is laid out [image: ref, dist][frame][plane of the group][h[s]][w[s]].
struct vif_layout {
    int w[VIF_LEVELS], h[VIF_LEVELS];
    int64_t off[VIF_LEVELS];   // off[0] unused (level 0 is the caller's memory)
    int64_t total;             // floats
};
inline vif_layout vif_levels(int n, int count, int h, int w)
{
    vif_layout L;
    L.w[0] = w; L.h[0] = h; L.off[0] = 0;
    int64_t at = 0;
    for (int s = 1; s < VIF_LEVELS; s++) {
        L.w[s] = L.w[s - 1] / 2;
        L.h[s] = L.h[s - 1] / 2;
        L.off[s] = at;
        at += 2 * (int64_t)n * count * L.h[s] * L.w[s];
    }
    L.total = at;
    return L;
}
// level `level` (1..3) of both images from level - 1, filtered with the taps of scale `level`, even rows and columns only
void launch_vif_decimate(hipStream_t st, const uint8_t *ref, const uint8_t *dist, int n, int64_t ref_frame_stride,
                         int64_t dist_frame_stride, const vqa_plane_desc *planes, const int *idx, int count, int depth,
                         int level, float *scratch);
// one level's num / den, added to acc[((frame * n_planes + plane) * 4 + level) * 2 + {0, 1}] in 2^-27 fixed point (acc zeroed
// by the caller; integer atomics: the totals do not depend on the launch geometry or the order of the workgroups)
void launch_vif_stats(hipStream_t st, const uint8_t *ref, const uint8_t *dist, int n, int64_t ref_frame_stride,
                      int64_t dist_frame_stride, const vqa_plane_desc *planes, const int *idx, int count, int n_planes,
                      int depth, int level, const float *scratch, long long *acc);
void launch_vif_finalize(hipStream_t st, const long long *acc, int n_entries, vqa_vif_metrics *res);

// ADM on four scales (vqa_adm_submit): k_adm.hip
constexpr int ADM_LEVELS = 4;
constexpr int ADM_MIN_DIM = 16;   // the bands of scale 3 of a 16 x 16 plane are 1 x 1
// The input of every scale of one group of same-geometry planes: level 0 is the caller's planes, level s > 0 the a bands of scale
// s - 1 as k_adm_scale writes them (fp32, dims ceil(dim / 2) per level); level 4 is never stored, its dims are the bands of
// scale 3.  Level s starts off[s] floats into the scratch and is laid out [image: ref, dist][frame][plane of the group][h[s]][w[s]].
struct adm_layout {
    int w[ADM_LEVELS + 1], h[ADM_LEVELS + 1];
    int64_t off[ADM_LEVELS];   // off[0] unused (level 0 is the caller's memory)
    int64_t total;             // floats
};
inline adm_layout adm_levels(int n, int count, int h, int w)
{
    adm_layout L;
    L.w[0] = w; L.h[0] = h; L.off[0] = 0;
    int64_t at = 0;
    for (int s = 1; s <= ADM_LEVELS; s++) {
        L.w[s] = (L.w[s - 1] + 1) / 2;
        L.h[s] = (L.h[s - 1] + 1) / 2;
        if (s < ADM_LEVELS) {
            L.off[s] = at;
            at += 2 * (int64_t)n * count * L.h[s] * L.w[s];
        }
    }
    L.total = at;
    return L;
}
// workgroups (32 x 16 band samples each) that cover the bands of one plane at one scale: the tiling depends on nothing else
inline int adm_tiles(int bh, int bw) { return ((bw + 31) / 32) * ((bh + 15) / 16); }
// the pooled region of a bh x bw band: rows [top, bottom), columns [left, right)
struct adm_region { int top, bottom, left, right; int64_t area; };
inline adm_region adm_region_of(int bh, int bw)
{
    adm_region r;
    r.left = (int)(bw * 0.1 - 0.5);
    r.top = (int)(bh * 0.1 - 0.5);
    r.right = bw - r.left;
    r.bottom = bh - r.top;
    r.area = (int64_t)(r.bottom - r.top) * (r.right - r.left);
    return r;
}
// the contrast sensitivity weights of scale s: rf[h] = rf[v] = 1 / Q(s, 1), rf[d] = 1 / Q(s, 2) (include/vqa.h)
void adm_rf(int scale, double *rf_hv, double *rf_d);
// one scale of a group: reads level `scale`, writes the a bands (level scale + 1, scales 0..2) into `scratch` and one partial of six
// doubles (num h, v, d; den h, v, d: sums of cubes over the region) per workgroup into part[frame][plane of the group][tile][6]
void launch_adm_scale(hipStream_t st, const uint8_t *ref, const uint8_t *dist, int n, int64_t ref_frame_stride,
                      int64_t dist_frame_stride, const vqa_plane_desc *planes, const int *idx, int count, int depth, int scale,
                      float *scratch, double *part);
// the partials of that launch, added in a fixed order into sums[((frame * n_planes + plane) * 4 + scale) * 6 + k]
void launch_adm_reduce(hipStream_t st, const double *part, int n, const vqa_plane_desc *planes, const int *idx, int count,
                       int n_planes, int scale, double *sums);
// six sums per scale -> the record: cube roots and quotients in double, on the host (h x w: the plane)
void adm_finalize(const double *sums, int h, int w, vqa_adm_metrics *out);

// VMAF's motion feature (vqa_motion_submit): k_motion.hip
constexpr int MOTION_MIN_DIM = 16;
constexpr int MOTION_RADIUS = 2;
// the 5-tap blur of include/vqa.h; the device uses each tap rounded once to fp32
constexpr double MOTION_TAPS[5] = {0.054488685, 0.244201342, 0.402619947, 0.244201342, 0.054488685};
// one group of same-geometry planes of n reference frames: frame i against frame i - 1 (frame 0 against prev0; nullptr: frame 0
// is skipped and keeps its zero).  Adds sum |blur(x_i) - blur(x_{i-1})| in 2^-16 fixed point into acc[frame * n_planes + plane],
// which the caller has zeroed.
void launch_motion_sad(hipStream_t st, const uint8_t *ref, const uint8_t *prev0, int n, int64_t frame_stride,
                       const vqa_plane_desc *planes, const int *idx, int count, int n_planes, int depth, long long *acc);

// ITU-T P.910 spatial and temporal information (vqa_siti_submit): k_siti.hip
constexpr int SITI_MIN_DIM = 16;
constexpr int SITI_WORDS = 5;                 // per (frame, plane): lo, hi (grad_fix = hi 2^32 + lo), grad_sq, diff_sum, diff_sq
constexpr double SITI_FIX = 4294967296.0;     // 2^32: the quantum of the summed gradient magnitudes is 2^-32
// one group of same-geometry planes of n reference frames: Sobel on the interior of frame i, frame i against frame i - 1 (frame 0
// against prev0; nullptr: frame 0 forms its gradient sums only).  Adds the five integer words into
// acc[(frame * n_planes + plane) * SITI_WORDS ..], which the caller has zeroed.
void launch_siti(hipStream_t st, const uint8_t *ref, const uint8_t *prev0, int n, int64_t frame_stride,
                 const vqa_plane_desc *planes, const int *idx, int count, int n_planes, int depth, unsigned long long *acc);
// five words -> the record: the divisions and square roots of include/vqa.h in double, on the host (h x w: the plane)
void siti_finalize(const unsigned long long *words, int h, int w, int depth, vqa_siti_metrics *out);

// PSNR-HVS and PSNR-HVS-M (vqa_psnr_hvs_submit): k_psnr_hvs.hip
constexpr int PSNR_HVS_MIN_DIM = 16;
constexpr int PSNR_HVS_WORDS = 4;                  // per (frame, plane): S_hvs lo, hi and S_hvsm lo, hi (a sum = hi 2^32 + lo)
constexpr float PSNR_HVS_FIX = 1048576.f;          // 2^20: the quantum of a block's two sums is 2^-20
constexpr double PSNR_HVS_CSF_SCALE = 25.735088;   // csf = scale / Q
constexpr int PSNR_HVS_Q[8][8] = {                 // JPEG Annex K, luminance
    {16, 11, 10, 16, 24, 40, 51, 61},     {12, 12, 14, 19, 26, 58, 60, 55},     {14, 13, 16, 24, 40, 57, 69, 56},
    {14, 17, 22, 29, 51, 87, 80, 62},     {18, 22, 37, 56, 68, 109, 103, 77},   {24, 35, 55, 64, 81, 104, 113, 92},
    {49, 64, 78, 87, 103, 121, 120, 101}, {72, 92, 95, 98, 112, 100, 103, 99}};
// one group of same-geometry planes of n frame pairs: the whole 8x8 blocks of every plane.  Adds the four integer words into
// acc[(frame * n_planes + plane) * PSNR_HVS_WORDS ..], which the caller has zeroed.
void launch_psnr_hvs(hipStream_t st, const uint8_t *ref, const uint8_t *dist, int n, int64_t ref_frame_stride,
                     int64_t dist_frame_stride, const vqa_plane_desc *planes, const int *idx, int count, int n_planes, int depth,
                     unsigned long long *acc);
// four words -> the record: the divisions and logarithms of include/vqa.h in double, on the host (h x w: the plane)
void psnr_hvs_finalize(const unsigned long long *words, int h, int w, int depth, vqa_psnr_hvs_metrics *out);

// CIEDE2000 (vqa_ciede_submit): k_ciede.hip
constexpr int CIEDE_MIN_DIM = 16;
constexpr float CIEDE_FIX = 1048576.f;             // 2^20: the quantum of a pixel's dE00 is 2^-20
constexpr float CIEDE_SATURATE = 4096.f;           // 2^12: a pixel counts min(dE00, 4096) (include/vqa.h)
// n frame pairs of three planes (checked by the caller: plane 0 the full grid, planes 1 and 2 of one geometry, the grid's or its
// ceil-half in either direction).  Adds each frame's integer word into acc[frame], which the caller has zeroed.
void launch_ciede(hipStream_t st, const uint8_t *ref, const uint8_t *dist, int n, int64_t ref_frame_stride,
                  int64_t dist_frame_stride, const vqa_plane_desc *planes, int depth, int model, const double *weights,
                  unsigned long long *acc);
// the word -> the record: the division and the logarithm of include/vqa.h in double, on the host (h x w: the luma grid)
void ciede_finalize(unsigned long long word, int h, int w, vqa_ciede_metrics *out);

// GMSD (vqa_gmsd_submit): k_gmsd.hip
constexpr int GMSD_MIN_DIM = 16;
constexpr int GMSD_WORDS = 3;                      // per (frame, plane): sum u, and sum u^2 as lo, hi (the sum = hi 2^32 + lo)
constexpr double GMSD_FIX = 16777216.0;            // 2^24: u = rint(gms 2^24)
constexpr double GMSD_T8 = 170.0;                  // the paper's constant on the 8-bit scale: T = 170 (peak / 255)^2
// 144 T for a depth, as the kernel and vqa.h use it: 144 (170 ((peak / 255) (peak / 255))), every step rounded to double
double gmsd_constant(int depth);
// one group of same-geometry planes of n frame pairs.  Adds the three integer words into
// acc[(frame * n_planes + plane) * GMSD_WORDS ..], which the caller has zeroed.
void launch_gmsd(hipStream_t st, const uint8_t *ref, const uint8_t *dist, int n, int64_t ref_frame_stride,
                 int64_t dist_frame_stride, const vqa_plane_desc *planes, const int *idx, int count, int n_planes, int depth,
                 unsigned long long *acc);
// three words -> the record: the 128-bit variance numerator, the division and the square root of include/vqa.h, on the host
// (h x w: the plane)
void gmsd_finalize(const unsigned long long *words, int h, int w, vqa_gmsd_metrics *out);

// CAMBI (vqa_cambi_submit): k_cambi.hip
constexpr int CAMBI_MIN_DIM = 16;
constexpr int CAMBI_SCALES = 5;
constexpr int CAMBI_WINDOW = 65;                   // the contrast window, centred: 32 samples each way
constexpr int CAMBI_TILE = 32;                     // k_cambi_contrast's tile (the tests' seam shape follows it)
constexpr int CAMBI_MASK_HITS = 24;                // m0 = more than 24 of the 49 Z in the 7 x 7 window
constexpr int CAMBI_WORDS = 2 * CAMBI_SCALES;      // per (frame, plane): top[5], then masked[5]
constexpr int CAMBI_HIST_WORDS = 256 * 257;        // the histogram of u = 0 .. 65536 (65537 bins), rounded up for k_cambi_topk
// device scratch of one group of `count` same-geometry planes of ONE frame: the five scales as 16-bit words and the histogram
size_t cambi_scratch_bytes(int count, int h, int w);
// K_s = max(1, 3 N_s / 10) of an h x w plane
int64_t cambi_top_count(int h, int w, int scale);
// what launch_cambi calls around the launches of one kernel id, so that the caller can bracket them with that id's events:
// mark(ctx, id, 1) before them, mark(ctx, id, 0) after them
typedef void (*cambi_mark)(void *ctx, int kernel_id, int begin);
// one group of same-geometry planes of n frames: every scale's masked count and top-K sum into
// acc[(frame * n_planes + plane) * CAMBI_WORDS ..], which the caller has zeroed.  scratch: n * cambi_scratch_bytes(count, h, w)
void launch_cambi(hipStream_t st, const uint8_t *frames, int n, int64_t frame_stride, const vqa_plane_desc *planes, const int *idx,
                  int count, int n_planes, int depth, void *scratch, unsigned long long *acc, cambi_mark mark, void *mark_ctx);
// ten words -> the record: pool and cambi of include/vqa.h in double, on the host (h x w: the plane)
void cambi_finalize(const unsigned long long *words, int h, int w, vqa_cambi_metrics *out);

// XPSNR (vqa_xpsnr_submit): k_xpsnr.hip
constexpr int XPSNR_MIN_DIM = 16;
// the block grid and the activity grid of a W x H luma plane, as include/vqa.h states them
struct xpsnr_geom {
    int block;      // B
    int nbx, nby;   // ceil(W / B), ceil(H / B)
    int bv;         // 1, or 2 above 2048 x 1152 samples
    int gw, gh;     // the activity grid G: floor(W / bv) x floor(H / bv)
    double rho;     // W H / (3840 * 2160)
};
xpsnr_geom xpsnr_geometry(int w, int h);
// the device words of one frame: nbx nby pairs (sa, ta), then per plane of the submit nbx nby words sse
inline size_t xpsnr_frame_words(const xpsnr_geom &g, int n_planes) { return (size_t)g.nbx * g.nby * (2 + n_planes); }
// sa and ta of the luma plane (planes[0]) of n reference frames; frame 0's predecessor is prev0 (nullptr: none).  Adds into
// words[frame * frame_words + 2 k ..], which the caller has zeroed.
void launch_xpsnr_act(hipStream_t st, const uint8_t *ref, const uint8_t *prev0, int n, int64_t ref_frame_stride,
                      const vqa_plane_desc &luma, const xpsnr_geom &g, int depth, size_t frame_words, unsigned long long *words);
// sse per block of one group of same-geometry planes of n frame pairs.  Adds into
// words[frame * frame_words + (2 + plane) nbx nby + k], which the caller has zeroed.
void launch_xpsnr_sse(hipStream_t st, const uint8_t *ref, const uint8_t *dist, int n, int64_t ref_frame_stride,
                      int64_t dist_frame_stride, const vqa_plane_desc *planes, const int *idx, int count, const xpsnr_geom &g,
                      int depth, size_t frame_words, unsigned long long *words);
// one frame's device words -> its n_planes records, and (blocks != nullptr) its nbx nby (3 + n_planes) words of the weight map:
// the host part of include/vqa.h in double
void xpsnr_finalize(const unsigned long long *words, const xpsnr_geom &g, int depth, int n_planes, const int *pw, const int *ph,
                    vqa_xpsnr_metrics *out, uint64_t *blocks);

// HaarPSI (vqa_haarpsi_submit): k_haarpsi.hip
constexpr int HAARPSI_MIN_DIM = 16;
constexpr int HAARPSI_WORDS = 3;                   // per (frame, plane): den, and num as lo, hi (num = hi 2^32 + lo)
constexpr double HAARPSI_FIX = 1073741824.0;       // 2^30: u = rint(2^30 / (1 + exp(-alpha ls)))
constexpr double HAARPSI_ALPHA = 4.2;              // the paper's alpha
constexpr double HAARPSI_C8 = 30.0;                // the paper's C on the 8-bit scale
// 30 (k k), k = peak / 255, every step rounded to double once: c_s = 4^(s+2) times it, which is exact
double haarpsi_constant(int depth);
// U1 = rint(2^30 / (1 + exp(-alpha))): u where the local similarity is exactly 1, formed on the host
unsigned long long haarpsi_u1();
// one group of same-geometry planes of n frame pairs.  Adds the three integer words into
// acc[(frame * n_planes + plane) * HAARPSI_WORDS ..], which the caller has zeroed.
void launch_haarpsi(hipStream_t st, const uint8_t *ref, const uint8_t *dist, int n, int64_t ref_frame_stride,
                    int64_t dist_frame_stride, const vqa_plane_desc *planes, const int *idx, int count, int n_planes, int depth,
                    unsigned long long *acc);
// three words -> the record: the 128-bit quotient and the two logits of include/vqa.h, on the host
void haarpsi_finalize(const unsigned long long *words, vqa_haarpsi_metrics *out);

// VCA texture features (vqa_vca_submit): k_vca.hip
constexpr int VCA_MIN_DIM = 32;                    // one whole 32 x 32 block
constexpr int VCA_WORDS = 3;                       // per (frame, plane): e_sum, h_sum, l_sum
constexpr int VCA_TABLE_FLOATS = 48 * 64;          // T in both operand orders and w, as the lanes hold them
void vca_tables(float *tabs);
// the block grids of a submit's planes and where each plane's blocks start in a map slot (in blocks; 3 words a block)
struct vca_geom {
    int nbx[4], nby[4], off[4];
    size_t slot_words;   // 3 sum_p nbx nby: one frame's map
};
vca_geom vca_geometry(const int *pw, const int *ph, int n_planes);
// qH, S, qL of every block of one group of same-geometry planes of n frames, and of prev0 (nullptr: none) into the slot before
// frame 0's.  map: frame 0's slot.
void launch_vca_blocks(hipStream_t st, const uint8_t *ref, const uint8_t *prev0, int n, int64_t frame_stride,
                       const vqa_plane_desc *planes, const int *idx, int count, const vca_geom &g, int depth, const float *tabs,
                       unsigned long long *map);
// the three words of n frames and every plane from the map: acc[(frame * n_planes + plane) * VCA_WORDS ..].  first_has_prev: the
// slot before frame 0's is filled.
void launch_vca_sum(hipStream_t st, int n, int n_planes, const vca_geom &g, bool first_has_prev, const unsigned long long *map,
                    unsigned long long *acc);
// three words -> the record: E, h and L of include/vqa.h in double, on the host
void vca_finalize(const unsigned long long *words, int nbx, int nby, int depth, vqa_vca_metrics *out);

// no-reference blockiness, blur and noise (vqa_artifacts_submit): k_artifacts.hip
constexpr int ARTIFACTS_MIN_DIM = 16;              // the family's limit
constexpr int ARTIFACTS_WORDS = 21;                // per (frame, plane): edge_h[8], edge_v[8], blur_f_h, blur_v_h, blur_f_v, blur_v_v, lap
constexpr double ARTIFACTS_SQRT_HALF_PI = 1.2533141373155003;   // the double nearest sqrt(pi / 2)
// the 21 integer sums of n frames of one group of same-geometry planes, added to acc[(frame * n_planes + plane) *
// ARTIFACTS_WORDS ..], which the caller has zeroed
void launch_artifacts(hipStream_t st, const uint8_t *frames, int n, int64_t frame_stride, const vqa_plane_desc *planes,
                      const int *idx, int count, int n_planes, int depth, unsigned long long *acc);
// 21 words -> the record: the phases, blockiness, blur and noise of include/vqa.h in double, on the host
void artifacts_finalize(const unsigned long long *words, int h, int w, int depth, vqa_artifacts_metrics *out);

// BRISQUE's natural-scene statistics (vqa_brisque_submit): k_brisque.hip
constexpr int BRISQUE_MIN_DIM = 16;                // the family's limit
constexpr int BRISQUE_Q = 16;                      // u = rint(m 2^Q)
constexpr int BRISQUE_WORDS = 60;                  // per (frame, plane): 30 per scale - sum |u|, sum u^2 and per orientation n_neg,
                                                   // n_pos, sum |p|, sum p^2 over p < 0 (low 32 bits, the rest), over p > 0 (likewise)
// bytes of scratch one frame of a group of `count` h x w planes needs: the scale-1 planes and the four strips
size_t brisque_scratch_bytes(int count, int h, int w);
// what launch_brisque calls around the launches of one kernel id, so that the caller can bracket them with that id's events
typedef void (*brisque_mark)(void *ctx, int kernel_id, int begin);
// the 60 integer sums of n frames of one group of same-geometry planes, added to acc[(frame * n_planes + plane) *
// BRISQUE_WORDS ..], which the caller has zeroed; scratch: n * brisque_scratch_bytes(count, h, w)
void launch_brisque(hipStream_t st, const uint8_t *frames, int n, int64_t frame_stride, const vqa_plane_desc *planes,
                    const int *idx, int count, int n_planes, int depth, void *scratch, unsigned long long *acc,
                    brisque_mark mark, void *mark_arg);
// 60 words -> the record: the fits and the 36 features of include/vqa.h in double, on the host
void brisque_finalize(const unsigned long long *words, int h, int w, vqa_brisque_metrics *out);

// MDSI (vqa_mdsi_submit): k_mdsi.hip
constexpr int MDSI_MIN_DIM = 16;                   // the limit of plane 0 (the chroma planes of 4:2:0 may be 8 x 8)
constexpr int MDSI_WORDS = 4;                      // per frame: A, B, n_neg, D (include/vqa.h)
constexpr double MDSI_FIX_G = 16777216.0;          // 2^24: g = rint(GCS 2^24)
constexpr double MDSI_FIX_Z = 268435456.0;         // 2^28: zq = rint(|g 2^-24|^(1/4) 2^28)
// f = max(1, floor(min(h, w) / 256 + 0.5)), in integers
int mdsi_factor(int h, int w);
// bytes of scratch one frame needs: the map of g, 4 bytes per downsampled sample
size_t mdsi_scratch_bytes(int h, int w);
// the twelve doubles of include/vqa.h: mat[channel L, H, M][plane 0, 1, 2, count]
void mdsi_matrix(int model, int depth, int f, double mat[3][4]);
// the four words of n frame pairs (planes checked by the caller: one plane, or plane 0 the full grid and planes 1 and 2 of one
// geometry, the grid's or its ceil-half in either direction), added to acc[frame * MDSI_WORDS ..], which the caller has zeroed;
// map: n * mdsi_scratch_bytes(h, w).  mark brackets the launch of each kernel id, as launch_brisque's does
void launch_mdsi(hipStream_t st, const uint8_t *ref, const uint8_t *dist, int n, int64_t ref_frame_stride,
                 int64_t dist_frame_stride, const vqa_plane_desc *planes, int n_planes, int depth, int model, void *map,
                 unsigned long long *acc, brisque_mark mark, void *mark_arg);
// four words -> the record: dev and mdsi of include/vqa.h in double, on the host (h x w: plane 0)
void mdsi_finalize(const unsigned long long *words, int h, int w, vqa_mdsi_metrics *out);

// dE_ITP (vqa_itp_submit): k_itp.hip
constexpr int ITP_MIN_DIM = 16;                    // the luma grid's limit (the chroma planes of 4:2:0 may be 8 x 8)
constexpr int ITP_WORDS = 2;                       // per frame: the sum and the maximum of q = rint(dE 2^20) (include/vqa.h)
constexpr double ITP_FIX = 1048576.0;              // 2^20: the quantum of a pixel's dE is 2^-20; dE < 2^13, no saturation
// n frame pairs of three planes (checked by the caller: plane 0 the full grid, planes 1 and 2 of one geometry, the grid's or its
// ceil-half in either direction; model, transfer and full_range known values).  Adds each frame's sum into acc[frame * ITP_WORDS]
// and raises acc[frame * ITP_WORDS + 1] to its maximum; the caller has zeroed both.
void launch_itp(hipStream_t st, const uint8_t *ref, const uint8_t *dist, int n, int64_t ref_frame_stride,
                int64_t dist_frame_stride, const vqa_plane_desc *planes, int depth, int model, int transfer, int full_range,
                unsigned long long *acc);
// two words -> the record: the divisions of include/vqa.h in double, on the host (h x w: the luma grid)
void itp_finalize(const unsigned long long *words, int h, int w, vqa_itp_metrics *out);

// PU21-PSNR / PU21-SSIM (vqa_pu21_submit): k_pu21.hip
constexpr int PU21_MIN_DIM = 16;                   // the luma grid's limit (the chroma planes of 4:2:0 may be 8 x 8)
constexpr int PU21_WORDS = 5;                      // per frame: sse_y lo, hi; sse_rgb lo, hi; ssim_q (include/vqa.h)
constexpr double PU21_FIX = 65536.0;               // 2^16: q = rint(V 2^16), below 2^26
constexpr double PU21_SSIM_FIX = 16777216.0;       // 2^24: u = rint(ssim 2^24)
constexpr double PU21_PEAK = 256.0;                // the peak of both PSNRs: PU21 puts 100 cd/m2 at 256
constexpr double PU21_C1 = (0.01 * 256.0) * (0.01 * 256.0), PU21_C2 = (0.03 * 256.0) * (0.03 * 256.0);
constexpr int PU21_SSIM_TILE = 16;                 // k_pu21_ssim: a workgroup owns 16 x 16 windows (26 x 26 samples of both maps)
constexpr size_t PU21_MAP_BUDGET = (size_t)1 << 28;   // the two maps of a sub-slice of frames stay within 256 MiB
// the bytes of the two q_Y maps of one frame: 8 per luma sample
inline size_t pu21_map_bytes(int h, int w) { return 2 * sizeof(uint32_t) * (size_t)h * (size_t)w; }
// n frame pairs of three planes (checked by the caller as for launch_itp).  Writes q_Y of both images into map
// [frame][2][h][w] and adds each frame's four squared-error half-words into acc[frame * PU21_WORDS + 0..3]; the caller has zeroed them.
void launch_pu21_encode(hipStream_t st, const uint8_t *ref, const uint8_t *dist, int n, int64_t ref_frame_stride,
                        int64_t dist_frame_stride, const vqa_plane_desc *planes, int depth, int model, int transfer,
                        int full_range, uint32_t *map, unsigned long long *acc);
// the Gaussian SSIM of n frames of the map -> adds each frame's signed sum of u into acc[frame * PU21_WORDS + 4]
void launch_pu21_ssim(hipStream_t st, const uint32_t *map, int n, int h, int w, unsigned long long *acc);
// V(cd/m2) of include/vqa.h, on the host
double pu21_encode_host(double cd_m2);
// five words -> the record: the joins and divisions of include/vqa.h in double, on the host (h x w: the luma grid)
void pu21_finalize(const unsigned long long *words, int h, int w, vqa_pu21_metrics *out);

// FSIM / FSIMc (vqa_fsim_submit): k_fsim.hip
constexpr int FSIM_MIN_DIM = 16;                   // the limit of plane 0 (the chroma planes of 4:2:0 may be 8 x 8)
constexpr int FSIM_MAX_GRID = 1024;                // the limit of either side of the downsampled grid
constexpr int FSIM_WORDS = 3;                      // per frame: P, A, B (include/vqa.h)
constexpr double FSIM_FIX = 16777216.0;            // 2^24: p = rint(PC 2^24), g = rint(S_L 2^24), gc = rint(S_L C 2^24)
constexpr int FSIM_IMAGE_DOUBLES = 35;             // scratch doubles per downsampled sample of ONE image: Y, I, Q; the row
                                                   // transform (2); F (2); the half and the whole inverse of the four scales of one
                                                   // orientation (8 + 8); Energy, An, |EO_0|^2 of the four orientations (12)
constexpr size_t FSIM_SCRATCH_BUDGET = (size_t)1 << 28;   // the scratch of a sub-slice of frames stays within 256 MiB
constexpr int FSIM_MAX_SUBSLICE = 4096;            // frames of a sub-slice at most (a launch's grid is 8 per frame in z)
// the per-geometry tables on the device: the two DFT matrices ([2][hd][hd] and [2][wd][wd] doubles: real parts, then imaginary
// ones), the sixteen filter tables [orientation][scale][hd wd], and the noise factors c_o
struct fsim_tabs {
    double *wh = nullptr, *ww = nullptr, *filt = nullptr;
    double c[4] = {0, 0, 0, 0};
};
// f of mdsi_factor and the downsampled grid ceil(h / f) x ceil(w / f)
void fsim_grid(int h, int w, int *f, int *hd, int *wd);
// the bytes of scratch ONE FRAME (both images) takes
size_t fsim_scratch_bytes(int h, int w);
// the host's tables, in double: filt_{scale,orient} (hd wd doubles); all sixteen (filt may be null) with the four c_o; c_o alone;
// the DFT matrix of length n (2 n n doubles)
void fsim_filter_host(int hd, int wd, int scale, int orient, double *dst);
void fsim_bank_host(int hd, int wd, double *filt, double c[4]);
double fsim_noise_factor_host(int hd, int wd, int orient);
void fsim_twiddle_host(int n, double *dst);
// [Y, I, Q][plane 0, 1, 2, count]: the channels from the box SUMS of the integer samples and the count of in-plane positions
void fsim_matrix(int model, int depth, int f, double mat[3][4]);
// the three words of n frame pairs (planes checked by the caller as for launch_mdsi), added to acc[frame * FSIM_WORDS ..], which
// the caller has zeroed; scratch: n * fsim_scratch_bytes(h, w); pmap: [n][2][hd wd] uint32, the p maps (ref, then dist).  mark
// brackets the launches of each kernel id, as launch_brisque's does
void launch_fsim(hipStream_t st, const uint8_t *ref, const uint8_t *dist, int n, int64_t ref_frame_stride,
                 int64_t dist_frame_stride, const vqa_plane_desc *planes, int n_planes, int depth, int model,
                 const fsim_tabs &tabs, void *scratch, uint32_t *pmap, unsigned long long *acc, brisque_mark mark, void *mark_arg);
// three words -> the record: the divisions of include/vqa.h in double, on the host (h x w: plane 0)
void fsim_finalize(const unsigned long long *words, int h, int w, vqa_fsim_metrics *out);

// Signal statistics (vqa_sigstats_submit): k_sigstats.hip
constexpr int SIGSTATS_MIN_DIM = 16;   // the limit of the family, whose planes it shares
// the words of an entry on the device, all uint64 (the four box words in two's complement): k_sigstats_scan stores the words up
// to SIG_ABOVE_PEAK and the box, k_sigstats_accum adds or ORs the other four into words the submit has zeroed
enum sigstats_word {
    SIG_COUNT, SIG_SUM, SIG_SUM_SQ, SIG_MIN, SIG_MAX, SIG_LOW, SIG_MEDIAN, SIG_HIGH, SIG_BELOW_BLACK, SIG_UNDER, SIG_OVER_LUMA,
    SIG_OVER_CHROMA, SIG_ABOVE_PEAK, SIG_OR, SIG_NAND /* the OR of ~x */, SIG_SAD, SIG_CHANGED, SIG_TOP, SIG_BOTTOM, SIG_LEFT,
    SIG_RIGHT, SIGSTATS_WORDS
};
constexpr size_t SIGSTATS_HIST_BUDGET = (size_t)1 << 28;   // the histograms of a sub-slice of frames stay within 256 MiB
// the bins of an entry's histogram: the sample TYPE's range, not the depth's
inline int sigstats_bins(int depth) { return depth > 8 ? 65536 : 256; }
// n frames of one group of same-geometry planes: the histograms hist[(frame * n_planes + plane) * bins ..], the words SIG_OR,
// SIG_NAND, SIG_SAD, SIG_CHANGED of acc[(frame * n_planes + plane) * SIGSTATS_WORDS ..] and the row and column sums
// prof[frame * prof_words + prof_off[plane] ..] (height row sums, then width column sums); the caller has zeroed all three
void launch_sigstats_accum(hipStream_t st, const uint8_t *ref, const uint8_t *prev0, int n, int64_t frame_stride,
                           const vqa_plane_desc *planes, const int *idx, int count, int n_planes, int depth,
                           const int *prof_off, int prof_words, uint32_t *hist, unsigned long long *acc, unsigned long long *prof);
// the remaining words of the n * n_planes entries from their histograms and profiles
void launch_sigstats_scan(hipStream_t st, int n, const vqa_plane_desc *planes, int n_planes, int depth, int black_level,
                          int crop_level, const int *prof_off, int prof_words, const uint32_t *hist,
                          const unsigned long long *prof, unsigned long long *acc);
// the words -> the record; mean, stdev and dif in double on the host (include/vqa.h)
void sigstats_finalize(const unsigned long long *words, int depth, vqa_sigstats_metrics *out);

// The resampler (vqa_scale_submit): k_scale.hip
constexpr int SCALE_MIN_DIM = 16;       // the limit of the family, on both sides
constexpr int SCALE_BITS = 22;          // the tables are integers in 2^-22 fixed point
constexpr int SCALE_KSIZE_MAX = 25;     // 2 ceil(3 * 4) + 1: lanczos at 4x down
constexpr int SCALE_TILE_W = 64, SCALE_TILE_H = 32;   // a workgroup's tile of the destination plane
// the source footprint of a tile that k_scale's LDS holds: 63 * 4 + 2 * 12 + 2 = 278 columns and 31 * 4 + 26 = 150 rows at the
// limits; the submit checks every tile of the tables it built against both
constexpr int SCALE_FW = 288, SCALE_FH = 152;
constexpr int SCALE_RC = 16;            // the source rows of one chunk of the footprint
bool scale_filter_known(int filter);
bool scale_ratio_ok(int in, int out);   // 1/4 <= out / in <= 8
int scale_ksize(int filter, int in, int out);
// one axis' tables on the host, as include/vqa.h states them: k[out][ksize] (0 past count), xmin[out], count[out]
void scale_build_axis(int filter, int in, int out, int32_t *k, int32_t *xmin, int32_t *count);
// the most source samples the windows of `tile` consecutive outputs span, over the tiles of an axis
int scale_footprint(const int32_t *xmin, const int32_t *count, int out, int tile);
// one group of planes alike on both sides; every stride in bytes, the tables in device memory
struct scale_job {
    const uint8_t *src;
    uint8_t *dst;
    int64_t src_fs, dst_fs;            // frame strides
    int64_t src_off[4], dst_off[4];    // plane offsets inside a frame
    int64_t src_rs, dst_rs;            // row strides
    int src_step, dst_step;
    int sw, sh, dw, dh;
    int peak;                          // 2^depth - 1
    int peak_x;                        // what the horizontal pass clips to: peak, or the sample type's largest value where the
                                       // width does not change - that pass is a copy, and a copy does not clip
    const int32_t *kx, *xmin, *xcount, *ky, *ymin, *ycount;
    int ksx, ksy;
};
// n frames of `count` planes (the job's offsets): grid (tiles, n, count)
void launch_scale(hipStream_t st, const scale_job &job, int n, int count, int depth);

// Conform (vqa_conform_submit): k_conform.hip
constexpr int CONFORM_MIN_DIM = 16;         // the limit of plane 0 of the destination (the other planes: 8, the chroma of 4:2:0)
constexpr int CONFORM_MAX_OUT = 32768;      // output frames of one submit (they ride in gridDim.y)
constexpr int CONFORM_LDS_DEPTH = 12;       // up to this depth the tables sit in LDS: 2^12 samples a plane
constexpr int CONFORM_LDS_SAMPLES = 1 << CONFORM_LDS_DEPTH;
constexpr int64_t CONFORM_MAX_COEF = 1ll << 20, CONFORM_MAX_BIAS = 1ll << 33;   // |M[k][i]|, i < 3; |M[k][3]|
// one plane of a job: the window's corner in the source plane, the window's size, both sides' addressing in bytes.  inter > 1:
// `inter` planes that interleave on both sides, taken as one plane of inter times the samples (w and x0 count those); lut0: the
// table of the plane (of the first of the interleaved planes)
struct conform_plane {
    int64_t src_off, dst_off, src_rs, dst_rs;
    int src_step, dst_step;
    int w, h, y0, x0;
    int inter, lut0;
};
struct conform_job {
    const uint8_t *src;
    uint8_t *dst;
    int64_t src_fs, dst_fs;
    const int32_t *index;              // on the device; null: output frame j is source frame j
    const void *lut;                   // on the device: [planes][2^depth] of the sample type; null: none
    long long m[3][4];                 // the matrix path only
    conform_plane plane[4];
    int peak;                          // 2^depth - 1
};
// the source cells the matrix path walks (filled by launch_conform_matrix)
struct conform_cells {
    int sh, sw, ch, cw;                // the source's luma and chroma sizes
    int sx, sy;                        // the chroma shifts
    int cy0, cy1, X0, patches, tiles_x;
};
// n_out frames of the job's first `count` planes: window, gather and table; gather: a lane a sample (any pixel step)
void launch_conform_copy(hipStream_t st, const conform_job &job, int n_out, int count, int depth, bool gather);
// n_out frames of three planes taken together, the job's m applied after its table; sh x sw, ch x cw: the SOURCE planes' sizes
void launch_conform_matrix(hipStream_t st, const conform_job &job, int sh, int sw, int ch, int cw, int n_out, int depth);

// Convert (vqa_convert_submit): k_convert.hip
constexpr int CONVERT_MIN_DIM = 16;         // the limit of plane 0 on both sides (the other planes: 8, the chroma of 4:2:0)
constexpr int CONVERT_MAX_FRAMES = 32768;   // frames of one submit (they ride in gridDim.y)
enum convert_relation { CONVERT_SAME = 0, CONVERT_UP = 1, CONVERT_DOWN = 2 };
// the relation of one axis by include/vqa.h's rule, or -1 where there is none
inline int convert_relation_of(int n_s, int n_d)
{
    if (n_d == n_s) return CONVERT_SAME;
    if (n_s == (n_d + 1) >> 1) return CONVERT_UP;
    if (n_d == (n_s + 1) >> 1) return CONVERT_DOWN;
    return -1;
}
// one plane of a job: both sides' sizes and addressing in bytes, the relation per axis.  pair: the vertical relation is UP and
// the destination's row stride is a multiple of 16, so a lane of k_convert_rows takes its granule in the two destination rows
// that the same two source rows feed
struct convert_plane {
    int64_t src_off, dst_off, src_rs, dst_rs;
    int src_step, dst_step;
    int sw, sh, dw, dh;
    int rx, ry, pair;
};
struct convert_job {
    const uint8_t *src;
    uint8_t *dst;
    int64_t src_fs, dst_fs;
    convert_plane plane[4];
    int chroma, siting, range;         // vqa_convert_chroma, vqa_convert_siting, vqa_convert_range
    int ds, dd;                        // the two depths
    float inv_ps;                      // VQA_RANGE_FULL: 1 / Ps, the first guess of the one division
};
// n frames of the job's first `count` planes.  gather false: k_convert_rows, the planes have a contiguous pixel step on both
// sides and share ONE horizontal relation `rx`; gather true: k_convert_gather, a lane a sample, any pixel step and relation
void launch_convert(hipStream_t st, const convert_job &job, int n, int count, int rx, bool gather);

// Fields and weave (vqa_fields_submit, vqa_weave_submit): k_fields.hip
constexpr int FIELDS_MIN_DIM = 16;          // the limit of the measured plane
constexpr int FIELDS_BAND_ROWS = 32;        // the rows a lane of k_fields_accum marches (even: a band starts on a top-field row)
constexpr int FIELDS_WORDS = 10;            // the sums a frame keeps on the device: [comb, fwd, bwd, sad, changed][parity]
constexpr int FIELDS_MAX_FRAMES = 32768;    // frames of one submit (they ride in gridDim.y)
constexpr int WEAVE_MIN_DIM = 16;           // the limit of plane 0 (the other planes: 8, the chroma of 4:2:0)
constexpr int WEAVE_MAX_OUT = 32768;        // output frames of one submit (they ride in gridDim.y)
// n frames of one plane, frame i against frame i - 1 and frame 0 against prev0 (null: it has none): adds the FIELDS_WORDS sums of
// frame i into acc[i * FIELDS_WORDS ..], which the caller has zeroed
void launch_fields_accum(hipStream_t st, const uint8_t *frames, const uint8_t *prev0, int n, int64_t frame_stride,
                         const vqa_plane_desc &plane, int depth, unsigned long long *acc);
// a weave: conform's planes (y0 = x0 = 0, no table) and the source frame of the even and of the odd rows of every output frame
struct weave_job {
    const uint8_t *src;
    uint8_t *dst;
    int64_t src_fs, dst_fs;
    const int32_t *top, *bottom;       // on the device: [n_out] each
    conform_plane plane[4];
};
// n_out frames of the job's first `count` planes; gather: a lane a sample (any pixel step)
void launch_fields_weave(hipStream_t st, const weave_job &job, int n_out, int count, int depth, bool gather);

// Temporal alignment (vqa_align_submit): k_align.hip
constexpr int ALIGN_MAX_DIST = 32768, ALIGN_MAX_REF = 32768 + 64;   // frames of one submit
// One launch for the whole band of the whole submit: adds C[j][i] = sum X_d,j X_r,i into cross[j * (2 radius + 1) + c] for the pairs
// of the band (c = i - j - offset + radius, 0 <= i < n_ref), sum X_d,j^2 into e_dist[j] and sum X_r,i^2 into e_ref[i] for every
// frame some pair of the band names; two's complement uint64 words the submit has zeroed.  false: no pair of the band exists
// and nothing was launched.  |offset| must be small enough for 16 n + offset + radius to stay inside int: the caller launches
// only where a pair exists, which bounds it by the frame counts.
bool launch_align_cross(hipStream_t st, const uint8_t *ref, int n_ref, const uint8_t *dist, int n_dist, int64_t ref_frame_stride,
                        int64_t dist_frame_stride, const vqa_plane_desc &plane, int depth, int offset, int radius,
                        unsigned long long *cross, unsigned long long *e_dist, unsigned long long *e_ref);

// Spatial registration (vqa_shift_submit): k_shift.hip
constexpr int SHIFT_MAX_FRAMES = 32768;   // frames of one submit (they ride in gridDim.y)
constexpr int SHIFT_ROWS = 8;             // reference rows of a workgroup's visit
// the 16 x 16 tiles per axis that cover the 2R + 1 shifts of an axis: 1 (R <= 7), 2 (R <= 15), 3 (R = 16)
constexpr int shift_tiles(int radius) { return (2 * radius + 16) / 16; }
// row blocks of the reference rows M - R .. h - M + R - 1 a core row can meet
constexpr int shift_row_blocks(int h, int radius, int margin) { return (h - 2 * margin + 2 * radius + SHIFT_ROWS - 1) / SHIFT_ROWS; }
// gridDim.x: every row block its own workgroup while the launch stays below 2^31 threads of 64-lane workgroups, else the
// workgroups stride over the blocks
constexpr int shift_grid_x(int blocks, int n, int tiles)
{
    const int64_t cap = (int64_t(1) << 25) / ((int64_t)n * tiles);
    return (int)(blocks < cap ? blocks : (cap > 1 ? cap : 1));
}
// One launch per submit: adds E_r(dy, dx) - 2 C(dy, dx) of frame j into out[(j (2R + 1) + dy + R) (2R + 1) + dx + R] and the core's
// sum of X_d^2 into e_dist[j]; two's complement uint64 words the submit has zeroed.  The caller has checked 1 <= radius <= 16,
// margin >= radius, h, w >= 2 margin + 1 and n <= SHIFT_MAX_FRAMES.
void launch_shift(hipStream_t st, const uint8_t *ref, const uint8_t *dist, int n, int64_t ref_frame_stride, int64_t dist_frame_stride,
                  const vqa_plane_desc &plane, int depth, int radius, int margin, unsigned long long *out, unsigned long long *e_dist);

// HDR light levels and gamut QC (vqa_light_submit): k_light.hip
constexpr int LIGHT_MIN_DIM = 16;                  // the luma grid's limit (the chroma planes of 4:2:0 may be 8 x 8)
constexpr int LIGHT_BINS = VQA_LIGHT_BINS;         // the histogram of m >> 4
constexpr int LIGHT_WALK = 8;                      // chunks of 256 patches a workgroup walks before it flushes (16384 pixels)
constexpr int LIGHT_SUB_FRAMES = 16384;            // frames of one sub-slice: their histograms stay within 256 MiB
// the words of a frame: sums, maxima (LIGHT_MAX_Y .. LIGHT_MIN_INV: raised, not added), counts, then pct_bin[10]
enum light_word {
    LIGHT_SUM_Q, LIGHT_SUM_Y, LIGHT_MAX_Y, LIGHT_MAX_R, LIGHT_MAX_G, LIGHT_MAX_B, LIGHT_MAX_M,
    LIGHT_MIN_INV,   // the largest 65535 - m: the smallest m, in a word the submit can zero
    LIGHT_OUT_709, LIGHT_OUT_P3, LIGHT_CLAMPED, LIGHT_PCT,
    LIGHT_WORDS = LIGHT_PCT + VQA_LIGHT_PERCENTILES
};
// n frames of three planes of one stream (checked by the caller as for launch_itp).  Adds / raises the first LIGHT_PCT words of
// acc[frame * LIGHT_WORDS ..] and counts m >> 4 into hist[frame * LIGHT_BINS ..]; the caller has zeroed both.  table: T[65536] on
// the device.
void launch_light_accum(hipStream_t st, const uint8_t *frames, int n, int64_t frame_stride, const vqa_plane_desc *planes, int depth,
                        int model, int full_range, const unsigned long long *table, uint32_t *hist, unsigned long long *acc);
// the ten percentile bins of n frames of h x w pixels off their histograms -> acc[frame * LIGHT_WORDS + LIGHT_PCT ..]
void launch_light_scan(hipStream_t st, int n, int h, int w, const uint32_t *hist, unsigned long long *acc);
// vqa_light_table's PQ table and vqa_light_gamut's matrix (false: an unknown gamut), in double on the host
void light_table_host(uint64_t *table);
bool light_gamut_host(int gamut, int64_t m[9]);
// the words -> the record: the doubles of include/vqa.h, on the host (h x w: the luma grid; table: the call's, on the host)
void light_finalize(const unsigned long long *words, int h, int w, const uint64_t *table, vqa_light_metrics *out);

// Clip-wide sync (vqa_sig_submit, vqa_sig_cross_submit): k_sig.hip
// the signatures of n frames of one plane (at least 16 x 16, checked by the caller) -> out[frame * VQA_SIG_BYTES ..], every byte
// written; n rides in gridDim.y (<= VQA_SIG_MAX_BATCH)
void launch_sig(hipStream_t st, const uint8_t *frames, int n, int64_t frame_stride, const vqa_plane_desc &plane, int depth,
                uint8_t *out);
// dist_sig [n_dist][256] and ref_sig [n_ref][256] on the device, 16-byte aligned.  diag: adds the sums of D along every diagonal
// into diag[k + n_dist - 1], n_dist + n_ref - 1 words the caller has zeroed.  best: writes every word of best[n_dist].
void launch_sig_diag(hipStream_t st, const uint8_t *dist_sig, int n_dist, const uint8_t *ref_sig, int n_ref, unsigned long long *diag);
void launch_sig_best(hipStream_t st, const uint8_t *dist_sig, int n_dist, const uint8_t *ref_sig, int n_ref, unsigned long long *best);

// Colour registration (vqa_colorfit_submit): k_colorfit.hip
constexpr int COLORFIT_MIN_DIM = 16;   // the luma grid's limit (the chroma planes of 4:2:0 may be 8 x 8)
constexpr int COLORFIT_WALK = 8;       // chunks of 256 patches a workgroup walks before it flushes (16384 positions)
// the words of a frame: sum_r[3], sum_d[3], rr[6], rd[9], dd[3] of vqa_colorfit_metrics, in its order
enum colorfit_word { COLORFIT_SUM_R = 0, COLORFIT_SUM_D = 3, COLORFIT_RR = 6, COLORFIT_RD = 12, COLORFIT_DD = 21, COLORFIT_WORDS = 24 };
// the bins of one plane's transfer table
constexpr int colorfit_bins(int depth) { return 1 << (depth < 10 ? depth : 10); }
// n frame pairs of one or three planes (checked by the caller as for launch_ciede; n rides in gridDim.y).  Adds into
// acc[frame * COLORFIT_WORDS ..] and, unless tables is null, into tables[plane][bin][3] of the whole call; the caller has zeroed both.
void launch_colorfit(hipStream_t st, const uint8_t *ref, const uint8_t *dist, int n, int64_t ref_frame_stride,
                     int64_t dist_frame_stride, const vqa_plane_desc *planes, int n_planes, int depth, unsigned long long *acc,
                     unsigned long long *tables);
// the words -> the record (h x w: the luma grid): count, the words, and sse = dd - 2 rd + rr of the planes the submit had
void colorfit_finalize(const unsigned long long *words, int h, int w, int n_planes, vqa_colorfit_metrics *out);

} // namespace vqa
