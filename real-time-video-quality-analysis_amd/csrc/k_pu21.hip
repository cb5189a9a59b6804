// k_pu21.hip — PU21 HDR quality (PU21-PSNR, PU21-SSIM) for gfx950: the three planes of a pixel read as a PQ or HLG BT.2020
// signal, turned into display light, PU21-encoded and quantised once, by the definition stated in include/vqa.h
// (vqa_pu21_submit).  Two kernels per sub-slice of frames:
//
//   k_pu21_encode<T, MODEL, TRANSFER, VEC>   the tiling and the loads of k_itp: ONE THREAD OWNS A 2 x 4 LUMA PATCH of both images, a
//                        workgroup of 64 threads (one wave) owns 64 consecutive patches; no LDS and no barrier.  load4 / load2x2 /
//                        load_chroma and the signal -> display light chain are k_itp's, copied: that kernel stays as it is.  It
//                        writes q_Y = rint(V(Y) 2^16) of both images into the map [frame][2][h][w] uint32 and adds the four
//                        half-words of the two squared-error sums (luminance; the three channels).
//   k_pu21_ssim          a workgroup of 256 threads owns a 16 x 16 tile of the valid-window grid: it loads the 26 x 26 samples of
//                        both maps as doubles into LDS, filters the five moments (x_r, x_d, x_r^2, x_d^2, x_r x_d) horizontally into
//                        LDS (26 rows x 16 columns each), and ONE THREAD PER WINDOW runs the vertical pass and forms
//                        u = rint(ssim 2^24).  LDS: 2 * 26 * 26 * 8 + 5 * 26 * 16 * 8 + 32 = 27488 bytes a workgroup: two workgroups
//                        fit 64 KB, five fit a compute unit's 160 KB.
//
// Precision: everything is DOUBLE with contraction off, every step rounded once in the order vqa.h writes it.
//
// Code size: a pixel pair takes 28 double powers under PQ (six in the EOTF, eight in the four PU21 encodings, two images).  The
// channels of a stage and the two images of a pair go through loops that are NOT unrolled and ROTATE their registers, as in
// k_itp: four pow sites per kernel.
//
// Sums: q is below 2^26, so a squared difference is below 2^52; its low 32 bits and its bits above them are added into two
// 64-bit words (a frame has at most 3 * 2^28 terms: both stay below 2^62).  u is a signed 64-bit sum.  Integer addition is
// associative and commutative: neither the tiling nor the order in which workgroups retire can change a bit.  A window's value is
// a fixed-order sum of the same doubles whichever tile or thread computes it.
#include <cmath>

#include "vqa_dev.hpp"
#include "vqa_kernels.hpp"

namespace vqa {

namespace {

// both images of n frames of three planes; every stride in bytes.  Plane 0 (Y, or B) is the full-size grid; planes 1 and 2
// (Cb and Cr, or G and R) share one geometry, the grid's or its ceil-half in either direction (sh, sv).
struct pu21_src {
    const uint8_t *ref, *dist;
    int64_t ref_fs, dist_fs;   // frame strides
    int64_t off[3];            // plane offsets inside a frame
    int64_t rs0, rs1;          // row strides of plane 0 and of planes 1, 2
    int step0, step1;          // pixel steps likewise
    int w, h, cw, ch;          // the grid; planes 1, 2
    int sh, sv;                // 1: planes 1, 2 are halved in width / height
    int pw, npatch;            // patches per row of patches, patches per frame
    int o0, o12;               // YUV limited: 16 s and 128 s; YUV full: 0 and 2^(depth-1); BGR: 0
    double d0, d12;            // YUV limited: 219 s and 224 s; YUV full and BGR: 2^depth - 1
};

// BT.2100 PQ
constexpr double PQ_M1 = 2610.0 / 16384.0, PQ_M2 = 2523.0 / 4096.0 * 128.0;
constexpr double PQ_C1 = 3424.0 / 4096.0, PQ_C2 = 2413.0 / 4096.0 * 32.0, PQ_C3 = 2392.0 / 4096.0 * 32.0;
// BT.2100 HLG
constexpr double HLG_A = 0.17883277, HLG_B = 0.28466892, HLG_C = 0.55991073;
// PU21, the banding_glare fit
constexpr double PU_P1 = 0.353487901, PU_P2 = 0.3734658629, PU_P3 = 8.277049286e-05, PU_P4 = 0.9062562627;
constexpr double PU_P5 = 0.09150303166, PU_P6 = 0.9099517204, PU_P7 = 596.3148142;
constexpr double PU_LMIN = 0.005, PU_LMAX = 10000.0;

// four samples of a row -> four 16-bit fields (field j = sample j); VEC: one load; else the first `valid` samples, one by one
template <typename T, bool VEC> __device__ __forceinline__ unsigned long long load4(const uint8_t *p, int step, int valid)
{
    if constexpr (VEC && sizeof(T) == 1) {
        const unsigned long long u = *reinterpret_cast<const uint32_t *>(p);
        return (u & 0xffull) | ((u & 0xff00ull) << 8) | ((u & 0xff0000ull) << 16) | ((u & 0xff000000ull) << 24);
    } else if constexpr (VEC) {
        const uint2 u = *reinterpret_cast<const uint2 *>(p);
        return (unsigned long long)u.x | ((unsigned long long)u.y << 32);
    } else {
        unsigned long long r = 0;
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (j < valid) r |= (unsigned long long)*reinterpret_cast<const T *>(p + (int64_t)j * step) << (16 * j);
        return r;
    }
}

// two samples of a halved row, each standing for two columns -> fields (s0, s0, s1, s1)
template <typename T, bool VEC> __device__ __forceinline__ unsigned long long load2x2(const uint8_t *p, int step, int valid)
{
    unsigned long long s0 = 0, s1 = 0;
    if constexpr (VEC && sizeof(T) == 1) {
        const unsigned u = *reinterpret_cast<const uint16_t *>(p);
        s0 = u & 0xffu; s1 = u >> 8;
    } else if constexpr (VEC) {
        const uint32_t u = *reinterpret_cast<const uint32_t *>(p);
        s0 = u & 0xffffu; s1 = u >> 16;
    } else {
        if (valid > 0) s0 = *reinterpret_cast<const T *>(p);
        if (valid > 1) s1 = *reinterpret_cast<const T *>(p + step);
    }
    return s0 * 0x00010001ull | s1 * 0x0001000100000000ull;
}

// the two rows of a patch of planes 1 and 2 of one image, expanded to the luma grid
template <typename T, bool VEC>
__device__ __forceinline__ void load_chroma(const pu21_src &s, const uint8_t *base, int py, int px, unsigned long long (&r)[2])
{
    const int y0 = (2 * py) >> s.sv, y1 = (2 * py + 1) >> s.sv;       // y1 may lie below the plane when sv = 0: not loaded then
    if (s.sh) {
        const uint8_t *p = base + (int64_t)y0 * s.rs1 + (int64_t)(2 * px) * s.step1;
        const int valid = s.cw - 2 * px;
        r[0] = load2x2<T, VEC>(p, s.step1, valid);
        r[1] = (y1 != y0 && y1 < s.ch) ? load2x2<T, VEC>(p + s.rs1, s.step1, valid) : r[0];
    } else {
        const uint8_t *p = base + (int64_t)y0 * s.rs1 + (int64_t)(4 * px) * s.step1;
        const int valid = s.cw - 4 * px;
        r[0] = load4<T, VEC>(p, s.step1, valid);
        r[1] = (y1 != y0 && y1 < s.ch) ? load4<T, VEC>(p + s.rs1, s.step1, valid) : r[0];
    }
}

// a non-linear signal in [0, 1] -> display light in cd/m2 (the PQ EOTF; 0 -> 0, 1 -> 10000)
__device__ __forceinline__ double pq_eotf(double e)
{
#pragma clang fp contract(off)
    const double ep = pow(e, 1.0 / PQ_M2);
    const double num = fmax(ep - PQ_C1, 0.0), den = PQ_C2 - PQ_C3 * ep;   // den >= c2 - c3 > 0 for e <= 1
    return 10000.0 * pow(num / den, 1.0 / PQ_M1);
}

// an HLG signal in [0, 1] -> scene light in [0, 1] (the inverse OETF)
__device__ __forceinline__ double hlg_scene(double e)
{
#pragma clang fp contract(off)
    return e <= 0.5 ? e * e / 3.0 : (exp((e - HLG_C) / HLG_A) + HLG_B) / 12.0;
}

// cd/m2 -> q = rint(V 2^16), V the PU21 encoding of vqa.h; below 2^26
__device__ __forceinline__ unsigned pu21_q(double l)
{
#pragma clang fp contract(off)
    l = fmin(fmax(l, PU_LMIN), PU_LMAX);
    const double lp = pow(l, PU_P4);
    const double v = fmax(PU_P7 * (pow((PU_P1 + PU_P2 * lp) / (1.0 + PU_P3 * lp), PU_P5) - PU_P6), 0.0);
    return __double2uint_rn(v * PU21_FIX);
}

struct pu4 { unsigned y, r, g, b; };

// the three integer samples of a pixel (MODEL 0: Y, Cb, Cr; 1: B, G, R) -> q of the luminance and of the three channels
template <int MODEL, int TRANSFER> __device__ __forceinline__ pu4 to_pu(int p0, int p1, int p2, const pu21_src &s)
{
#pragma clang fp contract(off)
    double r, g, b;
    if constexpr (MODEL == VQA_ITP_YUV2020) {
        const double y = (double)(p0 - s.o0) / s.d0, cb = (double)(p1 - s.o12) / s.d12, cr = (double)(p2 - s.o12) / s.d12;
        r = y + 1.4746 * cr;
        b = y + 1.8814 * cb;
        g = ((y - 0.2627 * r) - 0.0593 * b) / 0.6780;
    } else {
        b = (double)p0 / s.d0; g = (double)p1 / s.d0; r = (double)p2 / s.d0;
    }
    r = fmin(fmax(r, 0.0), 1.0); g = fmin(fmax(g, 0.0), 1.0); b = fmin(fmax(b, 0.0), 1.0);
    // the signal -> display light, channel by channel: (r, g, b) <- (g, b, f(r)) three times
#pragma unroll 1
    for (int k = 0; k < 3; k++) {
        double f;
        if constexpr (TRANSFER == VQA_ITP_PQ) f = pq_eotf(r);
        else f = hlg_scene(r);
        r = g; g = b; b = f;
    }
    if constexpr (TRANSFER == VQA_ITP_HLG) {   // the OOTF of a 1000 cd/m2 display: gamma 1.2, black level 0
        const double ys = (0.2627 * r + 0.6780 * g) + 0.0593 * b;
        const double k = ys > 0.0 ? 1000.0 * pow(ys, 0.2) : 0.0;
        r = k * r; g = k * g; b = k * b;
    }
    double l = (0.2627 * r + 0.6780 * g) + 0.0593 * b;
    // the four encodings: (l, r, g, b) <- (r, g, b, l) with q rotating behind them
    pu4 o = {0u, 0u, 0u, 0u};
#pragma unroll 1
    for (int k = 0; k < 4; k++) {
        const unsigned v = pu21_q(l);
        l = r; r = g; g = b; b = 0.0;
        o.y = o.r; o.r = o.g; o.g = o.b; o.b = v;
    }
    return o;
}

// grid = (workgroups, n_frames); block = 64.  map: [frame][2][h][w] uint32; acc: [frame][PU21_WORDS] uint64, zeroed by the submit
template <typename T, int MODEL, int TRANSFER, bool VEC>
__global__ __launch_bounds__(64) void k_pu21_encode(pu21_src s, uint32_t *__restrict__ map, unsigned long long *__restrict__ acc)
{
#pragma clang fp contract(off)
    const int f = blockIdx.y;
    const int patch = blockIdx.x * 64 + (int)threadIdx.x;
    unsigned long long y_lo = 0, y_hi = 0, c_lo = 0, c_hi = 0;
    if (patch < s.npatch) {
        const int py = patch / s.pw, px = patch - py * s.pw;
        const int rows = min(2, s.h - 2 * py), cols = min(4, s.w - 4 * px);
        const uint8_t *fr = s.ref + (int64_t)f * s.ref_fs, *fd = s.dist + (int64_t)f * s.dist_fs;
        const int64_t o0 = s.off[0] + (int64_t)(2 * py) * s.rs0 + (int64_t)(4 * px) * s.step0;
        unsigned long long ra[3][2], rb[3][2];   // [plane][row]: four 16-bit fields
        ra[0][0] = load4<T, VEC>(fr + o0, s.step0, cols);
        rb[0][0] = load4<T, VEC>(fd + o0, s.step0, cols);
        ra[0][1] = rows > 1 ? load4<T, VEC>(fr + o0 + s.rs0, s.step0, cols) : 0ull;
        rb[0][1] = rows > 1 ? load4<T, VEC>(fd + o0 + s.rs0, s.step0, cols) : 0ull;
        load_chroma<T, VEC>(s, fr + s.off[1], py, px, ra[1]);
        load_chroma<T, VEC>(s, fr + s.off[2], py, px, ra[2]);
        load_chroma<T, VEC>(s, fd + s.off[1], py, px, rb[1]);
        load_chroma<T, VEC>(s, fd + s.off[2], py, px, rb[2]);
        const size_t plane = (size_t)s.h * (size_t)s.w;
        uint32_t *mr = map + (size_t)f * 2 * plane, *md = mr + plane;
#pragma unroll 1
        for (int k = 0; k < 8; k++) {
            const int r = k >> 2, c = k & 3;
            if (r >= rows || c >= cols) continue;
            const int sft = 16 * c;
            int x0 = (int)(((r ? ra[0][1] : ra[0][0]) >> sft) & 0xffffu), y0 = (int)(((r ? rb[0][1] : rb[0][0]) >> sft) & 0xffffu);
            int x1 = (int)(((r ? ra[1][1] : ra[1][0]) >> sft) & 0xffffu), y1 = (int)(((r ? rb[1][1] : rb[1][0]) >> sft) & 0xffffu);
            int x2 = (int)(((r ? ra[2][1] : ra[2][0]) >> sft) & 0xffffu), y2 = (int)(((r ? rb[2][1] : rb[2][0]) >> sft) & 0xffffu);
            const bool same = x0 == y0 && x1 == y1 && x2 == y2;   // equal triples: the second chain is skipped
            // both images through ONE copy of the chain: (x, y) <- (y, x), the result of the first kept in q
            pu4 p = {0u, 0u, 0u, 0u}, q = p;
#pragma unroll 1
            for (int img = 0; img < 2; img++) {
                q = p;
                if (img == 0 || !same) p = to_pu<MODEL, TRANSFER>(x0, x1, x2, s);
                x0 = y0; x1 = y1; x2 = y2;
            }
            const size_t at = (size_t)(2 * py + r) * (size_t)s.w + (size_t)(4 * px + c);   // row < h and column < w: checked above
            mr[at] = q.y;
            md[at] = p.y;
            const long long dy = (long long)q.y - (long long)p.y, dr = (long long)q.r - (long long)p.r;
            const long long dg = (long long)q.g - (long long)p.g, db = (long long)q.b - (long long)p.b;
            const unsigned long long ty = (unsigned long long)(dy * dy), tr = (unsigned long long)(dr * dr);   // each below 2^52
            const unsigned long long tg = (unsigned long long)(dg * dg), tb = (unsigned long long)(db * db);
            y_lo += ty & 0xffffffffull; y_hi += ty >> 32;
            c_lo += (tr & 0xffffffffull) + (tg & 0xffffffffull) + (tb & 0xffffffffull);
            c_hi += (tr >> 32) + (tg >> 32) + (tb >> 32);
        }
    }
    y_lo = wave_sum(y_lo); y_hi = wave_sum(y_hi); c_lo = wave_sum(c_lo); c_hi = wave_sum(c_hi);
    if (threadIdx.x == 0 && (y_lo | y_hi | c_lo | c_hi)) {
        unsigned long long *a = acc + (size_t)PU21_WORDS * (size_t)f;
        atomicAdd(a + 0, y_lo);
        atomicAdd(a + 1, y_hi);
        atomicAdd(a + 2, c_lo);
        atomicAdd(a + 3, c_hi);
    }
}

// PU21-SSIM over the map
constexpr int ST = PU21_SSIM_TILE;       // windows of a tile, each way
constexpr int SA = ST + 10;              // samples of a tile with its apron, each way
struct pu21_win { double g[11]; };       // the normalised Gaussian window

// grid = (tiles across, tiles down, n_frames); block = 256, thread (ty, tx) = (tid / 16, tid % 16) owns window (ty, tx) of its tile
__global__ __launch_bounds__(256) void k_pu21_ssim(const uint32_t *__restrict__ map, int h, int w, pu21_win win,
                                                   unsigned long long *__restrict__ acc)
{
#pragma clang fp contract(off)
    __shared__ double xs[2][SA][SA];      // the samples x = q 2^-16 of both maps (outside the frame: 0, feeding no valid window)
    __shared__ double hm[5][SA][ST];      // the five moments after the horizontal pass
    __shared__ long long red[4];
    const int f = blockIdx.z, tid = (int)threadIdx.x;
    const int wx0 = blockIdx.x * ST, wy0 = blockIdx.y * ST;
    const size_t plane = (size_t)h * (size_t)w;
    const uint32_t *mr = map + (size_t)f * 2 * plane, *md = mr + plane;
    for (int i = tid; i < SA * SA; i += 256) {
        const int yy = i / SA, xx = i - yy * SA;
        const int sy = wy0 + yy, sx = wx0 + xx;
        double a = 0.0, b = 0.0;
        if (sy < h && sx < w) {
            const size_t at = (size_t)sy * (size_t)w + (size_t)sx;
            a = (double)mr[at] * (1.0 / PU21_FIX);
            b = (double)md[at] * (1.0 / PU21_FIX);
        }
        xs[0][yy][xx] = a;
        xs[1][yy][xx] = b;
    }
    __syncthreads();
    for (int i = tid; i < SA * ST; i += 256) {
        const int yy = i / ST, xx = i - yy * ST;
        double sr = 0.0, sd = 0.0, srr = 0.0, sdd = 0.0, srd = 0.0;
#pragma unroll
        for (int k = 0; k < 11; k++) {
            const double g = win.g[k], a = xs[0][yy][xx + k], b = xs[1][yy][xx + k];
            sr = sr + g * a;
            sd = sd + g * b;
            srr = srr + g * (a * a);
            sdd = sdd + g * (b * b);
            srd = srd + g * (a * b);
        }
        hm[0][yy][xx] = sr; hm[1][yy][xx] = sd; hm[2][yy][xx] = srr; hm[3][yy][xx] = sdd; hm[4][yy][xx] = srd;
    }
    __syncthreads();
    const int ty = tid / ST, tx = tid - ty * ST;
    long long u = 0;
    if (wy0 + ty < h - 10 && wx0 + tx < w - 10) {
        double mu_r = 0.0, mu_d = 0.0, e_rr = 0.0, e_dd = 0.0, e_rd = 0.0;
#pragma unroll
        for (int k = 0; k < 11; k++) {
            const double g = win.g[k];
            mu_r = mu_r + g * hm[0][ty + k][tx];
            mu_d = mu_d + g * hm[1][ty + k][tx];
            e_rr = e_rr + g * hm[2][ty + k][tx];
            e_dd = e_dd + g * hm[3][ty + k][tx];
            e_rd = e_rd + g * hm[4][ty + k][tx];
        }
        const double var_r = e_rr - mu_r * mu_r, var_d = e_dd - mu_d * mu_d, cov = e_rd - mu_r * mu_d;
        const double num = (2.0 * (mu_r * mu_d) + PU21_C1) * (2.0 * cov + PU21_C2);
        const double den = ((mu_r * mu_r + mu_d * mu_d) + PU21_C1) * ((var_r + var_d) + PU21_C2);
        u = __double2ll_rn((num / den) * PU21_SSIM_FIX);
    }
    u = wave_sum(u);
    if ((tid & 63) == 0) red[tid >> 6] = u;
    __syncthreads();
    if (tid == 0) {
        const long long t = (red[0] + red[1]) + (red[2] + red[3]);
        if (t) atomicAdd(acc + (size_t)PU21_WORDS * (size_t)f + 4, (unsigned long long)t);
    }
}

template <typename T, int MODEL, int TRANSFER>
void launch_tmt(hipStream_t st, const pu21_src &s, bool vec, dim3 grid, uint32_t *map, unsigned long long *acc)
{
    if (vec) hipLaunchKernelGGL((k_pu21_encode<T, MODEL, TRANSFER, true>), grid, dim3(64), 0, st, s, map, acc);
    else hipLaunchKernelGGL((k_pu21_encode<T, MODEL, TRANSFER, false>), grid, dim3(64), 0, st, s, map, acc);
}

template <typename T, int MODEL>
void launch_tm(hipStream_t st, const pu21_src &s, int transfer, bool vec, dim3 grid, uint32_t *map, unsigned long long *acc)
{
    if (transfer == VQA_ITP_PQ) launch_tmt<T, MODEL, VQA_ITP_PQ>(st, s, vec, grid, map, acc);
    else launch_tmt<T, MODEL, VQA_ITP_HLG>(st, s, vec, grid, map, acc);
}

} // namespace

void launch_pu21_encode(hipStream_t st, const uint8_t *ref, const uint8_t *dist, int n, int64_t ref_frame_stride,
                        int64_t dist_frame_stride, const vqa_plane_desc *planes, int depth, int model, int transfer,
                        int full_range, uint32_t *map, unsigned long long *acc)
{
    if (n <= 0) return;
    pu21_src s;
    s.ref = ref; s.dist = dist; s.ref_fs = ref_frame_stride; s.dist_fs = dist_frame_stride;
    for (int i = 0; i < 3; i++) s.off[i] = planes[i].offset;
    s.rs0 = planes[0].row_stride; s.step0 = planes[0].pixel_step;
    s.rs1 = planes[1].row_stride; s.step1 = planes[1].pixel_step;
    s.w = planes[0].width; s.h = planes[0].height;
    s.cw = planes[1].width; s.ch = planes[1].height;
    s.sh = s.cw != s.w; s.sv = s.ch != s.h;
    s.pw = (s.w + 3) / 4;
    s.npatch = s.pw * ((s.h + 1) / 2);
    const int scale = 1 << (depth - 8);
    if (model == VQA_ITP_YUV2020 && !full_range) {
        s.o0 = 16 * scale; s.o12 = 128 * scale;
        s.d0 = (double)(219 * scale); s.d12 = (double)(224 * scale);
    } else {
        s.o0 = 0; s.o12 = model == VQA_ITP_YUV2020 ? 1 << (depth - 1) : 0;
        s.d0 = s.d12 = (double)((1 << depth) - 1);
    }
    const int bps = depth > 8 ? 2 : 1;
    // a row of a patch as one load: unit steps, whole patches, and every address a multiple of the load's size - 4 samples of
    // plane 0, and 4 or (halved) 2 samples of planes 1 and 2 (k_itp's rule)
    uint64_t bits0 = (uint64_t)(uintptr_t)ref | (uint64_t)(uintptr_t)dist | (uint64_t)s.rs0 | (uint64_t)s.off[0];
    if (n > 1) bits0 |= (uint64_t)ref_frame_stride | (uint64_t)dist_frame_stride;
    const uint64_t bits1 = bits0 | (uint64_t)s.rs1 | (uint64_t)s.off[1] | (uint64_t)s.off[2];
    const int a0 = 4 * bps, a1 = (s.sh ? 2 : 4) * bps;
    const bool vec = s.step0 == bps && s.step1 == bps && s.w % 4 == 0 && (bits0 & (uint64_t)(a0 - 1)) == 0 &&
                     (bits1 & (uint64_t)(a1 - 1)) == 0;
    const dim3 grid((s.npatch + 63) / 64, n);
    if (depth > 8) {
        if (model == VQA_ITP_YUV2020) launch_tm<uint16_t, VQA_ITP_YUV2020>(st, s, transfer, vec, grid, map, acc);
        else launch_tm<uint16_t, VQA_ITP_BGR>(st, s, transfer, vec, grid, map, acc);
    } else {
        if (model == VQA_ITP_YUV2020) launch_tm<uint8_t, VQA_ITP_YUV2020>(st, s, transfer, vec, grid, map, acc);
        else launch_tm<uint8_t, VQA_ITP_BGR>(st, s, transfer, vec, grid, map, acc);
    }
}

void launch_pu21_ssim(hipStream_t st, const uint32_t *map, int n, int h, int w, unsigned long long *acc)
{
    if (n <= 0) return;
    pu21_win win;
    double sum = 0.0;
    for (int i = 0; i < 11; i++) {
        win.g[i] = std::exp(-(double)((i - 5) * (i - 5)) / 4.5);
        sum += win.g[i];
    }
    for (int i = 0; i < 11; i++) win.g[i] /= sum;
    const dim3 grid((w - 10 + ST - 1) / ST, (h - 10 + ST - 1) / ST, n);
    hipLaunchKernelGGL(k_pu21_ssim, grid, dim3(256), 0, st, map, h, w, win, acc);
}

// the host statement of V (vqa_pu21_encode): the device's formula, step for step
double pu21_encode_host(double l)
{
#pragma clang fp contract(off)
    l = std::fmin(std::fmax(l, PU_LMIN), PU_LMAX);
    const double lp = std::pow(l, PU_P4);
    return std::fmax(PU_P7 * (std::pow((PU_P1 + PU_P2 * lp) / (1.0 + PU_P3 * lp), PU_P5) - PU_P6), 0.0);
}

// the five words -> the record, in double on the host.  Contraction is off: the record is the formula vqa.h states.
void pu21_finalize(const unsigned long long *words, int h, int w, vqa_pu21_metrics *out)
{
#pragma clang fp contract(off)
    out->sse_y_lo = words[0]; out->sse_y_hi = words[1];
    out->sse_rgb_lo = words[2]; out->sse_rgb_hi = words[3];
    out->ssim_q = (int64_t)words[4];
    out->windows = (int64_t)(h - 10) * (int64_t)(w - 10);
    const unsigned __int128 sy = ((unsigned __int128)words[1] << 32) + (unsigned __int128)words[0];
    const unsigned __int128 sc = ((unsigned __int128)words[3] << 32) + (unsigned __int128)words[2];
    const double hw = (double)h * (double)w;
    out->mse_y = (double)sy / (4294967296.0 * hw);
    out->mse_rgb = (double)sc / (4294967296.0 * (3.0 * hw));
    out->pu_psnr = sy ? 10.0 * std::log10(PU21_PEAK * PU21_PEAK / out->mse_y) : INFINITY;
    out->pu_psnr_rgb = sc ? 10.0 * std::log10(PU21_PEAK * PU21_PEAK / out->mse_rgb) : INFINITY;
    out->pu_ssim = (double)out->ssim_q / (PU21_SSIM_FIX * (double)out->windows);
}

} // namespace vqa
