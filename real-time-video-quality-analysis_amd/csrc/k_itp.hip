// k_itp.hip — dE_ITP (ITU-R BT.2124) for gfx950: the HDR colour difference of every pixel of a frame pair, the three planes taken
// together, by the definition stated in include/vqa.h (vqa_itp_submit).
//
//   k_itp<T, MODEL, TRANSFER, VEC>   one fused launch per submit, the tiling and the loads of k_ciede: ONE THREAD OWNS A 2 x 4 LUMA
//                        PATCH of both images, the patches of a frame are numbered in raster order and a workgroup of 64 threads
//                        (one wave) owns 64 consecutive numbers.  A thread reads its two rows of four samples of every plane once
//                        (halved chroma: two samples per row, one row per two luma rows), as one load per row when the layout
//                        allows it (VEC) and sample by sample otherwise; the rows stay packed in 64-bit registers, four 16-bit
//                        fields each, and ONE loop that is not unrolled walks the eight pixels.  load4 / load2x2 / load_chroma are
//                        k_ciede's, copied: that kernel stays as it is.  There is no LDS and no barrier.
//
// Precision: the whole per-pixel chain is DOUBLE, contraction off, every step rounded once in the order vqa.h writes it.  In
// fp32 the PQ EOTF's E'^(1/m2) - c1 cancels on dark pixels and the 6.28th power that follows multiplies what is left: up to 0.1
// per pixel, 7e-4 on a frame's mean.  The powers are the accurate library pow / exp.
//
// Code size: a pixel pair takes 24 double powers (PQ; six per pixel in the EOTF, six in the inverse, two images).  Inlined 24
// times they would not fit the instruction cache, so the three channels of a stage and the two images of a pair go through
// loops that are NOT unrolled and ROTATE their registers (a, b, c) <- (b, c, f(a)) instead of indexing an array (which would
// live in scratch): four pow sites per kernel.
//
// Sums (vqa.h states the bounds): a pixel's dE is below 2^13, so q = rint(dE 2^20) is below 2^33; q is added as a 64-bit
// integer - in the thread, across the wave, then one atomicAdd per workgroup - and the largest q goes the same way through one
// atomicMax: two words per frame.  Integer addition and maximum are associative and commutative: neither the tiling nor the
// order in which workgroups retire can change a bit.
#include <cmath>

#include "vqa_dev.hpp"
#include "vqa_kernels.hpp"

namespace vqa {

namespace {

// both images of n frames of three planes; every stride in bytes.  Plane 0 (Y, or B) is the full-size grid; planes 1 and 2
// (Cb and Cr, or G and R) share one geometry, the grid's or its ceil-half in either direction (sh, sv).
struct itp_src {
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
__device__ __forceinline__ void load_chroma(const itp_src &s, const uint8_t *base, int py, int px, unsigned long long (&r)[2])
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

__device__ __forceinline__ unsigned long long wave_max(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long t = __shfl_down(v, o, 64);
        v = t > v ? t : v;
    }
    return v; // valid in lane 0
}

struct itp3 { double i, t, p; };

// a non-linear signal in [0, 1] -> display light in cd/m2 (the PQ EOTF; 0 -> 0, 1 -> 10000)
__device__ __forceinline__ double pq_eotf(double e)
{
#pragma clang fp contract(off)
    const double ep = pow(e, 1.0 / PQ_M2);
    const double num = fmax(ep - PQ_C1, 0.0), den = PQ_C2 - PQ_C3 * ep;   // den >= c2 - c3 > 0 for e <= 1
    return 10000.0 * pow(num / den, 1.0 / PQ_M1);
}

// display light in cd/m2 -> the PQ signal (the inverse EOTF)
__device__ __forceinline__ double pq_inverse(double x)
{
#pragma clang fp contract(off)
    const double yp = pow(x / 10000.0, PQ_M1);
    return pow((PQ_C1 + PQ_C2 * yp) / (1.0 + PQ_C3 * yp), PQ_M2);
}

// an HLG signal in [0, 1] -> scene light in [0, 1] (the inverse OETF)
__device__ __forceinline__ double hlg_scene(double e)
{
#pragma clang fp contract(off)
    return e <= 0.5 ? e * e / 3.0 : (exp((e - HLG_C) / HLG_A) + HLG_B) / 12.0;
}

// the three integer samples of a pixel (MODEL 0: Y, Cb, Cr; 1: B, G, R) -> I, T = Ct / 2, Cp of vqa.h
template <int MODEL, int TRANSFER> __device__ __forceinline__ itp3 to_itp(int p0, int p1, int p2, const itp_src &s)
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
    double l = ((1688.0 * r + 2146.0 * g) + 262.0 * b) / 4096.0;
    double m = ((683.0 * r + 2951.0 * g) + 462.0 * b) / 4096.0;
    double c = ((99.0 * r + 309.0 * g) + 3688.0 * b) / 4096.0;
#pragma unroll 1
    for (int k = 0; k < 3; k++) {
        const double f = pq_inverse(l);
        l = m; m = c; c = f;
    }
    itp3 o;
    o.i = 0.5 * (l + m);
    o.t = 0.5 * (((6610.0 * l - 13613.0 * m) + 7003.0 * c) / 4096.0);
    o.p = ((17933.0 * l - 17390.0 * m) - 543.0 * c) / 4096.0;
    return o;
}

// grid = (workgroups, n_frames); block = 64.  acc: [frame][2] uint64 (sum, maximum), zeroed by the submit
template <typename T, int MODEL, int TRANSFER, bool VEC>
__global__ __launch_bounds__(64) void k_itp(itp_src s, unsigned long long *__restrict__ acc)
{
#pragma clang fp contract(off)
    const int f = blockIdx.y;
    const int patch = blockIdx.x * 64 + (int)threadIdx.x;
    unsigned long long sum = 0, mx = 0;
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
#pragma unroll 1
        for (int k = 0; k < 8; k++) {
            const int r = k >> 2, c = k & 3;
            if (r >= rows || c >= cols) continue;
            const int sft = 16 * c;
            int x0 = (int)(((r ? ra[0][1] : ra[0][0]) >> sft) & 0xffffu), y0 = (int)(((r ? rb[0][1] : rb[0][0]) >> sft) & 0xffffu);
            int x1 = (int)(((r ? ra[1][1] : ra[1][0]) >> sft) & 0xffffu), y1 = (int)(((r ? rb[1][1] : rb[1][0]) >> sft) & 0xffffu);
            int x2 = (int)(((r ? ra[2][1] : ra[2][0]) >> sft) & 0xffffu), y2 = (int)(((r ? rb[2][1] : rb[2][0]) >> sft) & 0xffffu);
            if (x0 == y0 && x1 == y1 && x2 == y2) continue;   // equal triples: exactly 0
            // both colours through ONE copy of the chain: (x, y) <- (y, x), the result of the first kept in q
            itp3 p = {0.0, 0.0, 0.0}, q = p;
#pragma unroll 1
            for (int img = 0; img < 2; img++) {
                q = p;
                p = to_itp<MODEL, TRANSFER>(x0, x1, x2, s);
                x0 = y0; x1 = y1; x2 = y2;
            }
            const double di = p.i - q.i, dt = p.t - q.t, dp = p.p - q.p;
            const double de = 720.0 * sqrt((di * di + dt * dt) + dp * dp);
            const unsigned long long v = __double2ull_rn(de * ITP_FIX);   // below 2^33
            sum += v;
            mx = v > mx ? v : mx;
        }
    }
    sum = wave_sum(sum);
    mx = wave_max(mx);
    if (threadIdx.x == 0 && sum) {   // (a zero sum has a zero maximum)
        atomicAdd(acc + 2 * (size_t)f, sum);
        atomicMax(acc + 2 * (size_t)f + 1, mx);
    }
}

template <typename T, int MODEL, int TRANSFER>
void launch_tmt(hipStream_t st, const itp_src &s, bool vec, dim3 grid, unsigned long long *acc)
{
    if (vec) hipLaunchKernelGGL((k_itp<T, MODEL, TRANSFER, true>), grid, dim3(64), 0, st, s, acc);
    else hipLaunchKernelGGL((k_itp<T, MODEL, TRANSFER, false>), grid, dim3(64), 0, st, s, acc);
}

template <typename T, int MODEL>
void launch_tm(hipStream_t st, const itp_src &s, int transfer, bool vec, dim3 grid, unsigned long long *acc)
{
    if (transfer == VQA_ITP_PQ) launch_tmt<T, MODEL, VQA_ITP_PQ>(st, s, vec, grid, acc);
    else launch_tmt<T, MODEL, VQA_ITP_HLG>(st, s, vec, grid, acc);
}

} // namespace

void launch_itp(hipStream_t st, const uint8_t *ref, const uint8_t *dist, int n, int64_t ref_frame_stride,
                int64_t dist_frame_stride, const vqa_plane_desc *planes, int depth, int model, int transfer, int full_range,
                unsigned long long *acc)
{
    if (n <= 0) return;
    itp_src s;
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
    // plane 0, and 4 or (halved) 2 samples of planes 1 and 2 (k_ciede's rule)
    uint64_t bits0 = (uint64_t)(uintptr_t)ref | (uint64_t)(uintptr_t)dist | (uint64_t)s.rs0 | (uint64_t)s.off[0];
    if (n > 1) bits0 |= (uint64_t)ref_frame_stride | (uint64_t)dist_frame_stride;
    const uint64_t bits1 = bits0 | (uint64_t)s.rs1 | (uint64_t)s.off[1] | (uint64_t)s.off[2];
    const int a0 = 4 * bps, a1 = (s.sh ? 2 : 4) * bps;
    const bool vec = s.step0 == bps && s.step1 == bps && s.w % 4 == 0 && (bits0 & (uint64_t)(a0 - 1)) == 0 &&
                     (bits1 & (uint64_t)(a1 - 1)) == 0;
    const dim3 grid((s.npatch + 63) / 64, n);
    if (depth > 8) {
        if (model == VQA_ITP_YUV2020) launch_tm<uint16_t, VQA_ITP_YUV2020>(st, s, transfer, vec, grid, acc);
        else launch_tm<uint16_t, VQA_ITP_BGR>(st, s, transfer, vec, grid, acc);
    } else {
        if (model == VQA_ITP_YUV2020) launch_tm<uint8_t, VQA_ITP_YUV2020>(st, s, transfer, vec, grid, acc);
        else launch_tm<uint8_t, VQA_ITP_BGR>(st, s, transfer, vec, grid, acc);
    }
}

// the two words -> the record, in double on the host.  Contraction is off: the record is the formula vqa.h states.
void itp_finalize(const unsigned long long *words, int h, int w, vqa_itp_metrics *out)
{
#pragma clang fp contract(off)
    out->sum_q = words[0];
    out->max_q = words[1];
    out->de_sum = (double)words[0] * (1.0 / ITP_FIX);   // (the conversion is exact below 2^53; the bound of a frame is 2^61)
    out->de_mean = out->de_sum / ((double)h * (double)w);
    out->de_max = (double)words[1] * (1.0 / ITP_FIX);
}

} // namespace vqa
