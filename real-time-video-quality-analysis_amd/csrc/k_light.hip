// k_light.hip — HDR light levels and gamut QC for gfx950: MaxCLL / MaxFALL's per-frame words, the per-channel maxima, the BT.2020
// luminance, the 4096-bin maxRGB histogram with its percentiles and the outside-BT.709 / outside-P3 pixel counts of ONE stream,
// the three planes of a pixel taken together, by the definition stated in include/vqa.h (vqa_light_submit).
//
//   k_light_accum<T, MODEL, VEC>   the input side of k_itp: ONE THREAD OWNS A 2 x 4 LUMA PATCH, the patches of a frame are numbered
//                        in raster order and a chunk is 256 consecutive numbers.  load4 / load2x2 / load_chroma are k_itp's,
//                        copied: that kernel stays as it is.  A workgroup of 256 threads walks LIGHT_WALK consecutive chunks of
//                        ONE frame (16384 pixels) before it flushes, so the 4096-bin flush and the eleven atomics of the other
//                        words are paid once per 16384 pixels.  The decode is a handful of double operations, contraction off
//                        (the file is built with -ffp-contract=off: the Makefile says why the pragma alone is not enough); there
//                        is NO transcendental: the three light values are 8-byte gathers from the 512 KB table of the call.
//                        Histogram: 4096 x 32 bits in LDS.  A thread joins the equal adjacent bins of its eight pixels into one
//                        add, and a wave whose 64 pending adds all name one bin sends ONE - a flat frame costs one LDS atomic per
//                        wave and chunk, not 512.  Non-zero bins leave through 32-bit global atomics.  Every other word goes
//                        through a wave reduction, LDS, and one 64-bit atomicAdd / atomicMax per workgroup.
//   k_light_scan         one workgroup per frame: a thread owns 16 consecutive bins, one block-wide prefix sum, and the thread whose
//                        range holds rank k_p writes pct_bin[p].
//
// Range (vqa.h states the bounds): q < 2^34, |M| < 2^17, |S_k| < 3 2^51; a frame's sums stay below 2^62.  Everything after the one
// rounding is integer addition, maximum and comparison: neither the tiling nor the order in which workgroups retire can change a
// bit.
#include <cmath>

#include "vqa_dev.hpp"
#include "vqa_kernels.hpp"

namespace vqa {

namespace {

// one stream of n frames of three planes; every stride in bytes.  Plane 0 (Y, or B) is the full-size grid; planes 1 and 2
// (Cb and Cr, or G and R) share one geometry, the grid's or its ceil-half in either direction (sh, sv).
struct light_src {
    const uint8_t *frames;
    int64_t fs;                // frame stride
    int64_t off[3];            // plane offsets inside a frame
    int64_t rs0, rs1;          // row strides of plane 0 and of planes 1, 2
    int step0, step1;          // pixel steps likewise
    int w, h, cw, ch;          // the grid; planes 1, 2
    int sh, sv;                // 1: planes 1, 2 are halved in width / height
    int pw, npatch, chunks;    // patches per row of patches, patches per frame, chunks of 256 patches per frame
    int o0, o12;               // YUV limited: 16 s and 128 s; YUV full: 0 and 2^(depth-1); BGR: 0
    double d0, d12;            // YUV limited: 219 s and 224 s; YUV full and BGR: 2^depth - 1
    long long m709[9], mp3[9]; // rint(2^16 A_G), row-major, columns R, G, B
    const unsigned long long *table;   // T[65536] on the device
};

// the words a workgroup reduces (LIGHT_WORDS' first eleven)
constexpr int LIGHT_ACC = 11;

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

// the two rows of a patch of planes 1 and 2, expanded to the luma grid
template <typename T, bool VEC>
__device__ __forceinline__ void load_chroma(const light_src &s, const uint8_t *base, int py, int px, unsigned long long (&r)[2])
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

template <typename V> __device__ __forceinline__ V wave_max(V v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const V t = __shfl_down(v, o, 64);
        v = t > v ? t : v;
    }
    return v; // valid in lane 0
}

// a clamped signal -> its 16-bit code: THE ONE ROUNDING of the definition
__device__ __forceinline__ uint32_t code16(double e)
{
#pragma clang fp contract(off)
    return (uint32_t)(int)rint(fmin(fmax(e, 0.0), 1.0) * 65535.0);
}

// min_k S_k < -((qmax << 16) >> 6) - 2^32
__device__ __forceinline__ bool outside(const long long (&m)[9], long long qr, long long qg, long long qb, long long qmax)
{
    const long long s0 = m[0] * qr + m[1] * qg + m[2] * qb;
    const long long s1 = m[3] * qr + m[4] * qg + m[5] * qb;
    const long long s2 = m[6] * qr + m[7] * qg + m[8] * qb;
    const long long lo = min(s0, min(s1, s2));
    return lo < -((qmax << 16) >> VQA_LIGHT_GAMUT_REL_SHIFT) - VQA_LIGHT_GAMUT_FLOOR;
}

// grid = (ceil(chunks / LIGHT_WALK), n_frames); block = 256.  hist: [frame][LIGHT_BINS] uint32, acc: [frame][LIGHT_WORDS] uint64, both
// zeroed by the submit
template <typename T, int MODEL, bool VEC>
__global__ __launch_bounds__(256) void k_light_accum(light_src s, uint32_t *__restrict__ hist, unsigned long long *__restrict__ acc)
{
#pragma clang fp contract(off)
    __shared__ uint32_t lh[LIGHT_BINS];
    __shared__ unsigned long long red[4][LIGHT_ACC];
    const int f = blockIdx.y, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    for (int i = t; i < LIGHT_BINS; i += 256) lh[i] = 0;
    __syncthreads();
    unsigned long long sum_q = 0, sum_y = 0, max_y = 0;
    uint32_t mx_r = 0, mx_g = 0, mx_b = 0, mx_m = 0, mx_inv = 0;   // mx_inv: the largest 65535 - m, the smallest m
    uint32_t n709 = 0, np3 = 0, nclamp = 0;
    const uint8_t *fr = s.frames + (int64_t)f * s.fs;
    const unsigned long long *__restrict__ tab = s.table;
    for (int i = 0; i < LIGHT_WALK; i++) {
        const int chunk = blockIdx.x * LIGHT_WALK + i;   // (the whole workgroup)
        if (chunk >= s.chunks) break;
        const int patch = chunk * 256 + t;
        uint32_t run_bin = 0, run_cnt = 0;
        if (patch < s.npatch) {
            const int py = patch / s.pw, px = patch - py * s.pw;
            const int rows = min(2, s.h - 2 * py), cols = min(4, s.w - 4 * px);
            const int64_t o0 = s.off[0] + (int64_t)(2 * py) * s.rs0 + (int64_t)(4 * px) * s.step0;
            unsigned long long ra[3][2];   // [plane][row]: four 16-bit fields
            ra[0][0] = load4<T, VEC>(fr + o0, s.step0, cols);
            ra[0][1] = rows > 1 ? load4<T, VEC>(fr + o0 + s.rs0, s.step0, cols) : 0ull;
            load_chroma<T, VEC>(s, fr + s.off[1], py, px, ra[1]);
            load_chroma<T, VEC>(s, fr + s.off[2], py, px, ra[2]);
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const int r = k >> 2, c = k & 3;
                if (r >= rows || c >= cols) continue;
                const int p0 = (int)((ra[0][r] >> (16 * c)) & 0xffffu), p1 = (int)((ra[1][r] >> (16 * c)) & 0xffffu),
                          p2 = (int)((ra[2][r] >> (16 * c)) & 0xffffu);
                double er, eg, eb;
                if constexpr (MODEL == VQA_ITP_YUV2020) {
                    const double y = (double)(p0 - s.o0) / s.d0, cb = (double)(p1 - s.o12) / s.d12, cr = (double)(p2 - s.o12) / s.d12;
                    er = y + 1.4746 * cr;
                    eb = y + 1.8814 * cb;
                    eg = ((y - 0.2627 * er) - 0.0593 * eb) / 0.6780;
                } else {
                    eb = (double)p0 / s.d0; eg = (double)p1 / s.d0; er = (double)p2 / s.d0;
                }
                nclamp += (er < 0.0 || er > 1.0 || eg < 0.0 || eg > 1.0 || eb < 0.0 || eb > 1.0) ? 1u : 0u;
                const uint32_t cr_ = code16(er), cg_ = code16(eg), cb_ = code16(eb);
                const unsigned long long qr = tab[cr_], qg = tab[cg_], qb = tab[cb_];
                const uint32_t m = max(cr_, max(cg_, cb_));
                const unsigned long long qm = max(qr, max(qg, qb));   // T[m]: the table does not decrease
                const unsigned long long y = (2627ull * qr + 6780ull * qg + 593ull * qb + 5000ull) / 10000ull;
                sum_q += qm;
                sum_y += y;
                max_y = max(max_y, y);
                mx_r = max(mx_r, cr_); mx_g = max(mx_g, cg_); mx_b = max(mx_b, cb_);
                mx_m = max(mx_m, m); mx_inv = max(mx_inv, 65535u - m);
                n709 += outside(s.m709, (long long)qr, (long long)qg, (long long)qb, (long long)qm) ? 1u : 0u;
                np3 += outside(s.mp3, (long long)qr, (long long)qg, (long long)qb, (long long)qm) ? 1u : 0u;
                const uint32_t bin = m >> 4;
                if (run_cnt && bin != run_bin) {   // the thread's run of equal bins ends: one add
                    atomicAdd(&lh[run_bin], run_cnt);
                    run_cnt = 0;
                }
                run_bin = bin;
                run_cnt++;
            }
        }
        // the thread's last run: one add for the wave when every pending add names the same bin (every lane comes here)
        const unsigned long long pending = __ballot(run_cnt > 0);
        if (pending) {
            const uint32_t b0 = __shfl(run_bin, __ffsll((long long)pending) - 1, 64);
            if (__all(run_cnt == 0 || run_bin == b0)) {
                const uint32_t total = wave_sum(run_cnt);
                if (lane == 0) atomicAdd(&lh[b0], total);
            } else if (run_cnt) {
                atomicAdd(&lh[run_bin], run_cnt);
            }
        }
    }
    {
        const unsigned long long v[LIGHT_ACC] = {wave_sum(sum_q), wave_sum(sum_y), wave_max(max_y),
                                                 wave_max(mx_r), wave_max(mx_g), wave_max(mx_b), wave_max(mx_m), wave_max(mx_inv),
                                                 wave_sum(n709), wave_sum(np3), wave_sum(nclamp)};
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < LIGHT_ACC; k++) red[wv][k] = v[k];
        }
    }
    __syncthreads();
    uint32_t *gh = hist + (size_t)f * LIGHT_BINS;
    for (int i = t; i < LIGHT_BINS; i += 256) {
        const uint32_t c = lh[i];
        if (c) atomicAdd(&gh[i], c);
    }
    if (t < LIGHT_ACC) {
        const bool is_max = t >= LIGHT_MAX_Y && t <= LIGHT_MIN_INV;
        unsigned long long v = red[0][t];
#pragma unroll
        for (int k = 1; k < 4; k++) v = is_max ? max(v, red[k][t]) : v + red[k][t];
        unsigned long long *a = acc + (size_t)f * LIGHT_WORDS + t;
        if (v) {
            if (is_max) atomicMax(a, v);
            else atomicAdd(a, v);
        }
    }
}

// grid = frames; block = 256.  Writes acc[frame][LIGHT_PCT + p], each once
__global__ __launch_bounds__(256) void k_light_scan(const uint32_t *__restrict__ hist, unsigned long long *__restrict__ acc,
                                                    unsigned long long npix)
{
    __shared__ uint32_t wtot[4];
    const int f = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const uint4 *hh = reinterpret_cast<const uint4 *>(hist + (size_t)f * LIGHT_BINS + 16 * t);
    uint32_t b[16];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint4 q = hh[j];
        b[4 * j] = q.x; b[4 * j + 1] = q.y; b[4 * j + 2] = q.z; b[4 * j + 3] = q.w;
    }
    uint32_t sum = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) sum += b[j];
    uint32_t incl = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    if (lane == 63) wtot[wv] = incl;
    __syncthreads();
    for (int k = 0; k < wv; k++) incl += wtot[k];
    const uint32_t excl = incl - sum;
    constexpr unsigned long long pp[VQA_LIGHT_PERCENTILES] = {100, 500, 1000, 2500, 5000, 7500, 9000, 9500, 9900, 9998};
#pragma unroll
    for (int p = 0; p < VQA_LIGHT_PERCENTILES; p++) {
        const uint32_t k = (uint32_t)((pp[p] * npix + 9999ull) / 10000ull);   // 1 <= k <= npix <= 2^28
        if (excl < k && k <= incl) {
            uint32_t r = k - excl, bin = 15;
            bool found = false;
#pragma unroll
            for (int j = 0; j < 16; j++) {
                if (!found) {
                    if (r <= b[j]) { bin = j; found = true; }
                    else r -= b[j];
                }
            }
            acc[(size_t)f * LIGHT_WORDS + LIGHT_PCT + p] = (unsigned long long)(16 * t) + bin;
        }
    }
}

template <typename T, int MODEL>
void launch_tm(hipStream_t st, const light_src &s, bool vec, dim3 grid, uint32_t *hist, unsigned long long *acc)
{
    if (vec) hipLaunchKernelGGL((k_light_accum<T, MODEL, true>), grid, dim3(256), 0, st, s, hist, acc);
    else hipLaunchKernelGGL((k_light_accum<T, MODEL, false>), grid, dim3(256), 0, st, s, hist, acc);
}

// BT.2100 PQ
constexpr double PQ_M1 = 2610.0 / 16384.0, PQ_M2 = 2523.0 / 4096.0 * 128.0;
constexpr double PQ_C1 = 3424.0 / 4096.0, PQ_C2 = 2413.0 / 4096.0 * 32.0, PQ_C3 = 2392.0 / 4096.0 * 32.0;

// a 3 x 3 matrix, row-major
struct mat3 { double v[9]; };

mat3 mul(const mat3 &a, const mat3 &b)
{
    mat3 r;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) r.v[3 * i + j] = (a.v[3 * i] * b.v[j] + a.v[3 * i + 1] * b.v[3 + j]) + a.v[3 * i + 2] * b.v[6 + j];
    return r;
}

mat3 inverse(const mat3 &m)
{
    const double *a = m.v;
    const double c0 = a[4] * a[8] - a[5] * a[7], c1 = a[5] * a[6] - a[3] * a[8], c2 = a[3] * a[7] - a[4] * a[6];
    const double det = (a[0] * c0 + a[1] * c1) + a[2] * c2;
    mat3 r = {{c0 / det, (a[2] * a[7] - a[1] * a[8]) / det, (a[1] * a[5] - a[2] * a[4]) / det,
               c1 / det, (a[0] * a[8] - a[2] * a[6]) / det, (a[2] * a[3] - a[0] * a[5]) / det,
               c2 / det, (a[1] * a[6] - a[0] * a[7]) / det, (a[0] * a[4] - a[1] * a[3]) / det}};
    return r;
}

// linear RGB of the primaries xy[0..5] = (xr, yr, xg, yg, xb, yb) with white D65 -> XYZ: the columns are the primaries' XYZ at
// unit Y, each scaled so that R = G = B = 1 gives the white point
mat3 rgb_to_xyz(const double *xy)
{
    const double xw = 0.3127, yw = 0.3290;
    mat3 p;
    for (int j = 0; j < 3; j++) {
        const double x = xy[2 * j], y = xy[2 * j + 1];
        p.v[j] = x / y; p.v[3 + j] = 1.0; p.v[6 + j] = ((1.0 - x) - y) / y;
    }
    const mat3 pi = inverse(p);
    const double wx = xw / yw, wz = ((1.0 - xw) - yw) / yw;
    mat3 r;
    for (int j = 0; j < 3; j++) {
        const double sj = (pi.v[3 * j] * wx + pi.v[3 * j + 1]) + pi.v[3 * j + 2] * wz;
        for (int i = 0; i < 3; i++) r.v[3 * i + j] = p.v[3 * i + j] * sj;
    }
    return r;
}

} // namespace

void launch_light_accum(hipStream_t st, const uint8_t *frames, int n, int64_t frame_stride, const vqa_plane_desc *planes, int depth,
                        int model, int full_range, const unsigned long long *table, uint32_t *hist, unsigned long long *acc)
{
    if (n <= 0) return;
    light_src s;
    s.frames = frames; s.fs = frame_stride;
    for (int i = 0; i < 3; i++) s.off[i] = planes[i].offset;
    s.rs0 = planes[0].row_stride; s.step0 = planes[0].pixel_step;
    s.rs1 = planes[1].row_stride; s.step1 = planes[1].pixel_step;
    s.w = planes[0].width; s.h = planes[0].height;
    s.cw = planes[1].width; s.ch = planes[1].height;
    s.sh = s.cw != s.w; s.sv = s.ch != s.h;
    s.pw = (s.w + 3) / 4;
    s.npatch = s.pw * ((s.h + 1) / 2);
    s.chunks = (s.npatch + 255) / 256;
    const int scale = 1 << (depth - 8);
    if (model == VQA_ITP_YUV2020 && !full_range) {
        s.o0 = 16 * scale; s.o12 = 128 * scale;
        s.d0 = (double)(219 * scale); s.d12 = (double)(224 * scale);
    } else {
        s.o0 = 0; s.o12 = model == VQA_ITP_YUV2020 ? 1 << (depth - 1) : 0;
        s.d0 = s.d12 = (double)((1 << depth) - 1);
    }
    int64_t m[9];
    light_gamut_host(VQA_LIGHT_GAMUT_709, m);
    for (int i = 0; i < 9; i++) s.m709[i] = m[i];
    light_gamut_host(VQA_LIGHT_GAMUT_P3, m);
    for (int i = 0; i < 9; i++) s.mp3[i] = m[i];
    s.table = table;
    const int bps = depth > 8 ? 2 : 1;
    // a row of a patch as one load: k_itp's rule, for one stream
    uint64_t bits0 = (uint64_t)(uintptr_t)frames | (uint64_t)s.rs0 | (uint64_t)s.off[0];
    if (n > 1) bits0 |= (uint64_t)frame_stride;
    const uint64_t bits1 = bits0 | (uint64_t)s.rs1 | (uint64_t)s.off[1] | (uint64_t)s.off[2];
    const int a0 = 4 * bps, a1 = (s.sh ? 2 : 4) * bps;
    const bool vec = s.step0 == bps && s.step1 == bps && s.w % 4 == 0 && (bits0 & (uint64_t)(a0 - 1)) == 0 &&
                     (bits1 & (uint64_t)(a1 - 1)) == 0;
    const dim3 grid((s.chunks + LIGHT_WALK - 1) / LIGHT_WALK, n);
    if (depth > 8) {
        if (model == VQA_ITP_YUV2020) launch_tm<uint16_t, VQA_ITP_YUV2020>(st, s, vec, grid, hist, acc);
        else launch_tm<uint16_t, VQA_ITP_BGR>(st, s, vec, grid, hist, acc);
    } else {
        if (model == VQA_ITP_YUV2020) launch_tm<uint8_t, VQA_ITP_YUV2020>(st, s, vec, grid, hist, acc);
        else launch_tm<uint8_t, VQA_ITP_BGR>(st, s, vec, grid, hist, acc);
    }
}

void launch_light_scan(hipStream_t st, int n, int h, int w, const uint32_t *hist, unsigned long long *acc)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_light_scan, dim3(n), dim3(256), 0, st, hist, acc, (unsigned long long)h * (unsigned long long)w);
}

// T[c] = rint(2^20 EOTF_PQ(c / 65535)), in double on the host
void light_table_host(uint64_t *table)
{
#pragma clang fp contract(off)
    for (int c = 0; c < 65536; c++) {
        const double ep = std::pow((double)c / 65535.0, 1.0 / PQ_M2);
        const double num = std::fmax(ep - PQ_C1, 0.0), den = PQ_C2 - PQ_C3 * ep;
        table[c] = (uint64_t)std::rint(1048576.0 * (10000.0 * std::pow(num / den, 1.0 / PQ_M1)));
    }
}

// rint(2^16 A_G), A_G = inverse(RGB_G -> XYZ) (BT.2020 RGB -> XYZ), from the published chromaticities
bool light_gamut_host(int gamut, int64_t m[9])
{
#pragma clang fp contract(off)
    static const double bt2020[6] = {0.708, 0.292, 0.170, 0.797, 0.131, 0.046};
    static const double bt709[6] = {0.64, 0.33, 0.30, 0.60, 0.15, 0.06};
    static const double p3[6] = {0.680, 0.320, 0.265, 0.690, 0.150, 0.060};
    if (gamut != VQA_LIGHT_GAMUT_709 && gamut != VQA_LIGHT_GAMUT_P3) return false;
    const mat3 a = mul(inverse(rgb_to_xyz(gamut == VQA_LIGHT_GAMUT_709 ? bt709 : p3)), rgb_to_xyz(bt2020));
    for (int i = 0; i < 9; i++) m[i] = (int64_t)std::rint(65536.0 * a.v[i]);
    return true;
}

// the words of a frame -> the record, in double on the host
void light_finalize(const unsigned long long *words, int h, int w, const uint64_t *table, vqa_light_metrics *out)
{
#pragma clang fp contract(off)
    const double unit = 1.0 / 1048576.0;
    const int64_t n = (int64_t)h * (int64_t)w;
    out->count = n;
    for (int k = 0; k < 3; k++) out->max_code[k] = (uint32_t)words[LIGHT_MAX_R + k];
    out->max_code_rgb = (uint32_t)words[LIGHT_MAX_M];
    out->min_code_rgb = 65535u - (uint32_t)words[LIGHT_MIN_INV];
    out->reserved = 0;
    out->sum_q = words[LIGHT_SUM_Q];
    out->sum_y = words[LIGHT_SUM_Y];
    out->max_y = words[LIGHT_MAX_Y];
    out->out_709 = words[LIGHT_OUT_709];
    out->out_p3 = words[LIGHT_OUT_P3];
    out->clamped = words[LIGHT_CLAMPED];
    out->max_nits = (double)table[out->max_code_rgb] * unit;
    out->min_nits = (double)table[out->min_code_rgb] * unit;
    out->avg_nits = (double)out->sum_q * unit / (double)n;
    out->y_avg = (double)out->sum_y * unit / (double)n;
    out->y_max = (double)out->max_y * unit;
    for (int k = 0; k < 3; k++) out->maxscl[k] = (double)table[out->max_code[k]] * unit;
    for (int p = 0; p < VQA_LIGHT_PERCENTILES; p++) {
        out->pct_bin[p] = (uint32_t)words[LIGHT_PCT + p];
        out->pct_nits[p] = (double)table[(out->pct_bin[p] & 4095u) << 4] * unit;
    }
    out->share_709 = (double)out->out_709 / (double)n;
    out->share_p3 = (double)out->out_p3 / (double)n;
}

} // namespace vqa
