// k_colorfit.hip — colour registration for gfx950: the joint first and second integer moments of the three planes of BOTH streams
// per frame pair and, per reference code, the count, sum and sum of squares of the distorted samples of the whole submit, by the
// definition stated in include/vqa.h (vqa_colorfit_submit).  The device needs no colour model: it forms integer sums only.
//
//   k_colorfit<T, NP, VEC, TABLES>   the input side of k_ciede: ONE THREAD OWNS A 2 x 4 LUMA PATCH of both images, the patches of a
//                        frame are numbered in raster order and a chunk is 256 consecutive numbers.  load4 / load2x2 / load_chroma
//                        are k_ciede's, copied: that kernel stays as it is.  A workgroup of 256 threads walks COLORFIT_WALK
//                        consecutive chunks of ONE frame (16384 positions) before it flushes, so every sample of both streams is
//                        read once, by one thread.
//                        Moments: a thread sees at most 64 positions, so its words are 32 bits wide for uint8 samples
//                        (64 x 255^2 < 2^22) and 64 bits for uint16 samples (a product reaches 2^32, the words stay below 2^38); a
//                        workgroup's stay below 2^46, a frame's below 2^60.  Then a wave reduction in 64 bits, LDS, and one 64-bit
//                        atomicAdd per word and workgroup (zero words are not sent).
//                        Tables (TABLES): NP x bins x (count 32, sum_d 32, sum_dd 64 bits) in LDS, 48 KB for three planes of
//                        1024 bins.  16384 positions bound them: count <= 2^14, sum_d < 2^30, sum_dd < 2^46.  A thread walks its
//                        patch column by column, so the up to four luma positions one 4:2:0 chroma sample serves follow each other,
//                        and joins every run of equal bins into one entry (count, sum, squares) - a chroma sample enters once with
//                        its weight.  A wave whose pending entries all name one bin sends ONE: flat content costs three LDS atomics
//                        per plane, wave and chunk, not 1536.  Non-empty bins leave through 64-bit global atomics.
//                        Without TABLES the kernel has no table code and no table LDS at all.
//
// Integer addition only: neither the tiling nor the order in which workgroups retire can change a bit.
#include <type_traits>

#include "vqa_dev.hpp"
#include "vqa_kernels.hpp"

namespace vqa {

namespace {

// both streams of n frames of one or three planes; every stride in bytes.  Plane 0 (Y, or B) is the full-size grid; planes 1 and 2
// (Cb and Cr, or G and R) share one geometry, the grid's or its ceil-half in either direction (sh, sv).
struct colorfit_src {
    const uint8_t *ref, *dist;
    int64_t ref_fs, dist_fs;   // frame strides
    int64_t off[3];            // plane offsets inside a frame
    int64_t rs0, rs1;          // row strides of plane 0 and of planes 1, 2
    int step0, step1;          // pixel steps likewise
    int w, h, cw, ch;          // the grid; planes 1, 2
    int sh, sv;                // 1: planes 1, 2 are halved in width / height
    int pw, npatch, chunks;    // patches per row of patches, patches per frame, chunks of 256 patches per frame
    int bin_shift, bins;       // bin = min(r >> bin_shift, bins - 1)
};

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
__device__ __forceinline__ void load_chroma(const colorfit_src &s, const uint8_t *base, int py, int px, unsigned long long (&r)[2])
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

// a thread's open table entry of one plane: a run of equal bins
struct tab_run {
    uint32_t bin = 0, cnt = 0, sum = 0;
    unsigned long long sq = 0;
};

constexpr int COLORFIT_BINS_MAX = VQA_COLORFIT_MAX_BINS;

// grid = (ceil(chunks / COLORFIT_WALK), n_frames); block = 256.  acc: [frame][COLORFIT_WORDS] uint64; tab: [NP][bins][3] uint64 of
// the whole submit; both zeroed by the submit
template <typename T, int NP, bool VEC, bool TABLES>
__global__ __launch_bounds__(256) void k_colorfit(colorfit_src s, unsigned long long *__restrict__ acc,
                                                  unsigned long long *__restrict__ tab)
{
    // a thread's words: it sees at most 64 positions, so 32 bits hold its sums of uint8 products (64 x 255^2 < 2^22); a uint16
    // product reaches 2^32, its sums stay below 2^38
    using word_t = typename std::conditional<sizeof(T) == 1, uint32_t, unsigned long long>::type;
    constexpr int TB = TABLES ? NP * COLORFIT_BINS_MAX : 1;
    __shared__ uint32_t lcnt[TB], lsum[TB];
    __shared__ unsigned long long lsq[TB];
    __shared__ unsigned long long red[4][COLORFIT_WORDS];
    const int f = blockIdx.y, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    if constexpr (TABLES) {
        for (int p = 0; p < NP; p++)
            for (int i = t; i < s.bins; i += 256) {
                lcnt[p * COLORFIT_BINS_MAX + i] = 0; lsum[p * COLORFIT_BINS_MAX + i] = 0; lsq[p * COLORFIT_BINS_MAX + i] = 0;
            }
        __syncthreads();
    }
    word_t sr[NP], sd[NP], rr[NP == 3 ? 6 : 1], rd[NP * NP], dd[NP];
#pragma unroll
    for (int p = 0; p < NP; p++) { sr[p] = 0; sd[p] = 0; dd[p] = 0; }
#pragma unroll
    for (int p = 0; p < (NP == 3 ? 6 : 1); p++) rr[p] = 0;
#pragma unroll
    for (int p = 0; p < NP * NP; p++) rd[p] = 0;
    const uint8_t *fr = s.ref + (int64_t)f * s.ref_fs, *fd = s.dist + (int64_t)f * s.dist_fs;
    for (int i = 0; i < COLORFIT_WALK; i++) {
        const int chunk = blockIdx.x * COLORFIT_WALK + i;   // (the whole workgroup)
        if (chunk >= s.chunks) break;
        const int patch = chunk * 256 + t;
        tab_run run[NP];
        if (patch < s.npatch) {
            const int py = patch / s.pw, px = patch - py * s.pw;
            const int rows = min(2, s.h - 2 * py), cols = min(4, s.w - 4 * px);
            const int64_t o0 = s.off[0] + (int64_t)(2 * py) * s.rs0 + (int64_t)(4 * px) * s.step0;
            unsigned long long ra[NP][2], rb[NP][2];   // [plane][row]: four 16-bit fields
            ra[0][0] = load4<T, VEC>(fr + o0, s.step0, cols);
            rb[0][0] = load4<T, VEC>(fd + o0, s.step0, cols);
            ra[0][1] = rows > 1 ? load4<T, VEC>(fr + o0 + s.rs0, s.step0, cols) : 0ull;
            rb[0][1] = rows > 1 ? load4<T, VEC>(fd + o0 + s.rs0, s.step0, cols) : 0ull;
            if constexpr (NP == 3) {
                load_chroma<T, VEC>(s, fr + s.off[1], py, px, ra[1]);
                load_chroma<T, VEC>(s, fr + s.off[2], py, px, ra[2]);
                load_chroma<T, VEC>(s, fd + s.off[1], py, px, rb[1]);
                load_chroma<T, VEC>(s, fd + s.off[2], py, px, rb[2]);
            }
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const int c = k >> 1, r = k & 1;   // column by column: the positions of one halved chroma sample are adjacent
                if (r >= rows || c >= cols) continue;
                uint32_t x[NP], y[NP];
#pragma unroll
                for (int p = 0; p < NP; p++) {
                    x[p] = (uint32_t)((ra[p][r] >> (16 * c)) & 0xffffu);
                    y[p] = (uint32_t)((rb[p][r] >> (16 * c)) & 0xffffu);
                    sr[p] += x[p];
                    sd[p] += y[p];
                    dd[p] += (word_t)y[p] * y[p];
                }
                int q = 0;
#pragma unroll
                for (int p = 0; p < NP; p++) {
#pragma unroll
                    for (int p2 = p; p2 < NP; p2++) rr[q++] += (word_t)x[p] * x[p2];
#pragma unroll
                    for (int p2 = 0; p2 < NP; p2++) rd[NP * p + p2] += (word_t)x[p] * y[p2];
                }
                if constexpr (TABLES) {
#pragma unroll
                    for (int p = 0; p < NP; p++) {
                        const uint32_t bin = min(x[p] >> s.bin_shift, (uint32_t)(s.bins - 1));
                        tab_run &u = run[p];
                        if (u.cnt && bin != u.bin) {   // the thread's run of equal bins ends: one entry
                            const int at = p * COLORFIT_BINS_MAX + (int)u.bin;
                            atomicAdd(&lcnt[at], u.cnt); atomicAdd(&lsum[at], u.sum); atomicAdd(&lsq[at], u.sq);
                            u.cnt = 0; u.sum = 0; u.sq = 0;
                        }
                        u.bin = bin;
                        u.cnt++;
                        u.sum += y[p];
                        u.sq += (unsigned long long)y[p] * y[p];
                    }
                }
            }
        }
        if constexpr (TABLES) {
            // the thread's last runs: one entry for the wave when every pending one names the same bin (every lane comes here)
#pragma unroll
            for (int p = 0; p < NP; p++) {
                const tab_run &u = run[p];
                const unsigned long long pending = __ballot(u.cnt > 0);
                if (!pending) continue;
                const uint32_t b0 = __shfl(u.bin, __ffsll((long long)pending) - 1, 64);
                if (__all(u.cnt == 0 || u.bin == b0)) {
                    const uint32_t tc = wave_sum(u.cnt), ts = wave_sum(u.sum);
                    const unsigned long long tq = wave_sum(u.sq);
                    if (lane == 0) {
                        const int at = p * COLORFIT_BINS_MAX + (int)b0;
                        atomicAdd(&lcnt[at], tc); atomicAdd(&lsum[at], ts); atomicAdd(&lsq[at], tq);
                    }
                } else if (u.cnt) {
                    const int at = p * COLORFIT_BINS_MAX + (int)u.bin;
                    atomicAdd(&lcnt[at], u.cnt); atomicAdd(&lsum[at], u.sum); atomicAdd(&lsq[at], u.sq);
                }
            }
        }
    }
    // the thread's words in the record's order (a one-plane kernel leaves the words of planes 1 and 2 at zero)
    unsigned long long a[COLORFIT_WORDS];
#pragma unroll
    for (int k = 0; k < COLORFIT_WORDS; k++) a[k] = 0;
#pragma unroll
    for (int p = 0; p < NP; p++) { a[COLORFIT_SUM_R + p] = sr[p]; a[COLORFIT_SUM_D + p] = sd[p]; a[COLORFIT_DD + p] = dd[p]; }
#pragma unroll
    for (int p = 0; p < (NP == 3 ? 6 : 1); p++) a[COLORFIT_RR + p] = rr[p];
#pragma unroll
    for (int p = 0; p < NP; p++)
#pragma unroll
        for (int p2 = 0; p2 < NP; p2++) a[COLORFIT_RD + 3 * p + p2] = rd[NP * p + p2];
#pragma unroll
    for (int k = 0; k < COLORFIT_WORDS; k++) {
        const unsigned long long v = wave_sum(a[k]);
        if (lane == 0) red[wv][k] = v;
    }
    __syncthreads();
    if constexpr (TABLES) {
        for (int p = 0; p < NP; p++)
            for (int i = t; i < s.bins; i += 256) {
                const int at = p * COLORFIT_BINS_MAX + i;
                const uint32_t c = lcnt[at];
                if (c) {
                    unsigned long long *g = tab + ((size_t)p * s.bins + i) * 3;
                    atomicAdd(g, (unsigned long long)c);
                    atomicAdd(g + 1, (unsigned long long)lsum[at]);
                    atomicAdd(g + 2, lsq[at]);
                }
            }
    }
    if (t < COLORFIT_WORDS) {
        const unsigned long long v = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
        if (v) atomicAdd(acc + (size_t)f * COLORFIT_WORDS + t, v);
    }
}

template <typename T, int NP>
void launch_tn(hipStream_t st, const colorfit_src &s, bool vec, bool tables, dim3 grid, unsigned long long *acc, unsigned long long *tab)
{
    if (vec) {
        if (tables) hipLaunchKernelGGL((k_colorfit<T, NP, true, true>), grid, dim3(256), 0, st, s, acc, tab);
        else hipLaunchKernelGGL((k_colorfit<T, NP, true, false>), grid, dim3(256), 0, st, s, acc, tab);
    } else {
        if (tables) hipLaunchKernelGGL((k_colorfit<T, NP, false, true>), grid, dim3(256), 0, st, s, acc, tab);
        else hipLaunchKernelGGL((k_colorfit<T, NP, false, false>), grid, dim3(256), 0, st, s, acc, tab);
    }
}

} // namespace

void launch_colorfit(hipStream_t st, const uint8_t *ref, const uint8_t *dist, int n, int64_t ref_frame_stride,
                     int64_t dist_frame_stride, const vqa_plane_desc *planes, int n_planes, int depth, unsigned long long *acc,
                     unsigned long long *tables)
{
    if (n <= 0) return;
    const bool three = n_planes == 3;
    colorfit_src s;
    s.ref = ref; s.dist = dist; s.ref_fs = ref_frame_stride; s.dist_fs = dist_frame_stride;
    for (int i = 0; i < 3; i++) s.off[i] = planes[three ? i : 0].offset;
    s.rs0 = planes[0].row_stride; s.step0 = planes[0].pixel_step;
    s.rs1 = planes[three ? 1 : 0].row_stride; s.step1 = planes[three ? 1 : 0].pixel_step;
    s.w = planes[0].width; s.h = planes[0].height;
    s.cw = planes[three ? 1 : 0].width; s.ch = planes[three ? 1 : 0].height;
    s.sh = s.cw != s.w; s.sv = s.ch != s.h;
    s.pw = (s.w + 3) / 4;
    s.npatch = s.pw * ((s.h + 1) / 2);
    s.chunks = (s.npatch + 255) / 256;
    s.bin_shift = depth > 10 ? depth - 10 : 0;
    s.bins = colorfit_bins(depth);
    const int bps = depth > 8 ? 2 : 1;
    // a row of a patch as one load: k_ciede's rule - unit steps, whole patches, and every address a multiple of the load's size
    uint64_t bits0 = (uint64_t)(uintptr_t)ref | (uint64_t)(uintptr_t)dist | (uint64_t)s.rs0 | (uint64_t)s.off[0];
    if (n > 1) bits0 |= (uint64_t)ref_frame_stride | (uint64_t)dist_frame_stride;
    const uint64_t bits1 = bits0 | (uint64_t)s.rs1 | (uint64_t)s.off[1] | (uint64_t)s.off[2];
    const int a0 = 4 * bps, a1 = (s.sh ? 2 : 4) * bps;
    const bool vec = s.step0 == bps && s.step1 == bps && s.w % 4 == 0 && (bits0 & (uint64_t)(a0 - 1)) == 0 &&
                     (bits1 & (uint64_t)(a1 - 1)) == 0;
    const dim3 grid((s.chunks + COLORFIT_WALK - 1) / COLORFIT_WALK, n);
    const bool tab = tables != nullptr;
    if (depth > 8) {
        if (three) launch_tn<uint16_t, 3>(st, s, vec, tab, grid, acc, tables);
        else launch_tn<uint16_t, 1>(st, s, vec, tab, grid, acc, tables);
    } else {
        if (three) launch_tn<uint8_t, 3>(st, s, vec, tab, grid, acc, tables);
        else launch_tn<uint8_t, 1>(st, s, vec, tab, grid, acc, tables);
    }
}

// the words of a frame -> the record; sse[k] = dd[k] - 2 rd[4 k] + rr(k, k) in 64-bit words (the true value is below 2^60, so the
// wrap-around arithmetic is exact)
void colorfit_finalize(const unsigned long long *words, int h, int w, int n_planes, vqa_colorfit_metrics *out)
{
    static const int diag[3] = {0, 3, 5};   // rr's (0,0), (1,1), (2,2)
    out->count = (uint64_t)h * (uint64_t)w;
    for (int k = 0; k < 3; k++) { out->sum_r[k] = words[COLORFIT_SUM_R + k]; out->sum_d[k] = words[COLORFIT_SUM_D + k]; }
    for (int k = 0; k < 6; k++) out->rr[k] = words[COLORFIT_RR + k];
    for (int k = 0; k < 9; k++) out->rd[k] = words[COLORFIT_RD + k];
    for (int k = 0; k < 3; k++) {
        out->dd[k] = words[COLORFIT_DD + k];
        out->sse[k] = k < n_planes ? out->dd[k] - 2 * out->rd[4 * k] + out->rr[diag[k]] : 0;
    }
}

} // namespace vqa
