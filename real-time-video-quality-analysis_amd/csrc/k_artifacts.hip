// k_artifacts.hip — no-reference blockiness, blur and noise for gfx950: the phase-resolved boundary steps of Wang, Sheikh and
// Bovik (ICIP 2002), the blur measure of Crete-Roffet, Dolmiere, Ladret and Nicolas (SPIE 2007) with its 9-tap mean telescoped
// away, and Immerkaer's Laplacian noise estimate (CVIU 1996), by the definition stated in include/vqa.h (vqa_artifacts_submit).
//
//   k_artifacts<T>   one fused launch per group of same-geometry planes.  A workgroup of 256 threads walks ARTIFACTS_RUN
//               consecutive 64 x 32 tiles of a plane.  A tile and its apron - 5 samples up, 4 down, 8 left (5 are needed; 8 keeps
//               the groups of four samples aligned) and 4 right - go to LDS once as raw integers: four samples per load
//               where the layout allows it (one dword of an 8-bit plane, two of a 16-bit plane, three of packed bgr24, whose
//               bytes are picked apart in registers), one sample per load at the plane's right edge and for frames that are not
//               aligned to the load.  A lane owns a column of the tile and a wave eight rows: the lane reads its column (17
//               samples), the two beside it (10 each) and the ones 4 to the right and 5 to the left (8 each) from LDS, 6.6 reads
//               per sample and bank-conflict free, and forms every term in 32-bit integers.  Tile origins are multiples of 8, so
//               a lane's column has one horizontal phase and its k-th row the vertical phase k: a lane carries one edge_h sum and
//               eight edge_v sums.  Every term belongs to the sample that is the right-hand or lower one of its boundary or the
//               centre of its window, and is counted only where its whole support lies in the plane: tiles neither share nor
//               drop a term.  The 21 sums are reduced per wave, added up in LDS and leave as one 64-bit integer atomic per word
//               and workgroup.  No floating point, no scratch beyond the 168 bytes per (frame, plane).
//
// Sums (vqa.h states the bounds): a sample's largest term is 9 * 65535 < 2^20 (blur_v_*), a lane's share is 8 rows of
// ARTIFACTS_RUN tiles = 64 samples, below 2^26: the lanes' partials are 32-bit.  Everything beyond a lane is 64-bit.  Integer
// addition is associative: neither the tiling nor the order in which workgroups retire can change a bit, so a plane gives the
// same 21 words at any place of any batch.
#include <cmath>
#include <type_traits>

#include "vqa_dev.hpp"
#include "vqa_kernels.hpp"

namespace vqa {

namespace {

constexpr int ARTIFACTS_RUN = 8;   // tiles per workgroup, consecutive in raster order: 21 atomics per 16384 samples

// the frames of one group of same-geometry planes; every stride in bytes
struct artifacts_src {
    const uint8_t *frames;  // frame 0 of the slice
    int64_t fs;             // frame stride
    int64_t off[4];         // plane offsets inside a frame
    int64_t row_stride;
    int step;
    int packed;             // the group is the three interleaved 8-bit channels of one packed pixel (bgr24): off[] - pixel0 = 0, 1, 2
    int64_t pixel0;         // packed: the offset of the pixel's first byte
    int w, h;
};

// byte k (0 .. 11) of three consecutive dwords
__device__ __forceinline__ int byte_of(uint32_t u0, uint32_t u1, uint32_t u2, int k)
{
    const uint32_t u = k < 4 ? u0 : k < 8 ? u1 : u2;
    return (int)((u >> (8 * (k & 3))) & 255u);
}

// grid = (ceil(tiles / ARTIFACTS_RUN) * count, n_frames); block = 256.  acc: [frame][plane of the submit][ARTIFACTS_WORDS]
// uint64, zeroed by the submit
template <typename T>
__global__ __launch_bounds__(256) void k_artifacts(artifacts_src s, int tiles_x, int tiles, int runs, int n_planes,
                                                   int4 plane_index, unsigned long long *__restrict__ acc)
{
    constexpr int TW = 64, TH = 32, AL = 8, AU = 5, IW = AL + TW + 4, IH = AU + TH + 4, GROUPS = IW / 4;   // 76 x 41, 19 groups
    constexpr int VB = 4 * (int)sizeof(T);   // bytes of a planar group of four samples
    __shared__ __attribute__((aligned(16))) int in[IH][IW];
    __shared__ unsigned long long tot[ARTIFACTS_WORDS];
    const int f = blockIdx.y;
    const int ch = blockIdx.x / runs, run = blockIdx.x % runs;
    const int t = threadIdx.x;
    if (t < ARTIFACTS_WORDS) tot[t] = 0;   // (the barriers of the first tile order this before the adds)
    const uint8_t *frame = s.frames + (int64_t)f * s.fs;
    const uint8_t *pc = frame + s.off[ch];
    // four samples per load: a planar group needs the plane and its rows aligned to the load, a packed one the pixels to a dword
    const bool planar4 = s.step == (int)sizeof(T) && ((((uint64_t)pc) | (uint64_t)s.row_stride) & (VB - 1)) == 0;
    const uint8_t *px = frame + s.pixel0;
    const int pk = (int)(s.off[ch] - s.pixel0);   // packed: the channel's byte inside the pixel
    const bool packed4 = sizeof(T) == 1 && s.packed && ((((uint64_t)px) | (uint64_t)s.row_stride) & 3) == 0;
    // lane = column c of the tile, wave = rows 8 b .. 8 b + 7
    const int c = t & 63, b8 = (t >> 6) * 8;
    unsigned eh = 0, ev[8] = {0, 0, 0, 0, 0, 0, 0, 0}, fh = 0, vh = 0, fv = 0, vv = 0, lap = 0;
    const int tile_end = min(tiles, (run + 1) * ARTIFACTS_RUN);
    for (int tile = run * ARTIFACTS_RUN; tile < tile_end; tile++) {
        const int y0 = (tile / tiles_x) * TH, x0 = (tile % tiles_x) * TW;
        __syncthreads();   // (the tile before has been read)
        for (int i = t; i < IH * GROUPS; i += 256) {
            const int j = i / GROUPS, g = i - j * GROUPS;
            const int y = y0 - AU + j, x = x0 - AL + 4 * g;   // x is a multiple of 4
            int4 v = make_int4(0, 0, 0, 0);                    // (what lies outside the plane enters no term)
            if (y >= 0 && y < s.h && x >= 0 && x < s.w) {
                const uint8_t *row = pc + (int64_t)y * s.row_stride;
                if (x + 3 < s.w && planar4) {
                    if constexpr (sizeof(T) == 1) {
                        const uint32_t u = *(const uint32_t *)(row + x);
                        v = make_int4(u & 255u, (u >> 8) & 255u, (u >> 16) & 255u, u >> 24);
                    } else {
                        const uint2 u = *(const uint2 *)(row + 2 * (int64_t)x);
                        v = make_int4(u.x & 65535u, u.x >> 16, u.y & 65535u, u.y >> 16);
                    }
                } else if (x + 3 < s.w && packed4) {
                    const uint32_t *q = (const uint32_t *)(px + (int64_t)y * s.row_stride + 3 * (int64_t)x);
                    const uint32_t u0 = q[0], u1 = q[1], u2 = q[2];
                    v = make_int4(byte_of(u0, u1, u2, pk), byte_of(u0, u1, u2, pk + 3), byte_of(u0, u1, u2, pk + 6),
                                  byte_of(u0, u1, u2, pk + 9));
                } else {
                    v.x = (int)*(const T *)(row + (int64_t)x * s.step);
                    if (x + 1 < s.w) v.y = (int)*(const T *)(row + (int64_t)(x + 1) * s.step);
                    if (x + 2 < s.w) v.z = (int)*(const T *)(row + (int64_t)(x + 2) * s.step);
                    if (x + 3 < s.w) v.w = (int)*(const T *)(row + (int64_t)(x + 3) * s.step);
                }
            }
            *reinterpret_cast<int4 *>(&in[j][4 * g]) = v;
        }
        __syncthreads();
        // tile row r is LDS row r + AU, tile column c LDS column c + AL
        int cj[17], cl[10], cr[10], c4[8], c5[8];
#pragma unroll
        for (int k = 0; k < 17; k++) cj[k] = in[b8 + k][c + AL];           // tile rows 8 b - 5 .. 8 b + 11
#pragma unroll
        for (int k = 0; k < 10; k++) {                                     // tile rows 8 b - 1 .. 8 b + 8
            cl[k] = in[b8 + 4 + k][c + AL - 1];
            cr[k] = in[b8 + 4 + k][c + AL + 1];
        }
#pragma unroll
        for (int k = 0; k < 8; k++) {                                      // tile rows 8 b .. 8 b + 7
            c4[k] = in[b8 + AU + k][c + AL + 4];
            c5[k] = in[b8 + AU + k][c + AL - 5];
        }
        const int x = x0 + c;
        const bool col_in = x < s.w, col_e = col_in && x >= 1, col_b = col_in && x >= 5 && x <= s.w - 5,
                   col_l = col_in && x >= 1 && x <= s.w - 2;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int y = y0 + b8 + k;
            if (y >= s.h) continue;
            const int ctr = cj[k + 5], up = cj[k + 4], dn = cj[k + 6];
            const unsigned dh = (unsigned)abs(ctr - cl[k + 1]), dv = (unsigned)abs(ctr - up);
            if (col_e) eh += dh;                          // phase x mod 8 = c mod 8
            if (col_in && y >= 1) ev[k] += dv;            // phase y mod 8 = k
            if (col_b) {
                fh += dh;
                vh += (unsigned)max(0, 9 * (int)dh - abs(c4[k] - c5[k]));
            }
            if (col_in && y >= 5 && y <= s.h - 5) {
                fv += dv;
                vv += (unsigned)max(0, 9 * (int)dv - abs(cj[k + 9] - cj[k]));
            }
            if (col_l && y >= 1 && y <= s.h - 2) {
                const int l = (cl[k] + cr[k] + cl[k + 2] + cr[k + 2]) - 2 * (up + dn + cl[k + 1] + cr[k + 1]) + 4 * ctr;
                lap += (unsigned)abs(l);
            }
        }
    }
    // edge_h: the lanes of one phase are those equal mod 8
    unsigned long long e = eh;
    e += __shfl_xor(e, 8, 64);
    e += __shfl_xor(e, 16, 64);
    e += __shfl_xor(e, 32, 64);
    if (lane_id() < 8) atomicAdd(&tot[lane_id()], e);
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const unsigned long long u = wave_sum((unsigned long long)ev[k]);
        if (lane_id() == 0) atomicAdd(&tot[8 + k], u);
    }
    const unsigned long long u0 = wave_sum((unsigned long long)fh), u1 = wave_sum((unsigned long long)vh),
                             u2 = wave_sum((unsigned long long)fv), u3 = wave_sum((unsigned long long)vv),
                             u4 = wave_sum((unsigned long long)lap);
    if (lane_id() == 0) {
        atomicAdd(&tot[16], u0); atomicAdd(&tot[17], u1); atomicAdd(&tot[18], u2); atomicAdd(&tot[19], u3);
        atomicAdd(&tot[20], u4);
    }
    __syncthreads();
    if (t < ARTIFACTS_WORDS && tot[t]) {
        const int pi = ch == 0 ? plane_index.x : ch == 1 ? plane_index.y : ch == 2 ? plane_index.z : plane_index.w;
        atomicAdd(acc + ((int64_t)f * n_planes + pi) * ARTIFACTS_WORDS + t, tot[t]);
    }
}

} // namespace

void launch_artifacts(hipStream_t st, const uint8_t *frames, int n, int64_t frame_stride, const vqa_plane_desc *planes,
                      const int *idx, int count, int n_planes, int depth, unsigned long long *acc)
{
    if (n <= 0 || count <= 0) return;
    const vqa_plane_desc &pd = planes[idx[0]];
    artifacts_src s;
    s.frames = frames; s.fs = frame_stride;
    int p4[4];
    group_slots(planes, idx, count, s.off, p4);
    s.row_stride = pd.row_stride; s.step = pd.pixel_step;
    s.w = pd.width; s.h = pd.height;
    // packed bgr24: three 8-bit planes, one byte apart, three bytes a pixel - a row then holds whole pixels of 3 bytes, so the 12
    // bytes behind four pixels inside the plane are the caller's
    s.pixel0 = s.off[0] < s.off[1] ? s.off[0] : s.off[1];
    s.pixel0 = s.off[2] < s.pixel0 ? s.off[2] : s.pixel0;
    s.packed = depth <= 8 && count == 3 && pd.pixel_step == 3 &&
               (s.off[0] - s.pixel0) + (s.off[1] - s.pixel0) + (s.off[2] - s.pixel0) == 3 &&
               s.off[0] != s.off[1] && s.off[1] != s.off[2] && s.off[0] != s.off[2] &&
               s.off[0] - s.pixel0 <= 2 && s.off[1] - s.pixel0 <= 2 && s.off[2] - s.pixel0 <= 2;
    const int tiles_x = (s.w + 63) / 64, tiles = tiles_x * ((s.h + 31) / 32);
    const int runs = (tiles + ARTIFACTS_RUN - 1) / ARTIFACTS_RUN;
    const int4 pi = make_int4(p4[0], p4[1], p4[2], p4[3]);
    const dim3 grid(runs * count, n), block(256);
    if (depth > 8)
        hipLaunchKernelGGL((k_artifacts<uint16_t>), grid, block, 0, st, s, tiles_x, tiles, runs, n_planes, pi, acc);
    else
        hipLaunchKernelGGL((k_artifacts<uint8_t>), grid, block, 0, st, s, tiles_x, tiles, runs, n_planes, pi, acc);
}

// how many boundaries c = 1 .. n - 1 have c mod 8 == p
static int64_t phase_count(int n, int p)
{
    return p == 0 ? (n - 1) / 8 : (n - 1 >= p ? (n - 1 - p) / 8 + 1 : 0);
}

// r[p] of include/vqa.h for one direction: edge[8] over `lines` rows (columns) of `n` samples
static void phase_ratios(const uint64_t *edge, int n, int lines, double r[8])
{
#pragma clang fp contract(off)
    uint64_t sum_e = 0;
    int64_t sum_c = 0;
    for (int p = 0; p < 8; p++) { sum_e += edge[p]; sum_c += phase_count(n, p) * lines; }
    for (int p = 0; p < 8; p++) {
        const int64_t cnt = phase_count(n, p) * lines;   // n >= 16: every phase has a boundary, and so have the others
        const double m_b = (double)edge[p] / (double)cnt;
        const double m_o = (double)(sum_e - edge[p]) / (double)(sum_c - cnt);
        const double den = m_b + m_o;
        r[p] = den == 0.0 ? 0.0 : (m_b - m_o) / den;
    }
}

// the 21 words -> the record, in double on the host, in the order of operations vqa.h states.  Contraction is off.
void artifacts_finalize(const unsigned long long *words, int h, int w, int depth, vqa_artifacts_metrics *out)
{
#pragma clang fp contract(off)
    for (int p = 0; p < 8; p++) { out->edge_h[p] = words[p]; out->edge_v[p] = words[8 + p]; }
    out->blur_f_h = words[16]; out->blur_v_h = words[17]; out->blur_f_v = words[18]; out->blur_v_v = words[19];
    out->lap = words[20];
    double rh[8], rv[8];
    phase_ratios(out->edge_h, w, h, rh);
    phase_ratios(out->edge_v, h, w, rv);
    int ph = 0, pv = 0;
    for (int p = 1; p < 8; p++) {
        if (rh[p] > rh[ph]) ph = p;
        if (rv[p] > rv[pv]) pv = p;
    }
    out->phase_h = ph; out->phase_v = pv;
    out->blockiness = (rh[0] + rv[0]) / 2.0;
    out->blockiness_max = (rh[ph] + rv[pv]) / 2.0;
    const double f9h = 9.0 * (double)out->blur_f_h, f9v = 9.0 * (double)out->blur_f_v;
    out->blur_h = out->blur_f_h == 0 ? 0.0 : (f9h - (double)out->blur_v_h) / f9h;
    out->blur_v = out->blur_f_v == 0 ? 0.0 : (f9v - (double)out->blur_v_v) / f9v;
    out->blur = out->blur_h > out->blur_v ? out->blur_h : out->blur_v;
    const double s = (double)(1 << (depth - 8));
    out->noise = ARTIFACTS_SQRT_HALF_PI * (double)out->lap / (6.0 * (double)((int64_t)(w - 2) * (h - 2)) * s);
}

} // namespace vqa
