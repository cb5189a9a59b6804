// k_psnr_hvs.hip — PSNR-HVS and PSNR-HVS-M for gfx950: the CSF-weighted squared error of the 8x8 DCT coefficients of a plane
// pair, without and with the contrast-masking threshold, by the definition stated in include/vqa.h (vqa_psnr_hvs_submit).
//
//   k_psnr_hvs<T, VEC>   one fused launch per group of same-geometry planes.  ONE THREAD OWNS ONE 8x8 BLOCK, whole: the
//                        blocks of a plane are numbered in raster order and a workgroup of 64 threads (one wave) owns 64
//                        consecutive numbers - a tiling that depends on the plane's geometry alone.  A thread reads the eight
//                        rows of its block of both images once, as one 8-byte (uint8) or 16-byte (uint16) load per row when the
//                        layout allows it (VEC: unit pixel step, aligned rows) - adjacent threads own adjacent blocks, so a
//                        wave's load of one row is up to 512 or 1024 contiguous bytes - and keeps them packed as loaded (16 or 32
//                        registers per image).  Everything else happens in that thread's registers, fully unrolled: the integer
//                        sums behind the variances, three 2-D DCTs as eight row and eight column passes of an even/odd 8-point
//                        DCT (40 multiply-adds each) on a float[8][8] that never leaves the register file, the two masking
//                        energies and the 64 weighted terms of both sums.  There is no LDS, no transpose and no barrier: the
//                        transpose between the row and the column pass is a renaming of registers.  The price is occupancy
//                        (the compiler uses 200 to 230 registers per lane on the one-load-per-row paths: two waves per SIMD),
//                        paid for by instruction-level parallelism - the 16 DCTs of a pass are independent.
//
// Three DCTs, not two: the DCT is linear, so |A - B| is formed as the DCT of the INTEGER difference a - b, which is exact in
// fp32 at every depth; subtracting two fp32 coefficient arrays instead loses the figure where the planes are close (a 16-bit
// block's DC is near 2^19, one ulp 2^-4, against a difference of a few units).  The DCTs of a and of b are needed for their own
// masking energies only.
//
// Variances from exact integers (vqa.h): per quadrant s1 = sum x and s2 = sum x^2; n s2 - s1^2 is an integer, below 2^44 for a
// block of uint16 samples, and the two quotients and their ratio are formed once in double.
//
// Sums (vqa.h states the bounds): a block's two sums are below 2^41; each is rounded to 2^-20 fixed point (below 2^61), split
// into its low and high 32 bits, and the halves are added as 64-bit integers - across the wave, then one atomic per word and
// workgroup: four words per (frame, plane).  Integer addition is associative: neither the tiling nor the order in which
// workgroups retire can change a bit.
#include <cmath>
#include <mutex>

#include "vqa_dev.hpp"
#include "vqa_kernels.hpp"

namespace vqa {

namespace {

// the tables of vqa.h, formed in double and rounded once to fp32 by the host (hvs_tables)
struct hvs_tabs {
    float c[8][4];     // C[k][n] for n < 4; C[k][7 - n] = (-1)^k C[k][n]
    float csf[8][8];   // 25.735088 / Q
    float msk[8][8];   // (10 / Q)^2
    float thr[8][8];   // (Q / 10)^2 = 1 / msk, and 0 at (0,0): u' = max(u - m thr, 0) leaves the DC term unmasked
};

// both images of one group of same-geometry planes; every stride in bytes
struct hvs_src {
    const uint8_t *ref, *dist;
    int64_t ref_fs, dist_fs;   // frame strides
    int64_t off[4];            // plane offsets inside a frame
    int64_t row_stride;
    int step;
    int bw, nblocks;           // blocks per row of blocks, blocks per plane
};

// one 8-point DCT-II in place on x[0], x[S], .. x[7 S]: even outputs from the sums, odd outputs from the differences of the
// mirrored pairs, four multiply-adds each in ascending n
template <int S>
__device__ __forceinline__ void dct8(float *x, const hvs_tabs &t)
{
    const float s0 = x[0] + x[7 * S], s1 = x[S] + x[6 * S], s2 = x[2 * S] + x[5 * S], s3 = x[3 * S] + x[4 * S];
    const float d0 = x[0] - x[7 * S], d1 = x[S] - x[6 * S], d2 = x[2 * S] - x[5 * S], d3 = x[3 * S] - x[4 * S];
#pragma unroll
    for (int k = 0; k < 8; k += 2) {
        x[k * S] = fmaf(t.c[k][3], s3, fmaf(t.c[k][2], s2, fmaf(t.c[k][1], s1, t.c[k][0] * s0)));
        x[(k + 1) * S] = fmaf(t.c[k + 1][3], d3, fmaf(t.c[k + 1][2], d2, fmaf(t.c[k + 1][1], d1, t.c[k + 1][0] * d0)));
    }
}

// A = C a C^T in place: z[k][l], k the vertical frequency
__device__ __forceinline__ void dct8x8(float (&z)[8][8], const hvs_tabs &t)
{
#pragma unroll
    for (int r = 0; r < 8; r++) dct8<1>(&z[r][0], t);
#pragma unroll
    for (int c = 0; c < 8; c++) dct8<8>(&z[0][c], t);
}

// a block as loaded: W 32-bit words per row, samples little-endian inside a word
template <typename T> struct hvs_raw {
    static constexpr int W = 2 * sizeof(T);
    uint32_t v[8][W];
    __device__ __forceinline__ int at(int r, int c) const
    {
        return sizeof(T) == 1 ? (int)((v[r][c >> 2] >> (8 * (c & 3))) & 0xffu) : (int)((v[r][c >> 1] >> (16 * (c & 1))) & 0xffffu);
    }
};

template <typename T, bool VEC>
__device__ __forceinline__ void load_block(hvs_raw<T> &b, const uint8_t *p, int64_t row_stride, int step)
{
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const uint8_t *q = p + (int64_t)r * row_stride;
        if constexpr (VEC && sizeof(T) == 1) {
            const uint2 u = *reinterpret_cast<const uint2 *>(q);
            b.v[r][0] = u.x; b.v[r][1] = u.y;
        } else if constexpr (VEC) {
            const uint4 u = *reinterpret_cast<const uint4 *>(q);
            b.v[r][0] = u.x; b.v[r][1] = u.y; b.v[r][2] = u.z; b.v[r][3] = u.w;
        } else {
            constexpr int PER = 4 / sizeof(T);   // samples per word
#pragma unroll
            for (int k = 0; k < hvs_raw<T>::W; k++) {
                uint32_t word = 0;
#pragma unroll
                for (int j = 0; j < PER; j++)
                    word |= (uint32_t)*(const T *)(q + (int64_t)(k * PER + j) * step) << (8 * sizeof(T) * j);
                b.v[r][k] = word;
            }
        }
    }
}

// m(z) of vqa.h: sqrt(E pop) / 32, E from the block's DCT (which is left in z), pop from the exact integer sums
template <typename T>
__device__ __forceinline__ float mask_of(const hvs_raw<T> &b, float (&z)[8][8], const hvs_tabs &t)
{
    // s1 <= 64 * 65535 < 2^22; s2 <= 16 * 65535^2 < 2^36 per quadrant (32 bits would do for uint8 samples: the compiler sees it)
    unsigned long long nq = 0, s2b = 0;
    unsigned s1b = 0;
#pragma unroll
    for (int qd = 0; qd < 4; qd++) {
        unsigned s1 = 0;
        unsigned long long s2 = 0;
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const unsigned x = (unsigned)b.at((qd >> 1) * 4 + (i >> 2), (qd & 1) * 4 + (i & 3));
            s1 += x;
            s2 += sizeof(T) == 1 ? (unsigned long long)(x * x) : (unsigned long long)x * x;
        }
        nq += 16ull * s2 - (unsigned long long)s1 * s1;   // 15 vari(quadrant), >= 0
        s1b += s1;
        s2b += s2;
    }
    const unsigned long long nb = 64ull * s2b - (unsigned long long)s1b * s1b;   // 63 vari(block), >= 0
    const double pop = nb > 0 ? ((double)nq / 15.0) / ((double)nb / 63.0) : 0.0;
#pragma unroll
    for (int r = 0; r < 8; r++)
#pragma unroll
        for (int c = 0; c < 8; c++) z[r][c] = (float)b.at(r, c);
    dct8x8(z, t);
    float e = 0.f;
#pragma unroll
    for (int k = 0; k < 8; k++)
#pragma unroll
        for (int l = 0; l < 8; l++)
            if (k | l) e = fmaf(z[k][l] * z[k][l], t.msk[k][l], e);
    return sqrtf(e * (float)pop) * (1.f / 32.f);
}

// grid = (workgroups * count, n_frames); block = 64.  acc: [frame][plane of the submit][PSNR_HVS_WORDS] uint64, zeroed by the submit
template <typename T, bool VEC>
__global__ __launch_bounds__(64) void k_psnr_hvs(hvs_src s, hvs_tabs t, int wgs, int n_planes, int4 plane_index,
                                                 unsigned long long *__restrict__ acc)
{
    const int f = blockIdx.y;
    const int ch = blockIdx.x / wgs, blk = (blockIdx.x % wgs) * 64 + (int)threadIdx.x;
    unsigned long long w0 = 0, w1 = 0, w2 = 0, w3 = 0;
    if (blk < s.nblocks) {
        const int by = blk / s.bw, bx = blk - by * s.bw;
        const int64_t o = s.off[ch] + (int64_t)(8 * by) * s.row_stride + (int64_t)(8 * bx) * s.step;
        hvs_raw<T> a, b;
        load_block<T, VEC>(a, s.ref + (int64_t)f * s.ref_fs + o, s.row_stride, s.step);
        load_block<T, VEC>(b, s.dist + (int64_t)f * s.dist_fs + o, s.row_stride, s.step);
        float z[8][8];
        const float ma = mask_of<T>(a, z, t);
        const float mb = mask_of<T>(b, z, t);
        const float m = fmaxf(ma, mb);
#pragma unroll
        for (int r = 0; r < 8; r++)
#pragma unroll
            for (int c = 0; c < 8; c++) z[r][c] = (float)(a.at(r, c) - b.at(r, c));   // exact: |a - b| < 2^16
        dct8x8(z, t);
        float hs = 0.f, hm = 0.f;
#pragma unroll
        for (int k = 0; k < 8; k++)
#pragma unroll
            for (int l = 0; l < 8; l++) {
                const float u = fabsf(z[k][l]);
                const float p = u * t.csf[k][l];
                const float q = fmaxf(u - m * t.thr[k][l], 0.f) * t.csf[k][l];
                hs = fmaf(p, p, hs);
                hm = fmaf(q, q, hm);
            }
        // both below 2^41 (vqa.h), so below 2^61 in units of 2^-20
        const unsigned long long fs = __float2ull_rn(hs * PSNR_HVS_FIX), fm = __float2ull_rn(hm * PSNR_HVS_FIX);
        w0 = fs & 0xffffffffull; w1 = fs >> 32; w2 = fm & 0xffffffffull; w3 = fm >> 32;
    }
    w0 = wave_sum(w0); w1 = wave_sum(w1); w2 = wave_sum(w2); w3 = wave_sum(w3);
    if (threadIdx.x == 0) {
        const int pi = ch == 0 ? plane_index.x : ch == 1 ? plane_index.y : ch == 2 ? plane_index.z : plane_index.w;
        unsigned long long *p = acc + ((int64_t)f * n_planes + pi) * PSNR_HVS_WORDS;
        atomicAdd(p + 0, w0);   // S_hvs: lo
        atomicAdd(p + 1, w1);   //        hi
        atomicAdd(p + 2, w2);   // S_hvsm: lo
        atomicAdd(p + 3, w3);   //         hi
    }
}

const hvs_tabs &hvs_tables()
{
    static hvs_tabs t;
    static std::once_flag once;
    std::call_once(once, [] {
        const double pi = 3.14159265358979323846;
        for (int k = 0; k < 8; k++)
            for (int n = 0; n < 4; n++)
                t.c[k][n] = (float)(std::sqrt((k == 0 ? 1.0 : 2.0) / 8.0) * std::cos((2 * n + 1) * k * pi / 16.0));
        for (int k = 0; k < 8; k++)
            for (int l = 0; l < 8; l++) {
                const double q = (double)PSNR_HVS_Q[k][l];
                t.csf[k][l] = (float)(PSNR_HVS_CSF_SCALE / q);
                t.msk[k][l] = (float)((10.0 / q) * (10.0 / q));
                t.thr[k][l] = (k | l) ? (float)((q / 10.0) * (q / 10.0)) : 0.f;
            }
    });
    return t;
}

} // namespace

void launch_psnr_hvs(hipStream_t st, const uint8_t *ref, const uint8_t *dist, int n, int64_t ref_frame_stride,
                     int64_t dist_frame_stride, const vqa_plane_desc *planes, const int *idx, int count, int n_planes, int depth,
                     unsigned long long *acc)
{
    if (n <= 0 || count <= 0) return;
    const vqa_plane_desc &pd = planes[idx[0]];
    hvs_src s;
    s.ref = ref; s.dist = dist; s.ref_fs = ref_frame_stride; s.dist_fs = dist_frame_stride;
    int p4[4];
    group_slots(planes, idx, count, s.off, p4);
    s.row_stride = pd.row_stride; s.step = pd.pixel_step;
    s.bw = pd.width / 8;
    s.nblocks = s.bw * (pd.height / 8);
    if (s.nblocks <= 0) return;
    const int bps = depth > 8 ? 2 : 1;
    // a row of a block as one load: unit step, and every address a multiple of the load's 8 * bps bytes
    uint64_t bits = (uint64_t)(uintptr_t)ref | (uint64_t)(uintptr_t)dist | (uint64_t)s.row_stride;
    if (n > 1) bits |= (uint64_t)ref_frame_stride | (uint64_t)dist_frame_stride;
    for (int i = 0; i < 4; i++) bits |= (uint64_t)s.off[i];
    const bool vec = s.step == bps && (bits & (uint64_t)(8 * bps - 1)) == 0;
    const int wgs = (s.nblocks + 63) / 64;
    const int4 pi = make_int4(p4[0], p4[1], p4[2], p4[3]);
    const dim3 grid(wgs * count, n), block(64);
    const hvs_tabs &t = hvs_tables();
    if (depth > 8) {
        if (vec) hipLaunchKernelGGL((k_psnr_hvs<uint16_t, true>), grid, block, 0, st, s, t, wgs, n_planes, pi, acc);
        else hipLaunchKernelGGL((k_psnr_hvs<uint16_t, false>), grid, block, 0, st, s, t, wgs, n_planes, pi, acc);
    } else {
        if (vec) hipLaunchKernelGGL((k_psnr_hvs<uint8_t, true>), grid, block, 0, st, s, t, wgs, n_planes, pi, acc);
        else hipLaunchKernelGGL((k_psnr_hvs<uint8_t, false>), grid, block, 0, st, s, t, wgs, n_planes, pi, acc);
    }
}

// the four words -> the record, in double on the host.  Contraction is off: the record is the formula vqa.h states.
void psnr_hvs_finalize(const unsigned long long *words, int h, int w, int depth, vqa_psnr_hvs_metrics *out)
{
#pragma clang fp contract(off)
    const double n_c = 64.0 * (double)((int64_t)(h / 8) * (w / 8));
    const double peak = (double)((1 << depth) - 1);
    double s[2];
    for (int k = 0; k < 2; k++) {
        // lo collects up to 2^22 halves below 2^32: its carry goes to hi first, so that both conversions are exact
        const unsigned long long lo = words[2 * k], hi = words[2 * k + 1] + (lo >> 32);
        const double fix = (double)hi * 4294967296.0 + (double)(lo & 0xffffffffull);
        s[k] = fix * (1.0 / (double)PSNR_HVS_FIX) / n_c;
    }
    out->s_hvs = s[0];
    out->s_hvsm = s[1];
    out->psnr_hvs = s[0] > 0.0 ? 10.0 * std::log10(peak * peak / s[0]) : HUGE_VAL;
    out->psnr_hvsm = s[1] > 0.0 ? 10.0 * std::log10(peak * peak / s[1]) : HUGE_VAL;
}

} // namespace vqa
