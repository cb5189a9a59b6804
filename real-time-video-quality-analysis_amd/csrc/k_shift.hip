// k_shift.hip — spatial registration for gfx950: the squared error of one plane between each distorted frame and its reference
// frame for every integer shift (dy, dx) of a square band -R .. R, over the same core of the distorted frame, by the definition
// stated in include/vqa.h (vqa_shift_submit).  Integers only.
//
//   k_shift<BPS, CUT>   sse(dy, dx) = E_d + E_r(dy, dx) - 2 C(dy, dx) with X = x - shift (the same shift on both sides, so it cancels):
//               E_d the core's sum of X_d^2, E_r(dy, dx) the sum of X_r^2 over the core moved by the shift, and the cross-correlation
//               C(dy, dx) = sum X_d(y, x) X_r(y + dy, x + dx) as a Toeplitz product on the int8 matrix cores
//               (v_mfma_i32_16x16x64_i8).  A workgroup is ONE wave; it owns one frame (blockIdx.y), one 16 x 16 tile of the grid
//               of shifts (blockIdx.z: 1 tile for R <= 7, 2 x 2 for R <= 15, 3 x 3 for R = 16) and SHIFT_ROWS reference rows y'
//               of M - R .. h - M + R - 1 at a time (blockIdx.x, grid-stride).  The waves of the tiles of a frame read the same
//               rows at the same time, one of them from HBM and the others from cache.
//               Operands (k_align_cross's map): lane l holds row / column l & 15 and the 16 consecutive k of group l >> 4.  For
//               reference row y' and the 64 columns from x0 on (x0 = 4 floor(M / 4) + 64 s: the A loads of a plane whose rows
//               start at multiples of 4 are then dword-aligned whatever the margin), A[m][k] = X_d(y' - dy_m, x0 + k), zero where
//               that row or column lies outside the core, and B[k][n] = X_r(y', x0 + k + dx_n): the same reference row read at
//               16 offsets, each lane's 16 samples an unaligned global load.  By the C/D map (col = l & 15, row = 4 (l >> 4) +
//               reg) register r of lane l is the entry a = 16 ty + 4 (l >> 4) + r, b = 16 tx + (l & 15) of the grid.  Rows and
//               columns that pad a tile beyond 2R + 1 hold zeros and are not read.
//               B is cut to the core's columns like A (k before the core's first or beyond its last column is zero on both
//               sides), so v_dot4_i32_i8 of B with itself is this lane's part of S(y', dx_n) = sum over the core's columns x of
//               X_r(y', x + dx_n)^2; the four lane groups are added once per row (two cross-lane moves) and S goes to
//               E_r(dy, dx_n) of exactly the dy whose core holds y' - dy.  E_d: the lanes whose A row is dy = 0 of the tile
//               that holds (0, *), tx = 0, square their own operand: every core row once.
//               uint16 samples (9 .. 16 bits, one path) are split into their low and high bytes, X = 256 (hi - 128) + (lo - 128):
//               four byte products, three accumulators.  The last, partial group of a row is read sample by sample, and so is
//               every group of a plane whose pixel_step is not its sample size (the slow path: a gather).  No byte outside the
//               w samples of a row is read: a column x0 + k + dx_n with x0 + k inside the core lies in 0 .. w - 1 because M >= R.
//
// Range: a product is at most 128 * 128 = 2^14 in magnitude and a matrix step adds 64 of them to an accumulator, two steps to
// the one HL and LH share; S adds 64 squares a step.  Every SHIFT_FLUSH = 512 steps, and at the end of the wave's rows, the
// accumulators leave through 64-bit integer vector atomics (2^14 * 64 * 2 * 512 = 2^30 < 2^31) into words the submit has
// zeroed, in two's complement: E_r - 2 C into the grid's word, E_d into the frame's.  Integer addition is associative and
// commutative: neither the tiling nor the order in which waves retire can change a bit.
#include "vqa_kernels.hpp"

namespace vqa {

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));

constexpr int SHIFT_FLUSH = 512;   // matrix steps of a wave between two flushes

struct shift_job {
    const uint8_t *ref, *dist;     // the first sample of the plane in frame 0 of either stream
    int64_t ref_fs, dist_fs, row_stride;
    int step;                      // bytes from a sample to the next of its row
    int w, h;
    int radius, margin;
    int blocks;                    // row blocks of SHIFT_ROWS reference rows
    unsigned long long *out, *e_dist;   // [n][2R + 1][2R + 1], [n]
};

// 16 samples of a row from sample x0 on, samples `first` .. `nval` - 1 of them wanted (0 <= first <= 3, nval <= 16), as signed
// bytes: lo (and hi for uint16 samples); the others, and every sample of a lane without a row (nval = 0), are X = 0.  Samples
// from nval on are not read; those before `first` are read only where the caller says they lie inside the row (head_ok)
template <int BPS>
__device__ __forceinline__ void load16(const uint8_t *row, int x0, int first, bool head_ok, int nval, int step, bool contig, v4i &lo,
                                       v4i &hi)
{
    lo = v4i{0, 0, 0, 0};
    hi = v4i{0, 0, 0, 0};
    if (nval <= first) return;
    const uint8_t *p = row + (int64_t)x0 * step;
    if (contig && nval == 16 && (first == 0 || head_ok)) {
        if (BPS == 1) {
            __builtin_memcpy(&lo, p, 16);
            lo ^= (int)0x80808080;
        } else {
            uint32_t d[8];
            __builtin_memcpy(d, p, 32);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t d0 = d[2 * k], d1 = d[2 * k + 1];
                const uint32_t l = (d0 & 0xffu) | ((d0 >> 8) & 0xff00u) | ((d1 & 0xffu) << 16) | ((d1 << 8) & 0xff000000u);
                const uint32_t u = ((d0 >> 8) & 0xffu) | ((d0 >> 16) & 0xff00u) | ((d1 << 8) & 0xff0000u) | (d1 & 0xff000000u);
                lo[k] = (int)(l ^ 0x80808080u);
                hi[k] = (int)(u ^ 0x80808080u);
            }
        }
        if (first) {   // (four samples a dword in lo and in hi alike)
            lo[0] &= (int)(~0u << (8 * first));
            hi[0] &= (int)(~0u << (8 * first));
        }
        return;
    }
    uint32_t l[4] = {0, 0, 0, 0}, u[4] = {0, 0, 0, 0};
    for (int k = first; k < nval; k++) {
        const uint8_t *s = p + (int64_t)k * step;
        const uint32_t v = BPS == 1 ? (uint32_t)*s : (uint32_t)*(const uint16_t *)s;
        l[k >> 2] |= ((v & 0xffu) ^ 0x80u) << (8 * (k & 3));
        if (BPS == 2) u[k >> 2] |= ((v >> 8) ^ 0x80u) << (8 * (k & 3));
    }
#pragma unroll
    for (int k = 0; k < 4; k++) { lo[k] = (int)l[k]; hi[k] = (int)u[k]; }
}

// sum over the 16 bytes of a[k] b[k], signed
__device__ __forceinline__ int dot16(v4i a, v4i b, int acc)
{
#pragma unroll
    for (int k = 0; k < 4; k++) acc = __builtin_amdgcn_sdot4(a[k], b[k], acc, false);
    return acc;
}

// the sum over the four lane groups of a wave, in every lane
__device__ __forceinline__ int sum_groups(int v)
{
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    return v;
}

// grid = (row blocks, at most the launch's cap; frames; tiles of the grid of shifts); block = 64.  CUT: the margin is no multiple
// of 4 and the first column step of a row starts before the core (without it the uint16 kernel keeps 5 waves a SIMD, not 4)
template <int BPS, bool CUT> __global__ __launch_bounds__(64) void k_shift(shift_job g)
{
    const int lane = threadIdx.x, f = lane & 15, q = lane >> 4;
    const int R = g.radius, M = g.margin, G = 2 * R + 1, T = shift_tiles(R);
    const int ty = (int)blockIdx.z / T, tx = (int)blockIdx.z % T;
    const int a = 16 * ty + f, b = 16 * tx + f;   // this lane's A row is dy = a - R, its B column dx = b - R
    const bool has_a = a < G, has_b = b < G;
    const int64_t j = blockIdx.y;
    const uint8_t *pd = g.dist + j * g.dist_fs, *pr = g.ref + j * g.ref_fs + (has_b ? (int64_t)(b - R) * g.step : 0);
    const bool contig = g.step == BPS;
    const bool sum_d = ty == R / 16 && tx == 0, lane_d = f == R % 16;   // (then a == R: the A row of dy = 0)
    // the column steps start at the multiple of 4 at or below M: the A loads of a plane whose rows start at multiples of 4 are
    // dword-aligned whatever the margin (those at other addresses cost about twice as much), and the up to three columns
    // before the core are zero on both sides like those behind it - loaded and masked where they lie inside the row, which
    // those of A always do and those of B unless x0 + dx < 0
    const int y_end = g.h - M, x_end = g.w - M, x_begin = M & ~3, rows = g.h - 2 * M + 2 * R, segs = (x_end - x_begin + 63) / 64;

    v4i c_ll = {0, 0, 0, 0}, c_m = {0, 0, 0, 0}, c_hh = {0, 0, 0, 0};
    v4i er_ll = {0, 0, 0, 0}, er_m = {0, 0, 0, 0}, er_hh = {0, 0, 0, 0};
    int s_ll = 0, s_m = 0, s_hh = 0, ed_ll = 0, ed_m = 0, ed_hh = 0, steps = 0;

    // S of reference row y so far, to E_r of the dy whose core holds row y - dy
    auto fold = [&](int y) {
        s_ll = sum_groups(s_ll);
        if (BPS == 2) { s_m = sum_groups(s_m); s_hh = sum_groups(s_hh); }
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int ar = 16 * ty + 4 * q + r, yd = y - (ar - R);
            if (ar < G && yd >= M && yd < y_end) {
                er_ll[r] += s_ll;
                if (BPS == 2) { er_m[r] += s_m; er_hh[r] += s_hh; }
            }
        }
        s_ll = s_m = s_hh = 0;
    };

    auto flush = [&]() {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int ar = 16 * ty + 4 * q + r;
            long long v = c_ll[r], e = er_ll[r];
            if (BPS == 2) {
                v += ((long long)c_hh[r] << 16) + ((long long)c_m[r] << 8);
                e += ((long long)er_hh[r] << 16) + ((long long)er_m[r] << 9);
            }
            const long long t = e - 2 * v;
            if (ar < G && has_b && t != 0) atomicAdd(g.out + (j * G + ar) * G + b, (unsigned long long)t);
        }
        if (sum_d && lane_d) {
            long long v = ed_ll;
            if (BPS == 2) v += ((long long)ed_hh << 16) + ((long long)ed_m << 9);
            if (v) atomicAdd(g.e_dist + j, (unsigned long long)v);
        }
        c_ll = c_m = c_hh = er_ll = er_m = er_hh = v4i{0, 0, 0, 0};
        ed_ll = ed_m = ed_hh = steps = 0;
    };

    for (int rb = (int)blockIdx.x; rb < g.blocks; rb += (int)gridDim.x) {
        const int e0 = rb * SHIFT_ROWS, e1 = e0 + SHIFT_ROWS < rows ? e0 + SHIFT_ROWS : rows;
        for (int e = e0; e < e1; e++) {
            const int y = M - R + e, yd = y - (a - R);   // the reference row, and the distorted row of this lane
            const bool row_a = has_a && yd >= M && yd < y_end;
            const uint8_t *rd = pd + (row_a ? (int64_t)yd * g.row_stride : 0), *rr = pr + (int64_t)y * g.row_stride;
            for (int s = 0; s < segs; s++) {
                const int x0 = x_begin + 64 * s + 16 * q, first = CUT && M > x0 ? M - x0 : 0;
                const int left = x_end - x0, nval = left >= 16 ? 16 : (left > 0 ? left : 0);
                v4i al, ah, bl, bh;
                load16<BPS>(rd, x0, first, true, row_a ? nval : 0, g.step, contig, al, ah);   // (x0 >= 0)
                load16<BPS>(rr, x0, first, x0 + b - R >= 0, has_b ? nval : 0, g.step, contig, bl, bh);
                c_ll = __builtin_amdgcn_mfma_i32_16x16x64_i8(al, bl, c_ll, 0, 0, 0);
                s_ll = dot16(bl, bl, s_ll);
                if (BPS == 2) {
                    c_m = __builtin_amdgcn_mfma_i32_16x16x64_i8(ah, bl, c_m, 0, 0, 0);
                    c_m = __builtin_amdgcn_mfma_i32_16x16x64_i8(al, bh, c_m, 0, 0, 0);
                    c_hh = __builtin_amdgcn_mfma_i32_16x16x64_i8(ah, bh, c_hh, 0, 0, 0);
                    s_m = dot16(bh, bl, s_m);
                    s_hh = dot16(bh, bh, s_hh);
                }
                if (sum_d) {
                    ed_ll = dot16(al, al, ed_ll);
                    if (BPS == 2) { ed_m = dot16(ah, al, ed_m); ed_hh = dot16(ah, ah, ed_hh); }
                }
                if (++steps >= SHIFT_FLUSH) {
                    fold(y);
                    flush();
                }
            }
            fold(y);
        }
    }
    flush();
}

} // namespace

void launch_shift(hipStream_t st, const uint8_t *ref, const uint8_t *dist, int n, int64_t ref_frame_stride, int64_t dist_frame_stride,
                  const vqa_plane_desc &plane, int depth, int radius, int margin, unsigned long long *out, unsigned long long *e_dist)
{
    shift_job g;
    g.ref = ref + plane.offset; g.dist = dist + plane.offset;
    g.ref_fs = ref_frame_stride; g.dist_fs = dist_frame_stride; g.row_stride = plane.row_stride;
    g.step = plane.pixel_step; g.w = plane.width; g.h = plane.height;
    g.radius = radius; g.margin = margin;
    g.blocks = shift_row_blocks(plane.height, radius, margin);
    g.out = out; g.e_dist = e_dist;
    const int tiles = shift_tiles(radius) * shift_tiles(radius);
    const dim3 grid(shift_grid_x(g.blocks, n, tiles), n, tiles), block(64);
    const bool cut = (margin & 3) != 0;
    if (depth > 8) {
        if (cut) hipLaunchKernelGGL((k_shift<2, true>), grid, block, 0, st, g);
        else hipLaunchKernelGGL((k_shift<2, false>), grid, block, 0, st, g);
    } else {
        if (cut) hipLaunchKernelGGL((k_shift<1, true>), grid, block, 0, st, g);
        else hipLaunchKernelGGL((k_shift<1, false>), grid, block, 0, st, g);
    }
}

} // namespace vqa
