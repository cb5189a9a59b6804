// k_align.hip — temporal alignment for gfx950: the squared error between distorted frame j and reference frame j + offset + k
// for every k of a band -R .. R, by the definition stated in include/vqa.h (vqa_align_submit).  Integers only.
//
//   k_align_cross<BPS>   sse = E_d[j] + E_r[i] - 2 C[j][i] with X = x - shift (the same shift on both sides, so it cancels),
//               E = sum X^2 per frame and the Gram matrix C[j][i] = sum_p X_d,j[p] X_r,i[p] on the int8 matrix cores
//               (v_mfma_i32_16x16x64_i8).  A workgroup of four waves owns ONE 16-frame tile of the distorted stream and
//               ALIGN_ROWS rows of the plane; wave t of it owns the t-th 16-frame tile of the reference stream that the band of
//               that distorted tile meets (gridDim.z carries the tiles beyond four: R > 16).  All waves of a workgroup therefore
//               read the same bytes of the distorted frames at the same time - one of them from HBM, the others from L2 - and
//               each its own reference tile.
//               Operands: lane l holds frame l & 15 of its tile and 16 consecutive samples of a row, group (l >> 4) of the
//               step; A is the distorted tile and B the reference tile, so by the C/D map (col = l & 15, row = 4 (l >> 4) + reg)
//               register r of lane l is C[16 jt + 4 (l >> 4) + r][16 it + (l & 15)].  How the 64 products of a step are ordered
//               inside the instruction does not matter: A and B hold the same samples at the same k, and the sum commutes.
//               A step of the loop is two matrix steps: a lane reads 32 consecutive samples of its frame, the four lane groups
//               128 - whole 128-byte lines (uint8) are consumed by the wave that touches them.  Contiguous rows need no LDS:
//               both operands are 16-byte global loads (unaligned where the row starts odd), `x ^ 0x80` per byte makes them
//               signed.  uint16 samples (9 .. 16 bits, one path) are split into their low and high bytes, X = 256 (hi - 128) +
//               (lo - 128), and the cross term is 65536 HH + 256 (HL + LH) + LL: four products, three accumulators.
//               The last, partial group of a row is read sample by sample, and so is every group of a plane whose pixel_step
//               is not its sample size (the slow path: a gather); missing samples enter as X = 0 on both sides.  No byte
//               outside the w samples of a row is read.  Frames that pad a tile to 16 are not read: their lanes hold 0.
//               E: the wave of the first reference tile of a distorted tile adds E_d of its frames, the wave of the last
//               reference tile of a distorted tile (every wave of distorted tile 0) adds E_r of its frames - every frame that
//               some band needs is covered exactly once per plane range - with v_dot4_i32_i8 on the operands already loaded.
//
// Range: a product is at most 128 * 128 = 2^14 in magnitude and a matrix step adds 64 of them to an accumulator, two steps to
// the one HL and LH share; every ALIGN_FLUSH = 512 steps, and at the end of the plane range, the accumulators leave through
// 64-bit integer vector atomics (2^14 * 64 * 2 * 512 = 2^30 < 2^31) into words the submit has zeroed, in two's complement.
// Integer addition is associative and commutative: neither the tiling nor the order in which waves retire can change a bit.
#include "vqa_kernels.hpp"

namespace vqa {

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));

constexpr int ALIGN_ROWS = 8;      // rows of the plane per workgroup
constexpr int ALIGN_FLUSH = 512;   // matrix steps of a wave between two flushes

struct align_job {
    const uint8_t *ref, *dist;     // the first sample of the plane in frame 0 of either stream
    int64_t ref_fs, dist_fs, row_stride;
    int step;                      // bytes from a sample to the next of its row
    int w, h;
    int n_ref, n_dist, offset, radius;
    int jt0;                       // the first distorted tile launched
    unsigned long long *cross, *e_dist, *e_ref;   // [n_dist][2R + 1], [n_dist], [n_ref]
};

// 16 samples of a row from sample x0 on, `nval` of them inside the row (0 .. 16), as signed bytes: lo (and hi for uint16
// samples); a sample outside the row, and every sample of a lane without a frame (nval = 0), is X = 0
template <int BPS> __device__ __forceinline__ void load16(const uint8_t *row, int x0, int nval, int step, bool contig, v4i &lo, v4i &hi)
{
    lo = v4i{0, 0, 0, 0};
    hi = v4i{0, 0, 0, 0};
    if (nval <= 0) return;
    const uint8_t *p = row + (int64_t)x0 * step;
    if (contig && nval == 16) {
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
        return;
    }
    uint32_t l[4] = {0, 0, 0, 0}, u[4] = {0, 0, 0, 0};
    for (int k = 0; k < nval; k++) {
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

// floor(a / 16) for any sign
__device__ __host__ inline int tile_of(int a) { return a >= 0 ? a / 16 : -((15 - a) / 16); }

// grid = (ceil(h / ALIGN_ROWS), distorted tiles that meet the band, ceil(reference tiles of a band / 4)); block = 256
template <int BPS> __global__ __launch_bounds__(256) void k_align_cross(align_job g)
{
    const int lane = threadIdx.x & 63, f = lane & 15, q = lane >> 4;
    const int jt = g.jt0 + (int)blockIdx.y;
    // the reference tiles the band of this distorted tile meets: frames 16 jt + offset - R .. 16 jt + 15 + offset + R
    const int it_lo = tile_of(16 * jt + g.offset - g.radius), it_hi = tile_of(16 * jt + 15 + g.offset + g.radius);
    const int it = it_lo + 4 * (int)blockIdx.z + (int)(threadIdx.x >> 6);
    if (it < 0 || it > it_hi || 16 * it >= g.n_ref) return;   // (wave-uniform; the kernel has no barrier)
    const bool sum_d = it == (it_lo > 0 ? it_lo : 0), sum_r = jt == 0 || it == it_hi;
    const int j = 16 * jt + f, i = 16 * it + f;
    const bool has_d = j < g.n_dist, has_r = i < g.n_ref;
    const uint8_t *pd = g.dist + (has_d ? (int64_t)j * g.dist_fs : 0), *pr = g.ref + (has_r ? (int64_t)i * g.ref_fs : 0);
    const bool contig = g.step == BPS;
    const int row0 = (int)blockIdx.x * ALIGN_ROWS, row1 = row0 + ALIGN_ROWS < g.h ? row0 + ALIGN_ROWS : g.h;
    const int groups = (g.w + 15) / 16, band = 2 * g.radius + 1;

    v4i c_ll = {0, 0, 0, 0}, c_m = {0, 0, 0, 0}, c_hh = {0, 0, 0, 0};
    int ed_ll = 0, ed_m = 0, ed_hh = 0, er_ll = 0, er_m = 0, er_hh = 0, steps = 0;

    auto flush = [&]() {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int jj = 16 * jt + 4 * q + r, c = i - jj - g.offset + g.radius;
            long long v = c_ll[r];
            if (BPS == 2) v += ((long long)c_hh[r] << 16) + ((long long)c_m[r] << 8);
            if (jj < g.n_dist && has_r && c >= 0 && c < band && v != 0)
                atomicAdd(g.cross + (int64_t)jj * band + c, (unsigned long long)v);
        }
        if (sum_d && has_d) {
            long long v = ed_ll;
            if (BPS == 2) v += ((long long)ed_hh << 16) + ((long long)ed_m << 9);
            if (v) atomicAdd(g.e_dist + j, (unsigned long long)v);
        }
        if (sum_r && has_r) {
            long long v = er_ll;
            if (BPS == 2) v += ((long long)er_hh << 16) + ((long long)er_m << 9);
            if (v) atomicAdd(g.e_ref + i, (unsigned long long)v);
        }
        c_ll = c_m = c_hh = v4i{0, 0, 0, 0};
        ed_ll = ed_m = ed_hh = er_ll = er_m = er_hh = steps = 0;
    };

    for (int row = row0; row < row1; row++) {
        const uint8_t *rd = pd + (int64_t)row * g.row_stride, *rr = pr + (int64_t)row * g.row_stride;
        for (int g0 = 0; g0 < groups; g0 += 8) {
#pragma unroll
            for (int u = 0; u < 2; u++) {
                const int x0 = 16 * (g0 + 2 * q + u);
                const int left = g.w - x0, nval = left >= 16 ? 16 : (left > 0 ? left : 0);
                v4i al, ah, bl, bh;
                load16<BPS>(rd, x0, has_d ? nval : 0, g.step, contig, al, ah);
                load16<BPS>(rr, x0, has_r ? nval : 0, g.step, contig, bl, bh);
                c_ll = __builtin_amdgcn_mfma_i32_16x16x64_i8(al, bl, c_ll, 0, 0, 0);
                if (BPS == 2) {
                    c_m = __builtin_amdgcn_mfma_i32_16x16x64_i8(ah, bl, c_m, 0, 0, 0);
                    c_m = __builtin_amdgcn_mfma_i32_16x16x64_i8(al, bh, c_m, 0, 0, 0);
                    c_hh = __builtin_amdgcn_mfma_i32_16x16x64_i8(ah, bh, c_hh, 0, 0, 0);
                }
                if (sum_d) {
                    ed_ll = dot16(al, al, ed_ll);
                    if (BPS == 2) { ed_m = dot16(ah, al, ed_m); ed_hh = dot16(ah, ah, ed_hh); }
                }
                if (sum_r) {
                    er_ll = dot16(bl, bl, er_ll);
                    if (BPS == 2) { er_m = dot16(bh, bl, er_m); er_hh = dot16(bh, bh, er_hh); }
                }
            }
            steps += 2;
            if (steps >= ALIGN_FLUSH) flush();
        }
    }
    flush();
}

} // namespace

bool launch_align_cross(hipStream_t st, const uint8_t *ref, int n_ref, const uint8_t *dist, int n_dist, int64_t ref_frame_stride,
                        int64_t dist_frame_stride, const vqa_plane_desc &plane, int depth, int offset, int radius,
                        unsigned long long *cross, unsigned long long *e_dist, unsigned long long *e_ref)
{
    // the distorted tiles whose band meets a reference frame: a contiguous range, since both ends of a band grow with the tile
    const int tiles = (n_dist + 15) / 16, last_ref = (n_ref - 1) / 16;
    int jt0 = -1, jt1 = -1;
    for (int jt = 0; jt < tiles; jt++) {
        const int lo = tile_of(16 * jt + offset - radius), hi = tile_of(16 * jt + 15 + offset + radius);
        if (hi >= 0 && lo <= last_ref) {
            if (jt0 < 0) jt0 = jt;
            jt1 = jt;
        }
    }
    if (jt0 < 0) return false;
    align_job g;
    g.ref = ref + plane.offset; g.dist = dist + plane.offset;
    g.ref_fs = ref_frame_stride; g.dist_fs = dist_frame_stride; g.row_stride = plane.row_stride;
    g.step = plane.pixel_step; g.w = plane.width; g.h = plane.height;
    g.n_ref = n_ref; g.n_dist = n_dist; g.offset = offset; g.radius = radius; g.jt0 = jt0;
    g.cross = cross; g.e_dist = e_dist; g.e_ref = e_ref;
    const int per_band = (15 + 2 * radius) / 16 + 2;   // the most reference tiles a band of 16 + 2R frames can meet
    const dim3 grid((plane.height + ALIGN_ROWS - 1) / ALIGN_ROWS, jt1 - jt0 + 1, (per_band + 3) / 4), block(256);
    if (depth > 8)
        hipLaunchKernelGGL((k_align_cross<2>), grid, block, 0, st, g);
    else
        hipLaunchKernelGGL((k_align_cross<1>), grid, block, 0, st, g);
    return true;
}

} // namespace vqa
