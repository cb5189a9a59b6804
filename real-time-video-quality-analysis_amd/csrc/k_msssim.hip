// k_msssim.hip — the image pyramid and the end formulas of multi-scale SSIM (VQA_SSIM_MS) for gfx950.
//
// MS-SSIM (Wang, Simoncelli, Bovik 2003) in the 2x2-mean form tf.image.ssim_multiscale and pytorch-msssim compute: level
// s + 1 is the mean of each 2x2 block of level s, an odd level first padded by duplicating its last row / column -
//     L[s+1][i][j] = 1/4 sum_{di,dj in {0,1}} L[s][min(2i + di, h_s - 1)][min(2j + dj, w_s - 1)],   dims ceil(dim / 2)
// - every level goes through the Gaussian window of k_quality.hip (k_ssim_gauss_p2<.., CS>), and
//     MS-SSIM = prod_{s<4} max(mean cs_s, 0)^w_s * max(mean ssim_4, 0)^w_4,   w = (.0448, .2856, .3001, .2363, .1333).
//
//   k_ms_pyramid   levels 1..4 of ref and dist from ONE read of level 0.  A workgroup of 256 threads owns a 64x64 tile of
//                  level 0; a thread owns a 4x4 block of it: 16 loads per image -> its 2x2 samples of level 1 and its one
//                  sample of level 2 in registers; level 2 of the tile (16x16) goes through LDS to 64 threads for level 3
//                  (8x8), and that to 16 threads for level 4 (4x4).  The clamp is applied PER LEVEL, on that level's own
//                  size: the rows a level-(s+1) sample reads are min(2i + di, h_s - 1), and since a sample i < h_{s+1} =
//                  ceil(h_s / 2) has 2i <= h_s - 1, both lie in the same tile as 2i - no level ever looks outside its tile.
//                  Samples are kept EXACT: a level stores the fp32 SUM of the 4^s level-0 samples behind each sample
//                  (<= 256 x 65535 < 2^24 at level 4 of a 16-bit plane: integers fp32 holds exactly), and the SSIM kernel
//                  scales by 4^-s - a power of two - on its way in.  Nothing is rounded to the sample type.
//                  Algorithmic HBM bytes per plane pair of P samples of b bytes: 2 P b read + 2 x 0.332 P x 4 written.
//                  Loads are per sample (global_load_ubyte / ushort at the plane's pixel_step: a channel of packed BGR24 at
//                  step 3 takes the same path); the kernel is a few percent of the mode's time.
//   k_ms_finalize  a level's 2^-27 fixed-point totals -> the means cs_s, ssim_s of every frame (vqa_ms_scales, device side)
//   k_ms_combine   the clamped product, in double
#include "vqa_dev.hpp"
#include "vqa_kernels.hpp"

namespace vqa {

struct ms_pyr_args {
    int64_t offset[4];        // byte offset of each plane of the group inside a frame
    int count;
    int w[MS_LEVELS], h[MS_LEVELS];
    int64_t off[MS_LEVELS];   // ms_layout::off
};

// grid = (tiles_x * tiles_y * count, n_frames); block = 256
template <typename T>
__global__ __launch_bounds__(256) void k_ms_pyramid(const uint8_t *__restrict__ ref, const uint8_t *__restrict__ dist,
                                                    int64_t ref_fs, int64_t dist_fs, ms_pyr_args a, int64_t row_stride,
                                                    int step, int tiles_x, int tiles, float *__restrict__ out)
{
    __shared__ float s2[2][16][17];
    __shared__ float s3[2][8][9];
    const int f = blockIdx.y, n = gridDim.y;
    const int ch = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const int by = tile / tiles_x, bx = tile % tiles_x;
    const int t = threadIdx.x, ty = t >> 4, tx = t & 15;
    // this thread's sample of level 2 and the two rows / columns of level 1 it is made of, clamped on level 1's size;
    // under those, the four rows / columns of level 0, clamped on level 0's size.  Every index is inside the plane, so a
    // thread beyond the plane's edge loads (and never stores) duplicates of the edge.
    const int i2 = 16 * by + ty, j2 = 16 * bx + tx;
    int r0[4], c0[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int i1 = min(2 * i2 + (k >> 1), a.h[1] - 1), j1 = min(2 * j2 + (k >> 1), a.w[1] - 1);
        r0[k] = min(2 * i1 + (k & 1), a.h[0] - 1);
        c0[k] = min(2 * j1 + (k & 1), a.w[0] - 1);
    }
    const bool st1r[2] = {2 * i2 < a.h[1], 2 * i2 + 1 < a.h[1]}, st1c[2] = {2 * j2 < a.w[1], 2 * j2 + 1 < a.w[1]};
    const bool st2 = i2 < a.h[2] && j2 < a.w[2];
#pragma unroll
    for (int img = 0; img < 2; img++) {
        const uint8_t *src = (img ? dist + (int64_t)f * dist_fs : ref + (int64_t)f * ref_fs) + a.offset[ch];
        uint32_t v[4][4];
#pragma unroll
        for (int k = 0; k < 4; k++)
#pragma unroll
            for (int l = 0; l < 4; l++)
                v[k][l] = (uint32_t)*(const T *)(src + (int64_t)r0[k] * row_stride + (int64_t)c0[l] * step);
        const int64_t pl = ((int64_t)img * n + f) * a.count + ch;   // plane number inside a level
        float *o1 = out + a.off[1] + pl * a.h[1] * a.w[1];
        float l2 = 0.f;
#pragma unroll
        for (int p = 0; p < 2; p++)
#pragma unroll
            for (int q = 0; q < 2; q++) {
                const float l1 = (float)(v[2 * p][2 * q] + v[2 * p][2 * q + 1] + v[2 * p + 1][2 * q] + v[2 * p + 1][2 * q + 1]);
                if (st1r[p] && st1c[q]) o1[(int64_t)(2 * i2 + p) * a.w[1] + 2 * j2 + q] = l1;
                l2 += l1;   // integers below 2^24: exact
            }
        if (st2) out[a.off[2] + pl * a.h[2] * a.w[2] + (int64_t)i2 * a.w[2] + j2] = l2;
        s2[img][ty][tx] = l2;
    }
    __syncthreads();
    if (t < 128) {   // level 3: 8x8 per image, clamped on level 2's size (local index: the tile starts at row 16 by)
        const int img = t >> 6, i = (t >> 3) & 7, j = t & 7;
        const int rl = a.h[2] - 1 - 16 * by, cl = a.w[2] - 1 - 16 * bx;   // >= 0: the tile holds level-0 samples
        const int ra = min(2 * i, rl), rb = min(2 * i + 1, rl), ca = min(2 * j, cl), cb = min(2 * j + 1, cl);
        const float l3 = (s2[img][ra][ca] + s2[img][ra][cb]) + (s2[img][rb][ca] + s2[img][rb][cb]);
        const int i3 = 8 * by + i, j3 = 8 * bx + j;
        const int64_t pl = ((int64_t)img * n + f) * a.count + ch;
        if (i3 < a.h[3] && j3 < a.w[3]) out[a.off[3] + pl * a.h[3] * a.w[3] + (int64_t)i3 * a.w[3] + j3] = l3;
        s3[img][i][j] = l3;
    }
    __syncthreads();
    if (t < 32) {    // level 4: 4x4 per image, clamped on level 3's size
        const int img = t >> 4, i = (t >> 2) & 3, j = t & 3;
        const int rl = a.h[3] - 1 - 8 * by, cl = a.w[3] - 1 - 8 * bx;
        const int ra = min(2 * i, rl), rb = min(2 * i + 1, rl), ca = min(2 * j, cl), cb = min(2 * j + 1, cl);
        const float l4 = (s3[img][ra][ca] + s3[img][ra][cb]) + (s3[img][rb][ca] + s3[img][rb][cb]);
        const int i4 = 4 * by + i, j4 = 4 * bx + j;
        const int64_t pl = ((int64_t)img * n + f) * a.count + ch;
        if (i4 < a.h[4] && j4 < a.w[4]) out[a.off[4] + pl * a.h[4] * a.w[4] + (int64_t)i4 * a.w[4] + j4] = l4;
    }
}

void launch_ms_pyramid(hipStream_t st, const uint8_t *ref, const uint8_t *dist, int n, int64_t ref_frame_stride,
                       int64_t dist_frame_stride, const vqa_plane_desc *planes, const int *idx, int count, int depth,
                       float *scratch)
{
    if (n <= 0 || count <= 0) return;
    const vqa_plane_desc &pd = planes[idx[0]];
    const ms_layout L = ms_levels(n, count, pd.height, pd.width);
    ms_pyr_args a;
    a.count = count;
    group_slots(planes, idx, count, a.offset, nullptr);
    for (int s = 0; s < MS_LEVELS; s++) { a.w[s] = L.w[s]; a.h[s] = L.h[s]; a.off[s] = L.off[s]; }
    const int tiles_x = (pd.width + 63) / 64, tiles = tiles_x * ((pd.height + 63) / 64);
    const dim3 grid(tiles * count, n), block(256);
    if (depth > 8)
        hipLaunchKernelGGL(k_ms_pyramid<uint16_t>, grid, block, 0, st, ref, dist, ref_frame_stride, dist_frame_stride, a,
                           pd.row_stride, pd.pixel_step, tiles_x, tiles, scratch);
    else
        hipLaunchKernelGGL(k_ms_pyramid<uint8_t>, grid, block, 0, st, ref, dist, ref_frame_stride, dist_frame_stride, a,
                           pd.row_stride, pd.pixel_step, tiles_x, tiles, scratch);
}

// The tile totals are integers (2^-27 fixed point): their sum does not depend on the order, so neither do the means.
// The means are total / count - a map of ones has a mean of exactly 1 (total * (1 / count) can miss it by an ulp) - except
// ssim of level 0, which is formed by k_ssim_finalize's own expression: it is VQA_SSIM_GAUSS's value, bit for bit.
__global__ void k_ms_finalize(const double *__restrict__ partials, int64_t cs_offset, int bpp, int n, double count,
                              int plane_index, int n_planes, int level, vqa_ms_scales *__restrict__ ms)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n) return;
    const long long *p = reinterpret_cast<const long long *>(partials) + (int64_t)f * bpp;
    long long s = 0, c = 0;
    for (int i = 0; i < bpp; i++) { s += p[i]; c += p[cs_offset + i]; }
    vqa_ms_scales &m = ms[(int64_t)f * n_planes + plane_index];
    const double fs = (double)s * (1.0 / 134217728.0), fc = (double)c * (1.0 / 134217728.0);   // (|s| < 2^53: exact)
    m.ssim[level] = level == 0 ? fs * (1.0 / count) : fs / count;
    m.cs[level] = fc / count;
}

void launch_ms_finalize(hipStream_t st, const double *partials, int64_t cs_offset, int bpp, int n, double count,
                        int plane_index, int n_planes, int level, vqa_ms_scales *ms)
{
    hipLaunchKernelGGL(k_ms_finalize, dim3((n + 63) / 64), dim3(64), 0, st, partials, cs_offset, bpp, n, count, plane_index,
                       n_planes, level, ms);
}

__global__ void k_ms_combine(const vqa_ms_scales *__restrict__ ms, int n_entries, vqa_plane_metrics *__restrict__ res)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_entries) return;
    const double wgt[MS_LEVELS] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};
    double v = 1.0;
    for (int s = 0; s < MS_LEVELS; s++) {
        const double x = s < MS_LEVELS - 1 ? ms[e].cs[s] : ms[e].ssim[s];
        v *= x > 0.0 ? pow(x, wgt[s]) : 0.0;   // relu: a negative mean gives 0, not NaN
    }
    res[e].ssim = v;
}

void launch_ms_combine(hipStream_t st, const vqa_ms_scales *ms, int n_entries, vqa_plane_metrics *res)
{
    hipLaunchKernelGGL(k_ms_combine, dim3((n_entries + 63) / 64), dim3(64), 0, st, ms, n_entries, res);
}

} // namespace vqa
