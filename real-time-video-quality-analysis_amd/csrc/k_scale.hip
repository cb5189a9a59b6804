// k_scale.hip — the resampler of vqa_scale_submit for gfx950: plane i of the source list into plane i of the destination list,
// horizontal pass first, by the definition stated in include/vqa.h (Pillow's Image.resize for 8-bit images: integer tables in
// 2^-22 fixed point, every pass rounded, clipped and stored at the sample type).
//
//   k_scale<T>   one fused launch per group of planes whose source AND destination geometries agree.  A workgroup of 256 threads
//                owns a 64 x 32 tile of the DESTINATION plane.  Its footprint in the source is the rows [ymin(first row),
//                ymin + count of the last row) and the columns likewise: at most SCALE_FH x SCALE_FW samples at the limits
//                (4x down, lanczos).  The footprint goes through LDS in chunks of SCALE_RC source rows: the chunk is loaded
//                coalesced, one lane a sample, every source sample once per tile that needs it; then a wave takes four rows of
//                the chunk and a lane one destination column, and the horizontal pass of those rows is formed into the LDS
//                intermediate inter[source row][destination column] at the sample type - clipped, as the definition says.
//                After the last chunk a wave takes destination rows and a lane a column; the vertical pass reads the
//                intermediate and the tile is written.  The intermediate never reaches HBM.  The tables of the tile's 64 columns
//                and 32 rows are copied to LDS once, before the first chunk (the horizontal one with an odd row stride, so the
//                lanes of a wave read their rows without a bank conflict; the vertical one is read wave-uniform, a broadcast).
//                Read from device memory row by row through the scalar path instead, the vertical table cost the 10-bit
//                cases a third more time and the 8-bit cases nothing.  Sums: 32-bit multiply-adds for uint8 samples (255 sum |k| < 2^31), v_mad_i64_i32 for uint16.
//
// No atomics and no reduction: a destination sample is a function of its own windows alone, so a frame gives the same bytes at
// any place of any batch.  The tables are built on the host (scale_build_axis below, in double with contraction off).
#include <cmath>
#include <type_traits>

#include "vqa_dev.hpp"
#include "vqa_kernels.hpp"

namespace vqa {

namespace {

constexpr int TW = SCALE_TILE_W, TH = SCALE_TILE_H;
constexpr int KROW = SCALE_KSIZE_MAX;   // 25: odd, so the 64 lanes of a wave read their rows of the table without a bank conflict

template <typename T>
__global__ __launch_bounds__(256) void k_scale(scale_job s, int tiles_x)
{
    using A = typename std::conditional<sizeof(T) == 1, int, long long>::type;
    // (at the sample type: with 16-bit words for uint8 samples too the 8-bit cases measured a quarter slower)
    __shared__ T stage[SCALE_RC][SCALE_FW];
    __shared__ T inter[SCALE_FH][TW];
    __shared__ int kx[TW][KROW], ky[TH][KROW];
    __shared__ int xo[TW], xc[TW], yo[TH], yc[TH];
    const int f = blockIdx.y, ch = blockIdx.z, tile = blockIdx.x;
    const int y0 = (tile / tiles_x) * TH, x0 = (tile % tiles_x) * TW;
    const int tw = min(TW, s.dw - x0), th = min(TH, s.dh - y0);
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    // the footprint: xmin and xmin + count never decrease along an axis
    const int fx0 = s.xmin[x0], fy0 = s.ymin[y0];
    const int fw = min(s.xmin[x0 + tw - 1] + s.xcount[x0 + tw - 1] - fx0, SCALE_FW);   // (the host has checked both bounds)
    const int fh = min(s.ymin[y0 + th - 1] + s.ycount[y0 + th - 1] - fy0, SCALE_FH);
    const uint8_t *src = s.src + (int64_t)f * s.src_fs + s.src_off[ch];
    uint8_t *dst = s.dst + (int64_t)f * s.dst_fs + s.dst_off[ch];
    const A half = (A)1 << (SCALE_BITS - 1), peak = (A)s.peak, peak_x = (A)s.peak_x;

    if (t < TW) {
        const bool in = t < tw;
        xo[t] = in ? s.xmin[x0 + t] - fx0 : 0;
        xc[t] = in ? min(s.xcount[x0 + t], s.ksx) : 0;
    } else if (t < TW + TH) {
        const int y = t - TW;
        const bool in = y < th;
        yo[y] = in ? s.ymin[y0 + y] - fy0 : 0;
        yc[y] = in ? min(s.ycount[y0 + y], s.ksy) : 0;
    }
    for (int i = t; i < tw * s.ksx; i += 256) {
        const int x = i / s.ksx, j = i - x * s.ksx;
        kx[x][j] = s.kx[(int64_t)(x0 + x) * s.ksx + j];
    }
    for (int i = t; i < th * s.ksy; i += 256) {
        const int y = i / s.ksy, j = i - y * s.ksy;
        ky[y][j] = s.ky[(int64_t)(y0 + y) * s.ksy + j];
    }

    for (int r0 = 0; r0 < fh; r0 += SCALE_RC) {
        const int rc = min(SCALE_RC, fh - r0);
        __syncthreads();   // the table before the first chunk; the pass over the chunk before
        for (int r = wave; r < rc; r += 4) {
            const uint8_t *row = src + (int64_t)(fy0 + r0 + r) * s.src_rs + (int64_t)fx0 * s.src_step;
            for (int c = lane; c < fw; c += 64) stage[r][c] = *(const T *)(row + (int64_t)c * s.src_step);
        }
        __syncthreads();
        // rows wave, wave + 4, wave + 8, wave + 12 of the chunk; lane = destination column
        const int n = xc[lane], o = min(xo[lane], SCALE_FW - KROW);
        A acc[4] = {half, half, half, half};
        for (int j = 0; j < n; j++) {
            const A k = (A)kx[lane][j];
#pragma unroll
            for (int q = 0; q < 4; q++) acc[q] += k * (A)(int)stage[wave + 4 * q][o + j];
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int r = wave + 4 * q;
            if (r < rc && lane < tw) inter[r0 + r][lane] = (T)min(max(acc[q] >> SCALE_BITS, (A)0), peak_x);
        }
    }
    __syncthreads();

    // rows wave, wave + 4, ... of the tile; lane = destination column
    for (int y = wave; y < th; y += 4) {
        const int Y = y0 + y;
        const int n = yc[y], o = yo[y];
        A acc = half;
        for (int j = 0; j < n; j++) acc += (A)ky[y][j] * (A)(int)inter[min(o + j, SCALE_FH - 1)][lane];
        if (lane < tw)
            *(T *)(dst + (int64_t)Y * s.dst_rs + (int64_t)(x0 + lane) * s.dst_step) = (T)min(max(acc >> SCALE_BITS, (A)0), peak);
    }
}

double scale_bilinear(double x)
{
#pragma clang fp contract(off)
    if (x < 0.0) x = -x;
    return x < 1.0 ? 1.0 - x : 0.0;
}

double scale_bicubic(double x)
{
#pragma clang fp contract(off)
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

double scale_sinc(double x)
{
#pragma clang fp contract(off)
    if (x == 0.0) return 1.0;
    x = x * M_PI;
    return std::sin(x) / x;
}

double scale_lanczos(double x)
{
#pragma clang fp contract(off)
    return (-3.0 <= x && x < 3.0) ? scale_sinc(x) * scale_sinc(x / 3) : 0.0;
}

} // namespace

bool scale_filter_known(int filter) { return filter == VQA_SCALE_BILINEAR || filter == VQA_SCALE_BICUBIC || filter == VQA_SCALE_LANCZOS; }

bool scale_ratio_ok(int in, int out) { return in > 0 && out > 0 && (int64_t)in <= 4 * (int64_t)out && (int64_t)out <= 8 * (int64_t)in; }

static double scale_support(int filter) { return filter == VQA_SCALE_BILINEAR ? 1.0 : filter == VQA_SCALE_BICUBIC ? 2.0 : 3.0; }

int scale_ksize(int filter, int in, int out)
{
#pragma clang fp contract(off)
    const double scale = (double)in / (double)out, fs = scale < 1.0 ? 1.0 : scale;
    return 2 * (int)std::ceil(scale_support(filter) * fs) + 1;
}

void scale_build_axis(int filter, int in, int out, int32_t *k, int32_t *xmin, int32_t *count)
{
#pragma clang fp contract(off)
    double (*f)(double) = filter == VQA_SCALE_BILINEAR ? scale_bilinear : filter == VQA_SCALE_BICUBIC ? scale_bicubic : scale_lanczos;
    const double scale = (double)in / (double)out, fs = scale < 1.0 ? 1.0 : scale;
    const double support = scale_support(filter) * fs, ss = 1.0 / fs;
    const int ksize = 2 * (int)std::ceil(support) + 1;
    double w[SCALE_KSIZE_MAX + 2];
    for (int x = 0; x < out; x++) {
        const double c = (x + 0.5) * scale;
        int lo = (int)(c - support + 0.5), hi = (int)(c + support + 0.5);
        lo = lo < 0 ? 0 : lo;
        hi = hi > in ? in : hi;
        int n = hi - lo;
        n = n < 0 ? 0 : n > ksize ? ksize : n;   // (n <= ksize by construction)
        double ww = 0.0;
        for (int j = 0; j < n; j++) {
            w[j] = f((j + lo - c + 0.5) * ss);
            ww += w[j];
        }
        int32_t *row = k + (size_t)x * ksize;
        for (int j = 0; j < ksize; j++) {
            if (j >= n) { row[j] = 0; continue; }
            const double v = ww != 0.0 ? w[j] / ww : w[j];
            row[j] = v < 0 ? (int32_t)(v * (double)(1 << SCALE_BITS) - 0.5) : (int32_t)(v * (double)(1 << SCALE_BITS) + 0.5);
        }
        xmin[x] = lo;
        count[x] = n;
    }
}

int scale_footprint(const int32_t *xmin, const int32_t *count, int out, int tile)
{
    int most = 0;
    for (int a = 0; a < out; a += tile) {
        const int b = (a + tile < out ? a + tile : out) - 1;
        const int span = xmin[b] + count[b] - xmin[a];
        most = span > most ? span : most;
    }
    return most;
}

void launch_scale(hipStream_t st, const scale_job &job, int n, int count, int depth)
{
    if (n <= 0 || count <= 0) return;
    const int tiles_x = (job.dw + TW - 1) / TW, tiles = tiles_x * ((job.dh + TH - 1) / TH);
    const dim3 grid(tiles, n, count), block(256);
    if (depth > 8)
        hipLaunchKernelGGL((k_scale<uint16_t>), grid, block, 0, st, job, tiles_x);
    else
        hipLaunchKernelGGL((k_scale<uint8_t>), grid, block, 0, st, job, tiles_x);
}

} // namespace vqa
