// k_siti.hip — ITU-T P.910 spatial and temporal information for gfx950: the spread of the Sobel gradient of a reference frame
// and the spread of its difference to the frame before, by the definition stated in include/vqa.h (vqa_siti_submit).
//
//   k_siti<T>   one fused launch per group of same-geometry planes.  A workgroup of 256 threads owns a 64 x 32 tile of the
//               plane: the tile and its apron of ONE sample of frame i go to LDS once, as raw integers; every thread then forms
//               Sobel's gx and gy of two rows of four adjacent samples from LDS, q = gx^2 + gy^2 as an integer, and
//               rint(sqrt((double) q) 2^32) - the double-precision square root of an exactly converted integer.  The sample of
//               frame i - 1 under each output is read straight from global memory, once and with no apron, and differenced
//               against the LDS copy of frame i.  Four integer quantities are summed per thread, per wave and per workgroup;
//               five 64-bit words leave the kernel, one integer atomic each per workgroup.  About two input samples are read
//               per output sample ((66 x 34) / (64 x 32) = 1.1 of the current frame, the apron mostly from L2, and 1 of its
//               predecessor) and there is no scratch beyond the 40 bytes per (frame, plane).
//
// Sums (vqa.h states the bounds): q < 2^21 for uint8 and < 2^37.01 for any uint16 samples, so the fixed-point root is below
// 2^50.51 and a workgroup's 2048 of them below 2^61.51; the workgroup splits that total into its low and its high 32 bits and
// adds them to two words, neither of which a plane of 2^28 samples can overflow.  Integer addition is associative: neither the
// tiling nor the order in which workgroups retire can change a bit, so a frame (with its predecessor) gives the same five
// words at any place of any batch.  The workgroups of a frame without a predecessor form the gradient sums and skip the
// difference: its two diff words stay the 0 the submit's memset wrote.
#include <cmath>
#include <type_traits>

#include "vqa_dev.hpp"
#include "vqa_kernels.hpp"

namespace vqa {

namespace {

// the reference frames of one group of same-geometry planes; every stride in bytes
struct siti_src {
    const uint8_t *ref;     // frame 0 of the slice
    const uint8_t *prev0;   // the frame before it, or nullptr
    int64_t fs;             // frame stride
    int64_t off[4];         // plane offsets inside a frame
    int64_t row_stride;
    int step;
    int w, h;
};

// Borders: there is no border rule - Sobel is taken on the interior only, whose neighbours all lie in the plane.  The clamp
// below serves the apron of edge tiles and tiles that hang over the plane's edge: they read (and mask) in-plane samples.

// grid = (tiles * count, n_frames); block = 256.  acc: [frame][plane of the submit][SITI_WORDS] uint64, zeroed by the submit
template <typename T>
__global__ __launch_bounds__(256) void k_siti(siti_src s, int tiles_x, int tiles, int n_planes, int4 plane_index,
                                              unsigned long long *__restrict__ acc)
{
    using G = typename std::conditional<sizeof(T) == 1, int, long long>::type;
    constexpr int TW = 64, TH = 32, IW = TW + 4, IH = TH + 2;   // IW: 66 used, rows padded to 16 bytes
    __shared__ __attribute__((aligned(16))) int in[IH][IW];
    __shared__ unsigned long long red[4][4];
    const int f = blockIdx.y;
    const bool has_prev = f > 0 || s.prev0 != nullptr;   // (the whole workgroup)
    const int ch = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const int y0 = (tile / tiles_x) * TH, x0 = (tile % tiles_x) * TW;
    const int t = threadIdx.x;
    const uint8_t *pc = s.ref + (int64_t)f * s.fs + s.off[ch];
    for (int i = t; i < IH * (TW + 2); i += 256) {
        const int j = i / (TW + 2), c = i - j * (TW + 2);
        const int y = min(max(y0 + j - 1, 0), s.h - 1), x = min(max(x0 + c - 1, 0), s.w - 1);
        in[j][c] = (int)*(const T *)(pc + (int64_t)y * s.row_stride + (int64_t)x * s.step);
    }
    __syncthreads();
    // thread = (rows r and r + 16, four adjacent columns)
    const int r = t >> 4, q4 = (t & 15) * 4;
    unsigned long long fix = 0, gsq = 0, dsq = 0;
    long long dsum = 0;
    const uint8_t *pp = has_prev ? (f == 0 ? s.prev0 : s.ref + (int64_t)(f - 1) * s.fs) + s.off[ch] : nullptr;
#pragma unroll
    for (int half = 0; half < 2; half++) {
        const int row = r + 16 * half, y = y0 + row;
        int v[3][6];
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const int4 u0 = *reinterpret_cast<const int4 *>(&in[row + a][q4]);
            const int2 u1 = *reinterpret_cast<const int2 *>(&in[row + a][q4 + 4]);
            v[a][0] = u0.x; v[a][1] = u0.y; v[a][2] = u0.z; v[a][3] = u0.w; v[a][4] = u1.x; v[a][5] = u1.y;
        }
        const bool row_in = y < s.h, row_int = y >= 1 && y <= s.h - 2;
#pragma unroll
        for (int o = 0; o < 4; o++) {
            const int x = x0 + q4 + o;
            if (row_int && x >= 1 && x <= s.w - 2) {
                // |gx|, |gy| <= 4 (2^depth - 1): q fits 32 bits for uint8 samples and needs 64 for uint16
                const G gx = (v[0][o + 2] + 2 * v[1][o + 2] + v[2][o + 2]) - (v[0][o] + 2 * v[1][o] + v[2][o]);
                const G gy = (v[2][o] + 2 * v[2][o + 1] + v[2][o + 2]) - (v[0][o] + 2 * v[0][o + 1] + v[0][o + 2]);
                const auto q = (typename std::make_unsigned<G>::type)(gx * gx + gy * gy);
                gsq += q;
                fix += (unsigned long long)__double2ll_rn(sqrt((double)q) * SITI_FIX);
            }
            if (has_prev && row_in && x < s.w) {
                const long long d = v[1][o + 1] - (int)*(const T *)(pp + (int64_t)y * s.row_stride + (int64_t)x * s.step);
                dsum += d;
                dsq += (unsigned long long)(d * d);
            }
        }
    }
    const unsigned long long u0 = wave_sum(fix), u1 = wave_sum(gsq), u2 = wave_sum((unsigned long long)dsum), u3 = wave_sum(dsq);
    if (lane_id() == 0) {
        red[wave_id()][0] = u0; red[wave_id()][1] = u1; red[wave_id()][2] = u2; red[wave_id()][3] = u3;
    }
    __syncthreads();
    if (t == 0) {
        const int pi = ch == 0 ? plane_index.x : ch == 1 ? plane_index.y : ch == 2 ? plane_index.z : plane_index.w;
        unsigned long long *a = acc + ((int64_t)f * n_planes + pi) * SITI_WORDS;
        unsigned long long w[4];
#pragma unroll
        for (int k = 0; k < 4; k++) w[k] = red[0][k] + red[1][k] + red[2][k] + red[3][k];
        atomicAdd(a + 0, w[0] & 0xffffffffull);   // lo
        atomicAdd(a + 1, w[0] >> 32);             // hi
        atomicAdd(a + 2, w[1]);                   // grad_sq
        if (has_prev) {
            atomicAdd(a + 3, w[2]);               // diff_sum (two's complement: the wrap-around sum is the signed sum)
            atomicAdd(a + 4, w[3]);               // diff_sq
        }
    }
}

} // namespace

void launch_siti(hipStream_t st, const uint8_t *ref, const uint8_t *prev0, int n, int64_t frame_stride,
                 const vqa_plane_desc *planes, const int *idx, int count, int n_planes, int depth, unsigned long long *acc)
{
    if (n <= 0 || count <= 0) return;
    const vqa_plane_desc &pd = planes[idx[0]];
    siti_src s;
    s.ref = ref; s.prev0 = prev0; s.fs = frame_stride;
    int p4[4];
    group_slots(planes, idx, count, s.off, p4);
    s.row_stride = pd.row_stride; s.step = pd.pixel_step;
    s.w = pd.width; s.h = pd.height;
    const int tiles_x = (s.w + 63) / 64, tiles = tiles_x * ((s.h + 31) / 32);
    const int4 pi = make_int4(p4[0], p4[1], p4[2], p4[3]);
    const dim3 grid(tiles * count, n), block(256);
    if (depth > 8)
        hipLaunchKernelGGL((k_siti<uint16_t>), grid, block, 0, st, s, tiles_x, tiles, n_planes, pi, acc);
    else
        hipLaunchKernelGGL((k_siti<uint8_t>), grid, block, 0, st, s, tiles_x, tiles, n_planes, pi, acc);
}

// the five words -> the record, in double on the host.  Contraction is off: `a - m m` as one fused operation would not be the
// formula vqa.h states (the two differ by far more than an ulp where the variance is small against m m).
void siti_finalize(const unsigned long long *words, int h, int w, int depth, vqa_siti_metrics *out)
{
#pragma clang fp contract(off)
    const double sc = 1.0 / (double)(1 << (depth - 8));
    const double n_i = (double)((int64_t)(h - 2) * (w - 2)), n_a = (double)((int64_t)h * w);
    out->grad_sum = (double)words[1] + (double)words[0] * (1.0 / 4294967296.0);
    out->grad_sq = words[2];
    out->diff_sum = (int64_t)words[3];
    out->diff_sq = words[4];
    const double m = out->grad_sum / n_i;
    const double mm = m * m;
    const double var = (double)out->grad_sq / n_i - mm;
    out->si = sc * std::sqrt(var > 0.0 ? var : 0.0);
    // (a frame with no predecessor: both diff words are 0 and so is ti)
    const double md = (double)out->diff_sum / n_a;
    const double mdd = md * md;
    const double vd = (double)out->diff_sq / n_a - mdd;
    out->ti = sc * std::sqrt(vd > 0.0 ? vd : 0.0);
}

} // namespace vqa
