// k_gmsd.hip — gradient magnitude similarity deviation (Xue, Zhang, Mou, Bovik 2014) for gfx950: the spread and the mean of
// the similarity of the Prewitt gradient magnitudes of a plane pair after a 2x2 mean at step 2, by the definition stated in
// include/vqa.h (vqa_gmsd_submit).
//
//   k_gmsd<T>   one fused launch per group of same-geometry planes.  A workgroup of 256 threads owns a 64 x 32 tile of the
//               DOWNSAMPLED grid D (hd x wd = ceil(h / 2) x ceil(w / 2)): for both images the tile and its apron of ONE sample
//               of S = 4 D - the integer sum of a 2x2 input quad, samples outside the plane counting 0 - go to LDS straight from
//               the input, every input sample read once plus the apron's, mostly from L2.  Outside D the apron holds 0: the
//               border rule is conv2 'same', a zero fill, not a clamp.  Every thread then forms, for two rows of four adjacent
//               samples, 12 gx and 12 gy of Prewitt's operator as integer sums of S from LDS, q = (12 gx)^2 + (12 gy)^2 as an
//               integer for both images, and in double
//                   gms = (2 sqrt(q_r q_d) + c) / ((q_r + q_d) + c),  c = 144 T,
//               which is (2 m_r m_d + T) / (m_r^2 + m_d^2 + T) with m^2 = q / 144.  sqrt(x x) = x in IEEE arithmetic and
//               2 x + c is the same rounding as (x + x) + c, so q_r = q_d gives exactly 1.  u = rint(gms 2^24) is summed as an
//               integer, and so is u^2; three 64-bit words leave the kernel, one integer atomic each per workgroup.  Nothing
//               intermediate reaches HBM and there is no scratch beyond the 24 bytes per (frame, plane).
//
// Sums (vqa.h states the bounds): |12 gx| <= 12 peak, so q < 2^25 for uint8 (32-bit integers) and < 2^41 for any uint16 samples
// (64-bit); u <= 2^24 and a workgroup's 2048 values of u^2 total less than 2^59; the workgroup splits that total into its low
// and its high 32 bits and adds them to two words, neither of which a plane of 2^28 samples (N <= 2^26) can overflow.  Integer
// addition is associative: neither the tiling nor the order in which workgroups retire can change a bit, so a pair gives the
// same three words at any place of any batch.
#include <cmath>
#include <type_traits>

#include "vqa_dev.hpp"
#include "vqa_kernels.hpp"

namespace vqa {

namespace {

// both images of one group of same-geometry planes; every stride in bytes
struct gmsd_src {
    const uint8_t *ref, *dist;
    int64_t ref_fs, dist_fs;   // frame strides
    int64_t off[4];            // plane offsets inside a frame
    int64_t row_stride;
    int step;
    int w, h;                  // the plane
    int wd, hd;                // the downsampled grid
    double c;                  // 144 T
};

// S(dy, dx) = the sum of the input quad at (2 dy, 2 dx); a sample outside the plane counts 0, and so does all of S outside D
template <typename T> __device__ __forceinline__ int quad_sum(const uint8_t *p, const gmsd_src &s, int dy, int dx)
{
    if (dy < 0 || dy >= s.hd || dx < 0 || dx >= s.wd) return 0;
    const int y = 2 * dy, x = 2 * dx;            // y <= h - 1 and x <= w - 1 by hd = ceil(h / 2), wd = ceil(w / 2)
    const bool y1 = y + 1 < s.h, x1 = x + 1 < s.w;
    const uint8_t *a = p + (int64_t)y * s.row_stride + (int64_t)x * s.step;
    int v = (int)*(const T *)a;
    if (x1) v += (int)*(const T *)(a + s.step);
    if (y1) {
        const uint8_t *b = a + s.row_stride;
        v += (int)*(const T *)b;
        if (x1) v += (int)*(const T *)(b + s.step);
    }
    return v;
}

// grid = (tiles * count, n_frames); block = 256.  acc: [frame][plane of the submit][GMSD_WORDS] uint64, zeroed by the submit
template <typename T>
__global__ __launch_bounds__(256) void k_gmsd(gmsd_src s, int tiles_x, int tiles, int n_planes, int4 plane_index,
                                              unsigned long long *__restrict__ acc)
{
    using G = typename std::conditional<sizeof(T) == 1, int, long long>::type;
    constexpr int TW = 64, TH = 32, IW = TW + 4, IH = TH + 2;   // IW: 66 used, rows padded to 16 bytes
    __shared__ __attribute__((aligned(16))) int in[2][IH][IW];
    __shared__ unsigned long long red[4][2];
    const int f = blockIdx.y;
    const int ch = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const int y0 = (tile / tiles_x) * TH, x0 = (tile % tiles_x) * TW;
    const int t = threadIdx.x;
    const uint8_t *pr = s.ref + (int64_t)f * s.ref_fs + s.off[ch];
    const uint8_t *pd = s.dist + (int64_t)f * s.dist_fs + s.off[ch];
    for (int i = t; i < IH * (TW + 2); i += 256) {
        const int j = i / (TW + 2), c = i - j * (TW + 2);
        in[0][j][c] = quad_sum<T>(pr, s, y0 + j - 1, x0 + c - 1);
        in[1][j][c] = quad_sum<T>(pd, s, y0 + j - 1, x0 + c - 1);
    }
    __syncthreads();
    // thread = (rows r and r + 16, four adjacent columns)
    const int r = t >> 4, q4 = (t & 15) * 4;
    unsigned long long su = 0, su2 = 0;
#pragma unroll
    for (int half = 0; half < 2; half++) {
        const int row = r + 16 * half, y = y0 + row;
        int v[2][3][6];
#pragma unroll
        for (int im = 0; im < 2; im++)
#pragma unroll
            for (int a = 0; a < 3; a++) {
                const int4 u0 = *reinterpret_cast<const int4 *>(&in[im][row + a][q4]);
                const int2 u1 = *reinterpret_cast<const int2 *>(&in[im][row + a][q4 + 4]);
                v[im][a][0] = u0.x; v[im][a][1] = u0.y; v[im][a][2] = u0.z; v[im][a][3] = u0.w;
                v[im][a][4] = u1.x; v[im][a][5] = u1.y;
            }
        if (y < s.hd) {
#pragma unroll
            for (int o = 0; o < 4; o++) {
                if (x0 + q4 + o >= s.wd) continue;
                double q[2];
#pragma unroll
                for (int im = 0; im < 2; im++) {
                    // |12 gx|, |12 gy| <= 12 (2^depth - 1): q fits 32 bits for uint8 samples and needs 64 for uint16
                    const G gx = (G)(v[im][0][o + 2] + v[im][1][o + 2] + v[im][2][o + 2]) - (G)(v[im][0][o] + v[im][1][o] + v[im][2][o]);
                    const G gy = (G)(v[im][2][o] + v[im][2][o + 1] + v[im][2][o + 2]) - (G)(v[im][0][o] + v[im][0][o + 1] + v[im][0][o + 2]);
                    q[im] = (double)(gx * gx + gy * gy);   // exact: below 2^41
                }
                const double g = (2.0 * sqrt(q[0] * q[1]) + s.c) / ((q[0] + q[1]) + s.c);   // in (0, 1]
                const unsigned long long u = (unsigned long long)__double2ll_rn(g * GMSD_FIX);
                su += u;
                su2 += u * u;
            }
        }
    }
    const unsigned long long w0 = wave_sum(su), w1 = wave_sum(su2);
    if (lane_id() == 0) { red[wave_id()][0] = w0; red[wave_id()][1] = w1; }
    __syncthreads();
    if (t == 0) {
        const int pi = ch == 0 ? plane_index.x : ch == 1 ? plane_index.y : ch == 2 ? plane_index.z : plane_index.w;
        unsigned long long *a = acc + ((int64_t)f * n_planes + pi) * GMSD_WORDS;
        const unsigned long long tu = red[0][0] + red[1][0] + red[2][0] + red[3][0];
        const unsigned long long tq = red[0][1] + red[1][1] + red[2][1] + red[3][1];   // below 2^59
        atomicAdd(a + 0, tu);                    // sum u
        atomicAdd(a + 1, tq & 0xffffffffull);    // sum u^2: lo
        atomicAdd(a + 2, tq >> 32);              //          hi
    }
}

} // namespace

double gmsd_constant(int depth)
{
#pragma clang fp contract(off)
    const double k = (double)((1 << depth) - 1) / 255.0;
    return 144.0 * (GMSD_T8 * (k * k));
}

void launch_gmsd(hipStream_t st, const uint8_t *ref, const uint8_t *dist, int n, int64_t ref_frame_stride,
                 int64_t dist_frame_stride, const vqa_plane_desc *planes, const int *idx, int count, int n_planes, int depth,
                 unsigned long long *acc)
{
    if (n <= 0 || count <= 0) return;
    const vqa_plane_desc &pd = planes[idx[0]];
    gmsd_src s;
    s.ref = ref; s.dist = dist; s.ref_fs = ref_frame_stride; s.dist_fs = dist_frame_stride;
    int p4[4];
    group_slots(planes, idx, count, s.off, p4);
    s.row_stride = pd.row_stride; s.step = pd.pixel_step;
    s.w = pd.width; s.h = pd.height;
    s.wd = (s.w + 1) / 2; s.hd = (s.h + 1) / 2;
    s.c = gmsd_constant(depth);
    const int tiles_x = (s.wd + 63) / 64, tiles = tiles_x * ((s.hd + 31) / 32);
    const int4 pi = make_int4(p4[0], p4[1], p4[2], p4[3]);
    const dim3 grid(tiles * count, n), block(256);
    if (depth > 8)
        hipLaunchKernelGGL((k_gmsd<uint16_t>), grid, block, 0, st, s, tiles_x, tiles, n_planes, pi, acc);
    else
        hipLaunchKernelGGL((k_gmsd<uint8_t>), grid, block, 0, st, s, tiles_x, tiles, n_planes, pi, acc);
}

// the three words -> the record on the host: N sum u^2 - (sum u)^2 as a 128-bit integer (N <= 2^26, sum u^2 <= 2^74, so below
// 2^100), then one conversion, one division and one square root in double.  Contraction is off: the record is the formula vqa.h
// states.
void gmsd_finalize(const unsigned long long *words, int h, int w, vqa_gmsd_metrics *out)
{
#pragma clang fp contract(off)
    const int64_t n = (int64_t)((h + 1) / 2) * ((w + 1) / 2);
    out->sum_u = words[0];
    out->sum_u2_lo = words[1];
    out->sum_u2_hi = words[2];
    out->count = n;
    const unsigned __int128 s2 = ((unsigned __int128)words[2] << 32) + words[1];
    const unsigned __int128 a = (unsigned __int128)(uint64_t)n * s2, b = (unsigned __int128)words[0] * words[0];
    const double num = a > b ? (double)(a - b) : 0.0;   // (Cauchy-Schwarz: a >= b for any integers u)
    out->gms_mean = (double)words[0] / ((double)n * GMSD_FIX);
    out->gmsd = n > 1 ? std::sqrt(num / ((double)n * (double)(n - 1))) / GMSD_FIX : 0.0;
}

} // namespace vqa
