// k_haarpsi.hip — the Haar wavelet-based perceptual similarity index (Reisenhofer, Bosse, Kutyniok, Wiegand 2018) for gfx950:
// the weighted mean of a sigmoid of the local similarity of Haar coefficients of a plane pair after a 2x2 mean at step 2, by
// the definition stated in include/vqa.h (vqa_haarpsi_submit).
//
//   k_haarpsi<T>   one fused launch per group of same-geometry planes.  A workgroup of 256 threads owns a 64 x 32 tile of the
//               DOWNSAMPLED grid D (hd x wd = ceil(h / 2) x ceil(w / 2)): for both images the tile and its apron - 3 samples
//               before, 4 after, the reach of the 8 x 8 window as MATLAB centres it - of S = 4 D, the integer sum of a 2x2
//               input quad, go to LDS straight from the input (k_gmsd's stage).  Outside D the apron holds 0: conv2 'same' is a
//               zero fill.  A thread owns EIGHT ADJACENT SAMPLES OF ONE ROW.  Per image it reads the 8 rows x 15 columns its
//               windows cover once (32 ds_read_b128), forms per column the sums of the upper and of the lower 1, 2 and 4 rows,
//               each from the one before, then per scale the sums of 1, 2 and 4 adjacent columns, again each from the one
//               before: 15 LDS samples per sample and image instead of the 168 of the three windows taken one by one.  The six
//               H per image are integers.  The two similarities per orientation, their mean and the sigmoid are formed in
//               double with contraction off; u = rint(2^30 sigmoid), u = U1 where the mean is exactly 1.  The weights and the
//               products u wI are summed as integers; three 64-bit words leave the kernel, one integer atomic each per
//               workgroup.  Nothing intermediate reaches HBM and there is no scratch beyond the 24 bytes per (frame, plane).
//
// Sums (vqa.h states the bounds): |H_2| <= 32 peak, so the products of the similarity fit 32 bits for uint8 and need 64 for
// uint16; wI = max |H_3| < 2^23 and u <= 2^30, so a thread's 16 terms total less than 2^57; the THREAD splits that total into its
// low and its high 32 bits, and only those halves are added further - a workgroup's 4096 terms would not fit one word.  Integer
// addition is associative: neither the tiling nor the order in which workgroups retire can change a bit, so a pair gives the
// same three words at any place of any batch.
#include <cmath>
#include <type_traits>

#include "vqa_dev.hpp"
#include "vqa_kernels.hpp"

namespace vqa {

namespace {

// both images of one group of same-geometry planes; every stride in bytes
struct haarpsi_src {
    const uint8_t *ref, *dist;
    int64_t ref_fs, dist_fs;   // frame strides
    int64_t off[4];            // plane offsets inside a frame
    int64_t row_stride;
    int step;
    int w, h;                  // the plane
    int wd, hd;                // the downsampled grid
    double c1, c2;             // c_s = 4^(s+2) (30 k^2)
    unsigned long long u1;     // u where the local similarity is exactly 1
};

constexpr int HP_TW = 64, HP_TH = 32, HP_PRE = 3, HP_POST = 4;
constexpr int HP_IH = HP_TH + HP_PRE + HP_POST;       // 39 rows
constexpr int HP_IW = HP_TW + HP_PRE + HP_POST + 1;   // 71 columns used, rows padded to 16 bytes

// S(dy, dx) = the sum of the input quad at (2 dy, 2 dx); a sample outside the plane counts 0, and so does all of S outside D
template <typename T> __device__ __forceinline__ int quad_sum(const uint8_t *p, const haarpsi_src &s, int dy, int dx)
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

// 16 adjacent samples of one LDS row (the last one is the row's pad or a neighbour's sample and is never used)
__device__ __forceinline__ void load_row(const int *p, int (&x)[16])
{
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int4 u = *reinterpret_cast<const int4 *>(p + 4 * k);
        x[4 * k] = u.x; x[4 * k + 1] = u.y; x[4 * k + 2] = u.z; x[4 * k + 3] = u.w;
    }
}

// one scale of one image: t, b = per column the sums of the HALF rows above and below the row seam.  H[0][o] sums t - b over
// the 2 HALF columns of sample o's window, H[1][o] takes t + b of its left HALF columns minus its right HALF columns.  Sample o
// sits at column o + 3 of the 15: its window is columns o + 4 - HALF .. o + 3 + HALF.
template <int HALF> __device__ __forceinline__ void haar_scale(const int (&t)[16], const int (&b)[16], int (&H)[2][8])
{
    int v[16], w[16];
#pragma unroll
    for (int c = 0; c < 15; c++) { v[c] = t[c] - b[c]; w[c] = t[c] + b[c]; }
    if (HALF >= 2) {
#pragma unroll
        for (int c = 0; c < 14; c++) { v[c] += v[c + 1]; w[c] += w[c + 1]; }   // two adjacent columns
    }
    if (HALF >= 4) {
#pragma unroll
        for (int c = 0; c < 12; c++) { v[c] += v[c + 2]; w[c] += w[c + 2]; }   // four
    }
#pragma unroll
    for (int o = 0; o < 8; o++) {
        H[0][o] = v[o + 4 - HALF] + v[o + 4];
        H[1][o] = w[o + 4 - HALF] - w[o + 4];
    }
}

// the six coefficients of eight adjacent samples of one image: H[orientation][scale - 1][sample].  p: the LDS row of the
// samples' row - 3, at the first sample's column - 3; rows are HP_IW apart.
__device__ __forceinline__ void haar_coefficients(const int *p, int (&H)[2][3][8])
{
    int t[16], b[16], x[16], hs[2][8];
    load_row(p + 3 * HP_IW, t);
    load_row(p + 4 * HP_IW, b);
    haar_scale<1>(t, b, hs);
#pragma unroll
    for (int o = 0; o < 8; o++) { H[0][0][o] = hs[0][o]; H[1][0][o] = hs[1][o]; }
    load_row(p + 2 * HP_IW, x);
#pragma unroll
    for (int c = 0; c < 15; c++) t[c] += x[c];
    load_row(p + 5 * HP_IW, x);
#pragma unroll
    for (int c = 0; c < 15; c++) b[c] += x[c];
    haar_scale<2>(t, b, hs);
#pragma unroll
    for (int o = 0; o < 8; o++) { H[0][1][o] = hs[0][o]; H[1][1][o] = hs[1][o]; }
#pragma unroll
    for (int a = 0; a < 2; a++) {
        load_row(p + a * HP_IW, x);
#pragma unroll
        for (int c = 0; c < 15; c++) t[c] += x[c];
        load_row(p + (6 + a) * HP_IW, x);
#pragma unroll
        for (int c = 0; c < 15; c++) b[c] += x[c];
    }
    haar_scale<4>(t, b, hs);
#pragma unroll
    for (int o = 0; o < 8; o++) { H[0][2][o] = hs[0][o]; H[1][2][o] = hs[1][o]; }
}

// (2 |H_r H_d| + c) / ((H_r^2 + H_d^2) + c): the integers are exact (G: 32 bits for uint8 samples, 64 for uint16), each of the
// two sums and the division rounds once
template <typename G> __device__ __forceinline__ double local_similarity(int hr, int hd, double c)
{
#pragma clang fp contract(off)
    G p = (G)hr * (G)hd;
    if (p < 0) p = -p;
    const G q = (G)hr * (G)hr + (G)hd * (G)hd;
    return (2.0 * (double)p + c) / ((double)q + c);
}

// grid = (tiles * count, n_frames); block = 256.  acc: [frame][plane of the submit][HAARPSI_WORDS] uint64, zeroed by the submit
template <typename T>
__global__ __launch_bounds__(256) void k_haarpsi(haarpsi_src s, int tiles_x, int tiles, int n_planes, int4 plane_index,
                                                 unsigned long long *__restrict__ acc)
{
#pragma clang fp contract(off)
    using G = typename std::conditional<sizeof(T) == 1, int, long long>::type;
    __shared__ __attribute__((aligned(16))) int in[2][HP_IH][HP_IW];
    __shared__ unsigned long long red[4][3];
    const int f = blockIdx.y;
    const int ch = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const int y0 = (tile / tiles_x) * HP_TH, x0 = (tile % tiles_x) * HP_TW;
    const int t = threadIdx.x;
    const uint8_t *pr = s.ref + (int64_t)f * s.ref_fs + s.off[ch];
    const uint8_t *pd = s.dist + (int64_t)f * s.dist_fs + s.off[ch];
    for (int i = t; i < HP_IH * HP_IW; i += 256) {
        const int j = i / HP_IW, c = i - j * HP_IW;
        in[0][j][c] = quad_sum<T>(pr, s, y0 + j - HP_PRE, x0 + c - HP_PRE);
        in[1][j][c] = quad_sum<T>(pd, s, y0 + j - HP_PRE, x0 + c - HP_PRE);
    }
    __syncthreads();
    // thread = (one row, eight adjacent columns)
    const int row = t >> 3, j0 = (t & 7) * 8;
    unsigned long long den = 0, num = 0;
    if (y0 + row < s.hd && x0 + j0 < s.wd) {
        int Hr[2][3][8], Hd[2][3][8];
        haar_coefficients(&in[0][row][j0], Hr);
        haar_coefficients(&in[1][row][j0], Hd);
#pragma unroll
        for (int o = 0; o < 8; o++) {
            if (x0 + j0 + o >= s.wd) continue;
#pragma unroll
            for (int ori = 0; ori < 2; ori++) {
                const double s1 = local_similarity<G>(Hr[ori][0][o], Hd[ori][0][o], s.c1);
                const double s2 = local_similarity<G>(Hr[ori][1][o], Hd[ori][1][o], s.c2);
                const double ls = (s1 + s2) * 0.5;
                const double e = exp(-HAARPSI_ALPHA * ls);
                unsigned long long u = (unsigned long long)__double2ll_rn(HAARPSI_FIX / (1.0 + e));   // in (2^29, 2^30)
                if (ls == 1.0) u = s.u1;
                const int ar = abs(Hr[ori][2][o]), ad = abs(Hd[ori][2][o]);
                const unsigned long long wi = (unsigned long long)(ar > ad ? ar : ad);               // below 2^23
                den += wi;
                num += u * wi;                                                                       // a term: below 2^53
            }
        }
    }
    // 16 terms: num < 2^57.  Split here; only the halves are added from now on
    const unsigned long long w0 = wave_sum(den), w1 = wave_sum(num & 0xffffffffull), w2 = wave_sum(num >> 32);
    if (lane_id() == 0) { red[wave_id()][0] = w0; red[wave_id()][1] = w1; red[wave_id()][2] = w2; }
    __syncthreads();
    if (t == 0) {
        const int pi = ch == 0 ? plane_index.x : ch == 1 ? plane_index.y : ch == 2 ? plane_index.z : plane_index.w;
        unsigned long long *a = acc + ((int64_t)f * n_planes + pi) * HAARPSI_WORDS;
        atomicAdd(a + 0, red[0][0] + red[1][0] + red[2][0] + red[3][0]);   // den: below 2^35 here
        atomicAdd(a + 1, red[0][1] + red[1][1] + red[2][1] + red[3][1]);   // num lo: below 2^40 here
        atomicAdd(a + 2, red[0][2] + red[1][2] + red[2][2] + red[3][2]);   //     hi: below 2^33 here
    }
}

} // namespace

double haarpsi_constant(int depth)
{
#pragma clang fp contract(off)
    const double k = (double)((1 << depth) - 1) / 255.0;
    return HAARPSI_C8 * (k * k);
}

unsigned long long haarpsi_u1()
{
#pragma clang fp contract(off)
    return (unsigned long long)std::llrint(HAARPSI_FIX / (1.0 + std::exp(-HAARPSI_ALPHA)));
}

void launch_haarpsi(hipStream_t st, const uint8_t *ref, const uint8_t *dist, int n, int64_t ref_frame_stride,
                    int64_t dist_frame_stride, const vqa_plane_desc *planes, const int *idx, int count, int n_planes, int depth,
                    unsigned long long *acc)
{
    if (n <= 0 || count <= 0) return;
    const vqa_plane_desc &pd = planes[idx[0]];
    haarpsi_src s;
    s.ref = ref; s.dist = dist; s.ref_fs = ref_frame_stride; s.dist_fs = dist_frame_stride;
    int p4[4];
    group_slots(planes, idx, count, s.off, p4);
    s.row_stride = pd.row_stride; s.step = pd.pixel_step;
    s.w = pd.width; s.h = pd.height;
    s.wd = (s.w + 1) / 2; s.hd = (s.h + 1) / 2;
    const double c0 = haarpsi_constant(depth);
    s.c1 = 64.0 * c0; s.c2 = 256.0 * c0;   // 4^(s+2): exact
    s.u1 = haarpsi_u1();
    const int tiles_x = (s.wd + HP_TW - 1) / HP_TW, tiles = tiles_x * ((s.hd + HP_TH - 1) / HP_TH);
    const int4 pi = make_int4(p4[0], p4[1], p4[2], p4[3]);
    const dim3 grid(tiles * count, n), block(256);
    if (depth > 8)
        hipLaunchKernelGGL((k_haarpsi<uint16_t>), grid, block, 0, st, s, tiles_x, tiles, n_planes, pi, acc);
    else
        hipLaunchKernelGGL((k_haarpsi<uint8_t>), grid, block, 0, st, s, tiles_x, tiles, n_planes, pi, acc);
}

static double logit(double x)
{
#pragma clang fp contract(off)
    return std::log(x / (1.0 - x));
}

// the three words -> the record on the host.  num = hi 2^32 + lo as a 128-bit integer; its quotient by den is below 2^30 and
// the remainder below den < 2^51, so both convert to double exactly and similarity takes two roundings.  Identical planes have
// num = U1 den: the remainder is 0, similarity is U1 / 2^30 and the two logits are the same number.  Contraction is off: the
// record is the formula vqa.h states.
void haarpsi_finalize(const unsigned long long *words, vqa_haarpsi_metrics *out)
{
#pragma clang fp contract(off)
    out->den = words[0];
    out->num_lo = words[1];
    out->num_hi = words[2];
    const double x1 = (double)haarpsi_u1() / HAARPSI_FIX;
    if (words[0] == 0) {   // both planes all zero
        out->similarity = x1;
        out->haarpsi = 1.0;
        return;
    }
    const unsigned __int128 num = ((unsigned __int128)words[2] << 32) + words[1];
    const uint64_t q = (uint64_t)(num / words[0]), r = (uint64_t)(num % words[0]);
    out->similarity = ((double)q + (double)r / (double)words[0]) / HAARPSI_FIX;
    const double l = logit(out->similarity) / logit(x1);
    out->haarpsi = l * l;
}

} // namespace vqa
