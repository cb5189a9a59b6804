// k_brisque.hip — BRISQUE's natural-scene statistics (Mittal, Moorthy and Bovik, IEEE TIP 2012) for gfx950, by the definition
// stated in include/vqa.h (vqa_brisque_submit): the 36 features of one plane from 60 integer words.
//
//   k_brisque_half<T>  scale 1: MATLAB's imresize(x, 0.5) - the eight taps [-3, -9, 29, 111, 111, 29, -9, -3] / 256 per axis,
//               indices mirrored - of the raw samples, as the EXACT integer over 65536 (|v| <= 304^2 * 65535 < 2^33, held in a
//               double, which holds every integer below 2^53).  One thread per output sample: eight row sums in 32 bits
//               (304 * 65535 < 2^25), their column sum in 64.
//   k_brisque_mscn<T>  once per scale (T = the plane's sample type at scale 0, double at scale 1).  A workgroup of 256 threads
//               walks BRISQUE_RUN consecutive 64 x 16 tiles.  A tile and its apron - 4 samples up, left and down, 3 right - go to
//               LDS as doubles; the 7-tap window runs over rows, then over columns, both moments in double (zero outside the
//               plane), for the tile and one sample up, left and down of it: mu, s, m = (x - mu) / (s + C) and ONCE
//               u = rint(m 2^16), an integer.  Everything after that is integer: |u| and u^2 of the tile's samples, and per
//               orientation (H, V, D1, D2) the pair's exact product u_a u_b, classed by its sign and rounded in magnitude to
//               2^-16, for every pair that lies inside the plane; a pair belongs to its sample (i, j).  The u of the plane's first
//               and last row and column go to four strips.
//   k_brisque_seam     the pairs that wrap around (circshift): column 0 against column W - 1, row 0 against row H - 1, and the
//               diagonal pairs of row 0, row H - 1 and column 0, corners included, from the strips.
//
// Sums: |u| <= 2.742 * 2^16 < 2^18, u^2 < 2^36, a rounded product below 2^19 and its square below 2^38; the squares of the
// products are summed as their low 32 bits and the rest apart (vqa.h states the ranges).  A thread's 30 partial sums are named
// registers (two 64-bit sums and four pair_acc; counts and the high parts in 32 bits, which a thread's share of at most 2^20
// pairs cannot fill), updated by selects: no local array, no scratch (0 bytes per lane in every kernel of this file).  The words
// leave through 64-bit integer atomics: integer addition is associative, so neither the tiling nor the order in which
// workgroups retire can change a bit.  u depends on the plane's samples and the tile grid alone, which starts at the plane's
// origin: a plane gives the same 60 words at any place of any batch, from any memory.
#include <cmath>
#include <mutex>
#include <type_traits>

#include "vqa_dev.hpp"
#include "vqa_kernels.hpp"

namespace vqa {

namespace {

constexpr int BRISQUE_RUN = 4;          // tiles per workgroup, consecutive in raster order
constexpr int SCALE_WORDS = BRISQUE_WORDS / 2;   // 30: sum |u|, sum u^2, 4 x (n_neg, n_pos, sum |p|, neg lo / hi, pos lo / hi)

// one group of same-geometry planes; every stride in bytes.  Scale 1 reads the doubles k_brisque_half wrote: fs, off and the
// strides then describe that scratch
struct brisque_src {
    const uint8_t *frames;  // frame 0 of the slice
    int64_t fs;             // frame stride
    int64_t off[4];         // plane offsets inside a frame
    int64_t row_stride;
    int step;
    int w, h;
};

struct brisque_taps { double g[7]; };   // g_k / sum g: the window is their outer product

__device__ __forceinline__ int mirror(int i, int n)   // aux = [0 .. n - 1, n - 1 .. 0], index mod 2 n
{
    int m = i % (2 * n);
    if (m < 0) m += 2 * n;
    return m < n ? m : 2 * n - 1 - m;
}

// grid = (ceil(w1 h1 / 256), count, n); out: [frame][plane of the group][h1][w1] doubles
template <typename T>
__global__ __launch_bounds__(256) void k_brisque_half(brisque_src s, int w1, int h1, int count, double *__restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= w1 * h1) return;
    const int oy = i / w1, ox = i - oy * w1;
    const int ch = blockIdx.y, f = blockIdx.z;
    const uint8_t *pc = s.frames + (int64_t)f * s.fs + s.off[ch];
    const int tap[8] = {-3, -9, 29, 111, 111, 29, -9, -3};
    int xi[8];
#pragma unroll
    for (int k = 0; k < 8; k++) xi[k] = mirror(2 * ox - 3 + k, s.w);
    long long v = 0;
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const uint8_t *row = pc + (int64_t)mirror(2 * oy - 3 + r, s.h) * s.row_stride;
        int hs = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) hs += tap[k] * (int)*(const T *)(row + (int64_t)xi[k] * s.step);
        v += (long long)tap[r] * hs;
    }
    out[((int64_t)f * count + ch) * ((int64_t)w1 * h1) + i] = (double)v;
}

// the seven partial sums of one orientation, in registers: named members, never indexed
struct pair_acc {
    unsigned n_neg = 0, n_pos = 0;                        // (a thread sees fewer than 2^32 pairs)
    unsigned long long abs_p = 0, neg_lo = 0, pos_lo = 0; // sums of values below 2^32
    unsigned neg_hi = 0, pos_hi = 0;                      // sums of values below 2^6
};

// one pair: the exact product's sign classes it, its magnitude is rounded to 2^-16 (half up); a zero product adds nothing.
// `on` = the pair exists.  Branch-free: every term is selected, nothing is addressed
__device__ __forceinline__ void pair_add(pair_acc &A, bool on, int ua, int ub)
{
    const long long e = on ? (long long)ua * (long long)ub : 0ll;
    const bool neg = e < 0, pos = e > 0;
    const unsigned long long mag = ((unsigned long long)(neg ? -e : e) + (1ull << (BRISQUE_Q - 1))) >> BRISQUE_Q;
    const unsigned long long sq = mag * mag;
    const unsigned lo = (unsigned)sq, hi = (unsigned)(sq >> 32);
    A.abs_p += (neg || pos) ? mag : 0ull;
    A.n_neg += neg ? 1u : 0u;
    A.n_pos += pos ? 1u : 0u;
    A.neg_lo += neg ? lo : 0u;
    A.neg_hi += neg ? hi : 0u;
    A.pos_lo += pos ? lo : 0u;
    A.pos_hi += pos ? hi : 0u;
}

// one word of one workgroup -> tot (LDS)
__device__ __forceinline__ void leave_word(unsigned long long *tot, int k, unsigned long long v)
{
    const unsigned long long u = wave_sum(v);
    if (lane_id() == 0 && u) atomicAdd(&tot[k], u);
}

// the seven words of one orientation, in the order of the record: n_neg, n_pos, sum |p|, neg lo, neg hi, pos lo, pos hi
__device__ __forceinline__ void leave_pairs(unsigned long long *tot, int k, const pair_acc &A)
{
    leave_word(tot, k, A.n_neg); leave_word(tot, k + 1, A.n_pos); leave_word(tot, k + 2, A.abs_p);
    leave_word(tot, k + 3, A.neg_lo); leave_word(tot, k + 4, A.neg_hi);
    leave_word(tot, k + 5, A.pos_lo); leave_word(tot, k + 6, A.pos_hi);
}

// tot (LDS, COUNT words) -> acc, from word FIRST of the scale on
template <int FIRST, int COUNT>
__device__ __forceinline__ void leave_all(const unsigned long long *tot, unsigned long long *dst)
{
    __syncthreads();
    if (threadIdx.x < COUNT && tot[threadIdx.x]) atomicAdd(dst + FIRST + threadIdx.x, tot[threadIdx.x]);
}

// grid = (runs * count, n); block = 256.  acc: [frame][plane of the submit][BRISQUE_WORDS], zeroed by the submit; strips:
// [frame][plane of the group][row 0 (w), row h - 1 (w), column 0 (h), column w - 1 (h)] ints
template <typename T>
__global__ __launch_bounds__(256) void k_brisque_mscn(brisque_src s, brisque_taps tp, double unit, double c_add, int tiles_x,
                                                      int tiles, int runs, int count, int n_planes, int4 plane_index, int scale,
                                                      unsigned long long *__restrict__ acc, int *__restrict__ strips)
{
    constexpr int TW = 64, TH = 16, XW = TW + 7, XH = TH + 8, MW = TW + 1, MH = TH + 2;
    __shared__ double xs[XH][XW + 1];      // samples: row j = plane row y0 - 4 + j, column i = plane column x0 - 4 + i
    __shared__ double hx[XH][MW], hxx[XH][MW];   // the row pass: column q = plane column x0 - 1 + q
    __shared__ int us[MH][MW];             // u: row r = plane row y0 - 1 + r, column q = plane column x0 - 1 + q
    __shared__ unsigned long long tot[SCALE_WORDS];
    const int f = blockIdx.y;
    const int ch = blockIdx.x / runs, run = blockIdx.x % runs;
    const int t = threadIdx.x;
    if (t < SCALE_WORDS) tot[t] = 0;       // (the barriers of the first tile order this before the adds)
    const uint8_t *pc = s.frames + (int64_t)f * s.fs + s.off[ch];
    int *strip = strips + ((int64_t)f * count + ch) * (2 * (int64_t)(s.w + s.h));
    int *row0 = strip, *rowl = strip + s.w, *col0 = strip + 2 * s.w, *coll = strip + 2 * s.w + s.h;
    unsigned long long sum_abs = 0, sum_sq = 0;
    pair_acc ah, av, ad1, ad2;
    const int tile_end = min(tiles, (run + 1) * BRISQUE_RUN);
    for (int tile = run * BRISQUE_RUN; tile < tile_end; tile++) {
        const int y0 = (tile / tiles_x) * TH, x0 = (tile % tiles_x) * TW;
        __syncthreads();   // (the tile before has been read)
        for (int i = t; i < XH * XW; i += 256) {
            const int j = i / XW, q = i - j * XW;
            const int y = y0 - 4 + j, x = x0 - 4 + q;
            double v = 0.0;                                    // zero outside the plane
            if (y >= 0 && y < s.h && x >= 0 && x < s.w)
                v = (double)*(const T *)(pc + (int64_t)y * s.row_stride + (int64_t)x * s.step) * unit;
            xs[j][q] = v;
        }
        __syncthreads();
        for (int i = t; i < XH * MW; i += 256) {
            const int j = i / MW, q = i - j * MW;
            double m1 = 0.0, m2 = 0.0;
#pragma unroll
            for (int k = 0; k < 7; k++) {
                const double v = xs[j][q + k];
                m1 += tp.g[k] * v;
                m2 += tp.g[k] * (v * v);
            }
            hx[j][q] = m1;
            hxx[j][q] = m2;
        }
        __syncthreads();
        for (int i = t; i < MH * MW; i += 256) {
            const int r = i / MW, q = i - r * MW;
            const int y = y0 - 1 + r, x = x0 - 1 + q;
            int u = 0;
            if (y >= 0 && y < s.h && x >= 0 && x < s.w) {
                double mu = 0.0, m2 = 0.0;
#pragma unroll
                for (int k = 0; k < 7; k++) {
                    mu += tp.g[k] * hx[r + k][q];
                    m2 += tp.g[k] * hxx[r + k][q];
                }
                const double sd = sqrt(fabs(m2 - mu * mu));
                u = (int)rint((xs[r + 3][q + 3] - mu) / (sd + c_add) * (double)(1 << BRISQUE_Q));
            }
            us[r][q] = u;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < TW * TH / 256; k++) {
            const int i = t + 256 * k;
            const int r = i / TW, q = i - r * TW;
            const int y = y0 + r, x = x0 + q;
            const bool in = y < s.h && x < s.w;
            const int u = in ? us[r + 1][q + 1] : 0;                            // (outside the plane: adds nothing)
            sum_abs += (unsigned long long)abs(u);
            sum_sq += (unsigned long long)((long long)u * u);
            pair_add(ah, in && x >= 1, u, us[r + 1][q]);                        // H:  m(i, j) m(i, j - 1)
            pair_add(av, in && y >= 1, u, us[r][q + 1]);                        // V:  m(i, j) m(i - 1, j)
            pair_add(ad1, in && x >= 1 && y >= 1, u, us[r][q]);                 // D1: m(i, j) m(i - 1, j - 1)
            pair_add(ad2, in && x >= 1 && y + 1 < s.h, u, us[r + 2][q]);        // D2: m(i, j) m(i + 1, j - 1)
            if (!in) continue;
            if (y == 0) row0[x] = u;
            if (y == s.h - 1) rowl[x] = u;
            if (x == 0) col0[y] = u;
            if (x == s.w - 1) coll[y] = u;
        }
    }
    const int pi = ch == 0 ? plane_index.x : ch == 1 ? plane_index.y : ch == 2 ? plane_index.z : plane_index.w;
    leave_word(tot, 0, sum_abs); leave_word(tot, 1, sum_sq);
    leave_pairs(tot, 2, ah); leave_pairs(tot, 9, av); leave_pairs(tot, 16, ad1); leave_pairs(tot, 23, ad2);
    leave_all<0, SCALE_WORDS>(tot, acc + ((int64_t)f * n_planes + pi) * BRISQUE_WORDS + scale * SCALE_WORDS);
}

// grid = (count, n); block = 256: the pairs of one plane that wrap around
__global__ __launch_bounds__(256) void k_brisque_seam(int w, int h, int count, int n_planes, int4 plane_index, int scale,
                                                      const int *__restrict__ strips, unsigned long long *__restrict__ acc)
{
    __shared__ unsigned long long tot[SCALE_WORDS - 2];
    const int ch = blockIdx.x, f = blockIdx.y, t = threadIdx.x;
    if (t < SCALE_WORDS - 2) tot[t] = 0;
    __syncthreads();
    const int *strip = strips + ((int64_t)f * count + ch) * (2 * (int64_t)(w + h));
    const int *row0 = strip, *rowl = strip + w, *col0 = strip + 2 * w, *coll = strip + 2 * w + h;
    pair_acc ah, av, ad1, ad2;
    for (int i = t; i < h; i += 256) {
        const int c = col0[i];
        pair_add(ah, true, c, coll[i]);                                     // H:  (i, 0) with (i, W - 1)
        pair_add(ad1, i >= 1, c, coll[i >= 1 ? i - 1 : i]);                 // D1: (i, 0) with (i - 1, W - 1)
        pair_add(ad2, i + 1 < h, c, coll[i + 1 < h ? i + 1 : i]);           // D2: (i, 0) with (i + 1, W - 1)
    }
    for (int j = t; j < w; j += 256) {
        const int jl = j == 0 ? w - 1 : j - 1;
        pair_add(av, true, row0[j], rowl[j]);                               // V:  (0, j) with (H - 1, j)
        pair_add(ad1, true, row0[j], rowl[jl]);                             // D1: (0, j) with (H - 1, j - 1)
        pair_add(ad2, true, rowl[j], row0[jl]);                             // D2: (H - 1, j) with (0, j - 1)
    }
    const int pi = ch == 0 ? plane_index.x : ch == 1 ? plane_index.y : ch == 2 ? plane_index.z : plane_index.w;
    leave_pairs(tot, 0, ah); leave_pairs(tot, 7, av); leave_pairs(tot, 14, ad1); leave_pairs(tot, 21, ad2);
    leave_all<2, SCALE_WORDS - 2>(tot, acc + ((int64_t)f * n_planes + pi) * BRISQUE_WORDS + scale * SCALE_WORDS);
}

template <typename T>
void launch_mscn(hipStream_t st, const brisque_src &s, double unit, double c_add, int n, int count, int n_planes, int4 pi,
                 int scale, unsigned long long *acc, int *strips, brisque_mark mark, void *mark_arg)
{
    brisque_taps tp;
    double sum = 0.0;
    for (int k = 0; k < 7; k++) { tp.g[k] = std::exp(-(double)((k - 3) * (k - 3)) / (2.0 * (7.0 / 6.0) * (7.0 / 6.0))); sum += tp.g[k]; }
    for (int k = 0; k < 7; k++) tp.g[k] /= sum;
    const int tiles_x = (s.w + 63) / 64, tiles = tiles_x * ((s.h + 15) / 16);
    const int runs = (tiles + BRISQUE_RUN - 1) / BRISQUE_RUN;
    mark(mark_arg, VQA_K_BRISQUE_MSCN, 1);
    hipLaunchKernelGGL((k_brisque_mscn<T>), dim3(runs * count, n), dim3(256), 0, st, s, tp, unit, c_add, tiles_x, tiles, runs,
                       count, n_planes, pi, scale, acc, strips);
    mark(mark_arg, VQA_K_BRISQUE_MSCN, 0);
    mark(mark_arg, VQA_K_BRISQUE_SEAM, 1);
    hipLaunchKernelGGL(k_brisque_seam, dim3(count, n), dim3(256), 0, st, s.w, s.h, count, n_planes, pi, scale, strips, acc);
    mark(mark_arg, VQA_K_BRISQUE_SEAM, 0);
}

} // namespace

size_t brisque_scratch_bytes(int count, int h, int w)
{
    const size_t h1 = (size_t)(h + 1) / 2, w1 = (size_t)(w + 1) / 2;
    return (size_t)count * (sizeof(double) * h1 * w1 + sizeof(int) * 2 * (size_t)(w + h));
}

void launch_brisque(hipStream_t st, const uint8_t *frames, int n, int64_t frame_stride, const vqa_plane_desc *planes,
                    const int *idx, int count, int n_planes, int depth, void *scratch, unsigned long long *acc,
                    brisque_mark mark, void *mark_arg)
{
    if (n <= 0 || count <= 0) return;
    const vqa_plane_desc &pd = planes[idx[0]];
    brisque_src s;
    s.frames = frames; s.fs = frame_stride;
    int p4[4];
    group_slots(planes, idx, count, s.off, p4);
    s.row_stride = pd.row_stride; s.step = pd.pixel_step;
    s.w = pd.width; s.h = pd.height;
    const int4 pi = make_int4(p4[0], p4[1], p4[2], p4[3]);
    const int h1 = (s.h + 1) / 2, w1 = (s.w + 1) / 2;
    double *half = (double *)scratch;                                   // [n][count][h1][w1]
    int *strips = (int *)(half + (size_t)n * count * h1 * w1);          // [n][count][2 (w + h)], both scales in turn
    const double c_add = (double)((1 << depth) - 1) / 255.0;
    mark(mark_arg, VQA_K_BRISQUE_HALF, 1);
    const dim3 hgrid((w1 * h1 + 255) / 256, count, n);
    if (depth > 8) hipLaunchKernelGGL((k_brisque_half<uint16_t>), hgrid, dim3(256), 0, st, s, w1, h1, count, half);
    else hipLaunchKernelGGL((k_brisque_half<uint8_t>), hgrid, dim3(256), 0, st, s, w1, h1, count, half);
    mark(mark_arg, VQA_K_BRISQUE_HALF, 0);
    if (depth > 8) launch_mscn<uint16_t>(st, s, 1.0, c_add, n, count, n_planes, pi, 0, acc, strips, mark, mark_arg);
    else launch_mscn<uint8_t>(st, s, 1.0, c_add, n, count, n_planes, pi, 0, acc, strips, mark, mark_arg);
    brisque_src s1;
    s1.frames = (const uint8_t *)half;
    s1.fs = (int64_t)sizeof(double) * count * h1 * w1;
    for (int k = 0; k < 4; k++) s1.off[k] = (int64_t)sizeof(double) * (k < count ? k : 0) * h1 * w1;
    s1.row_stride = (int64_t)sizeof(double) * w1; s1.step = (int)sizeof(double);
    s1.w = w1; s1.h = h1;
    launch_mscn<double>(st, s1, 1.0 / 65536.0, c_add, n, count, n_planes, pi, 1, acc, strips, mark, mark_arg);
}

// ---- the host's part: the fits of include/vqa.h in double, contraction off ----
namespace {

constexpr int GRID_N = 9801;            // gam = 0.200, 0.201 .. 10.000
struct fit_tables { double r[GRID_N], inv[GRID_N]; };

static const fit_tables &tables()
{
#pragma clang fp contract(off)
    static fit_tables T;
    static std::once_flag once;
    std::call_once(once, [] {
#pragma clang fp contract(off)
        for (int k = 0; k < GRID_N; k++) {
            const double g = (double)(200 + k) / 1000.0;
            const double l1 = std::lgamma(1.0 / g), l2 = std::lgamma(2.0 / g), l3 = std::lgamma(3.0 / g);
            T.r[k] = std::exp(l1 + l3 - 2.0 * l2);      // G(1/g) G(3/g) / G(2/g)^2
            T.inv[k] = std::exp(2.0 * l2 - l1 - l3);    // G(2/g)^2 / (G(1/g) G(3/g))
        }
    });
    return T;
}

// argmin_k of |x - tab[k]| (squared: of (tab[k] - x)^2, as the AGGD fit states it), the first on a tie.  Both tables are
// strictly monotone (`rising`: tab[k] < tab[k + 1]), so the minimum lies at one of the two entries that bracket x: a binary
// search and one comparison give what a scan of all 9801 entries gives
static int nearest(const double *tab, double x, bool rising, bool squared)
{
#pragma clang fp contract(off)
    int lo = 0, hi = GRID_N;                 // the first k whose entry lies on or past x
    while (lo < hi) {
        const int mid = (lo + hi) / 2;
        if (rising ? tab[mid] < x : tab[mid] > x) lo = mid + 1;
        else hi = mid;
    }
    if (lo == 0) return 0;
    if (lo == GRID_N) return GRID_N - 1;
    double a = std::fabs(x - tab[lo - 1]), b = std::fabs(x - tab[lo]);
    if (squared) { a = (tab[lo - 1] - x) * (tab[lo - 1] - x); b = (tab[lo] - x) * (tab[lo] - x); }
    return b < a ? lo : lo - 1;
}

static double to_double(uint64_t lo, uint64_t hi)   // hi 2^32 + lo as an exact integer, rounded once
{
    return (double)(((unsigned __int128)hi << 32) + lo);
}

} // namespace

void brisque_finalize(const unsigned long long *words, int h, int w, vqa_brisque_metrics *out)
{
#pragma clang fp contract(off)
    const fit_tables &T = tables();
    const double q1 = (double)(1 << BRISQUE_Q), q2 = q1 * q1;
    out->flags = 0;
    out->reserved = 0;
    for (int sc = 0; sc < 2; sc++) {
        const unsigned long long *x = words + sc * SCALE_WORDS;
        double *ft = out->features + 18 * sc;
        for (int k = 0; k < 18; k++) ft[k] = 0.0;
        const double cnt = sc == 0 ? (double)((int64_t)h * w) : (double)((int64_t)((h + 1) / 2) * ((w + 1) / 2));
        out->sum_abs_u[sc] = x[0];
        out->sum_u2[sc] = x[1];
        if (x[0] == 0) {
            out->flags |= 1u << (5 * sc);
        } else {
            const double sigma2 = (double)x[1] / q2 / cnt, e = (double)x[0] / q1 / cnt;
            const double rho = sigma2 / (e * e);
            const int best = nearest(T.r, rho, false, false);
            ft[0] = (double)(200 + best) / 1000.0;
            ft[1] = sigma2;
        }
        for (int o = 0; o < 4; o++) {
            const unsigned long long *p = x + 2 + 7 * o;
            out->n_neg[sc][o] = p[0]; out->n_pos[sc][o] = p[1]; out->sum_abs_p[sc][o] = p[2];
            out->sq_neg_lo[sc][o] = p[3]; out->sq_neg_hi[sc][o] = p[4];
            out->sq_pos_lo[sc][o] = p[5]; out->sq_pos_hi[sc][o] = p[6];
            const double sn = to_double(p[3], p[4]), sp = to_double(p[5], p[6]);
            if (p[0] == 0 || p[1] == 0 || sp == 0.0) {
                out->flags |= 1u << (5 * sc + 1 + o);
                continue;
            }
            const double l = std::sqrt(sn / q2 / (double)p[0]), r = std::sqrt(sp / q2 / (double)p[1]);
            const double gh = l / r;
            const double ea = (double)p[2] / q1 / cnt, e2 = to_double(p[3] + p[5], p[4] + p[6]) / q2 / cnt;
            const double rhat = ea * ea / e2;
            const double g2 = gh * gh;
            const double rn = rhat * (g2 * gh + 1.0) * (gh + 1.0) / ((g2 + 1.0) * (g2 + 1.0));
            const int best = nearest(T.inv, rn, true, true);
            const double al = (double)(200 + best) / 1000.0;
            const double l1 = std::lgamma(1.0 / al), l2 = std::lgamma(2.0 / al), l3 = std::lgamma(3.0 / al);
            ft[2 + 4 * o] = al;
            ft[3 + 4 * o] = (r - l) * std::exp(l2 - l1) * std::exp(0.5 * (l1 - l3));
            ft[4 + 4 * o] = l * l;
            ft[5 + 4 * o] = r * r;
        }
    }
}

} // namespace vqa
