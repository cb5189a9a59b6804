// k_fsim.hip — FSIM / FSIMc (Zhang, Zhang, Mou, Zhang 2011) for gfx950: phase congruency of the luminance through a bank of
// 16 log-Gabor filters applied in the frequency domain, Scharr gradients, the chromaticity of I and Q, pooled by the larger
// phase congruency - by the definition stated in include/vqa.h (vqa_fsim_submit).  Per sub-slice of frames:
//
//   k_fsim_luma<T>   k_mdsi_map's box stage without the apron: a workgroup of 256 threads owns a 64 x 32 tile of the DOWNSAMPLED
//                    grid (hd x wd) of ONE image, adds every sample of the tile's input rectangle as an integer into the LDS cell
//                    of its f x f window, and writes Y, I, Q (the 3 x 4 matrix on the sums) as doubles: yiq [image][3][N].
//   k_fsim_dft<NT>   a dense complex matrix product C = A B on v_mfma_f64_16x16x4_f64, the transform of every grid size.  A wave
//                    owns 16 rows x 16 NT columns of C; it walks k in steps of 4 IN ORDER, a lane loads A[i0 + (lane & 15)][k +
//                    (lane >> 4)] and NT times B[k + (lane >> 4)][j + (lane & 15)], each complex product is four real MFMAs in the
//                    fixed order (Ar Br, -Ai Bi) -> Re, (Ar Bi, Ai Br) -> Im.  Rows, columns and k past the edge are loaded as
//                    zeros (the address is not formed).  Four uses: T = (Y - Y(0,0)) W_w; F = W_h T; per orientation and scale
//                    U = conj(W_h) (F filt); EO = U conj(W_w) / N.  No LDS: a first version, bound by its loads.
//   k_fsim_energy    per sample, the four scales of one orientation: Energy_o, An_o, |EO_0|^2.
//   k_fsim_median    one workgroup per (image, orientation): the exact median of |EO_0|^2 by a radix-256 selection on the 64-bit
//                    patterns of the non-negative doubles (eight passes a rank, LDS histogram), then T_o = c_o sqrt(med_o).
//   k_fsim_pc        per sample: PC and p = rint(PC 2^24) into the map [frame][2][N] uint32.
//   k_fsim_pool      per sample of a frame: Scharr of Y of both images, S_G, S_PC, C, g, gc, pm and the three integer words.
//
// Everything is DOUBLE with contraction off.  An output of k_fsim_dft is a fixed-order sum over k of the same doubles whatever
// the batch, so the maps do not depend on it; all that is added across threads is integers.
#include <cmath>
#include <vector>

#include "vqa_dev.hpp"
#include "vqa_kernels.hpp"

// every double below is rounded once per written operation (the Makefile builds with -ffp-contract=fast)
#pragma clang fp contract(off)

namespace vqa {

namespace {

constexpr int TW = 64, TH = 32;
constexpr double FIX = FSIM_FIX;
constexpr double T1 = 0.85, T2 = 160.0, T3 = 200.0, LAMBDA = 0.03;

typedef double d4 __attribute__((ext_vector_type(4)));

// both images of n frames; every stride in bytes (k_mdsi's)
struct fsim_src {
    const uint8_t *ref, *dist;
    int64_t ref_fs, dist_fs;   // frame strides
    int64_t off[3];            // plane offsets inside a frame
    int64_t rs0, rs1;          // row strides of plane 0 and of planes 1, 2
    int step0, step1;          // pixel steps likewise
    int w, h;                  // plane 0
    int sh, sv;                // 1: planes 1, 2 are halved in width / height
    int np;                    // 1 or 3
    int f, o;                  // the factor; the first row of window 0: floor(f / 2) - (f - 1)
    int wd, hd;                // the downsampled grid
    double mat[3][4];          // [Y, I, Q][plane 0, 1, 2, count]
};

__device__ __forceinline__ double channel(const double (&m)[4], int s0, int s1, int s2, int cnt)
{
    return ((m[0] * (double)s0 + m[1] * (double)s1) + m[2] * (double)s2) + m[3] * (double)cnt;
}

// the in-plane positions of window k along an axis of length len
__device__ __forceinline__ int window_count(int k, int f, int o, int len)
{
    const int a = k * f + o, lo = a > 0 ? a : 0, hi = a + f - 1 < len - 1 ? a + f - 1 : len - 1;
    return hi - lo + 1;
}

// grid = (tiles, 2 n_frames); block = 256.  image = 2 frame + (0: ref, 1: dist).  yiq: [image][3][hd wd]
template <typename T>
__global__ __launch_bounds__(256) void k_fsim_luma(fsim_src s, int tiles_x, double *__restrict__ yiq)
{
    __shared__ int bs[3][TH][TW];
    const int img = blockIdx.y, tile = blockIdx.x, t = threadIdx.x, f = s.f;
    const int y0 = (tile / tiles_x) * TH, x0 = (tile % tiles_x) * TW;
    const uint8_t *p = (img & 1) ? s.dist + (int64_t)(img >> 1) * s.dist_fs : s.ref + (int64_t)(img >> 1) * s.ref_fs;
    for (int i = t; i < 3 * TH * TW; i += 256) (&bs[0][0][0])[i] = 0;
    __syncthreads();
    // the input rectangle of the tile, clipped to the plane
    const int ry0 = y0 * f + s.o, rx0 = x0 * f + s.o;
    const int ya = ry0 > 0 ? ry0 : 0, yb = ry0 + TH * f < s.h ? ry0 + TH * f : s.h;
    const int xa = rx0 > 0 ? rx0 : 0, xb = rx0 + TW * f < s.w ? rx0 + TW * f : s.w;
    const int cols = xb - xa, total = cols > 0 && yb > ya ? cols * (yb - ya) : 0;   // at most 4096 * 2048
    const uint8_t *p0 = p + s.off[0], *p1 = p + s.off[1], *p2 = p + s.off[2];
    for (int i = t; i < total; i += 256) {
        const int ry = i / cols, y = ya + ry, x = xa + (i - ry * cols);
        const int di = (y - ry0) / f, dj = (x - rx0) / f;   // 0 <= di < TH, 0 <= dj < TW by the clip
        atomicAdd(&bs[0][di][dj], (int)*(const T *)(p0 + (int64_t)y * s.rs0 + (int64_t)x * s.step0));
        if (s.np == 3) {
            const int64_t oc = (int64_t)(y >> s.sv) * s.rs1 + (int64_t)(x >> s.sh) * s.step1;
            atomicAdd(&bs[1][di][dj], (int)*(const T *)(p1 + oc));
            atomicAdd(&bs[2][di][dj], (int)*(const T *)(p2 + oc));
        }
    }
    __syncthreads();
    const int64_t N = (int64_t)s.hd * s.wd;
    double *out = yiq + (int64_t)img * 3 * N;
    for (int i = t; i < TH * TW; i += 256) {
        const int j = i / TW, c = i - j * TW;
        const int di = y0 + j, dj = x0 + c;
        if (di >= s.hd || dj >= s.wd) continue;
        const int cnt = window_count(di, f, s.o, s.h) * window_count(dj, f, s.o, s.w);
        const int64_t at = (int64_t)di * s.wd + dj;
        out[at] = channel(s.mat[0], bs[0][j][c], bs[1][j][c], bs[2][j][c], cnt);
        out[N + at] = channel(s.mat[1], bs[0][j][c], bs[1][j][c], bs[2][j][c], cnt);
        out[2 * N + at] = channel(s.mat[2], bs[0][j][c], bs[1][j][c], bs[2][j][c], cnt);
    }
}

// C[z] = A[z / a_zdiv] B[z / b_zdiv], complex, M x K times K x Nc.  A complex array is two planes of doubles, the imaginary one
// *_im doubles after the real one (a_im = 0: A is real).  Offsets and strides in doubles.
struct fsim_gemm {
    const double *a; int64_t a_bs, a_rs, a_cs, a_im; int a_zdiv; double a_sign;   // A[i][k] = a[i a_rs + k a_cs]; a_sign on Im
    const double *b; int64_t b_bs, b_rs, b_im; int b_zdiv; double b_sign;         // B[k][j] = b[k b_rs + j]
    const double *filt; int64_t f_bs; int f_mod;   // B[k][j] *= filt[(z % f_mod) f_bs + k b_rs + j] (real); null: none
    const double *centre; int64_t centre_bs;       // A[i][k] -= centre[z centre_bs] (real A only); null: none
    double *c; int64_t c_bs, c_rs, c_im;
    double div;                                    // C /= div
    int M, Nc, K;
};

// grid = (ceil(Nc / (64 NT)), ceil(M / 16), batch); block = 256: wave v of a workgroup owns columns (4 blockIdx.x + v) 16 NT ..
template <int NT>
__global__ __launch_bounds__(256) void k_fsim_dft(fsim_gemm g)
{
    const int z = blockIdx.z, lane = (int)lane_id();
    const int i0 = blockIdx.y * 16, j0 = ((int)blockIdx.x * 4 + (int)wave_id()) * 16 * NT;
    if (j0 >= g.Nc) return;   // (the whole wave; the kernel has no barrier)
    const int li = lane & 15, lk = lane >> 4;
    const bool a_ok = i0 + li < g.M;
    const double *ap = g.a + (int64_t)(z / g.a_zdiv) * g.a_bs + (int64_t)(a_ok ? i0 + li : 0) * g.a_rs;
    const double *bp = g.b + (int64_t)(z / g.b_zdiv) * g.b_bs;
    const double *fp = g.filt ? g.filt + (int64_t)(z % g.f_mod) * g.f_bs : nullptr;
    const double cen = g.centre ? g.centre[(int64_t)z * g.centre_bs] : 0.0;
    const bool a_cplx = g.a_im != 0;
    d4 cr[NT], ci[NT];
#pragma unroll
    for (int t = 0; t < NT; t++) cr[t] = ci[t] = d4{0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < g.K; k0 += 4) {
        const int k = k0 + lk;
        const bool k_ok = k < g.K;
        double ar = 0.0, ai = 0.0;
        if (a_ok && k_ok) {
            ar = ap[(int64_t)k * g.a_cs] - cen;
            if (a_cplx) ai = g.a_sign * ap[g.a_im + (int64_t)k * g.a_cs];
        }
        const double nai = -ai;
#pragma unroll
        for (int t = 0; t < NT; t++) {
            const int j = j0 + 16 * t + li;
            double br = 0.0, bi = 0.0;
            if (k_ok && j < g.Nc) {
                const int64_t at = (int64_t)k * g.b_rs + j;
                br = bp[at];
                bi = g.b_sign * bp[g.b_im + at];
                if (fp) {
                    const double fv = fp[at];
                    br = br * fv;
                    bi = bi * fv;
                }
            }
            cr[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, br, cr[t], 0, 0, 0);
            ci[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, bi, ci[t], 0, 0, 0);
            if (a_cplx) {
                cr[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(nai, bi, cr[t], 0, 0, 0);
                ci[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, br, ci[t], 0, 0, 0);
            }
        }
    }
    // C/D of the f64 form: col = lane & 15, row = (lane >> 4) + 4 reg
    double *cp = g.c + (int64_t)z * g.c_bs;
#pragma unroll
    for (int t = 0; t < NT; t++) {
        const int col = j0 + 16 * t + li;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int row = i0 + lk + 4 * r;
            if (row < g.M && col < g.Nc) {
                const int64_t at = (int64_t)row * g.c_rs + col;
                cp[at] = cr[t][r] / g.div;
                cp[g.c_im + at] = ci[t][r] / g.div;
            }
        }
    }
}

// grid = (ceil(N / 256), images); block = 256.  eo: [image][4 scales][2][N]; en: [image][4 orientations][3][N] (Energy, An, |EO_0|^2)
__global__ __launch_bounds__(256) void k_fsim_energy(const double *__restrict__ eo, int64_t N, int orient, double *__restrict__ en)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int img = blockIdx.y;
    const double *e = eo + (int64_t)img * 8 * N + i;
    double re[4], im[4];
#pragma unroll
    for (int s = 0; s < 4; s++) { re[s] = e[(int64_t)(2 * s) * N]; im[s] = e[(int64_t)(2 * s + 1) * N]; }
    double an = 0.0, se = 0.0, so = 0.0;
#pragma unroll
    for (int s = 0; s < 4; s++) {
        an = an + sqrt(re[s] * re[s] + im[s] * im[s]);
        se = se + re[s];
        so = so + im[s];
    }
    const double xe = sqrt(se * se + so * so) + 1e-4, me = se / xe, mo = so / xe;
    double en_o = 0.0;
#pragma unroll
    for (int s = 0; s < 4; s++) en_o = en_o + ((re[s] * me + im[s] * mo) - fabs(re[s] * mo - im[s] * me));
    double *o = en + ((int64_t)img * 4 + orient) * 3 * N + i;
    o[0] = en_o;
    o[N] = an;
    o[2 * N] = re[0] * re[0] + im[0] * im[0];
}

struct fsim_noise { double c[4]; };

// grid = (4, images); block = 1024.  thr: [image][4]
__global__ __launch_bounds__(1024) void k_fsim_median(const double *__restrict__ en, int64_t N, fsim_noise nf, double *__restrict__ thr)
{
    __shared__ unsigned hist[256];
    __shared__ unsigned long long sh_prefix;
    __shared__ unsigned sh_rank;
    const int orient = blockIdx.x, img = blockIdx.y, t = threadIdx.x;
    const unsigned long long *v = (const unsigned long long *)(en + (((int64_t)img * 4 + orient) * 3 + 2) * N);
    const int n_ranks = (N & 1) ? 1 : 2;
    double pick[2] = {0.0, 0.0};
    for (int r = 0; r < n_ranks; r++) {
        if (t == 0) {
            sh_prefix = 0ull;
            sh_rank = (unsigned)((N & 1) ? (N - 1) / 2 : N / 2 - 1 + r);   // 0-based, in ascending order
        }
        for (int shift = 56; shift >= 0; shift -= 8) {
            if (t < 256) hist[t] = 0u;
            __syncthreads();
            const unsigned long long prefix = sh_prefix, mask = shift == 56 ? 0ull : ~0ull << (shift + 8);
            for (int64_t i = t; i < N; i += 1024) {
                const unsigned long long u = v[i];
                if ((u & mask) == prefix) atomicAdd(&hist[(unsigned)(u >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (t == 0) {
                unsigned below = 0u, rank = sh_rank;
                int b = 0;
                for (; b < 255; b++) {
                    if (rank < below + hist[b]) break;
                    below += hist[b];
                }
                sh_prefix = prefix | ((unsigned long long)b << shift);
                sh_rank = rank - below;
            }
            __syncthreads();
        }
        pick[r] = __longlong_as_double((long long)sh_prefix);
        __syncthreads();
    }
    if (t == 0) {
        const double med = (N & 1) ? pick[0] : 0.5 * (pick[0] + pick[1]);
        thr[img * 4 + orient] = nf.c[orient] * sqrt(med);
    }
}

// grid = (ceil(N / 256), images); block = 256.  p: [image][N]
__global__ __launch_bounds__(256) void k_fsim_pc(const double *__restrict__ en, const double *__restrict__ thr, int64_t N,
                                                 uint32_t *__restrict__ p)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int img = blockIdx.y;
    const double *e = en + (int64_t)img * 12 * N + i;
    double num = 0.0, den = 0.0;
#pragma unroll
    for (int o = 0; o < 4; o++) {
        num = num + fmax(e[(int64_t)(3 * o) * N] - thr[img * 4 + o], 0.0);
        den = den + e[(int64_t)(3 * o + 1) * N];
    }
    const double pc = den > 0.0 ? num / den : 0.0;
    p[(int64_t)img * N + i] = (uint32_t)__double2ll_rn(pc * FIX);
}

// Y at (y, x) of the grid, 0 outside (conv2 'same')
__device__ __forceinline__ double y_at(const double *y, int hd, int wd, int r, int c)
{
    return (r >= 0 && r < hd && c >= 0 && c < wd) ? y[(int64_t)r * wd + c] : 0.0;
}

// q = gx^2 + gy^2 of the Scharr pair at (r, c) (include/vqa.h states the order)
__device__ __forceinline__ double scharr_q(const double *y, int hd, int wd, int r, int c)
{
    const double a = y_at(y, hd, wd, r - 1, c - 1), b = y_at(y, hd, wd, r - 1, c), cc = y_at(y, hd, wd, r - 1, c + 1);
    const double d = y_at(y, hd, wd, r, c - 1), e = y_at(y, hd, wd, r, c + 1);
    const double f = y_at(y, hd, wd, r + 1, c - 1), g = y_at(y, hd, wd, r + 1, c), h = y_at(y, hd, wd, r + 1, c + 1);
    const double gx = (((3.0 * cc + 10.0 * e) + 3.0 * h) - ((3.0 * a + 10.0 * d) + 3.0 * f)) / 16.0;
    const double gy = (((3.0 * f + 10.0 * g) + 3.0 * h) - ((3.0 * a + 10.0 * b) + 3.0 * cc)) / 16.0;
    return gx * gx + gy * gy;
}

__device__ __forceinline__ double ratio(double ab, double aa_bb, double c) { return (2.0 * ab + c) / (aa_bb + c); }

// grid = (ceil(N / 256), n_frames); block = 256.  acc: [frame][FSIM_WORDS], zeroed by the submit
__global__ __launch_bounds__(256) void k_fsim_pool(const double *__restrict__ yiq, const uint32_t *__restrict__ p, int hd, int wd,
                                                   double cos_lambda_pi, unsigned long long *__restrict__ acc)
{
    __shared__ unsigned long long red[4][3];
    const int64_t N = (int64_t)hd * wd, i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int fr = blockIdx.y;
    unsigned long long wp = 0, wa = 0, wb = 0;
    if (i < N) {
        const double *yr = yiq + (int64_t)(2 * fr) * 3 * N, *yd = yr + 3 * N;
        const int r = (int)(i / wd), c = (int)(i - (int64_t)r * wd);
        const long long p_r = p[(int64_t)(2 * fr) * N + i], p_d = p[(int64_t)(2 * fr + 1) * N + i];
        const double pr = (double)p_r * (1.0 / FIX), pd = (double)p_d * (1.0 / FIX);
        const double qr = scharr_q(yr, hd, wd, r, c), qd = scharr_q(yd, hd, wd, r, c);
        const double s_g = (2.0 * sqrt(qr * qd) + T2) / ((qr + qd) + T2);
        const double s_pc = ratio(pr * pd, pr * pr + pd * pd, T1);
        const double s_l = s_g * s_pc;
        const double ir = yr[N + i], id = yd[N + i], qqr = yr[2 * N + i], qqd = yd[2 * N + i];
        const double x = ratio(ir * id, ir * ir + id * id, T3) * ratio(qqr * qqd, qqr * qqr + qqd * qqd, T3);
        double cpow = pow(fabs(x), LAMBDA);
        if (x < 0.0) cpow = cpow * cos_lambda_pi;
        const long long gq = __double2ll_rn(s_l * FIX), gc = __double2ll_rn((s_l * cpow) * FIX);
        const long long pm = p_r > p_d ? p_r : p_d;
        wp = (unsigned long long)pm;
        wa = (unsigned long long)((gq * pm + (1ll << 23)) >> 24);
        wb = (unsigned long long)((gc * pm + (1ll << 23)) >> 24);   // gc may be negative: two's complement, an arithmetic shift
    }
    wp = wave_sum(wp); wa = wave_sum(wa); wb = wave_sum(wb);
    if (lane_id() == 0) { red[wave_id()][0] = wp; red[wave_id()][1] = wa; red[wave_id()][2] = wb; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long *w = acc + (int64_t)fr * FSIM_WORDS;
        const unsigned long long tp = red[0][0] + red[1][0] + red[2][0] + red[3][0];
        if (tp) {   // pm = 0 in every sample: nothing to add to any word
            atomicAdd(w + 0, tp);
            atomicAdd(w + 1, red[0][1] + red[1][1] + red[2][1] + red[3][1]);
            atomicAdd(w + 2, red[0][2] + red[1][2] + red[2][2] + red[3][2]);
        }
    }
}

// the shifted frequency coordinate of index i of an axis of n samples: ifftshift(range(n))[i]
inline double freq(int i, int n)
{
    const int m = (i + n / 2) % n;
    return (n & 1) ? ((double)m - (double)((n - 1) / 2)) / (double)(n - 1) : ((double)m - (double)(n / 2)) / (double)n;
}

// the four radial and the four angular factors at (i, j) of an hd x wd grid
void fsim_factors(int hd, int wd, int i, int j, double lg[4], double sp[4])
{
    const double x = freq(j, wd), y = freq(i, hd);
    double radius = std::sqrt(x * x + y * y);
    const double theta = std::atan2(-y, x);
    const double lp = 1.0 / (1.0 + std::pow(radius / 0.45, 30.0));
    const bool dc = i == 0 && j == 0;
    if (dc) radius = 1.0;
    const double l055 = std::log(0.55), den = 2.0 * (l055 * l055);
    for (int s = 0; s < 4; s++) {
        const double fo = 1.0 / (6.0 * (double)(1 << s)), l = std::log(radius / fo);
        lg[s] = dc ? 0.0 : std::exp(-(l * l) / den) * lp;
    }
    const double st = std::sin(theta), ct = std::cos(theta), sigma = (M_PI / 4.0) / 1.2;
    for (int o = 0; o < 4; o++) {
        const double a = (double)o * M_PI / 4.0, sa = std::sin(a), ca = std::cos(a);
        const double ds = st * ca - ct * sa, dcs = ct * ca + st * sa;
        const double dt = std::fabs(std::atan2(ds, dcs));
        sp[o] = std::exp(-(dt * dt) / (2.0 * (sigma * sigma)));
    }
}

} // namespace

void fsim_filter_host(int hd, int wd, int scale, int orient, double *dst)
{
    double lg[4], sp[4];
    for (int i = 0; i < hd; i++)
        for (int j = 0; j < wd; j++) {
            fsim_factors(hd, wd, i, j, lg, sp);
            dst[(size_t)i * wd + j] = lg[scale] * sp[orient];
        }
}

// all sixteen tables, [orientation][scale][hd wd] (filt may be null), and the four noise factors c_o
void fsim_bank_host(int hd, int wd, double *filt, double c[4])
{
    const size_t N = (size_t)hd * wd;
    std::vector<double> ts(4 * N);   // [orientation][N]: the sum over the scales of filt_{s,o}
    double em[4] = {0, 0, 0, 0};
    double lg[4], sp[4];
    for (int i = 0; i < hd; i++)
        for (int j = 0; j < wd; j++) {
            const size_t at = (size_t)i * wd + j;
            fsim_factors(hd, wd, i, j, lg, sp);
            for (int o = 0; o < 4; o++) {
                double t = 0.0;
                for (int s = 0; s < 4; s++) {
                    const double v = lg[s] * sp[o];
                    if (filt) filt[((size_t)o * 4 + s) * N + at] = v;
                    t += v;
                }
                ts[(size_t)o * N + at] = t;
                em[o] += (lg[0] * sp[o]) * (lg[0] * sp[o]);
            }
        }
    for (int o = 0; o < 4; o++) {
        // S_o by Parseval: the sum over k of the square of the even part of the sum over the scales
        double S = 0.0;
        for (int i = 0; i < hd; i++)
            for (int j = 0; j < wd; j++) {
                const size_t at = (size_t)i * wd + j, mt = (size_t)((hd - i) % hd) * wd + (size_t)((wd - j) % wd);
                const double t = (ts[(size_t)o * N + at] + ts[(size_t)o * N + mt]) / 2.0;
                S += t * t;
            }
        c[o] = std::sqrt(S / (std::log(2.0) * em[o])) * (std::sqrt(M_PI / 2.0) + 2.0 * std::sqrt(2.0 - M_PI / 2.0)) / 1.7;
    }
}

double fsim_noise_factor_host(int hd, int wd, int orient)
{
    double c[4];
    fsim_bank_host(hd, wd, nullptr, c);
    return c[orient];
}

// W[j][k] = exp(-2 pi i (j k mod n) / n): dst[0 .. n n) the real parts, dst[n n .. 2 n n) the imaginary ones
void fsim_twiddle_host(int n, double *dst)
{
    std::vector<double> co(n), si(n);
    for (int m = 0; m < n; m++) {
        const double a = -2.0 * M_PI * (double)m / (double)n;
        co[m] = std::cos(a);
        si[m] = std::sin(a);
    }
    const size_t nn = (size_t)n * n;
    for (int j = 0; j < n; j++)
        for (int k = 0; k < n; k++) {
            const int m = (int)(((int64_t)j * k) % n);
            dst[(size_t)j * n + k] = co[m];
            dst[nn + (size_t)j * n + k] = si[m];
        }
}

void fsim_matrix(int model, int depth, int f, double mat[3][4])
{
    const double s = (double)(1 << (depth - 8)), peak = (double)((1 << depth) - 1);
    double rgb[3][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
    double o0 = 0.0, o1 = 0.0;
    if (model == VQA_FSIM_BGR) {
        const double k = 255.0 / peak;
        rgb[0][2] = k; rgb[1][1] = k; rgb[2][0] = k;
    } else {
        const double ky = 255.0 / (219.0 * s), kc = model == VQA_FSIM_GRAY ? 0.0 : 255.0 / (224.0 * s);
        rgb[0][0] = ky; rgb[0][2] = 1.5748 * kc;
        rgb[1][0] = ky; rgb[1][1] = -0.1873 * kc; rgb[1][2] = -0.4681 * kc;
        rgb[2][0] = ky; rgb[2][1] = 1.8556 * kc;
        o0 = 16.0 * s; o1 = 128.0 * s;
    }
    for (int c = 0; c < 3; c++) rgb[c][3] = -((o0 * rgb[c][0] + o1 * rgb[c][1]) + o1 * rgb[c][2]);
    static const double a[3][3] = {{0.299, 0.587, 0.114}, {0.596, -0.274, -0.322}, {0.211, -0.523, 0.312}};
    const double ff = (double)f * (double)f;
    for (int c = 0; c < 3; c++)
        for (int j = 0; j < 4; j++)
            mat[c][j] = (c > 0 && model == VQA_FSIM_GRAY) ? 0.0 : ((a[c][0] * rgb[0][j] + a[c][1] * rgb[1][j]) + a[c][2] * rgb[2][j]) / ff;
}

void fsim_grid(int h, int w, int *f, int *hd, int *wd)
{
    *f = mdsi_factor(h, w);
    *hd = (h + *f - 1) / *f;
    *wd = (w + *f - 1) / *f;
}

size_t fsim_scratch_bytes(int h, int w)
{
    int f, hd, wd;
    fsim_grid(h, w, &f, &hd, &wd);
    return sizeof(double) * (2 * (size_t)FSIM_IMAGE_DOUBLES * (size_t)hd * (size_t)wd + 2 * 4);
}

void launch_fsim(hipStream_t st, const uint8_t *ref, const uint8_t *dist, int n, int64_t ref_frame_stride,
                 int64_t dist_frame_stride, const vqa_plane_desc *planes, int n_planes, int depth, int model,
                 const fsim_tabs &tabs, void *scratch, uint32_t *pmap, unsigned long long *acc, brisque_mark mark, void *mark_arg)
{
    if (n <= 0) return;
    fsim_src s;
    s.ref = ref; s.dist = dist; s.ref_fs = ref_frame_stride; s.dist_fs = dist_frame_stride;
    const vqa_plane_desc &y = planes[0], &u = planes[n_planes == 3 ? 1 : 0];
    for (int i = 0; i < 3; i++) s.off[i] = planes[i < n_planes ? i : 0].offset;
    s.rs0 = y.row_stride; s.step0 = y.pixel_step;
    s.rs1 = u.row_stride; s.step1 = u.pixel_step;
    s.w = y.width; s.h = y.height;
    s.sh = u.width != y.width; s.sv = u.height != y.height;
    s.np = n_planes;
    fsim_grid(s.h, s.w, &s.f, &s.hd, &s.wd);
    s.o = s.f / 2 - (s.f - 1);
    fsim_matrix(model, depth, s.f, s.mat);
    const int hd = s.hd, wd = s.wd, images = 2 * n;
    const int64_t N = (int64_t)hd * wd;
    // the scratch of a sub-slice: regions of `images` entries each
    double *yiq = (double *)scratch;                    // [image][3][N]
    double *tt = yiq + (int64_t)images * 3 * N;          // [image][2][N]: (Y - Y(0,0)) W_w
    double *ff = tt + (int64_t)images * 2 * N;           // [image][2][N]: F
    double *uu = ff + (int64_t)images * 2 * N;           // [image][4][2][N]: conj(W_h) (F filt) of one orientation
    double *eo = uu + (int64_t)images * 8 * N;           // [image][4][2][N]: EO of one orientation
    double *en = eo + (int64_t)images * 8 * N;           // [image][4][3][N]: Energy, An, |EO_0|^2
    double *thr = en + (int64_t)images * 12 * N;         // [image][4]
    const int tiles_x = (wd + TW - 1) / TW, tiles = tiles_x * ((hd + TH - 1) / TH);
    mark(mark_arg, VQA_K_FSIM_LUMA, 1);
    if (depth > 8) hipLaunchKernelGGL((k_fsim_luma<uint16_t>), dim3(tiles, images), dim3(256), 0, st, s, tiles_x, yiq);
    else hipLaunchKernelGGL((k_fsim_luma<uint8_t>), dim3(tiles, images), dim3(256), 0, st, s, tiles_x, yiq);
    mark(mark_arg, VQA_K_FSIM_LUMA, 0);

    constexpr int NT = 4;
    const auto grid = [&](int M, int Nc, int batch) { return dim3((Nc + 64 * NT - 1) / (64 * NT), (M + 15) / 16, batch); };
    const int64_t hh = (int64_t)hd * hd, ww = (int64_t)wd * wd;
    fsim_gemm g;
    mark(mark_arg, VQA_K_FSIM_DFT, 1);
    // T = (Y - Y(0,0)) W_w
    g = fsim_gemm{yiq, 3 * N, wd, 1, 0, 1, 1.0, tabs.ww, 0, wd, ww, 1, 1.0, nullptr, 0, 1, yiq, 3 * N, tt, 2 * N, wd, N, 1.0, hd, wd, wd};
    hipLaunchKernelGGL((k_fsim_dft<NT>), grid(hd, wd, images), dim3(256), 0, st, g);
    // F = W_h T (W is symmetric: A[i][k] is read as W[k][i], consecutive lanes on consecutive doubles)
    g = fsim_gemm{tabs.wh, 0, 1, hd, hh, 1, 1.0, tt, 2 * N, wd, N, 1, 1.0, nullptr, 0, 1, nullptr, 0, ff, 2 * N, wd, N, 1.0, hd, wd, hd};
    hipLaunchKernelGGL((k_fsim_dft<NT>), grid(hd, wd, images), dim3(256), 0, st, g);
    mark(mark_arg, VQA_K_FSIM_DFT, 0);
    for (int o = 0; o < 4; o++) {
        mark(mark_arg, VQA_K_FSIM_DFT, 1);
        // U_s = conj(W_h) (F filt_{s,o}): batch z = 4 image + s
        g = fsim_gemm{tabs.wh, 0, 1, hd, hh, 1, -1.0, ff, 2 * N, wd, N, 4, 1.0, tabs.filt + (int64_t)o * 4 * N, N, 4, nullptr, 0,
                      uu, 2 * N, wd, N, 1.0, hd, wd, hd};
        hipLaunchKernelGGL((k_fsim_dft<NT>), grid(hd, wd, 4 * images), dim3(256), 0, st, g);
        // EO_s = U_s conj(W_w) / N
        g = fsim_gemm{uu, 2 * N, wd, 1, N, 1, 1.0, tabs.ww, 0, wd, ww, 1, -1.0, nullptr, 0, 1, nullptr, 0, eo, 2 * N, wd, N, (double)N,
                      hd, wd, wd};
        hipLaunchKernelGGL((k_fsim_dft<NT>), grid(hd, wd, 4 * images), dim3(256), 0, st, g);
        mark(mark_arg, VQA_K_FSIM_DFT, 0);
        mark(mark_arg, VQA_K_FSIM_ENERGY, 1);
        hipLaunchKernelGGL(k_fsim_energy, dim3((unsigned)((N + 255) / 256), images), dim3(256), 0, st, (const double *)eo, N, o, en);
        mark(mark_arg, VQA_K_FSIM_ENERGY, 0);
    }
    fsim_noise nf;
    for (int o = 0; o < 4; o++) nf.c[o] = tabs.c[o];
    mark(mark_arg, VQA_K_FSIM_MEDIAN, 1);
    hipLaunchKernelGGL(k_fsim_median, dim3(4, images), dim3(1024), 0, st, (const double *)en, N, nf, thr);
    mark(mark_arg, VQA_K_FSIM_MEDIAN, 0);
    mark(mark_arg, VQA_K_FSIM_PC, 1);
    hipLaunchKernelGGL(k_fsim_pc, dim3((unsigned)((N + 255) / 256), images), dim3(256), 0, st, (const double *)en, (const double *)thr, N, pmap);
    mark(mark_arg, VQA_K_FSIM_PC, 0);
    mark(mark_arg, VQA_K_FSIM_POOL, 1);
    hipLaunchKernelGGL(k_fsim_pool, dim3((unsigned)((N + 255) / 256), n), dim3(256), 0, st, (const double *)yiq, (const uint32_t *)pmap, hd, wd, std::cos(LAMBDA * M_PI), acc);
    mark(mark_arg, VQA_K_FSIM_POOL, 0);
}

// the three words -> the record, in double on the host.  Contraction is off: the record is the formula vqa.h states.
void fsim_finalize(const unsigned long long *words, int h, int w, vqa_fsim_metrics *out)
{
    int f, hd, wd;
    fsim_grid(h, w, &f, &hd, &wd);
    out->sum_pc = words[0];
    out->sum_sim = words[1];
    out->sum_simc = words[2];
    out->count = (int64_t)hd * wd;
    out->factor = f;
    out->flags = words[0] ? 0u : 1u;
    out->fsim = words[0] ? (double)words[1] / (double)words[0] : 1.0;
    out->fsimc = words[0] ? (double)(int64_t)words[2] / (double)words[0] : 1.0;
}

} // namespace vqa
