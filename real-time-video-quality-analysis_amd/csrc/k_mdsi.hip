// k_mdsi.hip — mean deviation similarity index (Nafchi, Shahkolaei, Hedjam, Cheriet 2016) for gfx950: gradient similarity of the
// luminance with the fused-image term, chromaticity similarity of two opponent channels, the planes of a pixel taken together,
// pooled by the mean absolute deviation of a complex quarter power - by the definition stated in include/vqa.h (vqa_mdsi_submit).
//
//   k_mdsi_map<T>   one launch per slice.  A workgroup of 256 threads owns a 64 x 32 tile of the DOWNSAMPLED grid (hd x wd =
//                   ceil(h / f) x ceil(w / f)) and its apron of one sample.  Per image: the input rectangle of tile and apron -
//                   34 f rows of 66 f columns, clipped to the plane - is walked row by row, consecutive threads on consecutive
//                   columns, and every sample of the one or three planes is added as an integer into the LDS cell of its f x f
//                   window (windows are disjoint and start at floor(f / 2) - (f - 1), so they are not f-aligned: the walk
//                   does not care, and ONE loop serves every f from 1 to 64).  Chroma is replicated: (y >> sv, x >> sh).  From
//                   the sums and the count of in-plane positions the 3 x 4 matrix gives L for tile and apron (LDS, double; 0
//                   outside the grid: conv2 'same') and H, M for the thread's own eight samples (registers).  Then Prewitt of
//                   L_r and L_d from LDS, the fused gradient, GS, CS and GCS in double, g = rint(GCS 2^24) to the map, and
//                   zq = rint(|g 2^-24|^(1/4) 2^28) into A (g >= 0) or B (g < 0), with the count n_neg.
//   k_mdsi_dev      one launch per slice, over the map: the mean from the frame's A and B, identically in every thread, and
//                   rint(|z - mean|) in 2^-28 units into D.
//
// Sums (vqa.h states the bounds): a box sum is at most 65535 * 64 * 64 < 2^28 (32-bit LDS atomics); zq < 2^29 and N <= 2^28, so
// A, B, D < 2^58.  A workgroup adds its totals with one 64-bit integer atomic per word.  Integer addition is associative: neither
// the tiling nor the order in which workgroups retire can change a bit.
#include <cmath>

#include "vqa_dev.hpp"
#include "vqa_kernels.hpp"

// every double below is rounded once per written operation (the Makefile builds with -ffp-contract=fast)
#pragma clang fp contract(off)

namespace vqa {

namespace {

constexpr int TW = 64, TH = 32, IW = TW + 2, IH = TH + 2;
constexpr double C1 = 140.0, C2 = 55.0, C3 = 550.0;
constexpr double SQRT_HALF = 0x1.6a09e667f3bcdp-1;   // sqrt(0.5) as a double

// both images of n frames; every stride in bytes.  Plane 0 (Y, or B) is the full-size grid; planes 1 and 2 (U and V, or G and
// R; absent when np = 1) share one geometry, the grid's or its ceil-half in either direction (sh, sv).
struct mdsi_src {
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
    double mat[3][4];          // [L, H, M][plane 0, 1, 2, count]
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

// one image of one frame: box sums of tile and apron into bs, L into ld, H and M of the thread's eight samples into registers.
// Ends with a barrier: ld is complete and bs is free.
template <typename T>
__device__ __forceinline__ void load_image(const mdsi_src &s, const uint8_t *p, int y0, int x0, int (&bs)[3][IH][IW],
                                           double (&ld)[IH][IW], double (&ch)[8], double (&cm)[8])
{
    const int t = threadIdx.x, f = s.f;
    for (int i = t; i < 3 * IH * IW; i += 256) (&bs[0][0][0])[i] = 0;
    __syncthreads();
    // the input rectangle of tile and apron, clipped to the plane
    const int ry0 = (y0 - 1) * f + s.o, rx0 = (x0 - 1) * f + s.o;
    const int ya = ry0 > 0 ? ry0 : 0, yb = ry0 + IH * f < s.h ? ry0 + IH * f : s.h;
    const int xa = rx0 > 0 ? rx0 : 0, xb = rx0 + IW * f < s.w ? rx0 + IW * f : s.w;
    const int cols = xb - xa, total = cols * (yb - ya);   // at most 4224 * 2176
    const uint8_t *p0 = p + s.off[0], *p1 = p + s.off[1], *p2 = p + s.off[2];
    for (int i = t; i < total; i += 256) {
        const int ry = i / cols, y = ya + ry, x = xa + (i - ry * cols);
        const int di = (y - ry0) / f, dj = (x - rx0) / f;   // 0 <= di < IH, 0 <= dj < IW by the clip
        atomicAdd(&bs[0][di][dj], (int)*(const T *)(p0 + (int64_t)y * s.rs0 + (int64_t)x * s.step0));
        if (s.np == 3) {
            const int64_t oc = (int64_t)(y >> s.sv) * s.rs1 + (int64_t)(x >> s.sh) * s.step1;
            atomicAdd(&bs[1][di][dj], (int)*(const T *)(p1 + oc));
            atomicAdd(&bs[2][di][dj], (int)*(const T *)(p2 + oc));
        }
    }
    __syncthreads();
    for (int i = t; i < IH * IW; i += 256) {
        const int j = i / IW, c = i - j * IW;
        const int di = y0 - 1 + j, dj = x0 - 1 + c;
        double v = 0.0;   // outside the grid: conv2 'same'
        if (di >= 0 && di < s.hd && dj >= 0 && dj < s.wd)
            v = channel(s.mat[0], bs[0][j][c], bs[1][j][c], bs[2][j][c], window_count(di, f, s.o, s.h) * window_count(dj, f, s.o, s.w));
        ld[j][c] = v;
    }
    const int r = t >> 4, q4 = (t & 15) * 4;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const int row = r + 16 * (k >> 2), col = q4 + (k & 3);
        const int di = y0 + row, dj = x0 + col;
        ch[k] = cm[k] = 0.0;
        if (di < s.hd && dj < s.wd) {
            const int cnt = window_count(di, f, s.o, s.h) * window_count(dj, f, s.o, s.w);
            const int s0 = bs[0][row + 1][col + 1], s1 = bs[1][row + 1][col + 1], s2 = bs[2][row + 1][col + 1];
            ch[k] = channel(s.mat[1], s0, s1, s2, cnt);
            cm[k] = channel(s.mat[2], s0, s1, s2, cnt);
        }
    }
    __syncthreads();
}

// Prewitt over 3 at (j, c) of tile and apron (include/vqa.h states the order)
__device__ __forceinline__ void prewitt(const double (&x)[IH][IW], int j, int c, double &gx, double &gy)
{
    gx = (((x[j - 1][c + 1] + x[j][c + 1]) + x[j + 1][c + 1]) - ((x[j - 1][c - 1] + x[j][c - 1]) + x[j + 1][c - 1])) / 3.0;
    gy = (((x[j + 1][c - 1] + x[j + 1][c]) + x[j + 1][c + 1]) - ((x[j - 1][c - 1] + x[j - 1][c]) + x[j - 1][c + 1])) / 3.0;
}

__device__ __forceinline__ double similarity(double qa, double qb, double c)
{
    return (2.0 * sqrt(qa * qb) + c) / ((qa + qb) + c);
}

// zq of include/vqa.h: |g| <= 1.6 * 2^24, so zq < 2^29
__device__ __forceinline__ unsigned long long quarter_root(int g)
{
    return (unsigned long long)__double2ll_rn(sqrt(sqrt(fabs((double)g) * (1.0 / MDSI_FIX_G))) * MDSI_FIX_Z);
}

// grid = (tiles, n_frames); block = 256.  map: [frame][hd][wd] int; acc: [frame][MDSI_WORDS] uint64, zeroed by the submit
template <typename T>
__global__ __launch_bounds__(256) void k_mdsi_map(mdsi_src s, int tiles_x, int *__restrict__ map, unsigned long long *__restrict__ acc)
{
    __shared__ double ld[2][IH][IW];
    __shared__ int bs[3][IH][IW];
    __shared__ unsigned long long red[4][3];
    const int fr = blockIdx.y, tile = blockIdx.x;
    const int y0 = (tile / tiles_x) * TH, x0 = (tile % tiles_x) * TW;
    const int t = threadIdx.x;
    double hr[8], mr[8], hd[8], md[8];
    load_image<T>(s, s.ref + (int64_t)fr * s.ref_fs, y0, x0, bs, ld[0], hr, mr);
    load_image<T>(s, s.dist + (int64_t)fr * s.dist_fs, y0, x0, bs, ld[1], hd, md);
    const int r = t >> 4, q4 = (t & 15) * 4;
    int *mp = map + (int64_t)fr * s.hd * s.wd;
    unsigned long long a = 0, b = 0, nn = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const int row = r + 16 * (k >> 2), col = q4 + (k & 3);
        const int di = y0 + row, dj = x0 + col;
        if (di >= s.hd || dj >= s.wd) continue;
        double rx, ry, dx, dy;
        prewitt(ld[0], row + 1, col + 1, rx, ry);
        prewitt(ld[1], row + 1, col + 1, dx, dy);
        const double fx = 0.5 * (rx + dx), fy = 0.5 * (ry + dy);
        const double qr = rx * rx + ry * ry, qd = dx * dx + dy * dy, qf = fx * fx + fy * fy;
        const double gs = (similarity(qr, qd, C1) + similarity(qd, qf, C2)) - similarity(qr, qf, C2);
        const double cs = (2.0 * (hr[k] * hd[k] + mr[k] * md[k]) + C3) /
                          (((hr[k] * hr[k] + hd[k] * hd[k]) + (mr[k] * mr[k] + md[k] * md[k])) + C3);
        const double gcs = 0.6 * gs + 0.4 * cs;
        const int g = (int)__double2ll_rn(gcs * MDSI_FIX_G);
        mp[(int64_t)di * s.wd + dj] = g;
        const unsigned long long zq = quarter_root(g);
        if (g < 0) { b += zq; nn += 1; }
        else a += zq;
    }
    const unsigned long long w0 = wave_sum(a), w1 = wave_sum(b), w2 = wave_sum(nn);
    if (lane_id() == 0) { red[wave_id()][0] = w0; red[wave_id()][1] = w1; red[wave_id()][2] = w2; }
    __syncthreads();
    if (t == 0) {
        unsigned long long *wds = acc + (int64_t)fr * MDSI_WORDS;
        atomicAdd(wds + 0, red[0][0] + red[1][0] + red[2][0] + red[3][0]);
        const unsigned long long tb = red[0][1] + red[1][1] + red[2][1] + red[3][1];
        if (tb) {
            atomicAdd(wds + 1, tb);
            atomicAdd(wds + 2, red[0][2] + red[1][2] + red[2][2] + red[3][2]);
        }
    }
}

constexpr int DEV_SPAN = 2048;   // samples of the map per workgroup of k_mdsi_dev

// grid = (ceil(N / DEV_SPAN), n_frames); block = 256
__global__ __launch_bounds__(256) void k_mdsi_dev(const int *__restrict__ map, int count, unsigned long long *__restrict__ acc)
{
    __shared__ unsigned long long red[4];
    const int fr = blockIdx.y, t = threadIdx.x;
    unsigned long long *wds = acc + (int64_t)fr * MDSI_WORDS;
    const int *mp = map + (int64_t)fr * count;
    // the mean in 2^-28 units: the same operations on the same words in every thread of every workgroup
    const double n = (double)count, bi = (double)wds[1] * SQRT_HALF;
    const double m_re = ((double)wds[0] + bi) / n, m_im = bi / n;
    const int i0 = blockIdx.x * DEV_SPAN, i1 = i0 + DEV_SPAN < count ? i0 + DEV_SPAN : count;
    unsigned long long d = 0;
    for (int i = i0 + t; i < i1; i += 256) {
        const int g = mp[i];
        const double zq = (double)quarter_root(g);
        double re = zq, im = 0.0;
        if (g < 0) re = im = zq * SQRT_HALF;
        const double dr = re - m_re, di = im - m_im;
        d += (unsigned long long)__double2ll_rn(sqrt(dr * dr + di * di));
    }
    d = wave_sum(d);
    if (lane_id() == 0) red[wave_id()] = d;
    __syncthreads();
    if (t == 0) {
        const unsigned long long td = red[0] + red[1] + red[2] + red[3];
        if (td) atomicAdd(wds + 3, td);
    }
}

} // namespace

int mdsi_factor(int h, int w)
{
    const int m = h < w ? h : w, f = (m + 128) / 256;   // floor(m / 256 + 0.5)
    return f > 1 ? f : 1;
}

size_t mdsi_scratch_bytes(int h, int w)
{
    const int f = mdsi_factor(h, w);
    return sizeof(int) * (size_t)((h + f - 1) / f) * (size_t)((w + f - 1) / f);
}

void mdsi_matrix(int model, int depth, int f, double mat[3][4])
{
    const double s = (double)(1 << (depth - 8)), peak = (double)((1 << depth) - 1);
    double rgb[3][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
    double o0 = 0.0, o1 = 0.0;
    if (model == VQA_MDSI_BGR) {
        const double k = 255.0 / peak;
        rgb[0][2] = k; rgb[1][1] = k; rgb[2][0] = k;
    } else {
        const double ky = 255.0 / (219.0 * s), kc = model == VQA_MDSI_GRAY ? 0.0 : 255.0 / (224.0 * s);
        rgb[0][0] = ky; rgb[0][2] = 1.5748 * kc;
        rgb[1][0] = ky; rgb[1][1] = -0.1873 * kc; rgb[1][2] = -0.4681 * kc;
        rgb[2][0] = ky; rgb[2][1] = 1.8556 * kc;
        o0 = 16.0 * s; o1 = 128.0 * s;
    }
    for (int c = 0; c < 3; c++) rgb[c][3] = -((o0 * rgb[c][0] + o1 * rgb[c][1]) + o1 * rgb[c][2]);
    static const double a[3][3] = {{0.2989, 0.5870, 0.1140}, {0.30, 0.04, -0.35}, {0.34, -0.60, 0.17}};
    const double ff = (double)f * (double)f;
    for (int c = 0; c < 3; c++)
        for (int j = 0; j < 4; j++) mat[c][j] = ((a[c][0] * rgb[0][j] + a[c][1] * rgb[1][j]) + a[c][2] * rgb[2][j]) / ff;
}

void launch_mdsi(hipStream_t st, const uint8_t *ref, const uint8_t *dist, int n, int64_t ref_frame_stride,
                 int64_t dist_frame_stride, const vqa_plane_desc *planes, int n_planes, int depth, int model, void *map,
                 unsigned long long *acc, brisque_mark mark, void *mark_arg)
{
    if (n <= 0) return;
    mdsi_src s;
    s.ref = ref; s.dist = dist; s.ref_fs = ref_frame_stride; s.dist_fs = dist_frame_stride;
    const vqa_plane_desc &y = planes[0], &u = planes[n_planes == 3 ? 1 : 0];
    for (int i = 0; i < 3; i++) s.off[i] = planes[i < n_planes ? i : 0].offset;
    s.rs0 = y.row_stride; s.step0 = y.pixel_step;
    s.rs1 = u.row_stride; s.step1 = u.pixel_step;
    s.w = y.width; s.h = y.height;
    s.sh = u.width != y.width; s.sv = u.height != y.height;
    s.np = n_planes;
    s.f = mdsi_factor(s.h, s.w);
    s.o = s.f / 2 - (s.f - 1);
    s.wd = (s.w + s.f - 1) / s.f; s.hd = (s.h + s.f - 1) / s.f;
    mdsi_matrix(model, depth, s.f, s.mat);
    const int tiles_x = (s.wd + TW - 1) / TW, tiles = tiles_x * ((s.hd + TH - 1) / TH);
    const int count = s.wd * s.hd;   // at most 2^28
    mark(mark_arg, VQA_K_MDSI_MAP, 1);
    if (depth > 8)
        hipLaunchKernelGGL((k_mdsi_map<uint16_t>), dim3(tiles, n), dim3(256), 0, st, s, tiles_x, (int *)map, acc);
    else
        hipLaunchKernelGGL((k_mdsi_map<uint8_t>), dim3(tiles, n), dim3(256), 0, st, s, tiles_x, (int *)map, acc);
    mark(mark_arg, VQA_K_MDSI_MAP, 0);
    mark(mark_arg, VQA_K_MDSI_DEV, 1);
    hipLaunchKernelGGL(k_mdsi_dev, dim3((count + DEV_SPAN - 1) / DEV_SPAN, n), dim3(256), 0, st, (const int *)map, count, acc);
    mark(mark_arg, VQA_K_MDSI_DEV, 0);
}

// the four words -> the record, in double on the host.  Contraction is off: the record is the formula vqa.h states.
void mdsi_finalize(const unsigned long long *words, int h, int w, vqa_mdsi_metrics *out)
{
    const int f = mdsi_factor(h, w);
    const int64_t n = (int64_t)((h + f - 1) / f) * ((w + f - 1) / f);
    out->sum_pos = words[0];
    out->sum_neg = words[1];
    out->n_neg = words[2];
    out->sum_dev = words[3];
    out->count = n;
    out->factor = f;
    out->reserved = 0;
    out->dev = (double)words[3] / ((double)n * MDSI_FIX_Z);
    out->mdsi = std::sqrt(std::sqrt(out->dev));
}

} // namespace vqa
