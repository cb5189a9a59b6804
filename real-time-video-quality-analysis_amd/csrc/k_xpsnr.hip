// k_xpsnr.hip — XPSNR, the activity-weighted PSNR with block weights (Helmrich et al., ICASSP 2020; JVET-H0047) for gfx950: per
// block of the picture the squared error of every plane and the spatial and temporal activity of the reference's luma, by the
// definition stated in include/vqa.h (vqa_xpsnr_submit).  Only integers leave the device; the one division per block and the one
// sum per plane are the host's (xpsnr_finalize).
//
//   k_xpsnr_act<T, BV>  the luma plane of the reference and of the frame before it.  k_siti's mapping: a workgroup of 256
//               threads owns a 64 x 32 tile of the activity grid G; the tile and its apron of ONE sample go to LDS as integers -
//               for BV = 2 the sum of a 2x2 input quad, formed on the way in as k_gmsd does.  Every thread forms, for two rows
//               of four adjacent origins, |f| of the high-pass and |G - Gp| against the predecessor, whose grid value is read
//               straight from global memory.  Origins are the interior of G only: no border rule exists.
//   k_xpsnr_sse<T>      every plane of both streams, one launch per group of same-geometry planes: (r - d)^2 of two rows of
//               four adjacent samples per thread, straight from global memory.
//
// Blocks and tiles do not line up (B = 68 gives 34 on G against a 64 x 32 tile): both kernels compute the block of every origin
// or sample by itself.  A thread adds a run of values that share a block into that block's 64-bit accumulator in LDS (one integer
// LDS atomic per run and word); after a barrier the workgroup sends one 64-bit integer global atomic per touched block and word.
// A tile of G touches at most 17 x 9 blocks (B >= 4), a tile of a plane at most 33 x 17 (chroma blocks of B / 2 >= 2).
// Integer addition is associative: neither the tiling nor the order in which workgroups retire can change a word, so a pair
// (with its predecessor) gives the same words at any place of any batch.  Bounds (vqa.h): |f| < 2^22, a block owns fewer than
// 2^20 origins and samples, every word stays below 2^53.
#include <cmath>
#include <type_traits>

#include "vqa_dev.hpp"
#include "vqa_kernels.hpp"

namespace vqa {

namespace {

constexpr int TW = 64, TH = 32;   // the tile of both kernels

// the reference's luma plane; every stride in bytes
struct xpsnr_act_src {
    const uint8_t *ref;     // frame 0 of the slice
    const uint8_t *prev0;   // the frame before it, or nullptr
    int64_t fs;             // frame stride
    int64_t off;            // the luma plane inside a frame
    int64_t row_stride;
    int step;
    int gw, gh;             // the activity grid G
    int g;                  // a block's side on G: B / bv
    int nbx;
};

// G(y, x), y < gh and x < gw: the sample, or the sum of its quad - whose last row 2 y + 1 <= 2 gh - 1 <= h - 1 lies in the plane
template <typename T, int BV> __device__ __forceinline__ int grid_at(const uint8_t *p, const xpsnr_act_src &s, int y, int x)
{
    const uint8_t *a = p + (int64_t)(BV * y) * s.row_stride + (int64_t)(BV * x) * s.step;
    int v = (int)*(const T *)a;
    if (BV == 2) {
        const uint8_t *b = a + s.row_stride;
        v += (int)*(const T *)(a + s.step) + (int)*(const T *)b + (int)*(const T *)(b + s.step);
    }
    return v;
}

// grid = (tiles, n_frames); block = 256.  words: [frame][frame_words] uint64, zeroed by the submit; block k's pair at 2 k
template <typename T, int BV>
__global__ __launch_bounds__(256) void k_xpsnr_act(xpsnr_act_src s, int tiles_x, int64_t frame_words,
                                                   unsigned long long *__restrict__ words)
{
    constexpr int IW = TW + 4, IH = TH + 2;   // IW: 66 used, rows padded to 16 bytes
    constexpr int LBX = 17, LBY = 9;          // the blocks a tile can touch: floor(63 / g) + 2, floor(31 / g) + 2 at g >= 4
    __shared__ __attribute__((aligned(16))) int in[IH][IW];
    __shared__ unsigned long long bacc[2][LBY * LBX];
    const int f = blockIdx.y;
    const bool has_prev = f > 0 || s.prev0 != nullptr;   // (the whole workgroup)
    const int tile = blockIdx.x;
    const int y0 = (tile / tiles_x) * TH, x0 = (tile % tiles_x) * TW;
    const int t = threadIdx.x;
    const uint8_t *pc = s.ref + (int64_t)f * s.fs + s.off;
    for (int i = t; i < 2 * LBY * LBX; i += 256) (&bacc[0][0])[i] = 0;
    // the clamp serves the apron of edge tiles and tiles that hang over G's edge: they read (and mask) in-grid values
    for (int i = t; i < IH * (TW + 2); i += 256) {
        const int j = i / (TW + 2), c = i - j * (TW + 2);
        const int y = min(max(y0 + j - 1, 0), s.gh - 1), x = min(max(x0 + c - 1, 0), s.gw - 1);
        in[j][c] = grid_at<T, BV>(pc, s, y, x);
    }
    __syncthreads();
    // the blocks of this tile: columns bx0 .. bx0 + lbx - 1, rows by0 .. by0 + lby - 1
    const int bx0 = x0 / s.g, by0 = y0 / s.g;
    const int lbx = min(x0 + TW - 1, s.gw - 1) / s.g - bx0 + 1, lby = min(y0 + TH - 1, s.gh - 1) / s.g - by0 + 1;
    const uint8_t *pp = has_prev ? (f == 0 ? s.prev0 : s.ref + (int64_t)(f - 1) * s.fs) + s.off : nullptr;
    // thread = (rows r and r + 16, four adjacent columns); a run: the values of consecutive origins of one block
    const int r = t >> 4, q4 = (t & 15) * 4;
    int cur = -1;
    unsigned run_sa = 0, run_ta = 0;   // at most 8 values below 2^22
    auto flush = [&]() {
        if (cur >= 0) {
            atomicAdd(&bacc[0][cur], (unsigned long long)run_sa);
            if (has_prev) atomicAdd(&bacc[1][cur], (unsigned long long)run_ta);
        }
        run_sa = run_ta = 0;
    };
#pragma unroll
    for (int half = 0; half < 2; half++) {
        const int row = r + 16 * half, y = y0 + row;
        if (y < 1 || y > s.gh - 2) continue;
        int v[3][6];
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const int4 u0 = *reinterpret_cast<const int4 *>(&in[row + a][q4]);
            const int2 u1 = *reinterpret_cast<const int2 *>(&in[row + a][q4 + 4]);
            v[a][0] = u0.x; v[a][1] = u0.y; v[a][2] = u0.z; v[a][3] = u0.w; v[a][4] = u1.x; v[a][5] = u1.y;
        }
        const int lrow = (y / s.g - by0) * lbx;
#pragma unroll
        for (int o = 0; o < 4; o++) {
            const int x = x0 + q4 + o;
            if (x < 1 || x > s.gw - 2) continue;
            const int lb = lrow + (x / s.g - bx0);   // < lby lbx: y <= gh - 2 and x <= gw - 2 lie in the tile's clamped range
            if (lb != cur) { flush(); cur = lb; }
            // |f| <= 12 (BV BV) (2^depth - 1) < 2^22
            const int hp = 12 * v[1][o + 1] - 2 * (v[0][o + 1] + v[2][o + 1] + v[1][o] + v[1][o + 2]) -
                           (v[0][o] + v[0][o + 2] + v[2][o] + v[2][o + 2]);
            run_sa += (unsigned)abs(hp);
            if (has_prev) run_ta += (unsigned)abs(v[1][o + 1] - grid_at<T, BV>(pp, s, y, x));
        }
    }
    flush();
    __syncthreads();
    unsigned long long *fw = words + (int64_t)f * frame_words;
    for (int i = t; i < lby * lbx; i += 256) {
        const int ly = i / lbx, lx = i - ly * lbx;
        const int64_t k = (int64_t)(by0 + ly) * s.nbx + (bx0 + lx);   // by0 + ly <= (gh - 1) / g < nby, likewise bx
        const unsigned long long a = bacc[0][i], b = bacc[1][i];
        if (a) atomicAdd(fw + 2 * k, a);          // sa
        if (b) atomicAdd(fw + 2 * k + 1, b);      // ta (0 without a predecessor: the submit's memset stands)
    }
}

// both images of one group of same-geometry planes; every stride in bytes
struct xpsnr_sse_src {
    const uint8_t *ref, *dist;
    int64_t ref_fs, dist_fs;   // frame strides
    int64_t off[4];            // plane offsets inside a frame
    int64_t row_stride;
    int step;
    int w, h;                  // the plane
    int bw, bh;                // its blocks: B, or B / 2 where it is subsampled
    int nbx, nb;               // the grid's width and its nbx nby blocks
};

// grid = (tiles * count, n_frames); block = 256.  words: as above; plane p's block k at (2 + p) nb + k
template <typename T>
__global__ __launch_bounds__(256) void k_xpsnr_sse(xpsnr_sse_src s, int tiles_x, int tiles, int4 plane_index, int64_t frame_words,
                                                   unsigned long long *__restrict__ words)
{
    constexpr int LBX = 33, LBY = 17;   // the blocks a tile can touch: floor(63 / bw) + 2, floor(31 / bh) + 2 at bw, bh >= 2
    __shared__ unsigned long long bacc[LBY * LBX];
    const int f = blockIdx.y;
    const int ch = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const int y0 = (tile / tiles_x) * TH, x0 = (tile % tiles_x) * TW;
    const int t = threadIdx.x;
    const uint8_t *pr = s.ref + (int64_t)f * s.ref_fs + s.off[ch];
    const uint8_t *pd = s.dist + (int64_t)f * s.dist_fs + s.off[ch];
    for (int i = t; i < LBY * LBX; i += 256) bacc[i] = 0;
    __syncthreads();
    const int bx0 = x0 / s.bw, by0 = y0 / s.bh;
    const int lbx = min(x0 + TW - 1, s.w - 1) / s.bw - bx0 + 1, lby = min(y0 + TH - 1, s.h - 1) / s.bh - by0 + 1;
    // thread = (rows r and r + 16, four adjacent columns); a run: the squares of consecutive samples of one block
    const int r = t >> 4, q4 = (t & 15) * 4;
    int cur = -1;
    unsigned long long run = 0;   // at most 8 squares below 2^32
    auto flush = [&]() {
        if (cur >= 0) atomicAdd(&bacc[cur], run);
        run = 0;
    };
#pragma unroll
    for (int half = 0; half < 2; half++) {
        const int y = y0 + r + 16 * half;
        if (y >= s.h) continue;
        const int lrow = (y / s.bh - by0) * lbx;
        const int64_t ro = (int64_t)y * s.row_stride;
#pragma unroll
        for (int o = 0; o < 4; o++) {
            const int x = x0 + q4 + o;
            if (x >= s.w) continue;
            const int lb = lrow + (x / s.bw - bx0);   // < lby lbx: y and x lie in the tile's clamped range
            if (lb != cur) { flush(); cur = lb; }
            const int64_t at = ro + (int64_t)x * s.step;
            const int d = (int)*(const T *)(pr + at) - (int)*(const T *)(pd + at);
            run += (unsigned long long)((unsigned)abs(d) * (unsigned)abs(d));   // |d| <= 65535: the square fits 32 bits
        }
    }
    flush();
    __syncthreads();
    const int pi = ch == 0 ? plane_index.x : ch == 1 ? plane_index.y : ch == 2 ? plane_index.z : plane_index.w;
    unsigned long long *pw = words + (int64_t)f * frame_words + (int64_t)(2 + pi) * s.nb;
    for (int i = t; i < lby * lbx; i += 256) {
        const int ly = i / lbx, lx = i - ly * lbx;
        const int64_t k = (int64_t)(by0 + ly) * s.nbx + (bx0 + lx);   // (h - 1) / bh < nby and (w - 1) / bw < nbx (vqa.h)
        const unsigned long long a = bacc[i];
        if (a) atomicAdd(pw + k, a);
    }
}

} // namespace

xpsnr_geom xpsnr_geometry(int w, int h)
{
#pragma clang fp contract(off)
    xpsnr_geom g;
    const int64_t area = (int64_t)w * h;
    g.rho = (double)area / (3840.0 * 2160.0);
    const int b = 4 * (int)std::floor(32.0 * std::sqrt(g.rho) + 0.5);
    g.block = b > 4 ? b : 4;
    g.nbx = (w + g.block - 1) / g.block;
    g.nby = (h + g.block - 1) / g.block;
    g.bv = area <= 2048 * 1152 ? 1 : 2;
    g.gw = w / g.bv;
    g.gh = h / g.bv;
    return g;
}

void launch_xpsnr_act(hipStream_t st, const uint8_t *ref, const uint8_t *prev0, int n, int64_t ref_frame_stride,
                      const vqa_plane_desc &luma, const xpsnr_geom &g, int depth, size_t frame_words, unsigned long long *words)
{
    if (n <= 0) return;
    xpsnr_act_src s;
    s.ref = ref; s.prev0 = prev0; s.fs = ref_frame_stride; s.off = luma.offset;
    s.row_stride = luma.row_stride; s.step = luma.pixel_step;
    s.gw = g.gw; s.gh = g.gh; s.g = g.block / g.bv; s.nbx = g.nbx;
    const int tiles_x = (s.gw + TW - 1) / TW, tiles = tiles_x * ((s.gh + TH - 1) / TH);
    const dim3 grid(tiles, n), block(256);
    const int64_t fw = (int64_t)frame_words;
    if (depth > 8) {
        if (g.bv == 2) hipLaunchKernelGGL((k_xpsnr_act<uint16_t, 2>), grid, block, 0, st, s, tiles_x, fw, words);
        else hipLaunchKernelGGL((k_xpsnr_act<uint16_t, 1>), grid, block, 0, st, s, tiles_x, fw, words);
    } else {
        if (g.bv == 2) hipLaunchKernelGGL((k_xpsnr_act<uint8_t, 2>), grid, block, 0, st, s, tiles_x, fw, words);
        else hipLaunchKernelGGL((k_xpsnr_act<uint8_t, 1>), grid, block, 0, st, s, tiles_x, fw, words);
    }
}

void launch_xpsnr_sse(hipStream_t st, const uint8_t *ref, const uint8_t *dist, int n, int64_t ref_frame_stride,
                      int64_t dist_frame_stride, const vqa_plane_desc *planes, const int *idx, int count, const xpsnr_geom &g,
                      int depth, size_t frame_words, unsigned long long *words)
{
    if (n <= 0 || count <= 0) return;
    const vqa_plane_desc &pd = planes[idx[0]], &luma = planes[0];
    xpsnr_sse_src s;
    s.ref = ref; s.dist = dist; s.ref_fs = ref_frame_stride; s.dist_fs = dist_frame_stride;
    int p4[4];
    group_slots(planes, idx, count, s.off, p4);
    s.row_stride = pd.row_stride; s.step = pd.pixel_step;
    s.w = pd.width; s.h = pd.height;
    s.bw = pd.width == luma.width ? g.block : g.block / 2;     // (the submit has checked the ratio)
    s.bh = pd.height == luma.height ? g.block : g.block / 2;
    s.nbx = g.nbx; s.nb = g.nbx * g.nby;
    const int tiles_x = (s.w + TW - 1) / TW, tiles = tiles_x * ((s.h + TH - 1) / TH);
    const int4 pi = make_int4(p4[0], p4[1], p4[2], p4[3]);
    const dim3 grid(tiles * count, n), block(256);
    const int64_t fw = (int64_t)frame_words;
    if (depth > 8)
        hipLaunchKernelGGL((k_xpsnr_sse<uint16_t>), grid, block, 0, st, s, tiles_x, tiles, pi, fw, words);
    else
        hipLaunchKernelGGL((k_xpsnr_sse<uint8_t>), grid, block, 0, st, s, tiles_x, tiles, pi, fw, words);
}

// a frame's words -> its records: one division per block, one sum per plane, in double with contraction off, blocks in
// ascending k - the record is the formula vqa.h states.  Every word is below 2^53 and converts exactly.
void xpsnr_finalize(const unsigned long long *words, const xpsnr_geom &g, int depth, int n_planes, const int *pw, const int *ph,
                    vqa_xpsnr_metrics *out, uint64_t *blocks)
{
#pragma clang fp contract(off)
    const int nb = g.nbx * g.nby, gs = g.block / g.bv;
    const double a_min = std::ldexp(1.0, depth - 6), s = (double)(g.bv * g.bv);
    const double avg = std::sqrt(16.0 * std::ldexp(1.0, 2 * depth - 9) / std::sqrt(g.rho > 1e-5 ? g.rho : 1e-5));
    const double peak = (double)((1 << depth) - 1);
    double sum[4] = {0.0, 0.0, 0.0, 0.0};
    uint64_t tot[4] = {0, 0, 0, 0};
    for (int k = 0; k < nb; k++) {
        const int by = k / g.nbx, bx = k - by * g.nbx;
        // the origins 1 .. gw - 2 (gh - 2) that fall into columns (rows) bx gs .. (bx + 1) gs - 1 of G
        const int cx0 = bx * gs > 1 ? bx * gs : 1, cx1 = (bx + 1) * gs < g.gw - 1 ? (bx + 1) * gs : g.gw - 1;
        const int cy0 = by * gs > 1 ? by * gs : 1, cy1 = (by + 1) * gs < g.gh - 1 ? (by + 1) * gs : g.gh - 1;
        const int64_t nk = (cx1 > cx0 && cy1 > cy0) ? (int64_t)(cx1 - cx0) * (cy1 - cy0) : 0;
        const unsigned long long sa = words[2 * k], ta = words[2 * k + 1];
        double a = a_min;
        if (nk > 0) {
            a = (double)(sa + 2 * ta) / (s * (double)nk);
            if (a < a_min) a = a_min;
        }
        if (blocks) { blocks[3 * k] = sa; blocks[3 * k + 1] = ta; blocks[3 * k + 2] = (uint64_t)nk; }
        for (int p = 0; p < n_planes; p++) {
            const unsigned long long e = words[(size_t)(2 + p) * nb + k];
            if (blocks) blocks[(size_t)(3 + p) * nb + k] = e;
            tot[p] += e;
            sum[p] += (double)e / a;
        }
    }
    for (int p = 0; p < n_planes; p++) {
        out[p].sse = tot[p];
        out[p].wsse = avg * sum[p];
        out[p].xpsnr = out[p].wsse > 0.0 ? 10.0 * std::log10(((double)((int64_t)pw[p] * ph[p]) * (peak * peak)) / out[p].wsse)
                                         : (double)INFINITY;
        out[p].block = g.block; out[p].nbx = g.nbx; out[p].nby = g.nby;
    }
}

} // namespace vqa
