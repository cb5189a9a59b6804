// k_vca.hip — the three texture features of the Video Complexity Analyzer for gfx950: energy E, its temporal gradient h and
// brightness L of a reference plane, from a weighted 32 x 32 block DCT, by the definition stated in include/vqa.h
// (vqa_vca_submit).
//
//   k_vca_blocks<T>  one wave owns one 32 x 32 block at a time and walks a grid-stride list of (frame slot, plane, block).
//                    Lane l = (hi = l >> 5, x = l & 31) loads the 16 samples X[2s + hi][x], s = 0 .. 15: a half-wave reads 32
//                    adjacent samples of one row, and every sample of the stream is read exactly once.  The samples are added
//                    up as integers first (S_k), and the block's rounded mean c = (S_k + 512) >> 10 is taken off every sample
//                    before the transform: the AC coefficients of X - c are those of X, and the DC, which the definition takes
//                    from S_k anyway, no longer leaks its rounding into them.  Both products run on v_mfma_f32_32x32x2_f32,
//                    whose operand map k_dct_full.hip writes down (A[i = l & 31][k = hi], B[k = hi][j = l & 31]; C / D: column
//                    l & 31, row rho(r, hi) = (r & 3) + 8 (r >> 2) + 4 hi of accumulator register r):
//                      P[x][u]  = sum_y X[y][x] T[u][y]      16 steps s: A = X[2s + hi][x],      B = T[u = x'][2s + hi]
//                      Dt[v][u] = sum_x T[v][x] P[x][u]      16 steps r: A = T[v = x'][rho(r, hi)], B = accumulator r of P
//                    (x' = l & 31).  Register r of P holds row rho(r, hi) of P in the half-wave hi - exactly what the B operand of a
//                    step that contracts over the two indices rho(r, 0), rho(r, 1) wants: the first product feeds the second
//                    from its registers, with no trip through LDS, and T's columns are permuted to match.  The order of both
//                    chains depends on nothing but the block.  Dt[v][u] = D[u][v]; the weight w is symmetric.  Each lane sums
//                    its 16 w |D| in double in register order, the wave in a fixed shuffle tree; lane 0 writes qH_k, S_k and
//                    qL_k to the block map.  The three tables (T in both operand orders and w, 4 KiB each, pre-permuted to
//                    [register][lane]) sit in 48 VGPRs for the whole walk.
//   k_vca_sum        one workgroup per (frame, plane): the map's qH and qL, and |qH - qH of the slot before|, added up as
//                    integers - any order gives the same three words.
//
// Map: (n + 1) slots of sum_p 3 C_p words; slot 0 is prev0's (computed only when there is one), slot i + 1 frame i's.  A slice
// after the first finds its predecessor's slot filled by the slice before it, on the same stream.
#include <cmath>

#include "vqa_dev.hpp"
#include "vqa_kernels.hpp"

namespace vqa {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// the reference frames of one group of same-geometry planes; every stride in bytes
struct vca_src {
    const uint8_t *ref;     // frame 0 of the slice
    const uint8_t *prev0;   // the frame of slot -1 (extra = 1), or nullptr
    int64_t fs;             // frame stride
    int64_t off[4];         // plane offsets inside a frame
    int64_t row_stride;
    int step;
    int extra;              // 1: the walk starts at slot -1
};

// grid = (workgroups); block = 256 = 4 waves.  items = slots * count * blocks.  map: the slice's slot 0, [slot][3 (plane_off +
// k)] uint64
template <typename T>
__global__ __launch_bounds__(256) void k_vca_blocks(vca_src s, const float *__restrict__ tabs, long long items, int nbx,
                                                    int blocks, int count, int4 plane_off, long long slot_words, double qscale,
                                                    unsigned long long *__restrict__ map)
{
    const int lane = threadIdx.x & 63, hi = lane >> 5, x = lane & 31;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    float t1[16], t2[16], wt[16];
#pragma unroll
    for (int r = 0; r < 16; r++) {
        t1[r] = tabs[r * 64 + lane];
        t2[r] = tabs[(16 + r) * 64 + lane];
        wt[r] = tabs[(32 + r) * 64 + lane];
    }
    const long long waves = (long long)gridDim.x * 4;
    for (long long item = (long long)blockIdx.x * 4 + wv; item < items; item += waves) {
        const long long per_slot = (long long)count * blocks;
        const long long slot = item / per_slot;
        const int rem = (int)(item - slot * per_slot), ch = rem / blocks, k = rem - ch * blocks;
        const int by = k / nbx, bx = k - by * nbx;
        const long long j = slot - s.extra;
        const uint8_t *p = (j < 0 ? s.prev0 : s.ref + j * s.fs) + s.off[ch] + (int64_t)(by * 32 + hi) * s.row_stride +
                           (int64_t)(bx * 32 + x) * s.step;
        int v[16];
#pragma unroll
        for (int q = 0; q < 16; q++) v[q] = (int)*(const T *)(p + (int64_t)(2 * q) * s.row_stride);
        unsigned sum = 0;
#pragma unroll
        for (int q = 0; q < 16; q++) sum += (unsigned)v[q];
        const unsigned S = __builtin_amdgcn_readfirstlane(wave_sum(sum));   // < 2^26
        const int c = (int)((S + 512u) >> 10);
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; r++) acc[r] = 0.f;
#pragma unroll
        for (int q = 0; q < 16; q++) acc = __builtin_amdgcn_mfma_f32_32x32x2f32((float)(v[q] - c), t1[q], acc, 0, 0, 0);
        f32x16 d;
#pragma unroll
        for (int r = 0; r < 16; r++) d[r] = 0.f;
#pragma unroll
        for (int r = 0; r < 16; r++) d = __builtin_amdgcn_mfma_f32_32x32x2f32(t2[r], acc[r], d, 0, 0, 0);
        double hsum = 0.0;
#pragma unroll
        for (int r = 0; r < 16; r++) hsum += (double)wt[r] * (double)fabsf(d[r]);   // (wt is 0 at the DC coefficient)
        hsum = wave_sum(hsum);
        if (lane == 0) {
            unsigned long long *m = map + j * slot_words + 3 * ((long long)(ch == 0 ? plane_off.x : ch == 1 ? plane_off.y : ch == 2 ? plane_off.z : plane_off.w) + k);
            m[0] = (unsigned long long)__double2ll_rn(hsum * qscale);
            m[1] = S;
            m[2] = (unsigned long long)__double2ll_rn(sqrt((double)S) * 16777216.0);
        }
    }
}

// grid = (n_planes, frames of the slice); block = 256.  map: the slice's slot 0; acc: [frame][plane][VCA_WORDS] of the slice
__global__ __launch_bounds__(256) void k_vca_sum(const unsigned long long *__restrict__ map, long long slot_words, int4 plane_off,
                                                 int4 plane_blocks, int n_planes, int first_has_prev,
                                                 unsigned long long *__restrict__ acc)
{
    __shared__ unsigned long long red[4];
    const int p = blockIdx.x, f = blockIdx.y;
    const long long off = p == 0 ? plane_off.x : p == 1 ? plane_off.y : p == 2 ? plane_off.z : plane_off.w;
    const int blocks = p == 0 ? plane_blocks.x : p == 1 ? plane_blocks.y : p == 2 ? plane_blocks.z : plane_blocks.w;
    const unsigned long long *cur = map + (long long)f * slot_words + 3 * off, *prev = cur - slot_words;
    const bool has_prev = f > 0 || first_has_prev;
    unsigned long long e = 0, h = 0, l = 0;
    for (int k = threadIdx.x; k < blocks; k += 256) {
        const unsigned long long q = cur[3 * k];
        e += q;
        l += cur[3 * k + 2];
        if (has_prev) {
            const unsigned long long q0 = prev[3 * k];
            h += q > q0 ? q - q0 : q0 - q;
        }
    }
    const unsigned long long te = block_sum_u64(e, red), th = block_sum_u64(h, red), tl = block_sum_u64(l, red);
    if (threadIdx.x == 0) {
        unsigned long long *a = acc + ((long long)f * n_planes + p) * VCA_WORDS;
        a[0] = te; a[1] = th; a[2] = tl;
    }
}

} // namespace

// T and w as the lanes hold them: [48][64] floats - rows 0 .. 15 T[x'][2s + hi], rows 16 .. 31 T[x'][rho(r, hi)], rows 32 .. 47
// w(x', rho(r, hi)) with the DC's weight 0.  Formed in double, rounded to fp32 once.
void vca_tables(float *tabs)
{
    const double pi = 3.14159265358979323846;
    auto T = [&](int u, int y) { return (u == 0 ? std::sqrt(1.0 / 32.0) : 0.25) * std::cos(pi * (2 * y + 1) * u / 64.0); };
    for (int r = 0; r < 16; r++)
        for (int lane = 0; lane < 64; lane++) {
            const int hi = lane >> 5, x = lane & 31, rho = (r & 3) + 8 * (r >> 2) + 4 * hi;
            tabs[r * 64 + lane] = (float)T(x, 2 * r + hi);
            tabs[(16 + r) * 64 + lane] = (float)T(x, rho);
            const double uv = (double)(x * rho) / 1024.0;
            tabs[(32 + r) * 64 + lane] = (x == 0 && rho == 0) ? 0.f : (float)std::exp(std::fabs(uv * uv - 1.0));
        }
}

void launch_vca_blocks(hipStream_t st, const uint8_t *ref, const uint8_t *prev0, int n, int64_t frame_stride,
                       const vqa_plane_desc *planes, const int *idx, int count, const vca_geom &g, int depth, const float *tabs,
                       unsigned long long *map)
{
    if (n <= 0 || count <= 0) return;
    const vqa_plane_desc &pd = planes[idx[0]];
    vca_src s;
    s.ref = ref; s.prev0 = prev0; s.fs = frame_stride;
    int p4[4];
    group_slots(planes, idx, count, s.off, p4);
    s.row_stride = pd.row_stride; s.step = pd.pixel_step;
    s.extra = prev0 ? 1 : 0;
    const int nbx = g.nbx[p4[0]], blocks = nbx * g.nby[p4[0]];
    const long long items = (long long)(n + s.extra) * count * blocks;
    const int4 po = make_int4(g.off[p4[0]], g.off[p4[1]], g.off[p4[2]], g.off[p4[3]]);
    // four waves a SIMD at about 110 VGPRs: 4096 waves fill the 256 CUs once; fewer items, fewer waves
    const long long wgs = (items + 3) / 4;
    const dim3 grid((unsigned)(wgs < 1024 ? wgs : 1024)), block(256);
    const double qscale = (double)(1 << (24 - depth));
    if (depth > 8)
        hipLaunchKernelGGL((k_vca_blocks<uint16_t>), grid, block, 0, st, s, tabs, items, nbx, blocks, count, po,
                           (long long)g.slot_words, qscale, map);
    else
        hipLaunchKernelGGL((k_vca_blocks<uint8_t>), grid, block, 0, st, s, tabs, items, nbx, blocks, count, po,
                           (long long)g.slot_words, qscale, map);
}

void launch_vca_sum(hipStream_t st, int n, int n_planes, const vca_geom &g, bool first_has_prev, const unsigned long long *map,
                    unsigned long long *acc)
{
    if (n <= 0) return;
    const int4 po = make_int4(g.off[0], g.off[1], g.off[2], g.off[3]);
    const int4 pb = make_int4(g.nbx[0] * g.nby[0], g.nbx[1] * g.nby[1], g.nbx[2] * g.nby[2], g.nbx[3] * g.nby[3]);
    hipLaunchKernelGGL(k_vca_sum, dim3(n_planes, n), dim3(256), 0, st, map, (long long)g.slot_words, po, pb, n_planes,
                       first_has_prev ? 1 : 0, acc);
}

vca_geom vca_geometry(const int *pw, const int *ph, int n_planes)
{
    vca_geom g = {};
    int off = 0;
    for (int p = 0; p < 4; p++) {
        const int q = p < n_planes ? p : 0;
        g.nbx[p] = pw[q] / 32; g.nby[p] = ph[q] / 32;
        g.off[p] = p < n_planes ? off : 0;
        if (p < n_planes) off += g.nbx[p] * g.nby[p];
    }
    g.slot_words = 3 * (size_t)off;
    return g;
}

// the three words -> the record, in double on the host (include/vqa.h)
void vca_finalize(const unsigned long long *words, int nbx, int nby, int depth, vqa_vca_metrics *out)
{
#pragma clang fp contract(off)
    const double sc = 1.0 / (double)(1 << (depth - 8)), q = 1.0 / (double)(1 << (24 - depth));
    const double C = (double)((int64_t)nbx * nby);
    out->e_sum = words[0]; out->h_sum = words[1]; out->l_sum = words[2];
    out->nbx = nbx; out->nby = nby;
    out->e = sc * (double)words[0] * q / (1024.0 * C);
    out->h = sc * (double)words[1] * q / (1024.0 * C);
    out->l = std::sqrt(sc / 32.0) * (double)words[2] * (1.0 / 16777216.0) / C;
}

} // namespace vqa
