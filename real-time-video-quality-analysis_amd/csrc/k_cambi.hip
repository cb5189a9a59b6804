// k_cambi.hip — CAMBI, the contrast-aware multiscale banding index (Tandon, Afonso, Sole, Krasula, PCS 2021) for gfx950, by
// the definition stated in include/vqa.h (vqa_cambi_submit): one stream, every plane by itself, integers only.
//
//   k_cambi_mask<T>    steps 1-3.  A workgroup of 256 threads owns a 64 x 16 tile: the tile and an apron of 3 + 2 samples go to
//                      LDS as 10-bit values t (indices clamped to the plane), then y0 (the 2x2 rounded mean), then Z (both
//                      forward neighbours equal; 0 outside the plane), then S, the 7 x 7 sum of Z, and m0 = S > 24.  What leaves
//                      is ONE 16-bit word per sample, v0 = m0 ? y0 : CAMBI_OUT, and the count of m0.  y0 computed at a clamped
//                      index equals y0 computed from clamped t, so the clamped apron serves both rules.
//   k_cambi_decimate   step 4, all four further scales in one launch: v_s(i, j) = v_0(i << s, j << s), which is what four
//                      steps of (2i, 2j) give, and the counts of m_s.  A contrast needs y only where m = 1 (its own pixel and
//                      the pixels it counts), so v carries all that the later steps read.
//   k_cambi_contrast   step 5, one launch per scale.  A workgroup owns a 32 x 32 tile; the tile and its 32-sample apron
//                      (96 x 96 words, 18 KiB) go to LDS, CAMBI_OUT outside the plane.  CAMBI_OUT = 65535 is more than 4 away
//                      from every y <= 1023, so a masked-out or out-of-plane sample is never counted.  A thread owns four
//                      pixels, one at a time; a wave (two tile rows) none of whose pixels is masked skips the walk.  The walk:
//                      65 rows of 65 LDS reads; within a row the nine counts ride in one 64-bit word as 7-bit fields (a row
//                      adds at most 65 to a field), unpacked into nine registers per row.  u is the largest of the eight
//                      rounded 64-bit quotients.  u > 0 adds 1 to word u of the entry's histogram (65537 bins): an integer
//                      atomic.  u = 0 adds nothing to any top-K sum and is not recorded.
//   k_cambi_topk       step 6, one workgroup per (frame, plane): the exact sum of the K largest u from the histogram, walked
//                      from the top bin down.  Pixels that are not in the histogram are the zeros.
//
// A histogram and the sums taken from it do not depend on the order in which pixels arrive: the same plane gives the same
// words at any place of any batch.  Bounds: n_d <= 4225, num 2^17 <= 4 4225^2 2^17 < 2^44, den <= 8450 4225 < 2^26;
// top_s <= K_s 2^16 < 2^43.
#include "vqa_dev.hpp"
#include "vqa_kernels.hpp"

namespace vqa {

namespace {

constexpr unsigned CAMBI_OUT = 0xffffu;   // masked out, or outside the plane

// the frames of one group of same-geometry planes; every stride in bytes
struct cambi_src {
    const uint8_t *frames;
    int64_t fs;             // frame stride
    int64_t off[4];         // plane offsets inside a frame
    int64_t row_stride;
    int step;
    int w, h;
    int depth;
};

// the five scales of one plane inside the scratch image of a (frame, plane): sizes and offsets in samples
struct cambi_levels {
    int w[CAMBI_SCALES], h[CAMBI_SCALES];
    int64_t off[CAMBI_SCALES];
    int64_t total;
};

// step 1: a raw sample -> 10 bits
__device__ __forceinline__ int to10(int x, int depth)
{
    if (depth < 10) return min(1023, x << (10 - depth));
    const int sh = depth - 10;
    return min(1023, (x + (sh ? 1 << (sh - 1) : 0)) >> sh);
}

// grid = (tiles * count, n_frames); block = 256.  pyr: [frame][slot][lv.total] uint16; acc: [frame][plane][CAMBI_WORDS]
template <typename T>
__global__ __launch_bounds__(256) void k_cambi_mask(cambi_src s, cambi_levels lv, int tiles_x, int tiles, int count, int n_planes,
                                                    int4 plane_index, uint16_t *__restrict__ pyr,
                                                    unsigned long long *__restrict__ acc)
{
    constexpr int TW = 64, TH = 16, LW = TW + 8;   // t: TH + 8 rows, y: TH + 7, z: TH + 6
    __shared__ uint16_t tt[TH + 8][LW];
    __shared__ uint16_t yy[TH + 7][LW];
    __shared__ uint8_t zz[TH + 6][LW];
    __shared__ unsigned long long red[4];
    const int f = blockIdx.y;
    const int ch = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const int y0 = (tile / tiles_x) * TH, x0 = (tile % tiles_x) * TW;
    const int t = threadIdx.x;
    const uint8_t *pc = s.frames + (int64_t)f * s.fs + s.off[ch];
    for (int i = t; i < (TH + 8) * LW; i += 256) {
        const int a = i / LW, b = i - a * LW;
        const int y = min(max(y0 - 3 + a, 0), s.h - 1), x = min(max(x0 - 3 + b, 0), s.w - 1);
        tt[a][b] = (uint16_t)to10((int)*(const T *)(pc + (int64_t)y * s.row_stride + (int64_t)x * s.step), s.depth);
    }
    __syncthreads();
    for (int i = t; i < (TH + 7) * (LW - 1); i += 256) {
        const int a = i / (LW - 1), b = i - a * (LW - 1);
        yy[a][b] = (uint16_t)(((int)tt[a][b] + tt[a][b + 1] + tt[a + 1][b] + tt[a + 1][b + 1] + 2) >> 2);
    }
    __syncthreads();
    for (int i = t; i < (TH + 6) * (LW - 2); i += 256) {
        const int a = i / (LW - 2), b = i - a * (LW - 2);
        const int y = y0 - 3 + a, x = x0 - 3 + b;
        const bool in = y >= 0 && y < s.h && x >= 0 && x < s.w;
        zz[a][b] = (uint8_t)(in && yy[a][b] == yy[a][b + 1] && yy[a][b] == yy[a + 1][b]);
    }
    __syncthreads();
    // thread = (row r, four adjacent columns)
    const int r = t >> 4, c4 = (t & 15) * 4;
    uint16_t *out = pyr + ((int64_t)f * count + ch) * lv.total;
    unsigned long long masked = 0;
    if (y0 + r < s.h) {
        int col[10];
#pragma unroll
        for (int b = 0; b < 10; b++) {
            int v = 0;
#pragma unroll
            for (int a = 0; a < 7; a++) v += zz[r + a][c4 + b];
            col[b] = v;
        }
#pragma unroll
        for (int o = 0; o < 4; o++) {
            const int x = x0 + c4 + o;
            if (x >= s.w) continue;
            const int S = col[o] + col[o + 1] + col[o + 2] + col[o + 3] + col[o + 4] + col[o + 5] + col[o + 6];
            const bool m = S > CAMBI_MASK_HITS;
            out[(int64_t)(y0 + r) * s.w + x] = m ? yy[r + 3][c4 + o + 3] : (uint16_t)CAMBI_OUT;
            masked += m;
        }
    }
    const unsigned long long tot = block_sum_u64(masked, red);
    if (t == 0 && tot) {
        const int pi = ch == 0 ? plane_index.x : ch == 1 ? plane_index.y : ch == 2 ? plane_index.z : plane_index.w;
        atomicAdd(acc + ((int64_t)f * n_planes + pi) * CAMBI_WORDS + CAMBI_SCALES, tot);
    }
}

// grid = (blocks * count, n_frames); block = 256: the samples of scales 1..4, one after the other
__global__ __launch_bounds__(256) void k_cambi_decimate(cambi_levels lv, int blocks, int count, int n_planes, int4 plane_index,
                                                        uint16_t *__restrict__ pyr, unsigned long long *__restrict__ acc)
{
    __shared__ unsigned long long red[4];
    const int f = blockIdx.y;
    const int ch = blockIdx.x / blocks, blk = blockIdx.x % blocks;
    uint16_t *img = pyr + ((int64_t)f * count + ch) * lv.total;
    const int64_t i = (int64_t)blk * 256 + threadIdx.x + lv.off[1];   // a block lies in one scale: the offsets are multiples of 256
    const int64_t b = (int64_t)blk * 256 + lv.off[1];
    const int sc = b >= lv.off[4] ? 4 : b >= lv.off[3] ? 3 : b >= lv.off[2] ? 2 : 1;
    unsigned long long masked = 0;
    const int64_t k = i - lv.off[sc];
    if (k < (int64_t)lv.w[sc] * lv.h[sc]) {
        const int y = (int)(k / lv.w[sc]), x = (int)(k - (int64_t)y * lv.w[sc]);
        const uint16_t v = img[((int64_t)y << sc) * lv.w[0] + ((int64_t)x << sc)];
        img[i] = v;
        masked = v != CAMBI_OUT;
    }
    const unsigned long long tot = block_sum_u64(masked, red);
    if (threadIdx.x == 0 && tot) {
        const int pi = ch == 0 ? plane_index.x : ch == 1 ? plane_index.y : ch == 2 ? plane_index.z : plane_index.w;
        atomicAdd(acc + ((int64_t)f * n_planes + pi) * CAMBI_WORDS + CAMBI_SCALES + sc, tot);
    }
}

// grid = (tiles * count, n_frames); block = 256.  hist: [frame][slot][CAMBI_HIST_WORDS] uint32, zeroed by the caller
__global__ __launch_bounds__(256) void k_cambi_contrast(int w, int h, int64_t level_off, int64_t image_stride, int tiles_x,
                                                        int tiles, int count, const uint16_t *__restrict__ pyr,
                                                        unsigned *__restrict__ hist)
{
    constexpr int T = CAMBI_TILE, R = CAMBI_WINDOW / 2, LW = T + 2 * R;   // 32, 32, 96
    __shared__ uint16_t in[LW][LW];
    const int f = blockIdx.y;
    const int ch = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const int y0 = (tile / tiles_x) * T, x0 = (tile % tiles_x) * T;
    const int t = threadIdx.x;
    const int64_t slot = (int64_t)f * count + ch;
    const uint16_t *img = pyr + slot * image_stride + level_off;
    for (int i = t; i < LW * LW; i += 256) {
        const int a = i / LW, b = i - a * LW;
        const int y = y0 - R + a, x = x0 - R + b;
        in[a][b] = (y >= 0 && y < h && x >= 0 && x < w) ? img[(int64_t)y * w + x] : (uint16_t)CAMBI_OUT;
    }
    __syncthreads();
    unsigned *hs = hist + slot * CAMBI_HIST_WORDS;
    const int cx = t & 31, r0 = t >> 5;   // a wave: two tile rows
#pragma unroll 1
    for (int q = 0; q < 4; q++) {
        const int cy = r0 + 8 * q;
        const unsigned c = in[cy + R][cx + R];
        const bool masked = c != CAMBI_OUT;   // (a pixel outside the plane reads CAMBI_OUT as well)
        if (__ballot(masked) == 0) continue;   // the whole wave
        unsigned n[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        const unsigned base = c - 4u;   // (modulo 2^32: e below is y - c + 4 whether or not this wraps)
#pragma unroll 1
        for (int dy = 0; dy <= 2 * R; dy++) {
            const uint16_t *row = &in[cy + dy][cx];
            unsigned long long pk = 0;
#pragma unroll 13
            for (int dx = 0; dx <= 2 * R; dx++) {
                const unsigned e = (unsigned)row[dx] - base;   // 0..8 <=> y = c - 4 .. c + 4
                pk += e <= 8u ? 1ull << (7 * e) : 0ull;
            }
#pragma unroll
            for (int d = 0; d < 9; d++) n[d] += (unsigned)(pk >> (7 * d)) & 127u;
        }
        if (!masked) continue;
        const int y = y0 + cy, x = x0 + cx;
        const int ay = min(y + R, h - 1) - max(y - R, 0) + 1, ax = min(x + R, w - 1) - max(x - R, 0) + 1;
        const unsigned long long A = (unsigned long long)(ay * ax), n0 = n[4];
        unsigned long long u = 0;
#pragma unroll
        for (int k = 1; k <= 4; k++) {
#pragma unroll
            for (int sg = 0; sg < 2; sg++) {
                const unsigned long long nk = n[sg ? 4 + k : 4 - k];
                if (nk == 0) continue;
                const unsigned long long num = (unsigned long long)k * n0 * nk, den = (n0 + nk) * A;
                const unsigned long long v = ((num << 17) + den) / (2 * den);
                u = v > u ? v : u;
            }
        }
        if (u) atomicAdd(hs + u, 1u);   // u <= 65536
    }
}

// grid = (count, n_frames); block = 256.  Thread t owns bins 257 t .. 257 t + 256 (256 x 257 = CAMBI_HIST_WORDS >= 65537)
__global__ __launch_bounds__(256) void k_cambi_topk(int scale, unsigned long long K, int count, int n_planes, int4 plane_index,
                                                    const unsigned *__restrict__ hist, unsigned long long *__restrict__ acc)
{
    constexpr int CH = CAMBI_HIST_WORDS / 256;
    __shared__ unsigned long long cnt[256], sum[256];
    const int f = blockIdx.y, ch = blockIdx.x, t = threadIdx.x;
    const unsigned *hs = hist + ((int64_t)f * count + ch) * CAMBI_HIST_WORDS;
    unsigned long long c = 0, s = 0;
    for (int b = 0; b < CH; b++) {
        const unsigned long long v = hs[t * CH + b];
        c += v;
        s += v * (unsigned long long)(t * CH + b);
    }
    cnt[t] = c; sum[t] = s;
    __syncthreads();
    if (t != 0) return;
    unsigned long long left = K, top = 0;
    for (int g = 255; g >= 0 && left; g--) {
        if (cnt[g] <= left) { top += sum[g]; left -= cnt[g]; continue; }
        for (int b = CH - 1; b >= 0 && left; b--) {   // the chunk that holds the K-th largest
            const unsigned long long v = hs[g * CH + b];
            const unsigned long long take = v < left ? v : left;
            top += take * (unsigned long long)(g * CH + b);
            left -= take;
        }
    }
    const int pi = ch == 0 ? plane_index.x : ch == 1 ? plane_index.y : ch == 2 ? plane_index.z : plane_index.w;
    acc[((int64_t)f * n_planes + pi) * CAMBI_WORDS + scale] = top;
}

cambi_levels levels_of(int h, int w)
{
    cambi_levels lv;
    int64_t off = 0;
    for (int s = 0; s < CAMBI_SCALES; s++) {
        lv.w[s] = w; lv.h[s] = h; lv.off[s] = off;
        off += ((int64_t)w * h + 255) / 256 * 256;   // (k_cambi_decimate: a block lies in one scale)
        w = (w + 1) / 2; h = (h + 1) / 2;
    }
    lv.total = off;
    return lv;
}

} // namespace

size_t cambi_scratch_bytes(int count, int h, int w)
{
    return (size_t)count * ((size_t)levels_of(h, w).total * sizeof(uint16_t) + (size_t)CAMBI_HIST_WORDS * sizeof(unsigned));
}

int64_t cambi_top_count(int h, int w, int scale)
{
    const cambi_levels lv = levels_of(h, w);
    const int64_t k = 3 * ((int64_t)lv.h[scale] * lv.w[scale]) / 10;
    return k > 1 ? k : 1;
}

void launch_cambi(hipStream_t st, const uint8_t *frames, int n, int64_t frame_stride, const vqa_plane_desc *planes, const int *idx,
                  int count, int n_planes, int depth, void *scratch, unsigned long long *acc, cambi_mark mark, void *mark_ctx)
{
    if (n <= 0 || count <= 0) return;
    const vqa_plane_desc &pd = planes[idx[0]];
    cambi_src s;
    s.frames = frames; s.fs = frame_stride;
    int p4[4];
    group_slots(planes, idx, count, s.off, p4);
    s.row_stride = pd.row_stride; s.step = pd.pixel_step;
    s.w = pd.width; s.h = pd.height; s.depth = depth;
    const cambi_levels lv = levels_of(s.h, s.w);
    const int4 pi = make_int4(p4[0], p4[1], p4[2], p4[3]);
    uint16_t *pyr = (uint16_t *)scratch;
    unsigned *hist = (unsigned *)(pyr + (size_t)n * count * lv.total);   // lv.total is a multiple of 256: aligned
    const dim3 block(256);
    // the launches of one kernel id, between the caller's marks
    auto timed = [&](int id, auto &&launch) {
        mark(mark_ctx, id, 1);
        launch();
        mark(mark_ctx, id, 0);
    };
    {
        const int tiles_x = (s.w + 63) / 64, tiles = tiles_x * ((s.h + 15) / 16);
        const dim3 grid(tiles * count, n);
        timed(VQA_K_CAMBI_MASK, [&] {
            if (depth > 8)
                hipLaunchKernelGGL((k_cambi_mask<uint16_t>), grid, block, 0, st, s, lv, tiles_x, tiles, count, n_planes, pi, pyr, acc);
            else
                hipLaunchKernelGGL((k_cambi_mask<uint8_t>), grid, block, 0, st, s, lv, tiles_x, tiles, count, n_planes, pi, pyr, acc);
        });
    }
    {
        const int blocks = (int)((lv.total - lv.off[1]) / 256);
        timed(VQA_K_CAMBI_DECIMATE, [&] {
            hipLaunchKernelGGL(k_cambi_decimate, dim3(blocks * count, n), block, 0, st, lv, blocks, count, n_planes, pi, pyr, acc);
        });
    }
    const size_t hist_bytes = (size_t)n * count * CAMBI_HIST_WORDS * sizeof(unsigned);
    for (int sc = 0; sc < CAMBI_SCALES; sc++) {
        const int tiles_x = (lv.w[sc] + CAMBI_TILE - 1) / CAMBI_TILE, tiles = tiles_x * ((lv.h[sc] + CAMBI_TILE - 1) / CAMBI_TILE);
        timed(VQA_K_CAMBI_TOPK, [&] { (void)hipMemsetAsync(hist, 0, hist_bytes, st); });
        timed(VQA_K_CAMBI_CONTRAST, [&] {
            hipLaunchKernelGGL(k_cambi_contrast, dim3(tiles * count, n), block, 0, st, lv.w[sc], lv.h[sc], lv.off[sc], lv.total,
                               tiles_x, tiles, count, pyr, hist);
        });
        timed(VQA_K_CAMBI_TOPK, [&] {
            hipLaunchKernelGGL(k_cambi_topk, dim3(count, n), block, 0, st, sc, (unsigned long long)cambi_top_count(s.h, s.w, sc),
                               count, n_planes, pi, hist, acc);
        });
    }
}

// the ten words -> the record, on the host in double.  Contraction is off: the record is the formula vqa.h states.
void cambi_finalize(const unsigned long long *words, int h, int w, vqa_cambi_metrics *out)
{
#pragma clang fp contract(off)
    static const double wt[CAMBI_SCALES] = {16.0, 8.0, 4.0, 2.0, 1.0};
    double sum = 0.0;
    for (int s = 0; s < CAMBI_SCALES; s++) {
        out->top[s] = words[s];
        out->k[s] = cambi_top_count(h, w, s);
        out->masked[s] = (int64_t)words[CAMBI_SCALES + s];
        out->pool[s] = (double)out->top[s] / ((double)out->k[s] * 65536.0);
        sum = sum + wt[s] * out->pool[s];
    }
    out->cambi = sum / 31.0;
}

} // namespace vqa
