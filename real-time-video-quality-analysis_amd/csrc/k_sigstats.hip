// k_sigstats.hip — signal statistics of one stream for gfx950: the exact histogram of every plane of every frame, its order
// statistics and level counts, the difference to the frame before, the bit masks and the dark-border box, by the definition
// stated in include/vqa.h (vqa_sigstats_submit).  Integers only: adds, min, max, or, compares.
//
//   k_sigstats_accum<T>  one launch per group of same-geometry planes of a sub-slice of frames.  A workgroup of 256 threads owns a
//                        256 x 32 tile: a thread reads four adjacent samples of eight rows of frame i and of frame i - 1, each
//                        sample of either frame ONCE, straight from global memory (one 4- or 8-byte load where the layout is
//                        planar and the address aligned, sample by sample otherwise - packed bgr24, odd offsets, the right edge).
//                        It adds sad and changed, ORs x and ~x (and_mask = ~OR(~x)), adds the tile's 32 row sums and 256 column
//                        sums into the entry's profile, and counts the samples into the entry's histogram:
//                          uint8   256 bins in LDS, eight interleaved sub-copies (k_gray_hist's scheme), flushed with one 32-bit
//                                  global atomic per non-empty bin and workgroup;
//                          uint16  65536 bins of 32 bits are 256 KiB and fit no LDS: 32-bit global vector atomics into the
//                                  entry's histogram in scratch, a thread's run of equal adjacent samples as ONE add.
//   k_sigstats_scan      one workgroup per (frame, plane).  It walks the histogram once - a wave reads 256 bins as one coalesced
//                        1 KiB access - for count, sum, sum_sq, min, max and the five level counts, keeping the count of every
//                        chunk of 256 bins in LDS; three waves then locate one order statistic each with two wave-wide prefix
//                        sums (the chunk of the rank, then the bin inside it); the row and column sums of the profile are
//                        compared with crop_level w and crop_level h for the box.
//
// Counters are 32 bits everywhere: a flat plane puts all N <= 2^28 samples into one bin, which no 16-bit counter holds from
// 65536 samples on.  Sums (vqa.h states the bounds): a thread's column sums (8 rows) and a row's tile sum (256 samples) of 16-bit
// samples stay below 2^24; the profile words, sum, sum_sq and sad are 64 bits.  Integer addition, or, min and max are associative
// and commutative: neither the tiling nor the order in which workgroups retire can change a bit.
#include <cmath>
#include <type_traits>

#include "vqa_dev.hpp"
#include "vqa_kernels.hpp"

namespace vqa {

namespace {

// the frames of one group of same-geometry planes; every stride in bytes
struct sig_src {
    const uint8_t *ref;     // frame 0 of the sub-slice
    const uint8_t *prev0;   // the frame before it, or nullptr
    int64_t fs;             // frame stride
    int64_t off[4];         // plane offsets inside a frame
    int64_t row_stride;
    int step;
    int w, h;
    int plane[4];           // the planes' indices in the submit
    int prof_off[4];        // words from the start of a frame's profile to the plane's row sums
};

constexpr int TW = 256, TH = 32;

// four adjacent samples of a row from x on, `nv` of them inside the plane (the others read as 0 and are never used)
template <typename T>
__device__ __forceinline__ void load4(const uint8_t *row, int x, int nv, int step, uint32_t v[4])
{
    const uint8_t *p = row + (int64_t)x * step;
    if (nv == 4 && step == (int)sizeof(T) && ((uintptr_t)p & (4 * sizeof(T) - 1)) == 0) {
        if (sizeof(T) == 1) {
            const uint32_t q = *(const uint32_t *)p;
            v[0] = q & 0xffu; v[1] = (q >> 8) & 0xffu; v[2] = (q >> 16) & 0xffu; v[3] = q >> 24;
        } else {
            const uint2 q = *(const uint2 *)p;
            v[0] = q.x & 0xffffu; v[1] = q.x >> 16; v[2] = q.y & 0xffffu; v[3] = q.y >> 16;
        }
        return;
    }
#pragma unroll
    for (int o = 0; o < 4; o++) v[o] = o < nv ? (uint32_t)*(const T *)(p + (int64_t)o * step) : 0u;
}

__device__ __forceinline__ uint32_t wave_or(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v |= __shfl_down(v, o, 64);
    return v; // valid in lane 0
}

// grid = (tiles * count, n_frames); block = 256.  hist: [frame][plane of the submit][bins] uint32, acc: [frame][plane]
// [SIGSTATS_WORDS] uint64, prof: [frame][prof_words] uint64 - all of the sub-slice, all zeroed by the submit
template <typename T>
__global__ __launch_bounds__(256) void k_sigstats_accum(sig_src s, int tiles_x, int tiles, int n_planes, int prof_words,
                                                        uint32_t *__restrict__ hist, unsigned long long *__restrict__ acc,
                                                        unsigned long long *__restrict__ prof)
{
    constexpr bool IN_LDS = sizeof(T) == 1;
    constexpr int BINS = IN_LDS ? 256 : 65536;
    __shared__ uint32_t lh[IN_LDS ? 256 * 8 : 1];
    __shared__ uint32_t colsum[4][TW];
    __shared__ uint32_t rowsum[TH];
    __shared__ unsigned long long red[4][2];
    __shared__ uint32_t msk[4][2];
    const int f = blockIdx.y;
    const bool has_prev = f > 0 || s.prev0 != nullptr;   // (the whole workgroup)
    const int ch = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const int y0 = (tile / tiles_x) * TH, x0 = (tile % tiles_x) * TW;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int64_t entry = (int64_t)f * n_planes + s.plane[ch];
    uint32_t *gh = hist + entry * BINS;
    if (IN_LDS) {
        for (int i = t; i < 256 * 8; i += 256) lh[i] = 0;
        __syncthreads();
    }
    const uint8_t *pc = s.ref + (int64_t)f * s.fs + s.off[ch];
    const uint8_t *pp = has_prev ? (f == 0 ? s.prev0 : s.ref + (int64_t)(f - 1) * s.fs) + s.off[ch] : nullptr;
    const int x = x0 + 4 * lane;
    const int nv = min(max(s.w - x, 0), 4);
    uint32_t cs[4] = {0, 0, 0, 0}, orm = 0, nand = 0;
    unsigned long long sad = 0, changed = 0;
    for (int k = 0; k < TH / 4; k++) {
        const int row = wv + 4 * k, y = y0 + row;   // (wave-uniform)
        if (y >= s.h) break;
        uint32_t v[4] = {0, 0, 0, 0}, u[4] = {0, 0, 0, 0};
        if (nv > 0) {
            load4<T>(pc + (int64_t)y * s.row_stride, x, nv, s.step, v);
            if (has_prev) load4<T>(pp + (int64_t)y * s.row_stride, x, nv, s.step, u);
        }
        uint32_t rs = 0;
#pragma unroll
        for (int o = 0; o < 4; o++) {
            if (o < nv) {
                rs += v[o];
                cs[o] += v[o];
                orm |= v[o];
                nand |= ~v[o];
                if (has_prev) {
                    sad += v[o] > u[o] ? v[o] - u[o] : u[o] - v[o];
                    changed += v[o] != u[o];
                }
                if (IN_LDS) atomicAdd(&lh[(v[o] << 3) | (t & 7)], 1u);
            }
        }
        if (!IN_LDS && nv > 0) {
            // a run of equal adjacent samples is one add
            uint32_t rv = v[0], rc = 1;
#pragma unroll
            for (int o = 1; o < 4; o++) {
                if (o < nv) {
                    if (v[o] == rv) {
                        rc++;
                    } else {
                        atomicAdd(&gh[rv], rc);
                        rv = v[o];
                        rc = 1;
                    }
                }
            }
            atomicAdd(&gh[rv], rc);
        }
        rs = wave_sum(rs);
        if (lane == 0) rowsum[row] = rs;
    }
#pragma unroll
    for (int o = 0; o < 4; o++) colsum[wv][4 * lane + o] = cs[o];
    const unsigned long long a0 = wave_sum(sad), a1 = wave_sum(changed);
    const uint32_t m0 = wave_or(orm), m1 = wave_or(nand);
    if (lane == 0) {
        red[wv][0] = a0; red[wv][1] = a1;
        msk[wv][0] = m0; msk[wv][1] = m1;
    }
    __syncthreads();
    unsigned long long *pr = prof + (int64_t)f * prof_words + s.prof_off[ch];   // h row sums, then w column sums
    if (x0 + t < s.w) {
        const uint32_t c = colsum[0][t] + colsum[1][t] + colsum[2][t] + colsum[3][t];
        if (c) atomicAdd(pr + s.h + x0 + t, (unsigned long long)c);
    }
    if (t < TH && y0 + t < s.h && rowsum[t]) atomicAdd(pr + y0 + t, (unsigned long long)rowsum[t]);
    if (IN_LDS) {
        uint32_t c = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) c += lh[(t << 3) | k];
        if (c) atomicAdd(&gh[t], c);
    }
    if (t == 0) {
        unsigned long long *a = acc + entry * SIGSTATS_WORDS;
        atomicOr(a + SIG_OR, (unsigned long long)(msk[0][0] | msk[1][0] | msk[2][0] | msk[3][0]));
        atomicOr(a + SIG_NAND, (unsigned long long)(msk[0][1] | msk[1][1] | msk[2][1] | msk[3][1]));
        if (has_prev) {
            atomicAdd(a + SIG_SAD, red[0][0] + red[1][0] + red[2][0] + red[3][0]);
            atomicAdd(a + SIG_CHANGED, red[0][1] + red[1][1] + red[2][1] + red[3][1]);
        }
    }
}

struct sig_scan {
    int n_planes, bins, prof_words;
    int w[4], h[4], prof_off[4];
    uint32_t black, t16, t235, t240, peak;
    unsigned long long crop;
};

// b: the counts of this lane's four consecutive slots, slot 4 lane + j; the slots of the wave in lane order hold `k` or more in
// all, k >= 1.  -> idx: the slot where the running count first reaches k; rem: k less the count before that slot (the whole wave)
__device__ __forceinline__ void wave_pick(const uint32_t b[4], uint32_t k, int &idx, uint32_t &rem)
{
    const int lane = threadIdx.x & 63;
    const uint32_t sum = b[0] + b[1] + b[2] + b[3];
    uint32_t incl = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    const uint32_t excl = incl - sum;
    const bool hit = excl < k && k <= incl;
    uint32_t r = k - excl;
    int j = 0;
#pragma unroll
    for (int q = 0; q < 3; q++)
        if (j == q && r > b[q]) { r -= b[q]; j = q + 1; }
    const unsigned long long who = __ballot(hit);
    const int src = who ? __ffsll((long long)who) - 1 : 0;
    idx = __shfl(4 * lane + j, src, 64);
    rem = __shfl(r, src, 64);
}

// grid = entries of the sub-slice; block = 256.  The words accum does not write are stored here, each once.
__global__ __launch_bounds__(256) void k_sigstats_scan(sig_scan g, const uint32_t *__restrict__ hist,
                                                       const unsigned long long *__restrict__ prof,
                                                       unsigned long long *__restrict__ acc)
{
    __shared__ uint32_t ccnt[256];
    __shared__ unsigned long long red[4][8];
    __shared__ uint32_t ext[4][2];
    __shared__ int box[4];
    __shared__ uint32_t stat[3];
    const int e = blockIdx.x, p = e % g.n_planes, f = e / g.n_planes;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const uint32_t *hh = hist + (int64_t)e * g.bins;
    const int chunks = g.bins >> 8, w = g.w[p], h = g.h[p];
    ccnt[t] = 0;
    if (t == 0) { box[0] = h; box[1] = -1; box[2] = w; box[3] = -1; }
    __syncthreads();
    unsigned long long cnt = 0, sum = 0, sq = 0, lv[5] = {0, 0, 0, 0, 0};
    uint32_t mn = 0xffffffffu, mx = 0;
    for (int c = wv; c < chunks; c += 4) {
        const uint32_t v0 = (uint32_t)c * 256u + 4u * lane;
        const uint4 q = *(const uint4 *)(hh + v0);
        const uint32_t b[4] = {q.x, q.y, q.z, q.w};
        uint32_t here = 0;
#pragma unroll
        for (int o = 0; o < 4; o++) {
            const unsigned long long n = b[o], v = v0 + o;
            if (n) {
                here += b[o];
                sum += n * v;
                sq += n * v * v;
                mn = min(mn, v0 + o);
                mx = max(mx, v0 + o);
                lv[0] += v < g.black ? n : 0;
                lv[1] += v < g.t16 ? n : 0;
                lv[2] += v > g.t235 ? n : 0;
                lv[3] += v > g.t240 ? n : 0;
                lv[4] += v > g.peak ? n : 0;
            }
        }
        cnt += here;
        here = wave_sum(here);
        if (lane == 0) ccnt[c] = here;
    }
    {
        const unsigned long long r0 = wave_sum(cnt), r1 = wave_sum(sum), r2 = wave_sum(sq), r3 = wave_sum(lv[0]),
                                 r4 = wave_sum(lv[1]), r5 = wave_sum(lv[2]), r6 = wave_sum(lv[3]), r7 = wave_sum(lv[4]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            mn = min(mn, (uint32_t)__shfl_down(mn, o, 64));
            mx = max(mx, (uint32_t)__shfl_down(mx, o, 64));
        }
        if (lane == 0) {
            red[wv][0] = r0; red[wv][1] = r1; red[wv][2] = r2; red[wv][3] = r3;
            red[wv][4] = r4; red[wv][5] = r5; red[wv][6] = r6; red[wv][7] = r7;
            ext[wv][0] = mn; ext[wv][1] = mx;
        }
    }
    // the box: the first and the last row and column whose sum is above the dark level
    const unsigned long long *pr = prof + (int64_t)f * g.prof_words + g.prof_off[p];
    {
        int lo = h, hi = -1;
        const unsigned long long lim = g.crop * (unsigned long long)w;
        for (int r = t; r < h; r += 256)
            if (pr[r] > lim) { lo = min(lo, r); hi = max(hi, r); }
        if (hi >= 0) { atomicMin(&box[0], lo); atomicMax(&box[1], hi); }
        lo = w; hi = -1;
        const unsigned long long limc = g.crop * (unsigned long long)h;
        for (int c = t; c < w; c += 256)
            if (pr[h + c] > limc) { lo = min(lo, c); hi = max(hi, c); }
        if (hi >= 0) { atomicMin(&box[2], lo); atomicMax(&box[3], hi); }
    }
    __syncthreads();
    // wave r: the smallest v with C(v) >= k_r
    if (wv < 3) {
        const unsigned long long n = (unsigned long long)w * h;
        const uint32_t k = (uint32_t)(wv == 0 ? (n + 9) / 10 : wv == 1 ? (n + 1) / 2 : (9 * n + 9) / 10);
        const uint32_t b[4] = {ccnt[4 * lane], ccnt[4 * lane + 1], ccnt[4 * lane + 2], ccnt[4 * lane + 3]};
        int chunk, bin;
        uint32_t rem, rest;
        wave_pick(b, k, chunk, rem);
        chunk = min(chunk, chunks - 1);   // (a histogram that holds fewer than k samples cannot occur; stay inside it anyway)
        const uint4 q = *(const uint4 *)(hh + (uint32_t)chunk * 256u + 4u * lane);
        const uint32_t d[4] = {q.x, q.y, q.z, q.w};
        wave_pick(d, rem, bin, rest);
        if (lane == 0) stat[wv] = (uint32_t)chunk * 256u + (uint32_t)bin;
    }
    __syncthreads();
    if (t == 0) {
        unsigned long long *a = acc + (int64_t)e * SIGSTATS_WORDS;
        unsigned long long tot[8];
#pragma unroll
        for (int k = 0; k < 8; k++) tot[k] = red[0][k] + red[1][k] + red[2][k] + red[3][k];
        a[SIG_COUNT] = tot[0];
        a[SIG_SUM] = tot[1];
        a[SIG_SUM_SQ] = tot[2];
        a[SIG_MIN] = min(min(ext[0][0], ext[1][0]), min(ext[2][0], ext[3][0]));
        a[SIG_MAX] = max(max(ext[0][1], ext[1][1]), max(ext[2][1], ext[3][1]));
        a[SIG_LOW] = stat[0];
        a[SIG_MEDIAN] = stat[1];
        a[SIG_HIGH] = stat[2];
        a[SIG_BELOW_BLACK] = tot[3];
        a[SIG_UNDER] = tot[4];
        a[SIG_OVER_LUMA] = tot[5];
        a[SIG_OVER_CHROMA] = tot[6];
        a[SIG_ABOVE_PEAK] = tot[7];
        a[SIG_TOP] = (unsigned long long)(long long)box[0];
        a[SIG_BOTTOM] = (unsigned long long)(long long)box[1];
        a[SIG_LEFT] = (unsigned long long)(long long)box[2];
        a[SIG_RIGHT] = (unsigned long long)(long long)box[3];
    }
}

} // namespace

void launch_sigstats_accum(hipStream_t st, const uint8_t *ref, const uint8_t *prev0, int n, int64_t frame_stride,
                           const vqa_plane_desc *planes, const int *idx, int count, int n_planes, int depth,
                           const int *prof_off, int prof_words, uint32_t *hist, unsigned long long *acc, unsigned long long *prof)
{
    if (n <= 0 || count <= 0) return;
    const vqa_plane_desc &pd = planes[idx[0]];
    sig_src s;
    s.ref = ref; s.prev0 = prev0; s.fs = frame_stride;
    group_slots(planes, idx, count, s.off, s.plane);
    for (int i = 0; i < 4; i++) s.prof_off[i] = prof_off[s.plane[i]];
    s.row_stride = pd.row_stride; s.step = pd.pixel_step;
    s.w = pd.width; s.h = pd.height;
    const int tiles_x = (s.w + TW - 1) / TW, tiles = tiles_x * ((s.h + TH - 1) / TH);
    const dim3 grid(tiles * count, n), block(256);
    if (depth > 8)
        hipLaunchKernelGGL((k_sigstats_accum<uint16_t>), grid, block, 0, st, s, tiles_x, tiles, n_planes, prof_words, hist, acc, prof);
    else
        hipLaunchKernelGGL((k_sigstats_accum<uint8_t>), grid, block, 0, st, s, tiles_x, tiles, n_planes, prof_words, hist, acc, prof);
}

void launch_sigstats_scan(hipStream_t st, int n, const vqa_plane_desc *planes, int n_planes, int depth, int black_level,
                          int crop_level, const int *prof_off, int prof_words, const uint32_t *hist,
                          const unsigned long long *prof, unsigned long long *acc)
{
    if (n <= 0) return;
    sig_scan g;
    g.n_planes = n_planes; g.bins = sigstats_bins(depth); g.prof_words = prof_words;
    for (int p = 0; p < 4; p++) {
        const int q = p < n_planes ? p : 0;
        g.w[p] = planes[q].width; g.h[p] = planes[q].height; g.prof_off[p] = prof_off[q];
    }
    const uint32_t sc = 1u << (depth - 8);
    g.black = (uint32_t)black_level; g.t16 = 16u * sc; g.t235 = 235u * sc; g.t240 = 240u * sc; g.peak = (1u << depth) - 1u;
    g.crop = (unsigned long long)crop_level;
    hipLaunchKernelGGL(k_sigstats_scan, dim3(n * n_planes), dim3(256), 0, st, g, hist, prof, acc);
}

// the words -> the record, and the three doubles of include/vqa.h on the host.  Contraction is off: `a - m m` as one fused
// operation would not be the formula vqa.h states.
void sigstats_finalize(const unsigned long long *w, int depth, vqa_sigstats_metrics *out)
{
#pragma clang fp contract(off)
    out->count = (int64_t)w[SIG_COUNT];
    out->sum = w[SIG_SUM];
    out->sum_sq = w[SIG_SUM_SQ];
    out->min = (uint32_t)w[SIG_MIN]; out->max = (uint32_t)w[SIG_MAX];
    out->low = (uint32_t)w[SIG_LOW]; out->median = (uint32_t)w[SIG_MEDIAN]; out->high = (uint32_t)w[SIG_HIGH];
    const uint32_t type_mask = depth > 8 ? 0xffffu : 0xffu;
    out->or_mask = (uint32_t)w[SIG_OR] & type_mask;
    out->and_mask = ~(uint32_t)w[SIG_NAND] & type_mask;
    out->bits_used = out->or_mask ? depth - __builtin_ctz(out->or_mask) : 0;
    out->below_black = w[SIG_BELOW_BLACK];
    out->under = w[SIG_UNDER];
    out->over_luma = w[SIG_OVER_LUMA];
    out->over_chroma = w[SIG_OVER_CHROMA];
    out->above_peak = w[SIG_ABOVE_PEAK];
    out->sad = w[SIG_SAD];
    out->changed = w[SIG_CHANGED];
    out->top = (int32_t)(int64_t)w[SIG_TOP]; out->bottom = (int32_t)(int64_t)w[SIG_BOTTOM];
    out->left = (int32_t)(int64_t)w[SIG_LEFT]; out->right = (int32_t)(int64_t)w[SIG_RIGHT];
    const double n = (double)out->count;
    out->mean = (double)out->sum / n;
    const double mm = out->mean * out->mean;
    const double var = (double)out->sum_sq / n - mm;
    out->stdev = std::sqrt(var > 0.0 ? var : 0.0);
    out->dif = (double)out->sad / n;
}

} // namespace vqa
