// k_sig.hip — clip-wide sync for gfx950: a 256-byte signature per frame and the squared distance between every distorted and
// every reference signature, by the definitions stated in include/vqa.h (vqa_sig_submit, vqa_sig_cross_submit).  Integers only.
//
//   k_sig<BPS>  A workgroup owns ONE (frame, cell row a): rows floor(a h / 16) .. floor((a + 1) h / 16) - 1 of the plane and all
//               16 cells along them, so it needs no global atomics: 16 64-bit sums in LDS, divided and written as 16 bytes by
//               its first 16 threads.  A thread owns chunks of 16 consecutive samples: chunk column cc (+ a multiple of the
//               columns a workgroup covers at once) on every `phases`-th row, so consecutive lanes read consecutive 16 (uint8)
//               or 32 (uint16) bytes of a row.  Which cells a chunk column feeds does not depend on the row.
//               The fast path - contiguous samples, w >= 256 (a cell is at least 16 samples wide, so a chunk meets at most two
//               cells: b0 and b0 + 1, split at a fixed sample), the chunk wholly inside the row - reads the chunk with one or
//               two 16-byte loads (unaligned where the row starts odd), four rows in flight, sums the samples below the split
//               and all samples (v_sad_u8 on masked dwords; masked halves for uint16) and keeps both in 64-bit registers until
//               the rows are done: two LDS atomics per chunk column.
//               Everything else - the last, partial chunk of a row, narrow planes, and every chunk of a plane whose
//               pixel_step is not its sample size (the slow path: a gather) - goes sample by sample, cell by cell, and adds a
//               run of samples of one cell to LDS when the cell changes.  No byte outside the w samples of a row is read, and
//               every sample is read exactly once.
//               Cell of column x: the largest b with floor(b w / 16) <= x, that is floor((16 x + 15) / w).
//
//   k_sig_diag, k_sig_best   D[j][i] = E_d[j] + E_r[i] - 2 C[j][i] with X = x - 128 (`x ^ 0x80` as a signed byte: the same shift
//               on both sides, so it cancels), E = sum X^2 <= 2^22 and the Gram tile C = sum_k X_d,j[k] X_r,i[k], |C| <= 2^22, by
//               four v_mfma_i32_16x16x64_i8 steps (K = 256) into one 32-bit accumulator.  Operands as in k_align.hip: lane l
//               holds signature l & 15 of its tile and the 16 bytes 64 s + 16 (l >> 4) .. of step s; A is the distorted tile
//               and B the reference tile, so by the C/D map (col = l & 15, row = 4 (l >> 4) + reg) register r of lane l is
//               C[16 jt + 4 (l >> 4) + r][16 it + (l & 15)].  E of a tile's 16 signatures comes from v_dot4 on the operands
//               already loaded: a lane sums its four 16-byte pieces, the four lane groups are joined by two xor-shuffles
//               (every lane then holds E of signature l & 15), and E_d of a register's row is fetched from lane 4 (l >> 4) + r.
//               Signatures that pad a tile to 16 are not read (their lanes hold X = 0) and their rows and columns are left out
//               of both results.
//               k_sig_diag: a wave owns one DIAGONAL OF TILES kt and walks (jt, jt + kt), (jt + 1, jt + kt + 1), ..  Register r of
//               lane l is always diagonal k = 16 kt + (l & 15) - 4 (l >> 4) - r, so its sum along the walk stays in a 64-bit
//               register; after the walk the 256 sums of a wave meet in 31 LDS words and leave through 31 64-bit global
//               atomics: their number grows with n_dist + n_ref, never with the product.
//               k_sig_best: a wave owns one STRIP of 16 distorted signatures (loaded once) and walks all reference tiles; a
//               register keeps min((D << 32) | i) over the columns it meets, in ascending i; 16 lanes are joined by four
//               xor-shuffles and each word of best is written once.  No atomics.
#include "vqa_kernels.hpp"

namespace vqa {

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));

constexpr int SIG_G = VQA_SIG_GRID;

struct sig_job {
    const uint8_t *frames;   // the first sample of the plane in frame 0
    int64_t fs, row_stride;
    int step;                // bytes from a sample to the next of its row
    int w, h, shift;         // shift: depth - 8
    uint8_t *out;            // [n][256]
};

// grid = (16 cell rows, n frames); block = 256
template <int BPS> __global__ __launch_bounds__(256) void k_sig(sig_job g)
{
    __shared__ unsigned long long cell[SIG_G];
    const int a = blockIdx.x, t = threadIdx.x;
    if (t < SIG_G) cell[t] = 0;
    __syncthreads();
    const int r0 = (int)((int64_t)a * g.h / SIG_G), r1 = (int)((int64_t)(a + 1) * g.h / SIG_G);
    const uint8_t *plane = g.frames + (int64_t)blockIdx.y * g.fs;
    const int chunks = (g.w + 15) / 16;
    const int cpb = chunks < 256 ? chunks : 256, phases = 256 / cpb;   // chunk columns and row phases of one sweep
    const int cc = t % cpb, ph = t / cpb;
    const bool wide = g.step == BPS && g.w >= 256;
    if (ph < phases) {
        for (int ch = cc; ch < chunks; ch += cpb) {
            const int x0 = 16 * ch;
            if (wide && x0 + 16 <= g.w) {
                const int b0 = (16 * x0 + 15) / g.w;                        // the cell of the chunk's first sample
                const int next = (int)((int64_t)(b0 + 1) * g.w / SIG_G);    // the first column of cell b0 + 1 (w for b0 = 15)
                const int split = next - x0 < 16 ? next - x0 : 16;           // samples 0 .. split - 1 belong to b0
                unsigned long long s_lo = 0, s_all = 0;
                const uint8_t *p = plane + (int64_t)x0 * BPS;
                if (BPS == 1) {
                    uint32_t m[4];   // the bytes below the split
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const int nb = split - 4 * k;
                        m[k] = nb >= 4 ? 0xffffffffu : (nb <= 0 ? 0u : (1u << (8 * nb)) - 1u);
                    }
                    for (int row = r0 + ph; row < r1; row += 4 * phases) {
                        uint32_t d[4][4];
#pragma unroll
                        for (int u = 0; u < 4; u++) {
                            const int rr = row + u * phases;
                            if (rr < r1)
                                __builtin_memcpy(d[u], p + (int64_t)rr * g.row_stride, 16);
                            else
                                d[u][0] = d[u][1] = d[u][2] = d[u][3] = 0;
                        }
                        uint32_t lo = 0, all = 0;
#pragma unroll
                        for (int u = 0; u < 4; u++)
#pragma unroll
                            for (int k = 0; k < 4; k++) {
                                lo = __builtin_amdgcn_sad_u8(d[u][k] & m[k], 0u, lo);
                                all = __builtin_amdgcn_sad_u8(d[u][k], 0u, all);
                            }
                        s_lo += lo;
                        s_all += all;
                    }
                } else {
                    uint32_t m[8];   // the halves below the split
#pragma unroll
                    for (int k = 0; k < 8; k++) {
                        const int nb = split - 2 * k;
                        m[k] = nb >= 2 ? 0xffffffffu : (nb == 1 ? 0xffffu : 0u);
                    }
                    for (int row = r0 + ph; row < r1; row += 4 * phases) {
                        uint32_t d[4][8];
#pragma unroll
                        for (int u = 0; u < 4; u++) {
                            const int rr = row + u * phases;
                            if (rr < r1)
                                __builtin_memcpy(d[u], p + (int64_t)rr * g.row_stride, 32);
                            else
#pragma unroll
                                for (int k = 0; k < 8; k++) d[u][k] = 0;
                        }
                        uint32_t lo = 0, all = 0;   // at most 64 samples of 65535 each
#pragma unroll
                        for (int u = 0; u < 4; u++)
#pragma unroll
                            for (int k = 0; k < 8; k++) {
                                const uint32_t v = d[u][k], vm = v & m[k];
                                all += (v & 0xffffu) + (v >> 16);
                                lo += (vm & 0xffffu) + (vm >> 16);
                            }
                        s_lo += lo;
                        s_all += all;
                    }
                }
                if (s_lo) atomicAdd(&cell[b0], s_lo);
                if (s_all != s_lo) atomicAdd(&cell[b0 + 1], s_all - s_lo);   // (split < 16 here, so b0 + 1 <= 15)
            } else {
                const int left = g.w - x0, nval = left < 16 ? left : 16;
                for (int row = r0 + ph; row < r1; row += phases) {
                    const uint8_t *p = plane + (int64_t)row * g.row_stride + (int64_t)x0 * g.step;
                    int cur = (16 * x0 + 15) / g.w;
                    uint32_t run = 0;
                    for (int k = 0; k < nval; k++) {
                        const uint8_t *s = p + (int64_t)k * g.step;
                        const uint32_t v = BPS == 1 ? (uint32_t)*s : (uint32_t)*(const uint16_t *)s;
                        const int b = (16 * (x0 + k) + 15) / g.w;
                        if (b != cur) {
                            if (run) atomicAdd(&cell[cur], (unsigned long long)run);
                            run = 0;
                            cur = b;
                        }
                        run += v;
                    }
                    if (run) atomicAdd(&cell[cur], (unsigned long long)run);
                }
            }
        }
    }
    __syncthreads();
    if (t < SIG_G) {
        const int c0 = (int)((int64_t)t * g.w / SIG_G), c1 = (int)((int64_t)(t + 1) * g.w / SIG_G);
        const unsigned long long cnt = (unsigned long long)(r1 - r0) * (unsigned long long)(c1 - c0);
        const unsigned long long q = cell[t] / (cnt << g.shift);
        g.out[(int64_t)blockIdx.y * VQA_SIG_BYTES + SIG_G * a + t] = (uint8_t)(q < 255 ? q : 255);
    }
}

// ---- the cross stage --------------------------------------------------------------------------------------------------------

// the four 16-byte pieces of signature 16 tile + (lane & 15) that lane `lane` feeds the four matrix steps, as signed bytes; a
// signature beyond n is not read and is X = 0
__device__ __forceinline__ void load_tile(const uint8_t *sig, int n, int tile, int lane, v4i x[4])
{
    const int f = 16 * tile + (lane & 15);
    if (f < n) {
        const v4i *p = (const v4i *)(sig + (int64_t)f * VQA_SIG_BYTES + 16 * (lane >> 4));
#pragma unroll
        for (int s = 0; s < 4; s++) x[s] = p[4 * s] ^ (int)0x80808080;
    } else {
#pragma unroll
        for (int s = 0; s < 4; s++) x[s] = v4i{0, 0, 0, 0};
    }
}

// E of signature 16 tile + (lane & 15), in every lane
__device__ __forceinline__ int tile_energy(const v4i x[4])
{
    int e = 0;
#pragma unroll
    for (int s = 0; s < 4; s++)
#pragma unroll
        for (int k = 0; k < 4; k++) e = __builtin_amdgcn_sdot4(x[s][k], x[s][k], e, false);
    e += __shfl_xor(e, 16);
    e += __shfl_xor(e, 32);
    return e;
}

// D of the tile (A: distorted, B: reference): d[r] = D[row 4 (lane >> 4) + r of A][column lane & 15 of B]
__device__ __forceinline__ void tile_distance(const v4i a[4], const v4i b[4], int ea, int eb, int lane, int d[4])
{
    v4i c = {0, 0, 0, 0};
#pragma unroll
    for (int s = 0; s < 4; s++) c = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[s], b[s], c, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; r++) d[r] = __shfl(ea, 4 * (lane >> 4) + r) + eb - 2 * c[r];
}

struct sigx_job {
    const uint8_t *dist, *ref;   // [n_dist][256], [n_ref][256], 16-byte aligned
    int n_dist, n_ref;
    unsigned long long *diag;    // [n_dist + n_ref - 1], zeroed by the submit
    unsigned long long *best;    // [n_dist]
};

// grid = ceil((Td + Tr - 1) / 4) with Td, Tr the tiles of either side; block = 256: wave v of workgroup b owns tile diagonal
// kt = 4 b + v - (Td - 1).  Every wave reaches both barriers.
__global__ __launch_bounds__(256) void k_sig_diag(sigx_job g)
{
    __shared__ unsigned long long bins[4][32];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int td = (g.n_dist + 15) / 16, tr = (g.n_ref + 15) / 16;
    const int kt = (int)blockIdx.x * 4 + wv - (td - 1);
    if (lane < 32) bins[wv][lane] = 0;
    __syncthreads();
    const int jt0 = kt < 0 ? -kt : 0, jt1 = td - 1 < tr - 1 - kt ? td - 1 : tr - 1 - kt;   // (empty for kt >= tr)
    unsigned long long sum[4] = {0, 0, 0, 0};
    for (int jt = jt0; jt <= jt1; jt++) {
        const int it = jt + kt;
        v4i a[4], b[4];
        load_tile(g.dist, g.n_dist, jt, lane, a);
        load_tile(g.ref, g.n_ref, it, lane, b);
        int d[4];
        tile_distance(a, b, tile_energy(a), tile_energy(b), lane, d);
        const bool has_r = 16 * it + (lane & 15) < g.n_ref;
#pragma unroll
        for (int r = 0; r < 4; r++)
            if (has_r && 16 * jt + 4 * (lane >> 4) + r < g.n_dist) sum[r] += (unsigned long long)d[r];
    }
#pragma unroll
    for (int r = 0; r < 4; r++)
        if (sum[r]) atomicAdd(&bins[wv][(lane & 15) - 4 * (lane >> 4) - r + 15], sum[r]);
    __syncthreads();
    if (lane < 31 && bins[wv][lane]) {
        // diagonal k = 16 kt + lane - 15 at word k + n_dist - 1; a non-zero bin names a pair of real frames, so the word exists
        const int64_t at = (int64_t)16 * kt + lane - 15 + g.n_dist - 1;
        if (at >= 0 && at < (int64_t)g.n_dist + g.n_ref - 1) atomicAdd(g.diag + at, bins[wv][lane]);
    }
}

// grid = ceil(Td / 4); block = 256: wave v of workgroup b owns distorted tile jt = 4 b + v.  No barrier.
__global__ __launch_bounds__(256) void k_sig_best(sigx_job g)
{
    const int lane = threadIdx.x & 63;
    const int td = (g.n_dist + 15) / 16, tr = (g.n_ref + 15) / 16;
    const int jt = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (jt >= td) return;   // (wave-uniform)
    v4i a[4];
    load_tile(g.dist, g.n_dist, jt, lane, a);
    const int ea = tile_energy(a);
    unsigned long long low[4] = {~0ull, ~0ull, ~0ull, ~0ull};
    for (int it = 0; it < tr; it++) {
        v4i b[4];
        load_tile(g.ref, g.n_ref, it, lane, b);
        int d[4];
        tile_distance(a, b, ea, tile_energy(b), lane, d);
        const int i = 16 * it + (lane & 15);
        if (i < g.n_ref) {
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const unsigned long long v = ((unsigned long long)(uint32_t)d[r] << 32) | (uint32_t)i;
                low[r] = v < low[r] ? v : low[r];
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
        unsigned long long v = low[r];
#pragma unroll
        for (int m = 1; m < 16; m <<= 1) {
            const unsigned long long o = __shfl_xor(v, m);
            v = o < v ? o : v;
        }
        const int j = 16 * jt + 4 * (lane >> 4) + r;
        if ((lane & 15) == 0 && j < g.n_dist) g.best[j] = v;
    }
}

} // namespace

void launch_sig(hipStream_t st, const uint8_t *frames, int n, int64_t frame_stride, const vqa_plane_desc &plane, int depth,
                uint8_t *out)
{
    sig_job g;
    g.frames = frames + plane.offset; g.fs = frame_stride; g.row_stride = plane.row_stride; g.step = plane.pixel_step;
    g.w = plane.width; g.h = plane.height; g.shift = depth - 8; g.out = out;
    const dim3 grid(SIG_G, n), block(256);
    if (depth > 8)
        hipLaunchKernelGGL((k_sig<2>), grid, block, 0, st, g);
    else
        hipLaunchKernelGGL((k_sig<1>), grid, block, 0, st, g);
}

static sigx_job cross_job(const uint8_t *dist_sig, int n_dist, const uint8_t *ref_sig, int n_ref, unsigned long long *diag,
                          unsigned long long *best)
{
    sigx_job g;
    g.dist = dist_sig; g.ref = ref_sig; g.n_dist = n_dist; g.n_ref = n_ref; g.diag = diag; g.best = best;
    return g;
}

void launch_sig_diag(hipStream_t st, const uint8_t *dist_sig, int n_dist, const uint8_t *ref_sig, int n_ref, unsigned long long *diag)
{
    const int td = (n_dist + 15) / 16, tr = (n_ref + 15) / 16;
    hipLaunchKernelGGL(k_sig_diag, dim3((td + tr - 1 + 3) / 4), dim3(256), 0, st, cross_job(dist_sig, n_dist, ref_sig, n_ref, diag, nullptr));
}

void launch_sig_best(hipStream_t st, const uint8_t *dist_sig, int n_dist, const uint8_t *ref_sig, int n_ref, unsigned long long *best)
{
    const int td = (n_dist + 15) / 16;
    hipLaunchKernelGGL(k_sig_best, dim3((td + 3) / 4), dim3(256), 0, st, cross_job(dist_sig, n_dist, ref_sig, n_ref, nullptr, best));
}

} // namespace vqa
