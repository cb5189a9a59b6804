// k_conform.hip — the kernels of vqa_conform_submit for gfx950: a registered copy of ONE stream, by the definition stated in
// include/vqa.h.  out[j][p][y][x] is a function of in[index[j]][p][y0_p + y][x0_p + x]: the window, the frame gather, then the
// per-plane table (LUT) and the 3 x 4 integer matrix where the submit has them.
//
//   k_conform_copy<T, LUT>   window, gather and table.  The planes of the job ride in gridDim.z, the output frames in gridDim.y,
//                bands of destination rows in gridDim.x.  A row of the destination is cut into the 16-byte granules of its
//                ADDRESS, so every full granule leaves as one aligned 16-byte store; a lane owns a granule.  The source bytes of
//                a granule sit at an arbitrary byte phase (an odd x0, packed bgr24, an odd plane offset): the lane loads the two
//                ALIGNED 16-byte words that hold them and realigns in registers - a dword select by phase / 4 and
//                v_alignbyte_b32 by phase % 4 - because a 16-byte load at an address that is no multiple of 4 costs about twice
//                as much.  An aligned word is loaded only where it holds a byte of the window's row, so no load
//                touches a 16-byte granule the caller did not hand over.  The granules at the two ends of a row are written
//                sample by sample: pad bytes are never written.  Planes that interleave (bgr24: pixel step 3 on both sides, the
//                same window) go out as ONE plane of 3 w samples, the table chosen by sample % 3.
//                LUT: 0 none; 1 the tables in LDS (depth <= 12: 8 KB a plane at most); 2 the tables read through L2.
//   k_conform_gather<T>      the same function, a lane a sample, for planes with a pixel step that is not the sample size
//                on either side and that do not interleave: the slow path, as in k_align.
//   k_conform_matrix<T, LUT> three planes taken together.  A lane owns a patch of SOURCE cells, 4 luma columns by one chroma row
//                (2 x 4 luma samples in 4:2:0), k_ciede's patch plan, so a chroma sample is loaded once for the luma outputs AND
//                the chroma outputs of its cell; it writes the luma samples of the patch that lie in plane 0's window and the
//                chroma samples that lie in the windows of planes 1 and 2.  Sums are 64-bit.
//
// No atomics and no reduction: a destination sample is a function of its own source samples alone, so a frame gives the same
// bytes at any place of any batch.
#include <type_traits>

#include "vqa_dev.hpp"
#include "vqa_kernels.hpp"

namespace vqa {

namespace {

// a sample above the peak reads the peak's entry (include/vqa.h): no table is read out of bounds
template <typename T> __device__ inline int lut_at(const T *tab, int v, int peak) { return (int)tab[min(v, peak)]; }

// an aligned 16-byte word, if it holds a byte of [lo, hi)
__device__ inline uint4 load_if_inside(uintptr_t a, uintptr_t lo, uintptr_t hi)
{
    if (a + 16 > lo && a < hi) return *(const uint4 *)a;
    return make_uint4(0, 0, 0, 0);
}

template <typename T, int LUT>
__global__ __launch_bounds__(256) void k_conform_copy(conform_job s, int band_rows)
{
    constexpr int BPS = sizeof(T), SPG = 16 / BPS;   // samples per granule
    __shared__ T tab[LUT == 1 ? CONFORM_LDS_SAMPLES * 3 : 1];
    const int p = blockIdx.z, j = blockIdx.y;
    const conform_plane &P = s.plane[p];
    const int r0 = blockIdx.x * band_rows;
    if (r0 >= P.h) return;                           // (uniform: the grid is sized for the tallest plane)
    const int rows = min(band_rows, P.h - r0), bins = s.peak + 1;
    if (LUT == 1) {
        for (int i = threadIdx.x; i < P.inter * bins; i += 256) tab[i] = ((const T *)s.lut)[(size_t)P.lut0 * bins + i];
        __syncthreads();
    }
    const T *gtab = LUT == 1 ? tab : (const T *)s.lut + (size_t)P.lut0 * bins;
    const int f = s.index ? s.index[j] : j;
    const uint8_t *src = s.src + (int64_t)f * s.src_fs + P.src_off + (int64_t)P.x0 * BPS;
    uint8_t *dst = s.dst + (int64_t)j * s.dst_fs + P.dst_off;
    const int wbytes = P.w * BPS;
    // the most granules a row of this plane meets: its bytes plus the phase of its first one
    const int gpr = (wbytes + 15 + 15) / 16;
    for (int i = threadIdx.x; i < rows * gpr; i += 256) {
        const int r = i / gpr, g = i - r * gpr, y = r0 + r;
        const uintptr_t d0 = (uintptr_t)(dst + (int64_t)y * P.dst_rs), d1 = d0 + wbytes;
        const uintptr_t s0 = (uintptr_t)(src + (int64_t)(P.y0 + y) * P.src_rs), s1 = s0 + wbytes;
        const uintptr_t D = (d0 & ~(uintptr_t)15) + (uintptr_t)g * 16;
        if (D >= d1) continue;
        const uintptr_t S = s0 + (D - d0);           // the source byte of the granule's first byte (may lie before s0)
        const unsigned ph = (unsigned)(S & 15);
        const uintptr_t A = S - ph;
        const uint4 lo = load_if_inside(A, s0, s1);
        const uint4 hi = ph ? load_if_inside(A + 16, s0, s1) : make_uint4(0, 0, 0, 0);
        // the five dwords that hold the granule, by phase / 4; then a byte shift by phase % 4
        const unsigned q[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        const unsigned ds = ph >> 2, bs = ph & 3;
        unsigned t[5];
#pragma unroll
        for (int k = 0; k < 5; k++) t[k] = ds == 0 ? q[k] : ds == 1 ? q[k + 1] : ds == 2 ? q[k + 2] : q[(k + 3) & 7];
        unsigned o[4];
#pragma unroll
        for (int k = 0; k < 4; k++) o[k] = __builtin_amdgcn_alignbyte(t[k + 1], t[k], bs);
        if (LUT) {
            // the sample index in the row of the granule's first sample picks the table of an interleaved plane
            const int x_first = (int)((intptr_t)(D - d0) / BPS);
            int c = P.inter > 1 ? ((x_first % P.inter) + P.inter) % P.inter : 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                unsigned v = 0;
#pragma unroll
                for (int e = 0; e < 4 / BPS; e++) {
                    const int sv = (int)((o[k] >> (8 * BPS * e)) & (BPS == 1 ? 0xffu : 0xffffu));
                    v |= (unsigned)lut_at(gtab + (size_t)c * bins, sv, s.peak) << (8 * BPS * e);
                    c = c + 1 == P.inter ? 0 : c + 1;
                }
                o[k] = v;
            }
        }
        if (D >= d0 && D + 16 <= d1) {
            *(uint4 *)D = make_uint4(o[0], o[1], o[2], o[3]);
        } else {
            // an end of the row: its samples one by one (the destination's samples are BPS-aligned with d0, not with D, where
            // d0 is odd: then the bytes go out one by one)
            if (BPS == 2 && !(d0 & 1)) {
#pragma unroll
                for (int e = 0; e < SPG; e++) {
                    const uintptr_t a = D + 2 * e;
                    if (a >= d0 && a + 2 <= d1) *(uint16_t *)a = (uint16_t)(o[e >> 1] >> (16 * (e & 1)));
                }
            } else {
#pragma unroll
                for (int e = 0; e < 16; e++) {
                    const uintptr_t a = D + e;
                    if (a >= d0 && a < d1) *(uint8_t *)a = (uint8_t)(o[e >> 2] >> (8 * (e & 3)));
                }
            }
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_conform_gather(conform_job s, int band_rows)
{
    const int p = blockIdx.z, j = blockIdx.y;
    const conform_plane &P = s.plane[p];
    const int r0 = blockIdx.x * band_rows;
    if (r0 >= P.h) return;
    const int rows = min(band_rows, P.h - r0), bins = s.peak + 1;
    const T *tab = s.lut ? (const T *)s.lut + (size_t)P.lut0 * bins : nullptr;
    const int f = s.index ? s.index[j] : j;
    const uint8_t *src = s.src + (int64_t)f * s.src_fs + P.src_off;
    uint8_t *dst = s.dst + (int64_t)j * s.dst_fs + P.dst_off;
    for (int i = threadIdx.x; i < rows * P.w; i += 256) {
        const int r = i / P.w, x = i - r * P.w, y = r0 + r;
        int v = (int)*(const T *)(src + (int64_t)(P.y0 + y) * P.src_rs + (int64_t)(P.x0 + x) * P.src_step);
        if (tab) v = lut_at(tab, v, s.peak);
        *(T *)(dst + (int64_t)y * P.dst_rs + (int64_t)x * P.dst_step) = (T)v;
    }
}

template <typename T, int LUT>
__global__ __launch_bounds__(256) void k_conform_matrix(conform_job s, conform_cells g)
{
    __shared__ T tab[LUT == 1 ? CONFORM_LDS_SAMPLES * 3 : 1];
    const int bins = s.peak + 1, j = blockIdx.y;
    if (LUT == 1) {
        for (int i = threadIdx.x; i < 3 * bins; i += 256) tab[i] = ((const T *)s.lut)[i];
        __syncthreads();
    }
    const T *gtab = LUT == 1 ? tab : (const T *)s.lut;
    const int tile = blockIdx.x, tx = tile % g.tiles_x, ty = tile / g.tiles_x;
    const int pc = tx * 64 + (threadIdx.x & 63), Cy = g.cy0 + ty * 4 + (threadIdx.x >> 6);
    if (pc >= g.patches || Cy >= g.cy1) return;
    const int sx = g.sx, sy = g.sy, ncell = 4 >> sx, nrow = 1 << sy;
    const int X0 = g.X0 + pc * 4, Y0 = Cy << sy;     // the patch's first luma sample, in source coordinates
    const int f = s.index ? s.index[j] : j;
    const uint8_t *src = s.src + (int64_t)f * s.src_fs;
    uint8_t *dst = s.dst + (int64_t)j * s.dst_fs;
    const conform_plane &P0 = s.plane[0], &P1 = s.plane[1], &P2 = s.plane[2];
    auto sample = [&](const conform_plane &P, int pl, int y, int x) {
        int v = (int)*(const T *)(src + P.src_off + (int64_t)y * P.src_rs + (int64_t)x * P.src_step);
        if (LUT) v = lut_at(gtab + (size_t)pl * bins, v, s.peak);
        return v;
    };
    auto mat = [&](int k, long long a, long long b, long long c) {
        const long long v = (s.m[k][0] * a + s.m[k][1] * b + s.m[k][2] * c + s.m[k][3] + 32768) >> 16;
        return (T)min(max(v, 0ll), (long long)s.peak);
    };
    // the luma samples of the patch that exist, after the table
    int lum[2][4];
#pragma unroll
    for (int r = 0; r < 2; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int Y = Y0 + r, X = X0 + c;
            lum[r][c] = r < nrow && Y < g.sh && X < g.sw ? sample(P0, 0, Y, X) : 0;
        }
#pragma unroll
    for (int q = 0; q < 4; q++) {
        if (q >= ncell) break;
        const int Xc = X0 + (q << sx);               // the cell's first luma column
        if (Xc >= g.sw) break;
        // (the chroma planes are the luma's size or its ceil-half per axis: the cell's chroma sample exists; min: the definition's)
        const int cx = min(Xc >> sx, g.cw - 1), cy = min(Cy, g.ch - 1);
        const int u = sample(P1, 1, cy, cx), v = sample(P2, 2, cy, cx);
        int sum = 0, cnt = 0;
#pragma unroll
        for (int r = 0; r < 2; r++)
#pragma unroll
            for (int c = 0; c < 2; c++) {
                if (r >= nrow || c >= (1 << sx)) continue;
                const int Y = Y0 + r, X = Xc + c, col = (q << sx) + c;
                if (Y >= g.sh || X >= g.sw) continue;
                const int l = col == 0 ? lum[r][0] : col == 1 ? lum[r][1] : col == 2 ? lum[r][2] : lum[r][3];
                sum += l;
                cnt++;
                const int oy = Y - P0.y0, ox = X - P0.x0;
                if (oy >= 0 && oy < P0.h && ox >= 0 && ox < P0.w)
                    *(T *)(dst + P0.dst_off + (int64_t)oy * P0.dst_rs + (int64_t)ox * P0.dst_step) = mat(0, l, u, v);
            }
        if (!cnt) continue;
        const int ybar = (sum + cnt / 2) / cnt;
        const int Ccx = Xc >> sx;
        int oy = Cy - P1.y0, ox = Ccx - P1.x0;
        if (oy >= 0 && oy < P1.h && ox >= 0 && ox < P1.w)
            *(T *)(dst + P1.dst_off + (int64_t)oy * P1.dst_rs + (int64_t)ox * P1.dst_step) = mat(1, ybar, u, v);
        oy = Cy - P2.y0; ox = Ccx - P2.x0;
        if (oy >= 0 && oy < P2.h && ox >= 0 && ox < P2.w)
            *(T *)(dst + P2.dst_off + (int64_t)oy * P2.dst_rs + (int64_t)ox * P2.dst_step) = mat(2, ybar, u, v);
    }
}

// the rows of a band: about 64 KB of destination bytes a workgroup (the tables of a workgroup are loaded once a band)
int band_rows_of(const conform_job &job, int count, int bps)
{
    int widest = 1;
    for (int p = 0; p < count; p++) widest = job.plane[p].w > widest ? job.plane[p].w : widest;
    const int64_t rows = 65536 / ((int64_t)widest * bps);
    return (int)(rows < 1 ? 1 : rows);
}

template <typename T> void launch_copy_t(hipStream_t st, const conform_job &job, int n_out, int count, int depth, bool gather)
{
    int tallest = 1;
    for (int p = 0; p < count; p++) tallest = job.plane[p].h > tallest ? job.plane[p].h : tallest;
    const int br = band_rows_of(job, count, (int)sizeof(T));
    const dim3 grid((tallest + br - 1) / br, n_out, count), block(256);
    if (gather) hipLaunchKernelGGL((k_conform_gather<T>), grid, block, 0, st, job, br);
    else if (!job.lut) hipLaunchKernelGGL((k_conform_copy<T, 0>), grid, block, 0, st, job, br);
    else if (depth <= CONFORM_LDS_DEPTH) hipLaunchKernelGGL((k_conform_copy<T, 1>), grid, block, 0, st, job, br);
    else hipLaunchKernelGGL((k_conform_copy<T, 2>), grid, block, 0, st, job, br);
}

template <typename T> void launch_matrix_t(hipStream_t st, const conform_job &job, const conform_cells &g, int n_out, int depth)
{
    const int tiles_y = (g.cy1 - g.cy0 + 3) / 4;
    const dim3 grid(g.tiles_x * tiles_y, n_out), block(256);
    if (!job.lut) hipLaunchKernelGGL((k_conform_matrix<T, 0>), grid, block, 0, st, job, g);
    else if (depth <= CONFORM_LDS_DEPTH) hipLaunchKernelGGL((k_conform_matrix<T, 1>), grid, block, 0, st, job, g);
    else hipLaunchKernelGGL((k_conform_matrix<T, 2>), grid, block, 0, st, job, g);
}

} // namespace

void launch_conform_copy(hipStream_t st, const conform_job &job, int n_out, int count, int depth, bool gather)
{
    if (n_out <= 0 || count <= 0) return;
    if (depth > 8) launch_copy_t<uint16_t>(st, job, n_out, count, depth, gather);
    else launch_copy_t<uint8_t>(st, job, n_out, count, depth, gather);
}

void launch_conform_matrix(hipStream_t st, const conform_job &job, int sh, int sw, int ch, int cw, int n_out, int depth)
{
    if (n_out <= 0) return;
    const conform_plane &P0 = job.plane[0], &P1 = job.plane[1], &P2 = job.plane[2];
    conform_cells g;
    g.sh = sh; g.sw = sw; g.ch = ch; g.cw = cw;
    g.sx = cw != sw; g.sy = ch != sh;
    // the source cells that hold a sample of any of the three windows
    const int cy_lo = min(P0.y0 >> g.sy, min(P1.y0, P2.y0));
    const int cy_hi = max(((P0.y0 + P0.h - 1) >> g.sy) + 1, max(P1.y0 + P1.h, P2.y0 + P2.h));
    const int x_lo = min(P0.x0, min(P1.x0, P2.x0) << g.sx), x_hi = max(P0.x0 + P0.w, max(P1.x0 + P1.w, P2.x0 + P2.w) << g.sx);
    g.cy0 = cy_lo; g.cy1 = cy_hi;
    g.X0 = x_lo & ~3;
    g.patches = (x_hi - g.X0 + 3) / 4;
    g.tiles_x = (g.patches + 63) / 64;
    if (depth > 8) launch_matrix_t<uint16_t>(st, job, g, n_out, depth);
    else launch_matrix_t<uint8_t>(st, job, g, n_out, depth);
}

} // namespace vqa
