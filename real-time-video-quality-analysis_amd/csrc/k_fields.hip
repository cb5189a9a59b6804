// k_fields.hip — the kernels of vqa_fields_submit and vqa_weave_submit for gfx950, by the definitions stated in include/vqa.h.
// Integers only.
//
//   k_fields_accum<BPS>   the ten sums of ONE plane of frame i against its predecessor: comb, fwd, bwd, sad and changed, each per
//                row parity.  The frames ride in gridDim.y.  A lane owns a column chunk of 16 bytes (16 or 8 samples) and a band of
//                FIELDS_BAND_ROWS rows: it marches down the band and keeps rows y - 1, y, y + 1 of the frame and of its
//                predecessor as packed 16-byte registers, so inside a band every sample of either frame is loaded once and
//                serves all of its roles (above, centre, below); the two rows around a band are read by both neighbours.  The
//                byte model is two reads per sample.  A workgroup is lanes_x chunk columns by 256 / lanes_x bands.
//                A chunk that lies wholly inside its row is loaded as the two ALIGNED 16-byte words that hold it and realigned
//                in registers (k_conform_copy's dword select and v_alignbyte_b32); both words hold a byte of the row, so no
//                load touches a 16-byte granule the caller did not hand over.  The chunk at the end of a row, and every chunk
//                of a plane whose pixel step is not its sample size or whose 16-bit samples sit at odd addresses (the gather
//                path), is packed sample by sample; samples beyond the row are 0 in both frames and add 0 to every sum.
//                Overflow: one row of a chunk adds at most 16 * 4 * 255 (8 bits) or 8 * 4 * 65535 < 2^21 (16 bits) to a term, held
//                in 32 bits; the per-lane partials over the rows of a band are 64-bit, as are the wave's and the workgroup's.
//                Reduction: the wave by shuffles, the four waves through 40 LDS words, then ONE 64-bit vector atomic add per word
//                and workgroup (a zero is not sent).  Integer sums commute: the same frame gives the same words in any batch.
//   k_fields_weave<T>     out[j][p][y][x] = in[(y & 1 ? bottom : top)[j]][p][y][x] on k_conform_copy's plan: a lane owns an
//                aligned 16-byte granule of the DESTINATION, loads the two aligned source words that hold its bytes, realigns
//                and stores once; the granules at the two ends of a row go out sample by sample, so pad bytes are never
//                written.  Interleaved planes (bgr24) ride as one plane of 3 w samples.
//   k_fields_weave_gather<T>   the same function, a lane a sample, for other pixel steps.
#include "vqa_dev.hpp"
#include "vqa_kernels.hpp"

namespace vqa {

namespace {

// the 16 bytes at S out of the aligned words lo (at S & ~15) and hi (the next one; unused when S is aligned)
__device__ inline void realign16(const uint4 &lo, const uint4 &hi, unsigned ph, unsigned o[4])
{
    const unsigned q[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    const unsigned ds = ph >> 2, bs = ph & 3;
    unsigned t[5];
#pragma unroll
    for (int k = 0; k < 5; k++) t[k] = ds == 0 ? q[k] : ds == 1 ? q[k + 1] : ds == 2 ? q[k + 2] : q[(k + 3) & 7];
#pragma unroll
    for (int k = 0; k < 4; k++) o[k] = __builtin_amdgcn_alignbyte(t[k + 1], t[k], bs);
}

struct chunk { unsigned d[4]; };   // 16 / BPS samples of a row, packed as they lie in memory

template <int BPS> __device__ inline int sample_of(const chunk &c, int e)
{
    constexpr int PER = 4 / BPS;
    return (int)((c.d[e / PER] >> (8 * BPS * (e % PER))) & (BPS == 1 ? 0xffu : 0xffffu));
}

// samples x0 .. x0 + 16 / BPS - 1 of the row at `row` (w samples, `step` bytes apart); vec: step == BPS and the addresses allow
// aligned words
template <int BPS> __device__ inline chunk load_chunk(const uint8_t *row, int x0, int w, int step, bool vec)
{
    constexpr int SPG = 16 / BPS;
    chunk c;
    if (vec && x0 + SPG <= w) {
        const uintptr_t S = (uintptr_t)row + (uintptr_t)x0 * BPS;
        const unsigned ph = (unsigned)(S & 15);
        const uintptr_t A = S - ph;
        // bytes S .. S + 15 belong to the row: A holds S, and A + 16 holds S + 15 whenever ph > 0
        const uint4 lo = *(const uint4 *)A;
        const uint4 hi = ph ? *(const uint4 *)(A + 16) : make_uint4(0, 0, 0, 0);
        realign16(lo, hi, ph, c.d);
    } else {
        c.d[0] = c.d[1] = c.d[2] = c.d[3] = 0;
        constexpr int PER = 4 / BPS;
#pragma unroll
        for (int e = 0; e < SPG; e++) {
            if (x0 + e < w) {
                const uint8_t *s = row + (int64_t)(x0 + e) * step;
                const unsigned v = BPS == 1 ? (unsigned)*s : (unsigned)*(const uint16_t *)s;
                c.d[e / PER] |= v << (8 * BPS * (e % PER));
            }
        }
    }
    return c;
}

struct fields_job {
    const uint8_t *frames;   // the first sample of the plane in frame 0
    const uint8_t *prev0;    // the same of the frame before frame 0, or null
    int64_t fs, row_stride;
    int step, w, h;
    int lanes_x, col_blocks; // chunk columns of a workgroup; workgroups across a row
    int vec;
    unsigned long long *acc; // [n][FIELDS_WORDS], zeroed by the submit
};

// grid = (col_blocks * band groups, n frames); block = 256
template <int BPS> __global__ __launch_bounds__(256) void k_fields_accum(fields_job g)
{
    constexpr int SPG = 16 / BPS;
    __shared__ unsigned long long red[4][FIELDS_WORDS];
    const int t = threadIdx.x, j = blockIdx.y;
    const int sub = 256 / g.lanes_x;                                   // bands of a workgroup
    const int cb = blockIdx.x % g.col_blocks, bg = blockIdx.x / g.col_blocks;
    const int x0 = (cb * g.lanes_x + t % g.lanes_x) * SPG;
    const int b0 = (bg * sub + t / g.lanes_x) * FIELDS_BAND_ROWS;
    const int b1 = min(b0 + FIELDS_BAND_ROWS, g.h);
    const uint8_t *cur = g.frames + (int64_t)j * g.fs;
    const uint8_t *prv = j > 0 ? cur - g.fs : g.prev0;                 // (uniform)
    const bool vec = g.vec != 0;

    // [comb, fwd, bwd, sad, changed][parity]
    unsigned long long acc[FIELDS_WORDS];
#pragma unroll
    for (int k = 0; k < FIELDS_WORDS; k++) acc[k] = 0;

    if (x0 < g.w && b0 < g.h) {
        const chunk zero = {{0, 0, 0, 0}};
        auto row_of = [&](const uint8_t *f, int y) { return load_chunk<BPS>(f + (int64_t)y * g.row_stride, x0, g.w, g.step, vec); };
        chunk cu = b0 > 0 ? row_of(cur, b0 - 1) : zero, cm = row_of(cur, b0), cd;
        chunk pu = zero, pm = zero, pd = zero;
        if (prv) {
            if (b0 > 0) pu = row_of(prv, b0 - 1);
            pm = row_of(prv, b0);
        }
        for (int y = b0; y < b1; y++) {
            cd = y + 1 < g.h ? row_of(cur, y + 1) : zero;
            if (prv) pd = y + 1 < g.h ? row_of(prv, y + 1) : zero;
            const bool inner = y >= 2 && y < g.h - 2;
            unsigned comb = 0, fwd = 0, bwd = 0, sad = 0, chg = 0;     // one row of a chunk: below 2^21 each
#pragma unroll
            for (int e = 0; e < SPG; e++) {
                const int u = sample_of<BPS>(cu, e), m = sample_of<BPS>(cm, e), d = sample_of<BPS>(cd, e);
                if (inner) comb += (unsigned)abs(u + d - 2 * m);
                if (prv) {
                    const int q = sample_of<BPS>(pm, e);
                    if (inner) {
                        fwd += (unsigned)abs(u + d - 2 * q);
                        bwd += (unsigned)abs(sample_of<BPS>(pu, e) + sample_of<BPS>(pd, e) - 2 * m);
                    }
                    sad += (unsigned)abs(m - q);
                    chg += m != q;
                }
            }
            // (bands start at even rows: the parity of y is the workgroup's)
            if (y & 1) { acc[1] += comb; acc[3] += fwd; acc[5] += bwd; acc[7] += sad; acc[9] += chg; }
            else       { acc[0] += comb; acc[2] += fwd; acc[4] += bwd; acc[6] += sad; acc[8] += chg; }
            cu = cm; cm = cd;
            pu = pm; pm = pd;
        }
    }
#pragma unroll
    for (int k = 0; k < FIELDS_WORDS; k++) {
        const unsigned long long v = wave_sum(acc[k]);
        if (lane_id() == 0) red[wave_id()][k] = v;
    }
    __syncthreads();
    if (t < FIELDS_WORDS) {
        const unsigned long long v = red[0][t] + red[1][t] + red[2][t] + red[3][t];
        if (v) atomicAdd(g.acc + (size_t)j * FIELDS_WORDS + t, v);
    }
}

// ---- weave ------------------------------------------------------------------------------------------------------------------

// an aligned 16-byte word, if it holds a byte of [lo, hi)
__device__ inline uint4 load_if_inside(uintptr_t a, uintptr_t lo, uintptr_t hi)
{
    if (a + 16 > lo && a < hi) return *(const uint4 *)a;
    return make_uint4(0, 0, 0, 0);
}

// grid = (bands of destination rows, output frames, planes of the job); block = 256
template <typename T> __global__ __launch_bounds__(256) void k_fields_weave(weave_job s, int band_rows)
{
    constexpr int BPS = sizeof(T), SPG = 16 / BPS;
    const int p = blockIdx.z, j = blockIdx.y;
    const conform_plane &P = s.plane[p];
    const int r0 = blockIdx.x * band_rows;
    if (r0 >= P.h) return;                           // (uniform: the grid is sized for the tallest plane)
    const int rows = min(band_rows, P.h - r0);
    const uint8_t *src[2] = {s.src + (int64_t)s.top[j] * s.src_fs + P.src_off, s.src + (int64_t)s.bottom[j] * s.src_fs + P.src_off};
    uint8_t *dst = s.dst + (int64_t)j * s.dst_fs + P.dst_off;
    const int wbytes = P.w * BPS;
    const int gpr = (wbytes + 15 + 15) / 16;         // the most granules a row meets: its bytes plus the phase of its first one
    for (int i = threadIdx.x; i < rows * gpr; i += 256) {
        const int r = i / gpr, g = i - r * gpr, y = r0 + r;
        const uintptr_t d0 = (uintptr_t)(dst + (int64_t)y * P.dst_rs), d1 = d0 + wbytes;
        const uintptr_t s0 = (uintptr_t)((y & 1 ? src[1] : src[0]) + (int64_t)y * P.src_rs), s1 = s0 + wbytes;
        const uintptr_t D = (d0 & ~(uintptr_t)15) + (uintptr_t)g * 16;
        if (D >= d1) continue;
        const uintptr_t S = s0 + (D - d0);           // the source byte of the granule's first byte (may lie before s0)
        const unsigned ph = (unsigned)(S & 15);
        const uintptr_t A = S - ph;
        const uint4 lo = load_if_inside(A, s0, s1);
        const uint4 hi = ph ? load_if_inside(A + 16, s0, s1) : make_uint4(0, 0, 0, 0);
        unsigned o[4];
        realign16(lo, hi, ph, o);
        if (D >= d0 && D + 16 <= d1) {
            *(uint4 *)D = make_uint4(o[0], o[1], o[2], o[3]);
        } else if (BPS == 2 && !(d0 & 1)) {
            // an end of the row: its samples one by one
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

template <typename T> __global__ __launch_bounds__(256) void k_fields_weave_gather(weave_job s, int band_rows)
{
    const int p = blockIdx.z, j = blockIdx.y;
    const conform_plane &P = s.plane[p];
    const int r0 = blockIdx.x * band_rows;
    if (r0 >= P.h) return;
    const int rows = min(band_rows, P.h - r0);
    const uint8_t *src[2] = {s.src + (int64_t)s.top[j] * s.src_fs + P.src_off, s.src + (int64_t)s.bottom[j] * s.src_fs + P.src_off};
    uint8_t *dst = s.dst + (int64_t)j * s.dst_fs + P.dst_off;
    for (int i = threadIdx.x; i < rows * P.w; i += 256) {
        const int r = i / P.w, x = i - r * P.w, y = r0 + r;
        *(T *)(dst + (int64_t)y * P.dst_rs + (int64_t)x * P.dst_step) =
            *(const T *)((y & 1 ? src[1] : src[0]) + (int64_t)y * P.src_rs + (int64_t)x * P.src_step);
    }
}

template <typename T> void launch_weave_t(hipStream_t st, const weave_job &job, int n_out, int count, bool gather)
{
    int tallest = 1, widest = 1;
    for (int p = 0; p < count; p++) {
        tallest = job.plane[p].h > tallest ? job.plane[p].h : tallest;
        widest = job.plane[p].w > widest ? job.plane[p].w : widest;
    }
    // about 64 KB of destination bytes a workgroup, as k_conform_copy
    const int64_t rows = 65536 / ((int64_t)widest * (int)sizeof(T));
    const int br = (int)(rows < 1 ? 1 : rows);
    const dim3 grid((tallest + br - 1) / br, n_out, count), block(256);
    if (gather) hipLaunchKernelGGL((k_fields_weave_gather<T>), grid, block, 0, st, job, br);
    else hipLaunchKernelGGL((k_fields_weave<T>), grid, block, 0, st, job, br);
}

} // namespace

void launch_fields_accum(hipStream_t st, const uint8_t *frames, const uint8_t *prev0, int n, int64_t frame_stride,
                         const vqa_plane_desc &plane, int depth, unsigned long long *acc)
{
    const int bps = depth > 8 ? 2 : 1, spg = 16 / bps;
    fields_job g;
    g.frames = frames + plane.offset;
    g.prev0 = prev0 ? prev0 + plane.offset : nullptr;
    g.fs = frame_stride; g.row_stride = plane.row_stride; g.step = plane.pixel_step;
    g.w = plane.width; g.h = plane.height;
    // 16-bit samples at odd addresses would straddle a word's dwords: the gather takes them
    const bool odd = bps == 2 && (((uintptr_t)g.frames | (uintptr_t)g.prev0 | (uintptr_t)frame_stride | (uintptr_t)plane.row_stride) & 1);
    g.vec = plane.pixel_step == bps && !odd;
    const int chunks = (plane.width + spg - 1) / spg;
    int lanes_x = 1;                                 // a power of two: 256 / lanes_x bands a workgroup
    while (lanes_x < 256 && lanes_x < chunks) lanes_x *= 2;
    g.lanes_x = lanes_x;
    g.col_blocks = (chunks + lanes_x - 1) / lanes_x;
    g.acc = acc;
    const int bands = (plane.height + FIELDS_BAND_ROWS - 1) / FIELDS_BAND_ROWS, sub = 256 / lanes_x;
    const dim3 grid(g.col_blocks * ((bands + sub - 1) / sub), n), block(256);
    if (bps == 2) hipLaunchKernelGGL((k_fields_accum<2>), grid, block, 0, st, g);
    else hipLaunchKernelGGL((k_fields_accum<1>), grid, block, 0, st, g);
}

void launch_fields_weave(hipStream_t st, const weave_job &job, int n_out, int count, int depth, bool gather)
{
    if (n_out <= 0 || count <= 0) return;
    if (depth > 8) launch_weave_t<uint16_t>(st, job, n_out, count, gather);
    else launch_weave_t<uint8_t>(st, job, n_out, count, gather);
}

} // namespace vqa
