// k_convert.hip — the kernels of vqa_convert_submit for gfx950: ONE stream written at another sample depth and / or chroma
// layout, by the definition stated in include/vqa.h.  Per plane and per axis the relation is same, up (2x) or down (2x); the
// horizontal taps, then the vertical taps, both with weights that sum to 4 and no rounding in between, then the depth / range
// step with the one rounding.
//
//   k_convert_rows<Ts, Td, RX>   a pixel step equal to the sample size on both sides; RX is the horizontal relation of every
//                plane of the launch.  The planes ride in gridDim.z, the frames in gridDim.y, bands of UNITS in gridDim.x.  A
//                unit is the destination rows that the same two source rows A, B feed: one row, or - where the vertical relation
//                is up and the destination's row stride is a multiple of 16, so both rows cut into granules alike - the pair
//                (2u - 1, 2u), which both read source rows u - 1 and u: each source row is then loaded once for the pair.  A row
//                of the destination is cut into the 16-byte granules of its ADDRESS and a lane owns a granule, so every full
//                granule leaves as one aligned 16-byte store.  The source samples of a granule (16 / sizeof(Td) outputs: as
//                many, half as many plus the neighbours, or twice as many plus the neighbours) sit at an arbitrary byte phase:
//                the lane loads the ALIGNED 16-byte words that hold them and realigns in registers - a dword select by
//                phase / 4 and v_alignbyte_b32 by phase % 4 - because a 16-byte load at an address that is no multiple of 4
//                costs about twice as much.  A word is loaded only where it holds a byte of the plane's row AND
//                of the window.  The neighbour a LINEAR tap needs across a granule boundary is in the window's first or last
//                aligned word: nothing goes through LDS.  The granules at the two ends of a row are written sample by sample
//                with convert_at, the function the gather runs: pad bytes are never written.
//   k_convert_gather<Ts, Td>     the same function, a lane a sample, for any other pixel step on either side (interleaved chroma,
//                one channel of a packed pixel) and for 16-bit samples at odd addresses: the slow path, as in k_conform.
//
// No atomics, no reduction and no LDS: a destination sample is a function of its own source samples alone, so a frame gives the
// same bytes at any place of any batch.
#include <type_traits>

#include "vqa_dev.hpp"
#include "vqa_kernels.hpp"

namespace vqa {

namespace {

// v, the exact value with denominator 16 -> the output sample: the depth / range step and the one rounding (include/vqa.h)
__device__ inline unsigned convert_round(const convert_job &s, int v)
{
    // v <= 16 * 65535 < 2^21 and the depths differ by 8 at most: the limited-range values fit 32 bits
    const unsigned pd = (1u << s.dd) - 1, u = (unsigned)v;
    unsigned out;
    if (s.range == VQA_RANGE_LIMITED) {
        if (s.dd >= s.ds) out = ((u << (s.dd - s.ds)) + 8) >> 4;
        else out = (u + (1u << (3 + s.ds - s.dd))) >> (4 + s.ds - s.dd);
    } else {
        // (2 v Pd + 16 Ps) / (32 Ps) = floor(n / Ps) with n = floor((v Pd + 8 Ps) / 16), since Ps divides whole sixteenths:
        // n <= 65535^2 + 32767 fits 32 bits.  The float product misses a quotient that is a code of the destination (<= 65535)
        // by far less than 1, and the two steps below make it the floor; a quotient far above every peak is clipped as it is.
        const unsigned ps = (1u << s.ds) - 1;
        const unsigned n = (unsigned)(((unsigned long long)u * pd + 8ull * ps) >> 4);
        out = (unsigned)((float)n * s.inv_ps);
        if (out > 65536u) return pd;
        if (out * ps > n) out--;
        if ((out + 1) * ps <= n) out++;
    }
    return out > pd ? pd : out;
}

// the taps of one axis at output x, times 4: s(i) reads source sample i of the axis, already edge-replicated
template <class S> __device__ inline int convert_taps(int rel, bool linear, bool left, int x, S s)
{
    if (rel == CONVERT_SAME) return 4 * s(x);
    if (rel == CONVERT_UP) {
        const int h = x >> 1;
        if (!linear) return 4 * s(h);
        if (left) return (x & 1) ? 2 * s(h) + 2 * s(h + 1) : 4 * s(h);
        return 3 * s(h) + s((x & 1) ? h + 1 : h - 1);
    }
    if (linear && left) return s(2 * x - 1) + 2 * s(2 * x) + s(2 * x + 1);
    return 2 * s(2 * x) + 2 * s(2 * x + 1);
}

// destination sample (y, x) of plane P from the frame at `src`: any pixel step, one sample at a time
template <typename Ts> __device__ inline unsigned convert_at(const convert_job &s, const convert_plane &P, const uint8_t *src, int y, int x)
{
    const bool linear = s.chroma == VQA_CHROMA_LINEAR, left = s.siting == VQA_SITING_LEFT;
    auto row = [&](int r) {
        r = min(max(r, 0), P.sh - 1);
        const uint8_t *rp = src + P.src_off + (int64_t)r * P.src_rs;
        return convert_taps(P.rx, linear, left, x, [&](int i) {
            i = min(max(i, 0), P.sw - 1);
            return (int)*(const Ts *)(rp + (int64_t)i * P.src_step);
        });
    };
    return convert_round(s, convert_taps(P.ry, linear, false, y, row));   // (the vertical axis is always centre-sited)
}

// an aligned 16-byte word, if it holds a byte of [lo, hi)
__device__ inline uint4 convert_load_if_inside(uintptr_t a, uintptr_t lo, uintptr_t hi)
{
    if (a + 16 > lo && a < hi) return *(const uint4 *)a;
    return make_uint4(0, 0, 0, 0);
}

// The horizontal taps, times 4, of the SPG destination samples xf .. xf + SPG - 1 of a full granule (0 <= xf, xf + SPG <= dw)
// from the source row at [s0, s0 + sw sizeof(Ts)).
template <typename Ts, int SPG, int RX> __device__ inline void convert_hrow(uintptr_t s0, int sw, int xf, bool linear, bool left, int (&H)[SPG])
{
    constexpr int BS = sizeof(Ts);
    // the window of source samples [base, base + NW): what the SPG outputs read, the neighbours of LINEAR included.  up: the
    // window starts at the cell of the even sample xf - (xf & 1), so that the taps below index it by constants.
    constexpr int NW = RX == CONVERT_SAME ? SPG : RX == CONVERT_UP ? SPG / 2 + 3 : 2 * SPG + 1;
    constexpr int ND = (NW * BS + 3) / 4, NWORDS = (ND + 4 + 3) / 4;
    const int par = RX == CONVERT_UP ? (xf & 1) : 0;
    const int base = RX == CONVERT_SAME ? xf : RX == CONVERT_UP ? ((xf - par) >> 1) - 1 : 2 * xf - 1;
    const uintptr_t s1 = s0 + (uintptr_t)sw * BS;
    const uintptr_t S = s0 + (intptr_t)base * BS;   // (may lie one sample before s0)
    const unsigned ph = (unsigned)(S & 15);
    const uintptr_t A = S - ph;
    unsigned q[4 * NWORDS];
#pragma unroll
    for (int k = 0; k < NWORDS; k++) {
        uint4 wd = make_uint4(0, 0, 0, 0);
        if (16 * k < (int)ph + NW * BS) wd = convert_load_if_inside(A + 16 * k, s0, s1);   // (a word past the window is not loaded)
        q[4 * k] = wd.x; q[4 * k + 1] = wd.y; q[4 * k + 2] = wd.z; q[4 * k + 3] = wd.w;
    }
    // the dwords that hold the window, by phase / 4; then a byte shift by phase % 4
    const unsigned dsel = ph >> 2, bs = ph & 3;
    unsigned t[ND + 1];
#pragma unroll
    for (int k = 0; k < ND + 1; k++) t[k] = dsel == 0 ? q[k] : dsel == 1 ? q[k + 1] : dsel == 2 ? q[k + 2] : q[k + 3];
    int win[NW];
#pragma unroll
    for (int k = 0; k < NW; k++) {
        constexpr int PER = 4 / BS;
        const unsigned d = __builtin_amdgcn_alignbyte(t[k / PER + 1], t[k / PER], bs);
        win[k] = (int)((d >> (8 * BS * (k % PER))) & (BS == 1 ? 0xffu : 0xffffu));
    }
    // the edge is replicated: sample -1 reads sample 0 (base >= -1), samples sw .. read sample sw - 1
    if (RX != CONVERT_SAME) {
        if (base < 0) win[0] = win[1];
#pragma unroll
        for (int k = 1; k < NW; k++)
            if (base + k >= sw) win[k] = win[k - 1];
    }
    if (RX == CONVERT_SAME) {
#pragma unroll
        for (int e = 0; e < SPG; e++) H[e] = 4 * win[e];
    } else if (RX == CONVERT_UP) {
        // outputs j = 0 .. SPG of the even start xf - par: cell (j >> 1) + 1 of the window; output e is j = e + par
        const int wc_even = !linear ? 4 : left ? 4 : 3, wl_even = linear && !left ? 1 : 0;
        const int wc_odd = !linear ? 4 : left ? 2 : 3, wr_odd = !linear ? 0 : left ? 2 : 1;
        // (one value after the other, selected as values: a select between G[e] and G[e + 1] of an array becomes an indexed
        // load, and the array would live in scratch)
        auto G = [&](int j, int lo, int mid, int hi) { return (j & 1) ? wc_odd * mid + wr_odd * hi : wc_even * mid + wl_even * lo; };
        int prev = G(0, win[0], win[1], win[2]);
#pragma unroll
        for (int e = 0; e < SPG; e++) {
            const int c = ((e + 1) >> 1) + 1;
            const int next = G(e + 1, win[c - 1], win[c], win[c + 1 < NW ? c + 1 : c]);
            H[e] = par ? next : prev;
            prev = next;
        }
    } else {
        const int wl = linear && left ? 1 : 0, wr = linear && left ? 1 : 2;
#pragma unroll
        for (int e = 0; e < SPG; e++) H[e] = wl * win[2 * e] + 2 * win[2 * e + 1] + wr * win[2 * e + 2];
    }
}

// the destination rows of unit u of a plane (one or two), the source rows A, B that feed them and the weight of A in each (B's
// is 4 less that): the vertical taps of include/vqa.h, regrouped
struct convert_unit {
    int A, B, ny, y[2], wa[2];
};

__device__ inline convert_unit convert_unit_of(const convert_plane &P, bool linear, int u)
{
    convert_unit U;
    U.ny = 1; U.y[1] = 0; U.wa[1] = 4;
    if (P.pair) {
        // rows 2u - 1 (3 A + B, or 4 A) and 2u (A + 3 B, or 4 B) with A = c(u - 1), B = c(u); u = 0 .. sh
        U.A = max(u - 1, 0); U.B = min(u, P.sh - 1);
        const int lo = 2 * u - 1, hi = 2 * u, w = linear ? 3 : 4;
        const bool has_lo = lo >= 0 && lo < P.dh, has_hi = hi < P.dh;
        U.ny = (int)has_lo + (int)has_hi;
        U.y[0] = has_lo ? lo : hi; U.wa[0] = has_lo ? w : 4 - w;
        U.y[1] = hi; U.wa[1] = 4 - w;
        return U;
    }
    U.y[0] = u;
    if (P.ry == CONVERT_SAME) { U.A = U.B = u; U.wa[0] = 4; }
    else if (P.ry == CONVERT_UP) {
        U.A = u >> 1;
        U.B = min(max((u & 1) ? U.A + 1 : U.A - 1, 0), P.sh - 1);
        U.wa[0] = linear ? 3 : 4;
    } else {
        U.A = 2 * u; U.B = min(2 * u + 1, P.sh - 1); U.wa[0] = 2;
    }
    return U;
}

__host__ __device__ inline int convert_units(const convert_plane &P) { return P.pair ? P.sh + 1 : P.dh; }

template <typename Ts, typename Td, int RX>
__global__ __launch_bounds__(256) void k_convert_rows(convert_job s, int band_units)
{
    constexpr int BD = sizeof(Td), SPG = 16 / BD;   // destination samples per granule
    const int p = blockIdx.z, j = blockIdx.y;
    const convert_plane &P = s.plane[p];
    const int u0 = blockIdx.x * band_units, nu = convert_units(P);
    if (u0 >= nu) return;                            // (uniform: the grid is sized for the plane with the most units)
    const int units = min(band_units, nu - u0);
    const bool linear = s.chroma == VQA_CHROMA_LINEAR, left = s.siting == VQA_SITING_LEFT;
    const uint8_t *src = s.src + (int64_t)j * s.src_fs;
    uint8_t *dst = s.dst + (int64_t)j * s.dst_fs + P.dst_off;
    const int wbytes = P.dw * BD;
    // the most granules a row of this plane meets: its bytes plus the phase of its first one
    const int gpr = (wbytes + 15 + 15) / 16;
    for (int i = threadIdx.x; i < units * gpr; i += 256) {
        const int r = i / gpr, g = i - r * gpr;
        const convert_unit U = convert_unit_of(P, linear, u0 + r);
        if (!U.ny) continue;
        const uintptr_t d0 = (uintptr_t)(dst + (int64_t)U.y[0] * P.dst_rs), d1 = d0 + wbytes;
        const uintptr_t D = (d0 & ~(uintptr_t)15) + (uintptr_t)g * 16;
        if (D >= d1) continue;
        // (a pair's second row: dst_rs is a multiple of 16, so its granules are this row's, dst_rs further on)
        const int64_t step = U.ny > 1 ? (int64_t)(U.y[1] - U.y[0]) * P.dst_rs : 0;
        if (!(D >= d0 && D + 16 <= d1)) {
            // an end of the row: its samples one by one
#pragma unroll
            for (int e = 0; e < SPG; e++) {
                const uintptr_t a = D + BD * e;
                if (a < d0 || a + BD > d1) continue;
                const int x = (int)((a - d0) / BD);
#pragma unroll
                for (int k = 0; k < 2; k++)
                    if (k < U.ny) *(Td *)(a + (k ? step : 0)) = (Td)convert_at<Ts>(s, P, src, U.y[k], x);
            }
            continue;
        }
        const int xf = (int)((D - d0) / BD);
        const uintptr_t sp = (uintptr_t)(src + P.src_off);
        int HA[SPG], HB[SPG];
        convert_hrow<Ts, SPG, RX>(sp + (uintptr_t)((int64_t)U.A * P.src_rs), P.sw, xf, linear, left, HA);
        // (row B has no weight where every weight of A is 4, and is row A where the edge is replicated)
        const bool need_b = U.B != U.A && (U.wa[0] != 4 || (U.ny > 1 && U.wa[1] != 4));
        if (need_b) convert_hrow<Ts, SPG, RX>(sp + (uintptr_t)((int64_t)U.B * P.src_rs), P.sw, xf, linear, left, HB);
        else {
#pragma unroll
            for (int e = 0; e < SPG; e++) HB[e] = HA[e];
        }
#pragma unroll
        for (int k = 0; k < 2; k++) {
            if (k >= U.ny) break;
            const int wa = U.wa[k], wb = 4 - wa;
            unsigned o[4] = {0, 0, 0, 0};
#pragma unroll
            for (int e = 0; e < SPG; e++) o[e * BD / 4] |= convert_round(s, wa * HA[e] + wb * HB[e]) << (8 * BD * (e % (4 / BD)));
            *(uint4 *)(D + (k ? step : 0)) = make_uint4(o[0], o[1], o[2], o[3]);
        }
    }
}

template <typename Ts, typename Td>
__global__ __launch_bounds__(256) void k_convert_gather(convert_job s, int band_rows)
{
    const int p = blockIdx.z, j = blockIdx.y;
    const convert_plane &P = s.plane[p];
    const int r0 = blockIdx.x * band_rows;
    if (r0 >= P.dh) return;
    const int rows = min(band_rows, P.dh - r0);
    const uint8_t *src = s.src + (int64_t)j * s.src_fs;
    uint8_t *dst = s.dst + (int64_t)j * s.dst_fs + P.dst_off;
    for (int i = threadIdx.x; i < rows * P.dw; i += 256) {
        const int r = i / P.dw, x = i - r * P.dw, y = r0 + r;
        *(Td *)(dst + (int64_t)y * P.dst_rs + (int64_t)x * P.dst_step) = (Td)convert_at<Ts>(s, P, src, y, x);
    }
}

template <typename Ts, typename Td> void launch_convert_t(hipStream_t st, const convert_job &job, int n, int count, int rx, bool gather)
{
    // a band: about 64 KB of destination bytes a workgroup
    int widest = 1, most = 1;
    for (int p = 0; p < count; p++) {
        const convert_plane &P = job.plane[p];
        widest = P.dw > widest ? P.dw : widest;
        const int units = gather ? P.dh : convert_units(P);
        most = units > most ? units : most;
    }
    const int64_t fit = 65536 / ((int64_t)widest * (int64_t)sizeof(Td));
    const int band = (int)(fit < 1 ? 1 : fit);
    const dim3 grid((most + band - 1) / band, n, count), block(256);
    if (gather) hipLaunchKernelGGL((k_convert_gather<Ts, Td>), grid, block, 0, st, job, band);
    else if (rx == CONVERT_SAME) hipLaunchKernelGGL((k_convert_rows<Ts, Td, CONVERT_SAME>), grid, block, 0, st, job, band);
    else if (rx == CONVERT_UP) hipLaunchKernelGGL((k_convert_rows<Ts, Td, CONVERT_UP>), grid, block, 0, st, job, band);
    else hipLaunchKernelGGL((k_convert_rows<Ts, Td, CONVERT_DOWN>), grid, block, 0, st, job, band);
}

} // namespace

void launch_convert(hipStream_t st, const convert_job &job, int n, int count, int rx, bool gather)
{
    if (n <= 0 || count <= 0) return;
    const bool ws = job.ds > 8, wd = job.dd > 8;
    if (ws && wd) launch_convert_t<uint16_t, uint16_t>(st, job, n, count, rx, gather);
    else if (ws) launch_convert_t<uint16_t, uint8_t>(st, job, n, count, rx, gather);
    else if (wd) launch_convert_t<uint8_t, uint16_t>(st, job, n, count, rx, gather);
    else launch_convert_t<uint8_t, uint8_t>(st, job, n, count, rx, gather);
}

} // namespace vqa
