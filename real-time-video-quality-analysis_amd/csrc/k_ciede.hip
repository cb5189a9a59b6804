// k_ciede.hip — CIEDE2000 for gfx950: the colour difference dE00 of every pixel of a frame pair, the three planes taken together,
// by the definition stated in include/vqa.h (vqa_ciede_submit).
//
//   k_ciede<T, MODEL, VEC>   one fused launch per submit.  ONE THREAD OWNS A 2 x 4 LUMA PATCH of both images: the patches of a
//                        frame are numbered in raster order and a workgroup of 64 threads (one wave) owns 64 consecutive
//                        numbers - a tiling that depends on the geometry alone.  A thread reads its two rows of four samples
//                        of every plane once - with halved chroma two samples per row, and with halved chroma height one row,
//                        so a 4:2:0 chroma sample is loaded once for its four luma samples - as one load per row when the layout
//                        allows it (VEC: unit pixel step, aligned rows, a width that is a multiple of 4: 4 or 8 bytes of luma, 2
//                        to 8 of chroma) and sample by sample otherwise (packed BGR, odd widths, windows).  The rows stay packed
//                        in 64-bit registers, four 16-bit fields each, and ONE loop that is not unrolled walks the eight pixels:
//                        the body - two Lab conversions (three pow and three cbrt each) and dE00 (two atan2, four cos, two sin,
//                        one exp, about ten sqrt) - is a few thousand instructions, and eight copies of it would not fit the
//                        instruction cache.  There is no LDS and no barrier.
//
// Transcendentals: the accurate library forms (powf, cbrtf, atan2f, sinf, cosf, expf).  a = 500 (f(X) - f(Y)) cancels on
// near-gray pixels - most of a video frame - so an error of a few ulp in the sRGB power shows up five hundred times larger in a;
// the cheaper exp2 / log2 forms are left for a version that has a measured parity margin to spend.
//
// Sums (vqa.h states the bounds): a pixel's dE00 is saturated at 2^12, rounded to 2^-20 fixed point (at most 2^32) and added as
// a 64-bit integer - in the thread, across the wave, then one atomic per workgroup: one word per frame.  Integer addition is
// associative: neither the tiling nor the order in which workgroups retire can change a bit.
#include <cmath>

#include "vqa_dev.hpp"
#include "vqa_kernels.hpp"

namespace vqa {

namespace {

// both images of n frames of three planes; every stride in bytes.  Plane 0 (Y, or B) is the full-size grid; planes 1 and 2
// (U and V, or G and R) share one geometry, the grid's or its ceil-half in either direction (sh, sv).
struct ciede_src {
    const uint8_t *ref, *dist;
    int64_t ref_fs, dist_fs;   // frame strides
    int64_t off[3];            // plane offsets inside a frame
    int64_t rs0, rs1;          // row strides of plane 0 and of planes 1, 2
    int step0, step1;          // pixel steps likewise
    int w, h, cw, ch;          // the grid; planes 1, 2
    int sh, sv;                // 1: planes 1, 2 are halved in width / height
    int pw, npatch;            // patches per row of patches, patches per frame
    int o0, o12;               // YUV: 16 s and 128 s; BGR: 0
    float d0, d12;             // YUV: 219 s and 224 s; BGR: 2^depth - 1
    float kl, kc, kh;          // the parametric weights
};

constexpr float D2R = 0.017453292519943295f, R2D = 57.29577951308232f;

// four samples of a row -> four 16-bit fields (field j = sample j); VEC: one load; else the first `valid` samples, one by one
template <typename T, bool VEC> __device__ __forceinline__ unsigned long long load4(const uint8_t *p, int step, int valid)
{
    if constexpr (VEC && sizeof(T) == 1) {
        const unsigned long long u = *reinterpret_cast<const uint32_t *>(p);
        return (u & 0xffull) | ((u & 0xff00ull) << 8) | ((u & 0xff0000ull) << 16) | ((u & 0xff000000ull) << 24);
    } else if constexpr (VEC) {
        const uint2 u = *reinterpret_cast<const uint2 *>(p);
        return (unsigned long long)u.x | ((unsigned long long)u.y << 32);
    } else {
        unsigned long long r = 0;
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (j < valid) r |= (unsigned long long)*reinterpret_cast<const T *>(p + (int64_t)j * step) << (16 * j);
        return r;
    }
}

// two samples of a halved row, each standing for two columns -> fields (s0, s0, s1, s1)
template <typename T, bool VEC> __device__ __forceinline__ unsigned long long load2x2(const uint8_t *p, int step, int valid)
{
    unsigned long long s0 = 0, s1 = 0;
    if constexpr (VEC && sizeof(T) == 1) {
        const unsigned u = *reinterpret_cast<const uint16_t *>(p);
        s0 = u & 0xffu; s1 = u >> 8;
    } else if constexpr (VEC) {
        const uint32_t u = *reinterpret_cast<const uint32_t *>(p);
        s0 = u & 0xffffu; s1 = u >> 16;
    } else {
        if (valid > 0) s0 = *reinterpret_cast<const T *>(p);
        if (valid > 1) s1 = *reinterpret_cast<const T *>(p + step);
    }
    return s0 * 0x00010001ull | s1 * 0x0001000100000000ull;
}

// the two rows of a patch of planes 1 and 2 of one image, expanded to the luma grid
template <typename T, bool VEC>
__device__ __forceinline__ void load_chroma(const ciede_src &s, const uint8_t *base, int py, int px, unsigned long long (&r)[2])
{
    const int y0 = (2 * py) >> s.sv, y1 = (2 * py + 1) >> s.sv;       // y1 may lie below the plane when sv = 0: not loaded then
    if (s.sh) {
        const uint8_t *p = base + (int64_t)y0 * s.rs1 + (int64_t)(2 * px) * s.step1;
        const int valid = s.cw - 2 * px;
        r[0] = load2x2<T, VEC>(p, s.step1, valid);
        r[1] = (y1 != y0 && y1 < s.ch) ? load2x2<T, VEC>(p + s.rs1, s.step1, valid) : r[0];
    } else {
        const uint8_t *p = base + (int64_t)y0 * s.rs1 + (int64_t)(4 * px) * s.step1;
        const int valid = s.cw - 4 * px;
        r[0] = load4<T, VEC>(p, s.step1, valid);
        r[1] = (y1 != y0 && y1 < s.ch) ? load4<T, VEC>(p + s.rs1, s.step1, valid) : r[0];
    }
}

struct lab3 { float L, a, b; };

__device__ __forceinline__ float srgb_linear(float c) { return c > 0.04045f ? powf((c + 0.055f) / 1.055f, 2.4f) : c / 12.92f; }
__device__ __forceinline__ float lab_f(float t) { return t > 0.008856f ? cbrtf(t) : 7.787f * t + 16.f / 116.f; }

// the three integer samples of a pixel (MODEL 0: Y, U, V; 1: B, G, R) -> CIELAB, no clamping (vqa.h)
template <int MODEL> __device__ __forceinline__ lab3 to_lab(int p0, int p1, int p2, const ciede_src &s)
{
    float R, G, B;
    if constexpr (MODEL == VQA_CIEDE_YUV709) {
        const float y = (float)(p0 - s.o0) / s.d0, u = (float)(p1 - s.o12) / s.d12, v = (float)(p2 - s.o12) / s.d12;
        R = y + 1.5748f * v;
        G = y - 0.1873f * u - 0.4681f * v;
        B = y + 1.8556f * u;
    } else {
        B = (float)p0 / s.d0; G = (float)p1 / s.d0; R = (float)p2 / s.d0;
    }
    R = srgb_linear(R); G = srgb_linear(G); B = srgb_linear(B);
    const float X = (0.4124f * R + 0.3576f * G + 0.1805f * B) / 0.9505f;
    const float Y = 0.2126f * R + 0.7152f * G + 0.0722f * B;
    const float Z = (0.0193f * R + 0.1192f * G + 0.9505f * B) / 1.0890f;
    const float fx = lab_f(X), fy = lab_f(Y), fz = lab_f(Z);
    lab3 o;
    o.L = 116.f * fy - 16.f; o.a = 500.f * (fx - fy); o.b = 200.f * (fy - fz);
    return o;
}

// sqrt(c^7 / (c^7 + 25^7)) as sqrt(1 / (1 + (25 / c)^7)): the power by multiplication, no overflow to NaN; 0 at c = 0
__device__ __forceinline__ float chroma_ratio(float c)
{
    const float q = 25.f / c, q2 = q * q, q4 = q2 * q2;
    return sqrtf(1.f / (1.f + q4 * q2 * q));
}

__device__ __forceinline__ float hue_deg(float b, float ap)
{
    if (ap == 0.f && b == 0.f) return 0.f;
    const float h = atan2f(b, ap) * R2D;
    return h < 0.f ? h + 360.f : h;
}

// dE00 of vqa.h; every step is symmetric in the pair (the two signed terms change sign together)
__device__ __forceinline__ float de00(const lab3 &p, const lab3 &q, const ciede_src &s)
{
    const float c1 = sqrtf(p.a * p.a + p.b * p.b), c2 = sqrtf(q.a * q.a + q.b * q.b);
    const float g = 0.5f * (1.f - chroma_ratio(0.5f * (c1 + c2)));
    const float a1 = (1.f + g) * p.a, a2 = (1.f + g) * q.a;
    const float cp1 = sqrtf(a1 * a1 + p.b * p.b), cp2 = sqrtf(a2 * a2 + q.b * q.b);
    const float h1 = hue_deg(p.b, a1), h2 = hue_deg(q.b, a2);
    const float dL = q.L - p.L, dC = cp2 - cp1, cc = cp1 * cp2;
    float dh = h2 - h1;
    if (dh > 180.f) dh -= 360.f;
    else if (dh < -180.f) dh += 360.f;
    const float hs = h1 + h2;
    float hm = hs;
    if (cc == 0.f) dh = 0.f;
    else if (fabsf(h1 - h2) <= 180.f) hm = 0.5f * hs;
    else hm = hs < 360.f ? 0.5f * (hs + 360.f) : 0.5f * (hs - 360.f);
    const float dH = 2.f * sqrtf(cc) * sinf(0.5f * dh * D2R);
    const float lm = 0.5f * (p.L + q.L), cm = 0.5f * (cp1 + cp2);
    const float t = 1.f - 0.17f * cosf((hm - 30.f) * D2R) + 0.24f * cosf(2.f * hm * D2R) + 0.32f * cosf((3.f * hm + 6.f) * D2R) -
                    0.20f * cosf((4.f * hm - 63.f) * D2R);
    const float x = (hm - 275.f) / 25.f;
    const float dtheta = 30.f * expf(-(x * x));
    const float rc = 2.f * chroma_ratio(cm);
    const float l2 = (lm - 50.f) * (lm - 50.f);
    const float sl = 1.f + 0.015f * l2 / sqrtf(20.f + l2);
    const float sc = 1.f + 0.045f * cm;
    const float shh = 1.f + 0.015f * cm * t;
    const float rt = -sinf(2.f * dtheta * D2R) * rc;
    const float tl = dL / (s.kl * sl), tc = dC / (s.kc * sc), th = dH / (s.kh * shh);
    const float v = tl * tl + tc * tc + th * th + (rt * tc) * th;
    return sqrtf(fmaxf(v, 0.f));
}

// grid = (workgroups, n_frames); block = 64.  acc: [frame] uint64, zeroed by the submit
template <typename T, int MODEL, bool VEC>
__global__ __launch_bounds__(64) void k_ciede(ciede_src s, unsigned long long *__restrict__ acc)
{
    const int f = blockIdx.y;
    const int patch = blockIdx.x * 64 + (int)threadIdx.x;
    unsigned long long sum = 0;
    if (patch < s.npatch) {
        const int py = patch / s.pw, px = patch - py * s.pw;
        const int rows = min(2, s.h - 2 * py), cols = min(4, s.w - 4 * px);
        const uint8_t *fr = s.ref + (int64_t)f * s.ref_fs, *fd = s.dist + (int64_t)f * s.dist_fs;
        const int64_t o0 = s.off[0] + (int64_t)(2 * py) * s.rs0 + (int64_t)(4 * px) * s.step0;
        unsigned long long ra[3][2], rb[3][2];   // [plane][row]: four 16-bit fields
        ra[0][0] = load4<T, VEC>(fr + o0, s.step0, cols);
        rb[0][0] = load4<T, VEC>(fd + o0, s.step0, cols);
        ra[0][1] = rows > 1 ? load4<T, VEC>(fr + o0 + s.rs0, s.step0, cols) : 0ull;
        rb[0][1] = rows > 1 ? load4<T, VEC>(fd + o0 + s.rs0, s.step0, cols) : 0ull;
        load_chroma<T, VEC>(s, fr + s.off[1], py, px, ra[1]);
        load_chroma<T, VEC>(s, fr + s.off[2], py, px, ra[2]);
        load_chroma<T, VEC>(s, fd + s.off[1], py, px, rb[1]);
        load_chroma<T, VEC>(s, fd + s.off[2], py, px, rb[2]);
#pragma unroll 1
        for (int k = 0; k < 8; k++) {
            const int r = k >> 2, c = k & 3;
            if (r >= rows || c >= cols) continue;
            const int sft = 16 * c;
            const int x0 = (int)(((r ? ra[0][1] : ra[0][0]) >> sft) & 0xffffu), y0 = (int)(((r ? rb[0][1] : rb[0][0]) >> sft) & 0xffffu);
            const int x1 = (int)(((r ? ra[1][1] : ra[1][0]) >> sft) & 0xffffu), y1 = (int)(((r ? rb[1][1] : rb[1][0]) >> sft) & 0xffffu);
            const int x2 = (int)(((r ? ra[2][1] : ra[2][0]) >> sft) & 0xffffu), y2 = (int)(((r ? rb[2][1] : rb[2][0]) >> sft) & 0xffffu);
            if (x0 == y0 && x1 == y1 && x2 == y2) continue;   // equal triples: exactly 0
            const lab3 p = to_lab<MODEL>(x0, x1, x2, s), q = to_lab<MODEL>(y0, y1, y2, s);
            const float de = fminf(de00(p, q, s), CIEDE_SATURATE);
            sum += __float2ull_rn(de * CIEDE_FIX);   // at most 2^32
        }
    }
    sum = wave_sum(sum);
    if (threadIdx.x == 0 && sum) atomicAdd(acc + f, sum);
}

template <typename T, int MODEL>
void launch_tm(hipStream_t st, const ciede_src &s, bool vec, dim3 grid, unsigned long long *acc)
{
    if (vec) hipLaunchKernelGGL((k_ciede<T, MODEL, true>), grid, dim3(64), 0, st, s, acc);
    else hipLaunchKernelGGL((k_ciede<T, MODEL, false>), grid, dim3(64), 0, st, s, acc);
}

} // namespace

void launch_ciede(hipStream_t st, const uint8_t *ref, const uint8_t *dist, int n, int64_t ref_frame_stride,
                  int64_t dist_frame_stride, const vqa_plane_desc *planes, int depth, int model, const double *weights,
                  unsigned long long *acc)
{
    if (n <= 0) return;
    ciede_src s;
    s.ref = ref; s.dist = dist; s.ref_fs = ref_frame_stride; s.dist_fs = dist_frame_stride;
    for (int i = 0; i < 3; i++) s.off[i] = planes[i].offset;
    s.rs0 = planes[0].row_stride; s.step0 = planes[0].pixel_step;
    s.rs1 = planes[1].row_stride; s.step1 = planes[1].pixel_step;
    s.w = planes[0].width; s.h = planes[0].height;
    s.cw = planes[1].width; s.ch = planes[1].height;
    s.sh = s.cw != s.w; s.sv = s.ch != s.h;
    s.pw = (s.w + 3) / 4;
    s.npatch = s.pw * ((s.h + 1) / 2);
    const int scale = 1 << (depth - 8);
    if (model == VQA_CIEDE_YUV709) {
        s.o0 = 16 * scale; s.o12 = 128 * scale;
        s.d0 = (float)(219 * scale); s.d12 = (float)(224 * scale);
    } else {
        s.o0 = s.o12 = 0;
        s.d0 = s.d12 = (float)((1 << depth) - 1);
    }
    s.kl = (float)weights[0]; s.kc = (float)weights[1]; s.kh = (float)weights[2];
    const int bps = depth > 8 ? 2 : 1;
    // a row of a patch as one load: unit steps, whole patches, and every address a multiple of the load's size - 4 samples of
    // plane 0, and 4 or (halved) 2 samples of planes 1 and 2
    uint64_t bits0 = (uint64_t)(uintptr_t)ref | (uint64_t)(uintptr_t)dist | (uint64_t)s.rs0 | (uint64_t)s.off[0];
    if (n > 1) bits0 |= (uint64_t)ref_frame_stride | (uint64_t)dist_frame_stride;
    const uint64_t bits1 = bits0 | (uint64_t)s.rs1 | (uint64_t)s.off[1] | (uint64_t)s.off[2];
    const int a0 = 4 * bps, a1 = (s.sh ? 2 : 4) * bps;
    const bool vec = s.step0 == bps && s.step1 == bps && s.w % 4 == 0 && (bits0 & (uint64_t)(a0 - 1)) == 0 &&
                     (bits1 & (uint64_t)(a1 - 1)) == 0;
    const dim3 grid((s.npatch + 63) / 64, n);
    if (depth > 8) {
        if (model == VQA_CIEDE_YUV709) launch_tm<uint16_t, VQA_CIEDE_YUV709>(st, s, vec, grid, acc);
        else launch_tm<uint16_t, VQA_CIEDE_BGR>(st, s, vec, grid, acc);
    } else {
        if (model == VQA_CIEDE_YUV709) launch_tm<uint8_t, VQA_CIEDE_YUV709>(st, s, vec, grid, acc);
        else launch_tm<uint8_t, VQA_CIEDE_BGR>(st, s, vec, grid, acc);
    }
}

// the word -> the record, in double on the host.  Contraction is off: the record is the formula vqa.h states.
void ciede_finalize(unsigned long long word, int h, int w, vqa_ciede_metrics *out)
{
#pragma clang fp contract(off)
    out->de_sum = (double)word * (1.0 / (double)CIEDE_FIX);   // (the conversion is exact below 2^53: any frame that is not saturated throughout)
    out->de_mean = out->de_sum / ((double)h * (double)w);
    out->ciede2000 = out->de_mean > 0.0 ? 45.0 - 20.0 * std::log10(out->de_mean) : HUGE_VAL;
}

} // namespace vqa
