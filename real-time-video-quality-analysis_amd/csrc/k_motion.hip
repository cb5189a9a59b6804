// k_motion.hip — VMAF's motion feature for gfx950: the mean absolute difference of two consecutive reference frames after a
// 5-tap blur, by the definition stated in include/vqa.h (vqa_motion_submit).
//
//   k_motion_sad<T>   one fused launch per group of same-geometry planes.  A workgroup of 256 threads owns a 64 x 32 tile of
//                     the plane: the tile and its apron of 2 samples of frame i AND of frame i-1 go to LDS once, as centred
//                     fp32 samples x = v / 2^(depth-8) - 128 (exact at every depth); the vertical pass blurs both images into
//                     a second LDS array (consecutive threads walk a row: no bank conflict), the horizontal pass reads its
//                     4 + 4 inputs per image as two ds_read_b128 and forms four adjacent outputs per thread and row; the
//                     absolute difference of the two blurred samples is rounded to 2^-16 fixed point and summed as 64-bit
//                     integers - per thread, per wave, per workgroup, and with one integer atomic per workgroup into the
//                     pair's total.  Nothing but that total goes back to HBM: about two input samples are read per output
//                     sample ((68 x 36) / (64 x 32) = 1.2 with the apron, which mostly hits L2) and there is no scratch.
//                     Every frame is blurred twice - as "current" of its own pair and as "previous" of the next - which costs
//                     20 FMAs per sample and saves 8 bytes of fp32 traffic per sample.
//
// Sums: |d| < 2^15 for ANY 16-bit input (depth 9 reaches x = 65535 / 2 - 128, and the blur is a convex combination up to
// rounding), so a term is below 2^31 and a plane of 2^28 samples sums to less than 2^59.  Integer addition is associative:
// neither the tiling nor the order in which workgroups retire can change a bit, so a pair gives the same bits at any place of
// any batch.  The workgroups of a frame without a predecessor return at once: its total stays the 0 the submit's memset wrote.
#include "vqa_dev.hpp"
#include "vqa_kernels.hpp"

namespace vqa {

namespace {

constexpr float MOTION_FIX = 65536.f;   // 2^16

struct motion_taps { float t[5]; };

// the reference frames of one group of same-geometry planes; every stride in bytes
struct motion_src {
    const uint8_t *ref;     // frame 0 of the slice
    const uint8_t *prev0;   // the frame before it, or nullptr
    int64_t fs;             // frame stride
    int64_t off[4];         // plane offsets inside a frame
    int64_t row_stride;
    int step;
    float sc;               // 2^-(depth - 8)
    int w, h;
};

// Borders: reflect_clamp (vqa_dev.hpp) is the border rule (VIF's), then a clamp: a tile that hangs over the plane's edge reads
// (and discards) in-plane samples.

// grid = (tiles * count, n_frames); block = 256.  acc: [frame][plane of the submit] int64, zeroed by the submit
template <typename T>
__global__ __launch_bounds__(256) void k_motion_sad(motion_src s, motion_taps tp, int tiles_x, int tiles, int n_planes,
                                                    int4 plane_index, unsigned long long *__restrict__ acc)
{
    constexpr int R = MOTION_RADIUS, TW = 64, TH = 32, IW = TW + 2 * R, IH = TH + 2 * R;
    __shared__ float in[2][IH][IW];
    __shared__ __attribute__((aligned(16))) float V[2][TH][IW];   // IW = 68: rows stay 16-byte aligned
    __shared__ unsigned long long red[4];
    const int f = blockIdx.y;
    if (f == 0 && s.prev0 == nullptr) return;   // (the whole workgroup: no barrier has been reached)
    const int ch = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const int y0 = (tile / tiles_x) * TH, x0 = (tile % tiles_x) * TW;
    const int t = threadIdx.x;
    const uint8_t *pc = s.ref + (int64_t)f * s.fs + s.off[ch];
    const uint8_t *pp = (f == 0 ? s.prev0 : s.ref + (int64_t)(f - 1) * s.fs) + s.off[ch];
    for (int i = t; i < IH * IW; i += 256) {
        const int j = i / IW, c = i - j * IW;
        const int64_t o = (int64_t)reflect_clamp(y0 + j - R, s.h) * s.row_stride + (int64_t)reflect_clamp(x0 + c - R, s.w) * s.step;
        in[0][j][c] = ld_centred<T>(pc + o, s.sc);
        in[1][j][c] = ld_centred<T>(pp + o, s.sc);
    }
    __syncthreads();
    // vertical pass, both images: taps in ascending order
    for (int i = t; i < 2 * TH * IW; i += 256) {
        const int g = i / (TH * IW), k = i - g * (TH * IW), j = k / IW, c = k - j * IW;
        float sum = 0.f;
#pragma unroll
        for (int a = 0; a < 2 * R + 1; a++) sum = fmaf(tp.t[a], in[g][j + a][c], sum);
        V[g][j][c] = sum;
    }
    __syncthreads();
    // horizontal pass: thread = (rows r and r + 16, four adjacent columns); taps in ascending order
    const int r = t >> 4, q = t & 15;
    long long tot = 0;
#pragma unroll
    for (int half = 0; half < 2; half++) {
        const int row = r + 16 * half;
        float m[2][4];
#pragma unroll
        for (int g = 0; g < 2; g++) {
            const float4 u0 = *reinterpret_cast<const float4 *>(&V[g][row][4 * q]);
            const float4 u1 = *reinterpret_cast<const float4 *>(&V[g][row][4 * q + 4]);
            const float v[8] = {u0.x, u0.y, u0.z, u0.w, u1.x, u1.y, u1.z, u1.w};
#pragma unroll
            for (int o = 0; o < 4; o++) {
                float sum = 0.f;
#pragma unroll
                for (int a = 0; a < 2 * R + 1; a++) sum = fmaf(tp.t[a], v[o + a], sum);
                m[g][o] = sum;
            }
        }
        const bool row_in = y0 + row < s.h;
#pragma unroll
        for (int o = 0; o < 4; o++) {
            const float d = fabsf(m[0][o] - m[1][o]);
            if (row_in && x0 + 4 * q + o < s.w) tot += __float2ll_rn(d * MOTION_FIX);
        }
    }
    const unsigned long long u = wave_sum((unsigned long long)tot);
    if (lane_id() == 0) red[wave_id()] = u;
    __syncthreads();
    if (t == 0) {
        const int pi = ch == 0 ? plane_index.x : ch == 1 ? plane_index.y : ch == 2 ? plane_index.z : plane_index.w;
        atomicAdd(acc + (int64_t)f * n_planes + pi, red[0] + red[1] + red[2] + red[3]);
    }
}

} // namespace

void launch_motion_sad(hipStream_t st, const uint8_t *ref, const uint8_t *prev0, int n, int64_t frame_stride,
                       const vqa_plane_desc *planes, const int *idx, int count, int n_planes, int depth, long long *acc)
{
    if (n <= 0 || count <= 0) return;
    const vqa_plane_desc &pd = planes[idx[0]];
    motion_src s;
    s.ref = ref; s.prev0 = prev0; s.fs = frame_stride;
    int p4[4];
    group_slots(planes, idx, count, s.off, p4);
    s.row_stride = pd.row_stride; s.step = pd.pixel_step;
    s.sc = 1.f / (float)(1 << (depth - 8));
    s.w = pd.width; s.h = pd.height;
    motion_taps tp;
    for (int k = 0; k < 5; k++) tp.t[k] = (float)MOTION_TAPS[k];
    const int tiles_x = (s.w + 63) / 64, tiles = tiles_x * ((s.h + 31) / 32);
    const int4 pi = make_int4(p4[0], p4[1], p4[2], p4[3]);
    const dim3 grid(tiles * count, n), block(256);
    unsigned long long *a = reinterpret_cast<unsigned long long *>(acc);
    if (depth > 8)
        hipLaunchKernelGGL((k_motion_sad<uint16_t>), grid, block, 0, st, s, tp, tiles_x, tiles, n_planes, pi, a);
    else
        hipLaunchKernelGGL((k_motion_sad<uint8_t>), grid, block, 0, st, s, tp, tiles_x, tiles, n_planes, pi, a);
}

} // namespace vqa
