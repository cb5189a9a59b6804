// k_vif.hip — VIF (visual information fidelity, Sheikh & Bovik 2006, pixel domain) on four scales for gfx950: the
// vif_scale0..3 features of VMAF, by the definition stated in include/vqa.h (vqa_vif_submit).
//
// Per plane pair: level 0 is the pair of planes as centred fp32 samples x = v / 2^(depth-8) - 128; level s > 0 is level
// s - 1 filtered with the Gaussian of scale s (17, 9, 5, 3 taps for s = 0..3) and kept at even rows and columns.  At
// every level the five moment maps F(x), F(y), F(xx), F(yy), F(xy) of that level's filter give a per-sample pair
// (num, den) of log2 terms, summed over the level.  Borders reflect: index i < 0 reads -i, i >= n reads 2n - i - 1.
//
//   k_vif_stats<T, R>     one level's statistic.  A workgroup of 256 threads owns a 64 x 16 tile of the level: the tile
//                         and its halo of R = taps / 2 samples (both images, centred) go to LDS once; the vertical pass
//                         forms the five products per input sample and slides them through eight output rows per thread
//                         (one LDS read per input sample, not one per tap); the horizontal pass reads its 4 + 2R inputs
//                         per product as ds_read_b128 and forms four adjacent outputs per thread; the per-sample num and
//                         den are rounded to 2^-27 fixed point and summed as 64-bit integers - per thread, per wave, per
//                         workgroup, and with one integer atomic per workgroup and sum into the plane pair's totals.
//                         Integer addition is associative: neither the tile geometry nor the order in which workgroups
//                         retire can change a bit of a total, so a pair gives the same bits at any place of any batch.
//   k_vif_decimate<T, R>  level s from level s - 1: only the kept (even, even) samples are computed - vertical pass on
//                         the even rows of a (64 + 2R)^2 input tile, horizontal pass on the even columns - and stored
//                         as fp32.  Level 1 re-reads the caller's planes (1-2 bytes per sample against the 170 FMAs per
//                         sample of the level-0 statistic); building all levels from one read would need a halo of
//                         8 + 2 (4 + 2 (2 + 2)) = 32 samples on every side of the tile.
//   k_vif_finalize        the eight integer totals of every plane pair -> vqa_vif_metrics (doubles; quotients in double)
//
// Sums: |num|, den < 64 per sample for ANY 16-bit input (s1 <= 65535^2 / 4 < 2^30, g <= 100: num <= log2(1 + 1e4 s1 / 2)
// < 43; in-range samples have s1 <= 2^14 and num < 27), so a plane of 2^28 samples sums to < 2^(6 + 28 + 27) = 2^61.
// 1 - s2 smi can be negative: the sums are signed (two's complement through the unsigned atomic).
#include "vqa_dev.hpp"
#include "vqa_kernels.hpp"

namespace vqa {

namespace {

constexpr float VIF_FIX = 134217728.f;   // 2^27

struct vif_taps { float t[17]; };

// One level of both images of a group is a pair_src (vqa_dev.hpp).  Borders: reflect_clamp is the border rule stated above
// (libvmaf's VIF), then a clamp: a tile that hangs over the plane's edge reads (and discards) in-plane samples.

// grid = (tiles * count, n_frames); block = 256.  acc: [frame][plane of the submit][level][num, den] int64
template <typename T, int R>
__global__ __launch_bounds__(256) void k_vif_stats(pair_src s, vif_taps tp, int tiles_x, int tiles, int level,
                                                   int n_planes, int4 plane_index, unsigned long long *__restrict__ acc)
{
    constexpr int TW = 64, TH = 16, IW = TW + 2 * R, IH = TH + 2 * R, NT = 2 * R + 1;
    constexpr int VP = (IW + 3) & ~3;              // row pitch of the vertical results: float4 reads stay aligned
    constexpr int NV = (4 + 2 * R + 3) / 4;        // float4 reads per product in the horizontal pass
    __shared__ float in[2][IH][IW];
    __shared__ __attribute__((aligned(16))) float V[5][TH][VP];
    __shared__ unsigned long long red[2][4];
    const int f = blockIdx.y, ch = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const int y0 = (tile / tiles_x) * TH, x0 = (tile % tiles_x) * TW;
    const int t = threadIdx.x;
    const uint8_t *pr = s.ref + (int64_t)f * s.ref_fs + s.off[ch], *pd = s.dist + (int64_t)f * s.dist_fs + s.off[ch];
    for (int i = t; i < IH * IW; i += 256) {
        const int j = i / IW, c = i - j * IW;
        const int64_t o = (int64_t)reflect_clamp(y0 + j - R, s.h) * s.row_stride + (int64_t)reflect_clamp(x0 + c - R, s.w) * s.step;
        in[0][j][c] = ld_centred<T>(pr + o, s.sc);
        in[1][j][c] = ld_centred<T>(pd + o, s.sc);
    }
    if (t < 5 * TH) {   // the pad columns of V are read (never used) by the last float4 of a row
        for (int c = IW; c < VP; c++) V[t / TH][t % TH][c] = 0.f;
    }
    __syncthreads();
    // vertical pass: thread = (column c, eight output rows); every input row feeds the output rows it is a tap of,
    // each output summing its taps in ascending order
    if (t < 2 * IW) {
        const int g = t / IW, c = t - g * IW;
        float a[8][5];
#pragma unroll
        for (int o = 0; o < 8; o++)
#pragma unroll
            for (int p = 0; p < 5; p++) a[o][p] = 0.f;
#pragma unroll
        for (int j = 0; j < 8 + 2 * R; j++) {
            const float x = in[0][8 * g + j][c], y = in[1][8 * g + j][c];
            const float xx = x * x, yy = y * y, xy = x * y;
#pragma unroll
            for (int o = 0; o < 8; o++) {
                if (j - o >= 0 && j - o < NT) {
                    const float w = tp.t[j - o];
                    a[o][0] = fmaf(w, x, a[o][0]);
                    a[o][1] = fmaf(w, y, a[o][1]);
                    a[o][2] = fmaf(w, xx, a[o][2]);
                    a[o][3] = fmaf(w, yy, a[o][3]);
                    a[o][4] = fmaf(w, xy, a[o][4]);
                }
            }
        }
#pragma unroll
        for (int o = 0; o < 8; o++)
#pragma unroll
            for (int p = 0; p < 5; p++) V[p][8 * g + o][c] = a[o][p];
    }
    __syncthreads();
    // horizontal pass: thread = (row r, four adjacent columns)
    const int r = t >> 4, q = t & 15;
    float m[5][4];
#pragma unroll
    for (int p = 0; p < 5; p++) {
        float v[4 * NV];
#pragma unroll
        for (int k = 0; k < NV; k++) {
            const float4 u = *reinterpret_cast<const float4 *>(&V[p][r][4 * q + 4 * k]);
            v[4 * k] = u.x; v[4 * k + 1] = u.y; v[4 * k + 2] = u.z; v[4 * k + 3] = u.w;
        }
#pragma unroll
        for (int o = 0; o < 4; o++) {
            float sum = 0.f;
#pragma unroll
            for (int k = 0; k < NT; k++) sum = fmaf(tp.t[k], v[o + k], sum);
            m[p][o] = sum;
        }
    }
    long long tn = 0, td = 0;
    const bool row_in = y0 + r < s.h;
#pragma unroll
    for (int o = 0; o < 4; o++) {
        const float eps = 1e-10f, nsq = 2.f, smi = 4.f / 65025.f;
        const float mu1 = m[0][o], mu2 = m[1][o];
        float s1 = fmaxf(fmaf(-mu1, mu1, m[2][o]), 0.f);
        const float s2 = fmaxf(fmaf(-mu2, mu2, m[3][o]), 0.f);
        const float s12 = fmaf(-mu1, mu2, m[4][o]);
        float g = s12 / (s1 + eps);          // correctly rounded: identical planes give exactly 1
        float sv = fmaf(-g, s12, s2);
        if (s1 < eps) { g = 0.f; sv = s2; s1 = 0.f; }
        if (s2 < eps) { g = 0.f; sv = 0.f; }
        if (g < 0.f) { sv = s2; g = 0.f; }
        sv = fmaxf(sv, eps);
        g = fminf(g, 100.f);
        float num = log2f(1.f + g * g * s1 / (sv + nsq));
        float den = log2f(1.f + s1 / nsq);
        if (s12 < 0.f) num = 0.f;
        if (s1 < nsq) { num = 1.f - s2 * smi; den = 1.f; }
        if (row_in && x0 + 4 * q + o < s.w) {
            tn += __float2ll_rn(num * VIF_FIX);
            td += __float2ll_rn(den * VIF_FIX);
        }
    }
    unsigned long long un = wave_sum((unsigned long long)tn), ud = wave_sum((unsigned long long)td);
    if (lane_id() == 0) { red[0][wave_id()] = un; red[1][wave_id()] = ud; }
    __syncthreads();
    if (t < 2) {
        const unsigned long long tot = red[t][0] + red[t][1] + red[t][2] + red[t][3];
        const int pi = ch == 0 ? plane_index.x : ch == 1 ? plane_index.y : ch == 2 ? plane_index.z : plane_index.w;
        atomicAdd(acc + (((int64_t)f * n_planes + pi) * VIF_LEVELS + level) * 2 + t, tot);
    }
}

// grid = (tiles * count, n_frames, 2 images); block = 256.  out: [image][frame][plane of the group][oh][ow] fp32
template <typename T, int R>
__global__ __launch_bounds__(256) void k_vif_decimate(pair_src s, vif_taps tp, int tiles_x, int tiles, int count, int ow,
                                                      int oh, float *__restrict__ out)
{
    constexpr int TO = 32, IW = 2 * TO + 2 * R, NT = 2 * R + 1;
    __shared__ float in[IW][IW];
    __shared__ float V[TO][IW];
    const int f = blockIdx.y, n = gridDim.y, img = blockIdx.z;
    const int ch = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const int oy0 = (tile / tiles_x) * TO, ox0 = (tile % tiles_x) * TO;
    const int t = threadIdx.x;
    const uint8_t *src = (img ? s.dist + (int64_t)f * s.dist_fs : s.ref + (int64_t)f * s.ref_fs) + s.off[ch];
    for (int i = t; i < IW * IW; i += 256) {
        const int j = i / IW, c = i - j * IW;
        in[j][c] = ld_centred<T>(src + (int64_t)reflect_clamp(2 * oy0 + j - R, s.h) * s.row_stride +
                                 (int64_t)reflect_clamp(2 * ox0 + c - R, s.w) * s.step, s.sc);
    }
    __syncthreads();
    for (int i = t; i < TO * IW; i += 256) {   // even rows only
        const int ro = i / IW, c = i - ro * IW;
        float sum = 0.f;
#pragma unroll
        for (int k = 0; k < NT; k++) sum = fmaf(tp.t[k], in[2 * ro + k][c], sum);
        V[ro][c] = sum;
    }
    __syncthreads();
    float *o = out + (((int64_t)img * n + f) * count + ch) * oh * ow;
    for (int i = t; i < TO * TO; i += 256) {   // even columns only
        const int ro = i / TO, co = i - ro * TO;
        float sum = 0.f;
#pragma unroll
        for (int k = 0; k < NT; k++) sum = fmaf(tp.t[k], V[ro][2 * co + k], sum);
        if (oy0 + ro < oh && ox0 + co < ow) o[(int64_t)(oy0 + ro) * ow + ox0 + co] = sum;
    }
}

__global__ void k_vif_finalize(const long long *__restrict__ acc, int n_entries, vqa_vif_metrics *__restrict__ res)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_entries) return;
    vqa_vif_metrics &m = res[e];
    double tn = 0.0, td = 0.0;
    for (int s = 0; s < VIF_LEVELS; s++) {
        const double num = (double)acc[((int64_t)e * VIF_LEVELS + s) * 2] * (1.0 / 134217728.0);       // (a total above
        const double den = (double)acc[((int64_t)e * VIF_LEVELS + s) * 2 + 1] * (1.0 / 134217728.0);   // 2^53 is rounded once, to double)
        m.num[s] = num;
        m.den[s] = den;
        m.scale[s] = den == 0.0 ? 1.0 : num / den;
        tn += num;
        td += den;
    }
    m.vif = td == 0.0 ? 1.0 : tn / td;
}

// t[k] = exp(-(k - n/2)^2 / (2 (n/5)^2)) / sum, n = 2^(4-s) + 1; formed in double, rounded once
vif_taps taps_of(int level)
{
    const int n = (1 << (4 - level)) + 1, half = n / 2;
    const double sd = n / 5.0;
    double g[17], sum = 0.0;
    for (int k = 0; k < n; k++) { g[k] = exp(-(double)((k - half) * (k - half)) / (2.0 * sd * sd)); sum += g[k]; }
    vif_taps tp;
    for (int k = 0; k < 17; k++) tp.t[k] = k < n ? (float)(g[k] / sum) : 0.f;
    return tp;
}

// level `lv` of the group as the kernels read it: the caller's planes (lv 0) or the fp32 scratch
pair_src source_of(int lv, const vif_layout &L, const uint8_t *ref, const uint8_t *dist, int n, int64_t ref_fs, int64_t dist_fs,
                  const vqa_plane_desc *planes, const int *idx, int count, int depth, const float *scratch)
{
    pair_src s;
    s.w = L.w[lv]; s.h = L.h[lv];
    if (lv == 0) {
        const vqa_plane_desc &pd = planes[idx[0]];
        s.ref = ref; s.dist = dist; s.ref_fs = ref_fs; s.dist_fs = dist_fs;
        group_slots(planes, idx, count, s.off, nullptr);
        s.row_stride = pd.row_stride; s.step = pd.pixel_step;
        s.sc = 1.f / (float)(1 << (depth - 8));
    } else {
        const int64_t plane = (int64_t)s.h * s.w * sizeof(float);
        s.ref = (const uint8_t *)(scratch + L.off[lv]);
        s.dist = s.ref + (int64_t)n * count * plane;
        s.ref_fs = s.dist_fs = count * plane;
        for (int i = 0; i < 4; i++) s.off[i] = (i < count ? i : 0) * plane;
        s.row_stride = (int64_t)s.w * sizeof(float); s.step = sizeof(float);
        s.sc = 1.f;
    }
    return s;
}

template <int R>
void stats_level(hipStream_t st, const pair_src &s, int lv, int n, int count, int n_planes, int4 pi, int depth,
                 unsigned long long *acc)
{
    const int tiles_x = (s.w + 63) / 64, tiles = tiles_x * ((s.h + 15) / 16);
    const dim3 grid(tiles * count, n), block(256);
    const vif_taps tp = taps_of(lv);
    if (lv > 0)
        hipLaunchKernelGGL((k_vif_stats<float, R>), grid, block, 0, st, s, tp, tiles_x, tiles, lv, n_planes, pi, acc);
    else if (depth > 8)
        hipLaunchKernelGGL((k_vif_stats<uint16_t, R>), grid, block, 0, st, s, tp, tiles_x, tiles, lv, n_planes, pi, acc);
    else
        hipLaunchKernelGGL((k_vif_stats<uint8_t, R>), grid, block, 0, st, s, tp, tiles_x, tiles, lv, n_planes, pi, acc);
}

template <int R>
void decimate_level(hipStream_t st, const pair_src &s, int lv, int n, int count, int depth, const vif_layout &L, float *scratch)
{
    const int ow = L.w[lv], oh = L.h[lv];
    const int tiles_x = (ow + 31) / 32, tiles = tiles_x * ((oh + 31) / 32);
    const dim3 grid(tiles * count, n, 2), block(256);
    const vif_taps tp = taps_of(lv);
    float *out = scratch + L.off[lv];
    if (lv > 1)
        hipLaunchKernelGGL((k_vif_decimate<float, R>), grid, block, 0, st, s, tp, tiles_x, tiles, count, ow, oh, out);
    else if (depth > 8)
        hipLaunchKernelGGL((k_vif_decimate<uint16_t, R>), grid, block, 0, st, s, tp, tiles_x, tiles, count, ow, oh, out);
    else
        hipLaunchKernelGGL((k_vif_decimate<uint8_t, R>), grid, block, 0, st, s, tp, tiles_x, tiles, count, ow, oh, out);
}

} // namespace

void launch_vif_stats(hipStream_t st, const uint8_t *ref, const uint8_t *dist, int n, int64_t ref_frame_stride,
                      int64_t dist_frame_stride, const vqa_plane_desc *planes, const int *idx, int count, int n_planes,
                      int depth, int level, const float *scratch, long long *acc)
{
    if (n <= 0 || count <= 0) return;
    const vif_layout L = vif_levels(n, count, planes[idx[0]].height, planes[idx[0]].width);
    const pair_src s = source_of(level, L, ref, dist, n, ref_frame_stride, dist_frame_stride, planes, idx, count, depth, scratch);
    int p4[4];
    group_slots(planes, idx, count, nullptr, p4);
    const int4 pi = make_int4(p4[0], p4[1], p4[2], p4[3]);
    unsigned long long *a = reinterpret_cast<unsigned long long *>(acc);
    switch (level) {
    case 0: stats_level<8>(st, s, 0, n, count, n_planes, pi, depth, a); break;
    case 1: stats_level<4>(st, s, 1, n, count, n_planes, pi, depth, a); break;
    case 2: stats_level<2>(st, s, 2, n, count, n_planes, pi, depth, a); break;
    default: stats_level<1>(st, s, 3, n, count, n_planes, pi, depth, a); break;
    }
}

void launch_vif_decimate(hipStream_t st, const uint8_t *ref, const uint8_t *dist, int n, int64_t ref_frame_stride,
                         int64_t dist_frame_stride, const vqa_plane_desc *planes, const int *idx, int count, int depth,
                         int level, float *scratch)
{
    if (n <= 0 || count <= 0 || level < 1 || level >= VIF_LEVELS) return;
    const vif_layout L = vif_levels(n, count, planes[idx[0]].height, planes[idx[0]].width);
    const pair_src s = source_of(level - 1, L, ref, dist, n, ref_frame_stride, dist_frame_stride, planes, idx, count, depth, scratch);
    switch (level) {
    case 1: decimate_level<4>(st, s, 1, n, count, depth, L, scratch); break;
    case 2: decimate_level<2>(st, s, 2, n, count, depth, L, scratch); break;
    default: decimate_level<1>(st, s, 3, n, count, depth, L, scratch); break;
    }
}

void launch_vif_finalize(hipStream_t st, const long long *acc, int n_entries, vqa_vif_metrics *res)
{
    hipLaunchKernelGGL(k_vif_finalize, dim3((n_entries + 63) / 64), dim3(64), 0, st, acc, n_entries, res);
}

} // namespace vqa
