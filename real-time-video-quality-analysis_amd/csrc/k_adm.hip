// k_adm.hip — ADM (detail loss metric, Li et al. 2011) on a four-level db2 wavelet pyramid for gfx950: the adm2 and
// adm_scale0..3 features of VMAF, by the definition stated in include/vqa.h (vqa_adm_submit).
//
// Per plane pair and scale s: both images go through one level of the db2 DWT (vertical pass first; four bands a, v, h, d of
// ceil(H/2) x ceil(W/2)); the distorted image's detail bands are decoupled per sample into a restored part r and an additive
// part t - r; the additive part, weighted by the contrast sensitivity rf of its band, masks r over a 3 x 3 neighbourhood;
// what is left of |rf r| and the reference's |rf o| are cubed and summed over the scale's centre region.  Scale s + 1 reads
// the a bands of scale s.
//
//   k_adm_scale<T>   one scale, one launch per group of same-geometry planes.  A workgroup of 256 threads owns a 32 x 16
//                    tile of the bands.  (1) The 70 x 38 input samples of both images that the tile and its one-sample halo
//                    read go to LDS once (u8 / u16 at scale 0, centred; the fp32 a band above), mirrored at the plane's
//                    edges by the DWT's index rule.  (2) Vertical pass: L and Hh of the 18 band rows at all 70 columns.
//                    (3) Horizontal pass per band sample of the tile + halo: a, v, h, d of both images in registers; the two
//                    a values go to the ctx scratch (scales 0..2, tile samples only - the only HBM writes besides the
//                    partial sums); decoupling; M = sum_bands |rf (t - r)|, the three |rf r| and the three |rf o| go to LDS
//                    (overlaid on the dead input tile).  (4) Per tile sample in the region: thr = M / 15 + (sum of the 8
//                    neighbours' M) / 30, the neighbours mirrored at the BAND's edges (-1 reads 1, n reads n - 1: always
//                    inside tile + halo); max(|rf r| - thr, 0)^3 is added to the num sums and |rf o|^3 to the den sums, by
//                    the same thread in the same order (identical planes: num = den bit for bit).
//                    (5) The six sums (fp32 per thread: two samples each) are reduced as doubles
//                    over the wave by a fixed shuffle tree, over the four waves in order, and stored as this tile's
//                    partial.  h, v, d, r and t - r never reach HBM.
//   k_adm_reduce     the tile partials of every (frame, plane, scale) of a group, summed in double in a fixed order: lane l
//                    of one wave adds tiles l, l + 64, ..., then the same shuffle tree.
//
// Sums: the tiling of a plane depends on its geometry alone and every order of addition above is fixed, so a pair gives the
// same six doubles per scale at any place of any batch, from host or device memory.  Fixed point was not used: a cube is
// below 242 at scale 0 for in-range samples but reaches 7.7e14 at scale 3 for arbitrary 16-bit samples declared 9 bits deep
// (include/vqa.h), too wide for one 64-bit scale; doubles hold both (the largest plane's total stays below 1e21).
// The cube roots and quotients are formed on the host, in double, by vqa_adm_wait.
#include "vqa_dev.hpp"
#include "vqa_kernels.hpp"

namespace vqa {

namespace {

constexpr int TW = 32, TH = 16;                // band tile
constexpr int EW = TW + 2, EH = TH + 2;        // + halo of one band sample
constexpr int IW = 2 * TW + 6, IH = 2 * TH + 6; // input samples: band index i reads inputs 2i - 1 .. 2i + 2

constexpr float LO0 = 0.482962913144690f, LO1 = 0.836516303737469f, LO2 = 0.224143868041857f, LO3 = -0.129409522550921f;
constexpr float HI0 = -0.129409522550921f, HI1 = -0.224143868041857f, HI2 = 0.836516303737469f, HI3 = -0.482962913144690f;
constexpr float COS2_1DEG = 0.99969541350954785f;   // cos^2(1 degree)

// One scale's input of both images of a group is a pair_src (vqa_dev.hpp; the fp32 a bands are centred already).  Borders:
// reflect_clamp is the DWT's index rule (|k|, then k >= n reads 2n - k - 1), then a clamp: positions no in-band sample reads
// stay in the plane.

struct adm_geo {
    int bw, bh;                      // band dims: ceil(h / 2), ceil(w / 2)
    int tiles_x, tiles;
    int top, bottom, left, right;    // the pooled region: rows [top, bottom), columns [left, right)
    float rf_hv, rf_d;
    int write_a;
};

// never contracted with the addition that follows: the num and the den sums of identical planes take the same roundings
__device__ __forceinline__ float cube(float x) { return __fmul_rn(__fmul_rn(x, x), x); }

// restored part of one band sample
__device__ __forceinline__ float adm_restore(float o, float t, bool flag)
{
    const float k = fminf(fmaxf(t / (o + 1e-30f), 0.f), 1.f);   // IEEE division: t == o gives exactly 1
    float r = k * o;
    if (flag && r > 0.f) r = fminf(100.f * r, t);
    if (flag && r < 0.f) r = fmaxf(100.f * r, t);
    return r;
}

// grid = (tiles * count, n_frames); block = 256
// a_out: [image][frame][plane of the group][bh][bw] fp32;  part: [frame][plane of the group][tile][6] doubles
template <typename T>
__global__ __launch_bounds__(256) void k_adm_scale(pair_src s, adm_geo g, int count, float *__restrict__ a_out,
                                                   double *__restrict__ part)
{
    __shared__ float in[2][IH][IW];       // after the vertical pass: M, the three |rf r| and the three |rf o| maps, [7][EH][EW]
    __shared__ float V[2][2][EH][IW];     // [image][L, Hh]
    __shared__ double red[6][4];
    const int f = blockIdx.y, n = gridDim.y, ch = blockIdx.x / g.tiles, tile = blockIdx.x % g.tiles;
    const int by0 = (tile / g.tiles_x) * TH, bx0 = (tile % g.tiles_x) * TW;
    const int t = threadIdx.x;
    const uint8_t *pr = s.ref + (int64_t)f * s.ref_fs + s.off[ch], *pd = s.dist + (int64_t)f * s.dist_fs + s.off[ch];
    // (1) tile position (j, c) holds input (2 by0 - 3 + j, 2 bx0 - 3 + c)
    for (int i = t; i < IH * IW; i += 256) {
        const int j = i / IW, c = i - j * IW;
        const int64_t o = (int64_t)reflect_clamp(2 * by0 - 3 + j, s.h) * s.row_stride + (int64_t)reflect_clamp(2 * bx0 - 3 + c, s.w) * s.step;
        in[0][j][c] = ld_centred<T>(pr + o, s.sc);
        in[1][j][c] = ld_centred<T>(pd + o, s.sc);
    }
    __syncthreads();
    // (2) band row by0 - 1 + e reads tile rows 2e .. 2e + 3
    for (int i = t; i < 2 * EH * IW; i += 256) {
        const int img = i / (EH * IW), k = i - img * (EH * IW), e = k / IW, c = k - e * IW;
        const float x0 = in[img][2 * e][c], x1 = in[img][2 * e + 1][c], x2 = in[img][2 * e + 2][c], x3 = in[img][2 * e + 3][c];
        V[img][0][e][c] = fmaf(LO3, x3, fmaf(LO2, x2, fmaf(LO1, x1, LO0 * x0)));
        V[img][1][e][c] = fmaf(HI3, x3, fmaf(HI2, x2, fmaf(HI1, x1, HI0 * x0)));
    }
    __syncthreads();
    float (*post)[EH][EW] = reinterpret_cast<float (*)[EH][EW]>(&in[0][0][0]);   // 7 * 18 * 34 floats < 2 * 38 * 70
    float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // num h, v, d; den h, v, d
    // (3) band column bx0 - 1 + ec reads columns 2 ec .. 2 ec + 3 of V
    for (int i = t; i < EH * EW; i += 256) {
        const int e = i / EW, ec = i - e * EW;
        const int bi = by0 - 1 + e, bj = bx0 - 1 + ec;
        float b[2][4];   // [image][a, v, h, d]
#pragma unroll
        for (int img = 0; img < 2; img++) {
            const float *L = &V[img][0][e][2 * ec], *H = &V[img][1][e][2 * ec];
            b[img][0] = fmaf(LO3, L[3], fmaf(LO2, L[2], fmaf(LO1, L[1], LO0 * L[0])));
            b[img][1] = fmaf(HI3, L[3], fmaf(HI2, L[2], fmaf(HI1, L[1], HI0 * L[0])));
            b[img][2] = fmaf(LO3, H[3], fmaf(LO2, H[2], fmaf(LO1, H[1], LO0 * H[0])));
            b[img][3] = fmaf(HI3, H[3], fmaf(HI2, H[2], fmaf(HI1, H[1], HI0 * H[0])));
        }
        const bool inband = bi >= 0 && bi < g.bh && bj >= 0 && bj < g.bw;
        const bool mine = inband && e >= 1 && e <= TH && ec >= 1 && ec <= TW;
        if (mine && g.write_a) {
            const int64_t plane = (int64_t)g.bh * g.bw;
            const int64_t at = ((int64_t)f * count + ch) * plane + (int64_t)bi * g.bw + bj;
            a_out[at] = b[0][0];
            a_out[(int64_t)n * count * plane + at] = b[1][0];
        }
        const float oh = b[0][2], ov = b[0][1], od = b[0][3], th = b[1][2], tv = b[1][1], td = b[1][3];
        const float dp = oh * th + ov * tv;
        const float om = oh * oh + ov * ov, tm = th * th + tv * tv;
        const bool flag = dp >= 0.f && dp * dp >= COS2_1DEG * om * tm;
        const float rh = adm_restore(oh, th, flag), rv = adm_restore(ov, tv, flag), rd = adm_restore(od, td, flag);
        post[0][e][ec] = fabsf(g.rf_hv * (th - rh)) + fabsf(g.rf_hv * (tv - rv)) + fabsf(g.rf_d * (td - rd));
        post[1][e][ec] = fabsf(g.rf_hv * rh);
        post[2][e][ec] = fabsf(g.rf_hv * rv);
        post[3][e][ec] = fabsf(g.rf_d * rd);
        post[4][e][ec] = fabsf(g.rf_hv * oh);
        post[5][e][ec] = fabsf(g.rf_hv * ov);
        post[6][e][ec] = fabsf(g.rf_d * od);
    }
    __syncthreads();
    // (4) thread = (column, rows r and r + 8) of the tile
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const int e = 1 + (t >> 5) + 8 * k, ec = 1 + (t & 31);
        const int bi = by0 - 1 + e, bj = bx0 - 1 + ec;
        if (bi >= g.top && bi < g.bottom && bj >= g.left && bj < g.right) {
            // the neighbours by the band's border rule: -1 reads 1, n reads n - 1 (a band of one row or column reads itself)
            int up = bi - 1, dn = bi + 1, lf = bj - 1, rt = bj + 1;
            up = up < 0 ? min(1, g.bh - 1) : up;
            dn = dn >= g.bh ? g.bh - 1 : dn;
            lf = lf < 0 ? min(1, g.bw - 1) : lf;
            rt = rt >= g.bw ? g.bw - 1 : rt;
            const int eu = up - (by0 - 1), ed = dn - (by0 - 1), el = lf - (bx0 - 1), er = rt - (bx0 - 1);
            const float nb = post[0][eu][el] + post[0][eu][ec] + post[0][eu][er] + post[0][e][el] + post[0][e][er] +
                             post[0][ed][el] + post[0][ed][ec] + post[0][ed][er];
            const float thr = post[0][e][ec] * (1.f / 15.f) + nb * (1.f / 30.f);
#pragma unroll
            for (int b = 0; b < 3; b++) {
                acc[b] = __fadd_rn(acc[b], cube(fmaxf(post[1 + b][e][ec] - thr, 0.f)));
                acc[3 + b] = __fadd_rn(acc[3 + b], cube(post[4 + b][e][ec]));
            }
        }
    }
    // (5)
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const double v = wave_sum((double)acc[k]);
        if (lane_id() == 0) red[k][wave_id()] = v;
    }
    __syncthreads();
    if (t < 6) part[(((int64_t)f * count + ch) * g.tiles + tile) * 6 + t] = ((red[t][0] + red[t][1]) + red[t][2]) + red[t][3];
}

// grid = (count, n_frames); block = 64.  sums: [frame][plane of the submit][scale][6] doubles
__global__ __launch_bounds__(64) void k_adm_reduce(const double *__restrict__ part, int tiles, int count, int scale, int n_planes,
                                                   int4 plane_index, double *__restrict__ sums)
{
    const int ch = blockIdx.x, f = blockIdx.y, l = threadIdx.x;
    const double *p = part + ((int64_t)f * count + ch) * tiles * 6;
    double a[6] = {0, 0, 0, 0, 0, 0};
    for (int i = l; i < tiles; i += 64)
#pragma unroll
        for (int k = 0; k < 6; k++) a[k] += p[(int64_t)i * 6 + k];
    const int pi = ch == 0 ? plane_index.x : ch == 1 ? plane_index.y : ch == 2 ? plane_index.z : plane_index.w;
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const double v = wave_sum(a[k]);
        if (l == 0) sums[(((int64_t)f * n_planes + pi) * ADM_LEVELS + scale) * 6 + k] = v;
    }
}

} // namespace

// Q(lambda, theta) = 2 * 0.495 * 10^(0.466 log10(2^(lambda + 1) 0.401 g[theta] / rho)^2) / A[lambda][theta], rho = 3 * 1080 pi / 180
void adm_rf(int scale, double *rf_hv, double *rf_d)
{
    static const double A[4][4] = {{0.62171, 0.67234, 0.72709, 0.67234}, {0.34537, 0.41317, 0.49428, 0.41317},
                                   {0.18004, 0.22727, 0.28688, 0.22727}, {0.091401, 0.11792, 0.15214, 0.11792}};
    static const double gain[4] = {1.501, 1.0, 0.534, 1.0};
    const double rho = 3.0 * 1080.0 * M_PI / 180.0;
    double q[3];
    for (int theta = 1; theta <= 2; theta++) {
        const double l = log10((double)(1 << (scale + 1)) * 0.401 * gain[theta] / rho);
        q[theta] = 2.0 * 0.495 * pow(10.0, 0.466 * l * l) / A[scale][theta];
    }
    *rf_hv = 1.0 / q[1];
    *rf_d = 1.0 / q[2];
}

void adm_finalize(const double *sums, int h, int w, vqa_adm_metrics *out)
{
    double tn = 0.0, td = 0.0;
    int bh = h, bw = w;
    for (int s = 0; s < ADM_LEVELS; s++) {
        bh = (bh + 1) / 2;
        bw = (bw + 1) / 2;
        const double c = cbrt((double)adm_region_of(bh, bw).area / 32.0);
        double num = 0.0, den = 0.0;
        for (int b = 0; b < 3; b++) {
            num += cbrt(sums[s * 6 + b]) + c;
            den += cbrt(sums[s * 6 + 3 + b]) + c;
        }
        out->num[s] = num;
        out->den[s] = den;
        out->scale[s] = num / den;   // den >= 3 cbrt(area / 32) > 0
        tn += num;
        td += den;
    }
    const double floor_ = 1e-10 * (double)h * (double)w / (1920.0 * 1080.0);
    if (tn < floor_) tn = 0.0;
    if (td < floor_) td = 0.0;
    out->adm2 = td == 0.0 ? 1.0 : tn / td;
}

void launch_adm_scale(hipStream_t st, const uint8_t *ref, const uint8_t *dist, int n, int64_t ref_frame_stride,
                      int64_t dist_frame_stride, const vqa_plane_desc *planes, const int *idx, int count, int depth, int scale,
                      float *scratch, double *part)
{
    if (n <= 0 || count <= 0 || scale < 0 || scale >= ADM_LEVELS) return;
    const adm_layout L = adm_levels(n, count, planes[idx[0]].height, planes[idx[0]].width);
    pair_src s;
    s.w = L.w[scale]; s.h = L.h[scale];
    if (scale == 0) {
        const vqa_plane_desc &pd = planes[idx[0]];
        s.ref = ref; s.dist = dist; s.ref_fs = ref_frame_stride; s.dist_fs = dist_frame_stride;
        group_slots(planes, idx, count, s.off, nullptr);
        s.row_stride = pd.row_stride; s.step = pd.pixel_step;
        s.sc = 1.f / (float)(1 << (depth - 8));
    } else {
        const int64_t plane = (int64_t)s.h * s.w * sizeof(float);
        s.ref = (const uint8_t *)(scratch + L.off[scale]);
        s.dist = s.ref + (int64_t)n * count * plane;
        s.ref_fs = s.dist_fs = count * plane;
        for (int i = 0; i < 4; i++) s.off[i] = (i < count ? i : 0) * plane;
        s.row_stride = (int64_t)s.w * sizeof(float); s.step = sizeof(float);
        s.sc = 1.f;
    }
    adm_geo g;
    g.bw = L.w[scale + 1]; g.bh = L.h[scale + 1];
    g.tiles_x = (g.bw + TW - 1) / TW;
    g.tiles = adm_tiles(g.bh, g.bw);
    const adm_region R = adm_region_of(g.bh, g.bw);
    g.top = R.top; g.bottom = R.bottom; g.left = R.left; g.right = R.right;
    double rf_hv, rf_d;
    adm_rf(scale, &rf_hv, &rf_d);
    g.rf_hv = (float)rf_hv; g.rf_d = (float)rf_d;
    g.write_a = scale + 1 < ADM_LEVELS;
    float *a_out = g.write_a ? scratch + L.off[scale + 1] : scratch;
    const dim3 grid(g.tiles * count, n), block(256);
    if (scale > 0)
        hipLaunchKernelGGL((k_adm_scale<float>), grid, block, 0, st, s, g, count, a_out, part);
    else if (depth > 8)
        hipLaunchKernelGGL((k_adm_scale<uint16_t>), grid, block, 0, st, s, g, count, a_out, part);
    else
        hipLaunchKernelGGL((k_adm_scale<uint8_t>), grid, block, 0, st, s, g, count, a_out, part);
}

void launch_adm_reduce(hipStream_t st, const double *part, int n, const vqa_plane_desc *planes, const int *idx, int count,
                       int n_planes, int scale, double *sums)
{
    if (n <= 0 || count <= 0) return;
    const adm_layout L = adm_levels(n, count, planes[idx[0]].height, planes[idx[0]].width);
    int p4[4];
    group_slots(planes, idx, count, nullptr, p4);
    const int4 pi = make_int4(p4[0], p4[1], p4[2], p4[3]);
    hipLaunchKernelGGL(k_adm_reduce, dim3(count, n), dim3(64), 0, st, part, adm_tiles(L.h[scale + 1], L.w[scale + 1]), count, scale,
                       n_planes, pi, sums);
}

} // namespace vqa
