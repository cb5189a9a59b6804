// vqa_capi.hip — the C ABI declared in include/vqa.h: context, memory, and the
// orchestration of the gfx950 kernels for one batch of frames.
//
// No CPU fallback lives here: every metric is produced by a HIP kernel or the
// call fails.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <optional>
#include <string>
#include <tuple>
#include <vector>

#include "vqa_kernels.hpp"

using namespace vqa;

namespace {

struct dbuf {
    void *p = nullptr;
    size_t cap = 0;
};

struct hbuf {   // pinned host staging of result records (grow-only, like dbuf)
    void *p = nullptr;
    size_t cap = 0;
};

struct resize_tabs {
    int32_t *xofs = nullptr, *xa = nullptr, *yofs = nullptr, *yb = nullptr;
    int mode = 0;
};

// one axis of the resampler (k_scale.hip) on the device, and the widest source footprint of a destination tile along it
struct scale_tabs {
    int32_t *k = nullptr, *xmin = nullptr, *count = nullptr;
    int ksize = 0, span_w = 0, span_h = 0;   // the footprint of SCALE_TILE_W / SCALE_TILE_H consecutive outputs
    int64_t abs_sum = 0;                     // the largest sum |k| of a row
};

inline int align_up(int v, int a) { return (v + a - 1) / a * a; }

// The plane-batch kinds: each has one batch_slot in the ctx, and a batch of one kind can be pending next to a batch of every
// other kind and the complexity batch.  A new kind adds its name here; busy() and release_scratch() walk the slots.
enum batch_kind {
    KIND_QUALITY,     // vqa_plane_metrics per entry (its extras are named members of the ctx: qpartials, qms_*)
    KIND_VIF,         // vqa_vif_metrics per entry; work: levels 1..3 of the largest plane group seen, the integer totals
    KIND_ADM,         // six sums per (entry, scale); work: the a bands of scales 0..2 of the largest plane group, one scale's tile partials
    KIND_MOTION,      // one integer total per entry (host frames and prev0: mot_stage, mot_prev)
    KIND_SITI,        // SITI_WORDS per entry (host frames and prev0: siti_stage, siti_prev)
    KIND_PSNR_HVS,    // PSNR_HVS_WORDS per entry
    KIND_CIEDE,       // one word per frame
    KIND_GMSD,        // GMSD_WORDS per entry
    KIND_CAMBI,       // CAMBI_WORDS per entry; work: the scales and histograms of the largest group of a slice
    KIND_XPSNR,       // the words per frame and block (prev0 of host frames: xpsnr_prev)
    KIND_HAARPSI,     // HAARPSI_WORDS per entry
    KIND_VCA,         // VCA_WORDS per entry, then the block map of n + 1 slots (pinned host: without the first slot); work: the tables
                      // of k_vca_blocks (host frames and prev0: SI/TI's siti_stage, siti_prev)
    KIND_ARTIFACTS,   // ARTIFACTS_WORDS per entry
    KIND_BRISQUE,     // BRISQUE_WORDS per entry; work: the scale-1 planes and strips of the largest plane group of a slice
    KIND_MDSI,        // MDSI_WORDS per frame; work: the map of g of a slice
    KIND_ITP,         // ITP_WORDS per frame
    KIND_PU21,        // PU21_WORDS per frame; work: the two q_Y maps of one sub-slice; lab build: the maps of the whole last batch
    KIND_FSIM,        // FSIM_WORDS per frame; work: the intermediates and the p maps of one sub-slice; lab build: the maps of the whole last batch
    KIND_SIGSTATS,    // SIGSTATS_WORDS per entry, then the row and column sums of every entry; work: the histograms of one sub-slice
                      // (host frames and prev0: SI/TI's siti_stage, siti_prev)
    KIND_SCALE,       // no result words: the batch writes the caller's dst (host frames: scale_stage)
    KIND_ALIGN,       // one word per (distorted frame, band column), then E of every distorted and every reference frame; the two
                      // frame counts, offset and radius of the batch in flight are named members of the ctx (align_*)
    KIND_SHIFT,       // one word per (frame, dy, dx), then E_d of every frame; the frame count and radius of the batch in flight are
                      // named members of the ctx (shift_*)
    KIND_LIGHT,       // LIGHT_WORDS per frame, then (want_histogram) the histograms of every frame in the pinned copy only; work: the
                      // table T on the device, the histograms of one sub-slice; the table's host copy and the histogram switch of
                      // the batch in flight are named members of the ctx (light_*)
    KIND_SIG,         // VQA_SIG_BYTES bytes per frame (host frames: qstage_dist)
    KIND_SIGX,        // the words of diag, then the words of best; work: the staged signatures of either side; the two counts of
                      // the batch in flight are named members of the ctx (sigx_*)
    KIND_COLORFIT,    // COLORFIT_WORDS per frame, then (want_tables) the table words of the submit; their count is a named member
                      // of the ctx (colorfit_table_words)
    KIND_CONFORM,     // no result words: the batch writes the caller's dst; work: host frames staged (0), the frame index and the
                      // tables on the device (1); the pinned copy holds what (1) is filled from
    KIND_CONVERT,     // no result words: the batch writes the caller's dst; work: host frames staged (0)
    KIND_FIELDS,      // FIELDS_WORDS per frame; work: host frames staged (0), prev0 (1); whether frame 0 had a predecessor is a
                      // named member of the ctx (fields_prev0)
    KIND_WEAVE,       // no result words: the batch writes the caller's dst; work: host frames staged (0), the two frame indices on
                      // the device (1); the pinned copy holds what (1) is filled from
    KIND_COUNT
};

// What every plane-batch kind keeps: its result words on the device and their pinned host copy, the kind's own work buffers
// (each body names them through local references) and the batch in flight - its entries (0 = idle) and the geometry the host
// needs to finish the records.  Host frames are staged in named members of the ctx, which the kinds share.
struct batch_slot {
    dbuf dev, work[3];
    hbuf host;
    int entries = 0, planes = 0, depth = 8, w[4] = {0}, h[4] = {0};
};

// one cached per-geometry table set and when it was last handed out (least recently used goes first, vqa.h "Memory")
template <class T> struct cached {
    T v;
    uint64_t used = 0;
};

} // namespace

struct vqa_ctx {
    int device = -1;
    hipStream_t stream = nullptr;
    hipStream_t side[3] = {nullptr, nullptr, nullptr};   // VQA_OPT_OVERLAP: block-SAD, the Canny chain and the full-frame DCT on their own streams
    hipEvent_t ev_fork = nullptr, ev_join[3] = {nullptr, nullptr, nullptr};
    hipEvent_t ev_xctx = nullptr;   // vqa_stream_wait: "everything enqueued on this ctx so far" for another ctx's stream to wait on
    hipEvent_t fb_ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}; // Farneback: expansions of level k ready (0..3), planes ready (4), chunk done (5)
    std::string last_err;
    // options (vqa_set_option)
    bool opt_overlap = true, opt_hyst_stats = false;
    // -DVQA_TEST_SEAMS only (lab build; read from the environment once, in vqa_create)
    int seam_hyst_max_rounds = 0;   // VQA_HYST_MAX_ROUNDS: the hysteresis tail's round bound (0 = the shipped bound)
    int seam_hyst_rescue_max_rounds = 0; // VQA_HYST_RESCUE_MAX_ROUNDS: the rescue pass's bound (0 = the proof's: edge_weak + 2)
    long seam_fail_at = 0;          // VQA_FAIL_ENSURE_AT=N: the N-th scratch reservation of this ctx reports VQA_ERR_OOM
    long seam_ensure_calls = 0;
    long long seam_fb_chunk_bytes = 0; // VQA_FB_CHUNK_BYTES: Farneback's scratch budget per chunk (0 = the shipped 12 GiB): lets a small batch span chunks
    int seam_qslice = 0;            // VQA_QSLICE: the frames of one slice of a plane batch (0 = the shipped QSLICE): lets a small batch span slices
    int seam_fsim_sub = 0;          // VQA_FSIM_SUBSLICE: the frames of one sub-slice of an FSIM batch (0 = the shipped budget): lets a small batch span sub-slices
    int seam_pu21_sub = 0;          // VQA_PU21_SUBSLICE: the frames of one sub-slice of a PU21 batch (0 = the shipped budget): lets a small batch span sub-slices

    // device scratch (grow-only)
    dbuf gray_full, planeA, planeB, state, res_dev, partials, tile_flags, dirty0, dirty1, again_dev;
    dbuf stage_frames, stage_prev, dct_scratch, dct_pe, dct_pt;
    dbuf qpartials;
    dbuf qms_pyr, qms_dev;   // VQA_SSIM_MS: pyramid levels 1..4 of the largest plane group seen; per-entry scale means
    // pinned host staging
    hbuf res_host, qms_host;
    // host frames staged on the device, shared between kinds (the stream orders a batch behind whatever the ctx has in flight):
    // the two streams of a pair submit, and the one stream of a one-stream submit in qstage_dist; the reference stream and its
    // prev0 of a motion submit; the same of an SI/TI or a VCA submit; prev0 of an XPSNR submit
    dbuf qstage_ref, qstage_dist, mot_stage, mot_prev, siti_stage, siti_prev, xpsnr_prev;
    dbuf scale_stage;   // the host frames of a scale submit: its own, so the frames it reads outlive every pair staged after it
    // the plane-batch kinds: results, work buffers and the batch in flight
    batch_slot slot[KIND_COUNT];

    // per-geometry tables, at most VQA_TABLE_CACHE_GEOMETRIES of each kind (cache_put evicts the least recently used)
    std::map<std::tuple<int, int, int, int>, cached<resize_tabs>> tabs;
    std::map<std::tuple<int, int, int, int>, cached<fb_resize_tabs>> fb_tabs;
    std::map<int, cached<float *>> dct_mats;
    std::map<std::pair<int, int>, cached<fsim_tabs>> fsim_tables;   // k_fsim.hip: DFT matrices, filter bank and noise factors per grid (hd, wd)
    std::map<int, cached<dct_fft_plan>> fft_plans;  // k_dct_fft.hip: twiddle / post-twiddle tables per transform length
    std::map<std::tuple<int, int, int>, cached<scale_tabs>> scale_tables;   // k_scale.hip: one axis' tables per (filter, in, out)
    uint64_t cache_clock = 0;
    int dct_wave_slots = 0;                 // wave slots of THIS device for the marching DCT's chunking (set in vqa_create)
    dbuf fb_tmp, fb_blur, fb_img, fb_R, fb_M, fb_flow0, fb_flow1, fb_part;

    // pending work: the complexity batch here, a plane batch in its slot
    int pend_c = 0;
    bool pend_q_ms = false;   // the pending quality batch is a VQA_SSIM_MS one (qms_host holds its scales)
    int align_n_ref = 0, align_n_dist = 0, align_offset = 0, align_radius = 0;   // the pending alignment batch (slot[KIND_ALIGN])
    int shift_n = 0, shift_radius = 0;   // the pending registration batch (slot[KIND_SHIFT])
    int sigx_n_dist = 0, sigx_n_ref = 0; // the pending cross batch (slot[KIND_SIGX])
    bool light_hist = false;             // the pending light batch (slot[KIND_LIGHT]) keeps its histograms for the wait
    std::vector<uint64_t> light_table;   // the table of the last light submit: what slot[KIND_LIGHT].work[0] holds, and what the wait reads
    int64_t colorfit_table_words = 0;    // the pending colour-fit batch (slot[KIND_COLORFIT]) keeps that many table words (0: none)
    bool fields_prev0 = false;           // frame 0 of the pending fields batch (slot[KIND_FIELDS]) had a predecessor
    int last_u_n = 0, last_u_w = 0, last_u_h = 0;   // lab build: what PU21's kept maps hold
    int last_f_n = 0, last_f_w = 0, last_f_h = 0;   // lab build: what FSIM's kept maps hold (the downsampled grid)
    bool pend_c_prev0 = false, pend_c_tail_only = false;
    // geometry of the last complexity batch (debug reads)
    int last_n = 0, last_h = 0, last_w = 0, last_ph = 0, last_pw = 0, last_pp = 0, last_gp = 0;
    bool last_resized = false, last_has_full = false, last_has_state = false, last_has_planes = false;
    // what the last chunk of the last Farneback submit left resident (vqa_debug_read_farneback): valid from the end of
    // run_farneback until the next one begins, fails or the buffers are released
    struct {
        bool valid = false, first_valid = false; // first_valid: pair 0 / plane 0 of the submit exist (prev0 was given)
        int levels = 0, h = 0, w = 0, lh[4] = {0, 0, 0, 0}, lw[4] = {0, 0, 0, 0};
        size_t Roff[4] = {0, 0, 0, 0};           // floats from fb_R to level k's expansions: [planes][5][lh][lw]
        int flow_buf = 0;                         // the final flow [pairs][h][w][2] is in fb_flow0 (0) or fb_flow1 (1)
        int first_pair = 0, pairs = 0;            // the chunk's pairs, counted from the submit's first
    } last_fb;

    // per-kernel timing
    bool prof_on = false;
    std::vector<hipEvent_t> ev_pool;                   // recycled events
    std::vector<std::tuple<int, hipEvent_t, hipEvent_t>> ev_open; // (kernel id, start, stop) not yet read
    double prof_ms[VQA_K_EAVE] = {0};
    int64_t prof_n[VQA_K_EAVE] = {0};
};

namespace {
// RAII bracket: records start now and stop at scope exit when profiling is on.
struct prof_scope {
    vqa_ctx *c; int id; hipEvent_t a = nullptr, b = nullptr;
    static hipEvent_t get(vqa_ctx *c)
    {
        if (!c->ev_pool.empty()) { hipEvent_t e = c->ev_pool.back(); c->ev_pool.pop_back(); return e; }
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        return e;
    }
    hipStream_t s;
    prof_scope(vqa_ctx *c_, int id_, hipStream_t s_ = nullptr) : c(c_), id(id_), s(s_ ? s_ : c_->stream)
    {
        if (!c->prof_on) return;
        a = get(c); b = get(c);
        if (a && b) (void)hipEventRecord(a, s);
    }
    ~prof_scope()
    {
        if (!a || !b) return;
        (void)hipEventRecord(b, s);
        c->ev_open.emplace_back(id, a, b);
    }
};

// after the stream has been synchronised: fold the open event pairs into the totals
void prof_collect(vqa_ctx *c)
{
    for (auto &t : c->ev_open) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, std::get<1>(t), std::get<2>(t)) == hipSuccess) {
            c->prof_ms[std::get<0>(t)] += ms;
            c->prof_n[std::get<0>(t)] += 1;
        }
        c->ev_pool.push_back(std::get<1>(t));
        c->ev_pool.push_back(std::get<2>(t));
    }
    c->ev_open.clear();
}

// a failed submit: its event pairs go back to the pool unread
void prof_discard(vqa_ctx *c)
{
    for (auto &t : c->ev_open) { c->ev_pool.push_back(std::get<1>(t)); c->ev_pool.push_back(std::get<2>(t)); }
    c->ev_open.clear();
}
} // namespace

#define HIPCHK(ctx, call)                                                                                  \
    do {                                                                                                   \
        hipError_t e_ = (call);                                                                            \
        if (e_ != hipSuccess) {                                                                            \
            char b_[512];                                                                                  \
            snprintf(b_, sizeof b_, "%s -> %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            (ctx)->last_err = b_;                                                                          \
            return e_ == hipErrorOutOfMemory ? VQA_ERR_OOM : VQA_ERR_HIP;                                  \
        }                                                                                                  \
    } while (0)

// every stream this ctx may have work on (the main one and, once created, the three side streams of VQA_OPT_OVERLAP)
static int sync_all(vqa_ctx *c)
{
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < 3; i++)
        if (c->side[i]) HIPCHK(c, hipStreamSynchronize(c->side[i]));
    return VQA_OK;
}

// a submitted batch of any kind has not been waited for
static bool busy(const vqa_ctx *c)
{
    for (const batch_slot &s : c->slot)
        if (s.entries) return true;
    return c->pend_c != 0;
}

// lab build: VQA_FAIL_ENSURE_AT=N makes the N-th device reservation of this ctx (scratch buffer or table) report OOM
static inline bool seam_reservation_fails(vqa_ctx *c)
{
#ifdef VQA_TEST_SEAMS
    if (c->seam_fail_at > 0 && ++c->seam_ensure_calls == c->seam_fail_at) {
        c->last_err = "test seam: device reservation #" + std::to_string(c->seam_fail_at) + " made to fail";
        return true;
    }
#else
    (void)c;
#endif
    return false;
}

static int ensure(vqa_ctx *c, dbuf &b, size_t bytes)
{
    if (seam_reservation_fails(c)) return VQA_ERR_OOM;
    if (bytes <= b.cap) return VQA_OK;
    // contents are scratch; a pending async user is on one of our own streams
    if (int rc = sync_all(c)) return rc;
    if (b.p) HIPCHK(c, hipFree(b.p));
    b.p = nullptr; b.cap = 0;
    const size_t want = bytes + bytes / 8 + 256;
    HIPCHK(c, hipMalloc(&b.p, want));
    b.cap = want;
    return VQA_OK;
}

static int ensure_pinned(vqa_ctx *c, hbuf &b, size_t bytes)
{
    if (bytes <= b.cap) return VQA_OK;
    if (int rc = sync_all(c)) return rc;
    if (b.p) HIPCHK(c, hipHostFree(b.p));
    b.p = nullptr; b.cap = 0;
    HIPCHK(c, hipHostMalloc(&b.p, bytes, hipHostMallocDefault));
    b.cap = bytes;
    return VQA_OK;
}

static void release(dbuf &b)
{
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr; b.cap = 0;
}

static void release(hbuf &b)
{
    if (b.p) (void)hipHostFree(b.p);
    b.p = nullptr; b.cap = 0;
}

// The device arrays of ONE table set while it is being built: whatever was reserved is given back unless the whole set
// made it (commit) - a failure after the first hipMalloc used to drop the earlier pointers.
struct table_builder {
    vqa_ctx *c;
    std::vector<void *> ptrs;
    bool kept = false;
    explicit table_builder(vqa_ctx *c_) : c(c_) {}
    ~table_builder()
    {
        if (!kept)
            for (void *p : ptrs) (void)hipFree(p);
    }
    template <class T> int upload(T **out, const void *src, size_t bytes)
    {
        if (seam_reservation_fails(c)) return VQA_ERR_OOM;
        void *d = nullptr;
        HIPCHK(c, hipMalloc(&d, bytes ? bytes : 1));
        ptrs.push_back(d);
        if (bytes) HIPCHK(c, hipMemcpy(d, src, bytes, hipMemcpyHostToDevice));
        *out = (T *)d;
        return VQA_OK;
    }
    void commit() { kept = true; }
};

static void free_table(resize_tabs &t)
{
    (void)hipFree(t.xofs); (void)hipFree(t.xa); (void)hipFree(t.yofs); (void)hipFree(t.yb);
}
static void free_table(fb_resize_tabs &t)
{
    (void)hipFree(t.xofs); (void)hipFree(t.xa); (void)hipFree(t.yofs); (void)hipFree(t.yb);
    if (t.cols) (void)hipFree(t.cols);
    if (t.rows) (void)hipFree(t.rows);
    if (t.sx) (void)hipFree(t.sx);
    if (t.sy) (void)hipFree(t.sy);
}
static void free_table(float *&m) { (void)hipFree(m); }
static void free_table(scale_tabs &t) { (void)hipFree(t.k); (void)hipFree(t.xmin); (void)hipFree(t.count); }
static void free_table(fsim_tabs &t) { (void)hipFree(t.wh); (void)hipFree(t.ww); (void)hipFree(t.filt); }
static void free_table(dct_fft_plan &P) { (void)hipFree((void *)P.tw); (void)hipFree((void *)P.post); }

// lookup that refreshes the entry's stamp
template <class Map, class Key, class T> static bool cache_get(vqa_ctx *c, Map &m, const Key &key, T &out)
{
    auto it = m.find(key);
    if (it == m.end()) return false;
    it->second.used = ++c->cache_clock;
    out = it->second.v;
    return true;
}

// insert; beyond VQA_TABLE_CACHE_GEOMETRIES entries the least recently used set is freed first.  One submit asks for
// fewer sets of a kind than the bound (<= 6: the Farneback pyramid's), and every set it asked for carries a newer stamp
// than any other, so an eviction can only hit tables of EARLIER submits - whose kernels have completed (a submit is
// refused while another is pending); sync_all before the free is the belt to those braces.
template <class Map, class Key, class T> static int cache_put(vqa_ctx *c, Map &m, const Key &key, const T &v)
{
    while (m.size() >= (size_t)VQA_TABLE_CACHE_GEOMETRIES) {
        auto old = m.begin();
        for (auto it = m.begin(); it != m.end(); ++it)
            if (it->second.used < old->second.used) old = it;
        if (int rc = sync_all(c)) return rc;
        free_table(old->second.v);
        m.erase(old);
    }
    cached<T> e;
    e.v = v;
    e.used = ++c->cache_clock;
    m[key] = e;
    return VQA_OK;
}

// OpenCV resize.cpp coefficient tables for INTER_LINEAR on 8-bit data (see
// DESIGN.md §4.2; restated independently of the oracle's copy).
static void build_axis(int ssize, int dsize, bool is_x, std::vector<int32_t> &ofs, std::vector<int32_t> &coef)
{
    ofs.resize(dsize);
    coef.resize(2 * (size_t)dsize);
    const double scale = 1.0 / ((double)dsize / (double)ssize);
    for (int d = 0; d < dsize; d++) {
        float fr = (float)((d + 0.5) * scale - 0.5);
        int s = (int)std::floor(fr);
        fr -= (float)s;
        if (is_x) {
            if (s < 0) { fr = 0.f; s = 0; }
            if (s >= ssize - 1) { fr = 0.f; s = ssize - 1; }
        }
        ofs[d] = s;
        long a0 = lrintf((1.f - fr) * 2048.f), a1 = lrintf(fr * 2048.f);
        a0 = a0 < -32768 ? -32768 : (a0 > 32767 ? 32767 : a0);
        a1 = a1 < -32768 ? -32768 : (a1 > 32767 ? 32767 : a1);
        coef[2 * (size_t)d] = (int32_t)a0;
        coef[2 * (size_t)d + 1] = (int32_t)a1;
    }
}

static int get_tabs(vqa_ctx *c, int h, int w, int rh, int rw, resize_tabs &out)
{
    auto key = std::make_tuple(h, w, rh, rw);
    if (cache_get(c, c->tabs, key, out)) return VQA_OK;
    resize_tabs t;
    t.mode = (w == 2 * rw && h == 2 * rh) ? 1 : 0;
    std::vector<int32_t> xo, xa, yo, yb;
    build_axis(w, rw, true, xo, xa);
    build_axis(h, rh, false, yo, yb);
    table_builder tb(c);
    int rc;
    if ((rc = tb.upload(&t.xofs, xo.data(), sizeof(int32_t) * rw))) return rc;
    if ((rc = tb.upload(&t.xa, xa.data(), sizeof(int32_t) * 2 * rw))) return rc;
    if ((rc = tb.upload(&t.yofs, yo.data(), sizeof(int32_t) * rh))) return rc;
    if ((rc = tb.upload(&t.yb, yb.data(), sizeof(int32_t) * 2 * rh))) return rc;
    if ((rc = cache_put(c, c->tabs, key, t))) return rc;
    tb.commit();
    out = t;
    return VQA_OK;
}

// one axis of the resampler: the tables of include/vqa.h (vqa_scale_submit); an axis whose size does not change is a copy
static int get_scale_tabs(vqa_ctx *c, int filter, int in, int out, scale_tabs &res)
{
    auto key = std::make_tuple(filter, in, out);
    if (cache_get(c, c->scale_tables, key, res)) return VQA_OK;
    scale_tabs t;
    t.ksize = in == out ? 1 : scale_ksize(filter, in, out);
    std::vector<int32_t> k((size_t)out * t.ksize), xmin(out), count(out);
    if (in == out) {
        for (int x = 0; x < out; x++) { k[x] = 1 << SCALE_BITS; xmin[x] = x; count[x] = 1; }
    } else {
        scale_build_axis(filter, in, out, k.data(), xmin.data(), count.data());
    }
    for (int x = 0; x < out; x++) {
        int64_t a = 0;
        for (int j = 0; j < t.ksize; j++) a += std::abs((int64_t)k[(size_t)x * t.ksize + j]);
        t.abs_sum = a > t.abs_sum ? a : t.abs_sum;
    }
    t.span_w = scale_footprint(xmin.data(), count.data(), out, SCALE_TILE_W);
    t.span_h = scale_footprint(xmin.data(), count.data(), out, SCALE_TILE_H);
    table_builder tb(c);
    int rc;
    if ((rc = tb.upload(&t.k, k.data(), sizeof(int32_t) * k.size()))) return rc;
    if ((rc = tb.upload(&t.xmin, xmin.data(), sizeof(int32_t) * out))) return rc;
    if ((rc = tb.upload(&t.count, count.data(), sizeof(int32_t) * out))) return rc;
    if ((rc = cache_put(c, c->scale_tables, key, t))) return rc;
    tb.commit();
    res = t;
    return VQA_OK;
}

// orthonormal DCT-II matrix C[k][i] = s_k cos(pi (2i+1) k / 2N)  (what cv2.dct applies)
static int get_dct_matrix(vqa_ctx *c, int n, float **out)
{
    if (cache_get(c, c->dct_mats, n, *out)) return VQA_OK;
    std::vector<float> m((size_t)n * n);
    for (int k = 0; k < n; k++) {
        const double s = k == 0 ? std::sqrt(1.0 / n) : std::sqrt(2.0 / n);
        for (int i = 0; i < n; i++) m[(size_t)k * n + i] = (float)(s * std::cos(M_PI * (2.0 * i + 1.0) * k / (2.0 * n)));
    }
    float *d = nullptr;
    table_builder tb(c);
    int rc;
    if ((rc = tb.upload(&d, m.data(), sizeof(float) * m.size()))) return rc;
    if ((rc = cache_put(c, c->dct_mats, n, d))) return rc;
    tb.commit();
    *out = d;
    return VQA_OK;
}

// k_dct_fft.hip's plan for length n (tables formed in double, rounded once); VQA_ERR_UNSUPPORTED if n does not factor
static int get_fft_plan(vqa_ctx *c, int n, dct_fft_plan *out)
{
    if (cache_get(c, c->fft_plans, n, *out)) return VQA_OK;
    dct_fft_plan P;
    memset(&P, 0, sizeof P);
    P.n = n;
    if (!dct_fft_factor(n, P.radix, &P.npass)) return VQA_ERR_UNSUPPORTED;
    for (int p = 0, Ns = 1; p < P.npass; Ns *= P.radix[p], p++) {
        P.m[p] = n / P.radix[p];
        P.tstep[p] = n / (Ns * P.radix[p]);
        // j / Ns = mulhi(j, ceil(2^32 / Ns)), exact while j * Ns < 2^32 (n <= 4000); the first pass (Ns = 1) does not use it
        P.ns_magic[p] = Ns == 1 ? 0u : (uint32_t)((0x100000000ull + (uint64_t)Ns - 1) / (uint64_t)Ns);
    }
    std::vector<float2> tw((size_t)n), post((size_t)n);
    for (int m = 0; m < n; m++) {
        const double a = -2.0 * M_PI * (double)m / (double)n;
        tw[m] = make_float2((float)std::cos(a), (float)std::sin(a));
        const double s = m == 0 ? std::sqrt(1.0 / n) : std::sqrt(2.0 / n), b = M_PI * (double)m / (2.0 * n);
        post[m] = make_float2((float)(s * std::cos(b)), (float)(s * std::sin(b)));
    }
    float2 *dtw = nullptr, *dpost = nullptr;
    table_builder tb(c);
    int rc;
    if ((rc = tb.upload(&dtw, tw.data(), sizeof(float2) * n))) return rc;
    if ((rc = tb.upload(&dpost, post.data(), sizeof(float2) * n))) return rc;
    P.tw = dtw; P.post = dpost;
    if ((rc = cache_put(c, c->fft_plans, n, P))) return rc;
    tb.commit();
    *out = P;
    return VQA_OK;
}

// k_fsim.hip's tables for an hd x wd grid, formed in double on the host
static int get_fsim_tabs(vqa_ctx *c, int hd, int wd, fsim_tabs *out)
{
    const auto key = std::make_pair(hd, wd);
    if (cache_get(c, c->fsim_tables, key, *out)) return VQA_OK;
    const size_t N = (size_t)hd * wd;
    fsim_tabs t;
    std::vector<double> filt(16 * N), wh(2 * (size_t)hd * hd), ww(2 * (size_t)wd * wd);
    fsim_bank_host(hd, wd, filt.data(), t.c);
    fsim_twiddle_host(hd, wh.data());
    fsim_twiddle_host(wd, ww.data());
    table_builder tb(c);
    int rc;
    if ((rc = tb.upload(&t.wh, wh.data(), sizeof(double) * wh.size()))) return rc;
    if ((rc = tb.upload(&t.ww, ww.data(), sizeof(double) * ww.size()))) return rc;
    if ((rc = tb.upload(&t.filt, filt.data(), sizeof(double) * filt.size()))) return rc;
    if ((rc = cache_put(c, c->fsim_tables, key, t))) return rc;
    tb.commit();
    *out = t;
    return VQA_OK;
}

// ---- Farneback (k_farneback.hip): host-side constants, tables and the level loop ---------------------
// getGaussianKernel(ksize, sigma, CV_32F): taps formed and normalised in double, rounded to float; the
// fixed 1/4,1/2,1/4 kernel when sigma == 0 (restated independently of the oracle's copy)
static fb_taps fb_gauss_taps(int ksize, double sigma)
{
    fb_taps T;
    memset(&T, 0, sizeof T);
    T.ksize = ksize;
    if (sigma <= 0 && ksize == 3) { T.k[0] = 0.25f; T.k[1] = 0.5f; T.k[2] = 0.25f; return T; }
    double kd[32], sum = 0;
    const int r = ksize / 2;
    const double sc = -0.5 / (sigma * sigma);
    for (int i = 0; i < ksize; i++) { const double x = i - r; kd[i] = std::exp(sc * x * x); sum += kd[i]; }
    for (int i = 0; i < ksize; i++) T.k[i] = (float)(kd[i] / sum);
    return T;
}

// FarnebackPrepareGaussian(5, 1.2): taps and the four needed entries of inv(G) (G is block-sparse: closed form)
static fb_poly fb_poly_consts()
{
    fb_poly C;
    const int n = 5;
    const double sigma = 1.2;
    double s = 0;
    for (int x = -n; x <= n; x++) { C.g[x + n] = (float)std::exp(-x * x / (2 * sigma * sigma)); s += C.g[x + n]; }
    s = 1. / s;
    for (int x = -n; x <= n; x++) {
        C.g[x + n] = (float)(C.g[x + n] * s);
        C.xg[x + n] = (float)(x * C.g[x + n]);
        C.xxg[x + n] = (float)(x * x * C.g[x + n]);
    }
    double a = 0, b = 0, c = 0, d = 0;
    for (int y = -n; y <= n; y++)
        for (int x = -n; x <= n; x++) {
            const double gg = (double)C.g[y + n] * C.g[x + n];
            a += gg; b += gg * x * x; c += gg * x * x * x * x; d += gg * x * x * y * y;
        }
    const double det = a * (c * c - d * d) - 2 * b * b * (c - d);
    C.ig11 = 1. / b;
    C.ig03 = -b * (c - d) / det;
    C.ig33 = (a * c - b * b) / det;
    C.ig55 = 1. / d;
    return C;
}

static void fb_build_axis(int ssize, int dsize, bool is_x, std::vector<int32_t> &ofs, std::vector<float> &coef)
{
    ofs.resize(dsize);
    coef.resize(2 * (size_t)dsize);
    const double scale = 1.0 / ((double)dsize / (double)ssize);
    for (int d = 0; d < dsize; d++) {
        float f = (float)((d + 0.5) * scale - 0.5);
        int s = (int)std::floor(f);
        f -= (float)s;
        if (is_x) {
            if (s < 0) { f = 0.f; s = 0; }
            if (s >= ssize - 1) { f = 0.f; s = ssize - 1; }
        }
        ofs[d] = s;
        coef[2 * (size_t)d] = 1.f - f;
        coef[2 * (size_t)d + 1] = f;
    }
}

static int get_fb_tabs(vqa_ctx *c, int sh, int sw, int dh, int dw, fb_resize_tabs &out)
{
    auto key = std::make_tuple(sh, sw, dh, dw);
    if (cache_get(c, c->fb_tabs, key, out)) return VQA_OK;
    fb_resize_tabs t;
    t.mode = (sw == 2 * dw && sh == 2 * dh) ? 1 : 0;
    std::vector<int32_t> xo, yo;
    std::vector<float> xa, yb;
    fb_build_axis(sw, dw, true, xo, xa);
    fb_build_axis(sh, dh, false, yo, yb);
    table_builder tb(c);
    int rc;
    if ((rc = tb.upload(&t.xofs, xo.data(), sizeof(int32_t) * dw))) return rc;
    if ((rc = tb.upload(&t.xa, xa.data(), sizeof(float) * 2 * dw))) return rc;
    if ((rc = tb.upload(&t.yofs, yo.data(), sizeof(int32_t) * dh))) return rc;
    if ((rc = tb.upload(&t.yb, yb.data(), sizeof(float) * 2 * dh))) return rc;
    if (dw <= sw && dh <= sh) {
        // the samples of each level column / row as the fused level kernel wants them, and their extent per tile
        std::vector<int32_t> sx(2 * (size_t)dw), sy(2 * (size_t)dh);
        for (int d = 0; d < dw; d++) {
            sx[2 * d] = t.mode == 1 ? 2 * d : xo[d];
            sx[2 * d + 1] = t.mode == 1 ? 2 * d + 1 : (xo[d] + 1 < sw ? xo[d] + 1 : sw - 1);
        }
        for (int d = 0; d < dh; d++) {
            const int y0 = yo[d] < 0 ? 0 : (yo[d] > sh - 1 ? sh - 1 : yo[d]);
            const int y1 = yo[d] + 1 < 0 ? 0 : (yo[d] + 1 > sh - 1 ? sh - 1 : yo[d] + 1);
            sy[2 * d] = t.mode == 1 ? 2 * d : y0;
            sy[2 * d + 1] = t.mode == 1 ? 2 * d + 1 : y1;
        }
        auto span = [](const std::vector<int32_t> &v, int n, int tile) {
            int m = 0;
            bool mono = true;
            for (size_t i = 1; i < v.size(); i++) mono = mono && v[i] >= v[i - 1];
            if (!mono) return -1;
            for (int a = 0; a < n; a++) { // every window of `tile` consecutive level columns / rows, aligned or not
                const int b = (a + tile < n ? a + tile : n) - 1;
                const int e = v[2 * b + 1] - v[2 * a] + 1;
                m = e > m ? e : m;
            }
            return m;
        };
        t.span_x32 = span(sx, dw, 32); t.span_y8 = span(sy, dh, 8); t.span_y32 = span(sy, dh, 32);
        if (t.span_x32 > 0 && t.span_y8 > 0 && t.span_y32 > 0) {
            if ((rc = tb.upload(&t.sx, sx.data(), sizeof(int32_t) * sx.size()))) return rc;
            if ((rc = tb.upload(&t.sy, sy.data(), sizeof(int32_t) * sy.size()))) return rc;
        }
    }
    if (t.mode == 0 && (dw < sw || dh < sh)) {
        // what the bilinear taps read: columns xofs, min(xofs + 1, sw - 1); rows clamp(yofs), clamp(yofs + 1)
        std::vector<int32_t> cs, rs;
        std::vector<char> cm(sw, 0), rm(sh, 0);
        for (int d = 0; d < dw; d++) { cm[xo[d]] = 1; cm[xo[d] + 1 < sw ? xo[d] + 1 : sw - 1] = 1; }
        for (int d = 0; d < dh; d++) {
            const int y0 = yo[d] < 0 ? 0 : (yo[d] > sh - 1 ? sh - 1 : yo[d]);
            const int y1 = yo[d] + 1 < 0 ? 0 : (yo[d] + 1 > sh - 1 ? sh - 1 : yo[d] + 1);
            rm[y0] = 1; rm[y1] = 1;
        }
        for (int x = 0; x < sw; x++) if (cm[x]) cs.push_back(x);
        for (int y = 0; y < sh; y++) if (rm[y]) rs.push_back(y);
        t.nc = (int)cs.size(); t.nr = (int)rs.size();
        if ((rc = tb.upload(&t.cols, cs.data(), sizeof(int32_t) * t.nc))) return rc;
        if ((rc = tb.upload(&t.rows, rs.data(), sizeof(int32_t) * t.nr))) return rc;
    }
    if ((rc = cache_put(c, c->fb_tabs, key, t))) return rc;
    tb.commit();
    out = t;
    return VQA_OK;
}

// gray: n + 1 planes (slot 0 = the frame before the batch); pair i = planes i, i + 1 -> res[i].flow_mag_mean.
// Pairs are processed in chunks whose planes (expansions: 20 B/pixel) stay resident in a bounded scratch.
static int run_farneback(vqa_ctx *c, hipStream_t st, const uint8_t *gray, int gp, int64_t plane_stride, int n, int h,
                         int w, bool first_has_prev, vqa_frame_metrics *res)
{
    const double pyr_scale = 0.5;
    const int iters = 3, min_size = 32;
    int levels = 3, k;
    double scale = 1;
    for (k = 0; k < levels; k++) {
        scale *= pyr_scale;
        if (w * scale < min_size || h * scale < min_size) break;
    }
    levels = k;
    c->last_fb.valid = false; // the buffers are about to be re-reserved and rewritten; set again when every launch is in
    const fb_poly PC = fb_poly_consts();
    const size_t P = (size_t)h * w;
    // per pair ~59 B/pixel of scratch (planes: blur tmp 4 + blurred 4 + level image 4 + expansions of every level 26.7;
    // pairs: two flow fields 16; + 20 for the products of the lab build's two-kernel form); a chunk stays under ~12 GiB of the
    // 288: a 64-frame 1080p batch is ONE chunk (round 3's 3 GiB cut it into 21 + 21 + 21 + 1 pairs, and the
    // one-pair tail ran fifty launches on an empty chip)
#ifdef VQA_AB_VARIANTS
    const bool two_kernel = ab_knob("VQA_FB_VARIANT", 0) == 1;
#else
    const bool two_kernel = false;
#endif
    // the level image: one fused kernel (blur + resize); the three-kernel form is the fallback for levels whose patch
    // exceeds the LDS budget (and VQA_FB_LEVEL_VARIANT=1 in the lab build)
#ifdef VQA_AB_VARIANTS
    const bool three_kernel = ab_knob("VQA_FB_LEVEL_VARIANT", 0) == 1;
#else
    const bool three_kernel = false;
#endif
    // Level geometry (coarse to fine: k = levels .. 0) and where each level's expansions live: with VQA_OPT_OVERLAP the level
    // images and expansions of ALL levels are formed on a side stream (they depend on the gray planes only) while the main
    // stream runs the flow iterations of the coarser levels - the finest level's expansion, a quarter of the pre-pass work,
    // is ready by the time the iterations reach it.  Each level keeps its own expansion planes for that (4/3 of one level's).
    int lwk[4], lhk[4], ksz[4];
    double sig[4];
    size_t Roff[4], Rtot = 0;
    for (k = levels; k >= 0; k--) {
        scale = 1;
        for (int i = 0; i < k; i++) scale *= pyr_scale;
        sig[k] = (1. / scale - 1) * 0.5;
        ksz[k] = (int)std::lrint(sig[k] * 5) | 1;
        if (ksz[k] < 3) ksz[k] = 3;
        lwk[k] = (int)std::lrint(w * scale);
        lhk[k] = (int)std::lrint(h * scale);
    }
    // pairs per chunk: ~12 GiB of scratch, and never more than 80 % of what the device can give right now (what this ctx
    // already holds for Farneback counts as available: ensure() re-uses or replaces it).  If a reservation still fails -
    // another context or process took the memory in between - the chunk is halved and everything re-reserved, down to
    // one pair, before the submit reports VQA_ERR_OOM.
    dbuf *const fb_bufs[] = {&c->fb_tmp, &c->fb_blur, &c->fb_img, &c->fb_R, &c->fb_M, &c->fb_flow0, &c->fb_flow1, &c->fb_part};
    const size_t per_pair = (size_t)(two_kernel ? 72 : 59) * P;
    size_t budget = 12ull << 30;
    if (c->seam_fb_chunk_bytes > 0) budget = (size_t)c->seam_fb_chunk_bytes; // (lab build only: never set in the shipped library)
    {
        size_t free_b = 0, total_b = 0, held = 0;
        for (dbuf *b : fb_bufs) held += b->cap;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            const size_t avail = (size_t)((double)(free_b + held) * 0.8);
            if (avail < budget) budget = avail;
        } else {
            (void)hipGetLastError();
        }
    }
    int mc = (int)(budget / per_pair);
    mc = mc < 1 ? 1 : (mc > n ? n : mc);
    const bool piped = c->opt_overlap && !two_kernel && !three_kernel;
    int rc;
    for (;;) {
        Rtot = 0;
        for (k = levels; k >= 0; k--) { Roff[k] = Rtot; Rtot += (size_t)5 * lhk[k] * lwk[k] * (mc + 1); }
        int nb = fb_iter_max_blocks(h, w); // partial |flow| sums per pair: one per workgroup of the last iteration
#ifdef VQA_AB_VARIANTS
        if (fb_mag_blocks() > nb) nb = fb_mag_blocks();
#endif
        rc = ensure(c, c->fb_tmp, sizeof(float) * P * (mc + 1));
        if (!rc) rc = ensure(c, c->fb_blur, sizeof(float) * P * (mc + 1));
        if (!rc) rc = ensure(c, c->fb_img, sizeof(float) * P * (mc + 1));
        if (!rc) rc = ensure(c, c->fb_R, sizeof(float) * Rtot);
        if (!rc && two_kernel) rc = ensure(c, c->fb_M, sizeof(float) * 5 * P * mc);
        if (!rc) rc = ensure(c, c->fb_flow0, sizeof(float) * 2 * P * mc);
        if (!rc) rc = ensure(c, c->fb_flow1, sizeof(float) * 2 * P * mc);
        if (!rc) rc = ensure(c, c->fb_part, sizeof(double) * (size_t)nb * mc);
        if (rc != VQA_ERR_OOM || mc == 1 || c->last_err.compare(0, 10, "test seam:") == 0) break; // (an injected failure is not retried)
        (void)hipGetLastError();
        if (int rs = sync_all(c)) return rs;
        for (dbuf *b : fb_bufs) release(*b);
        mc = (mc + 1) / 2;
    }
    if (rc) return rc;
    float *tmp = (float *)c->fb_tmp.p, *blur = (float *)c->fb_blur.p, *img = (float *)c->fb_img.p;
    float *Rall = (float *)c->fb_R.p;
#ifdef VQA_AB_VARIANTS
    float *M = (float *)c->fb_M.p;
#endif
    float *flow = (float *)c->fb_flow0.p, *prev_flow = (float *)c->fb_flow1.p;
    hipStream_t sp = st; // the stream of the level images and expansions
    if (piped) {
        if (!c->side[0]) HIPCHK(c, hipStreamCreateWithFlags(&c->side[0], hipStreamNonBlocking)); // block-SAD's stream: idle in this mode
        for (int i = 0; i < 6; i++)
            if (!c->fb_ev[i]) HIPCHK(c, hipEventCreateWithFlags(&c->fb_ev[i], hipEventDisableTiming));
        sp = c->side[0];
        HIPCHK(c, hipEventRecord(c->fb_ev[4], st)); // the gray planes exist in st's order
        HIPCHK(c, hipStreamWaitEvent(sp, c->fb_ev[4], 0));
    }
    // the level image and the expansion of level k for the chunk's planes, on stream s
    auto expand = [&](hipStream_t s, int k, const uint8_t *g0, int planes) -> int {
        const int lw = lwk[k], lh = lhk[k];
        const float *level_img = img;
        const fb_taps K = fb_gauss_taps(ksz[k], sig[k]);
        if (lw != w || lh != h) {
            fb_resize_tabs T;
            if (int r2 = get_fb_tabs(c, h, w, lh, lw, T)) return r2;
            if (three_kernel || !launch_fb_level(s, g0, gp, plane_stride, planes, h, w, K, &T, img, lh, lw)) {
                launch_fb_blur(s, g0, gp, plane_stride, planes, h, w, K, T.cols, T.nc, T.rows, T.nr, tmp, blur);
                launch_fb_resize(s, blur, h, w, 1, img, lh, lw, planes, T, 1.f, false);
            }
        } else if (three_kernel || !launch_fb_level(s, g0, gp, plane_stride, planes, h, w, K, nullptr, img, lh, lw)) {
            launch_fb_blur(s, g0, gp, plane_stride, planes, h, w, K, nullptr, 0, nullptr, 0, tmp, blur);
            level_img = blur;
        }
        launch_fb_polyexp(s, level_img, planes, lh, lw, PC, Rall + Roff[k]);
        return VQA_OK;
    };
    for (int a = 0; a < n; a += mc) {
        const int pairs = (n - a) < mc ? (n - a) : mc, planes = pairs + 1;
        const uint8_t *g0 = gray + (int64_t)a * plane_stride;
        if (piped) {
            // the previous chunk's iterations still read the expansion planes: the side stream waits for them
            if (a > 0) HIPCHK(c, hipStreamWaitEvent(sp, c->fb_ev[5], 0));
            for (k = levels; k >= 0; k--) {
                if ((rc = expand(sp, k, g0, planes))) return rc;
                HIPCHK(c, hipEventRecord(c->fb_ev[k], sp));
            }
        }
        int pw = 0, ph = 0;
        for (k = levels; k >= 0; k--) {
            const int lw = lwk[k], lh = lhk[k];
            const float *R = Rall + Roff[k];
            // flow of this level: zero at the coarsest, else the coarser level's flow resized and doubled
            fb_resize_tabs TF;
            const bool coarsest = (k == levels);
            // exact 2x decimation cannot occur here (this is an upscale), so the bilinear tables always apply
            if (!coarsest && (rc = get_fb_tabs(c, ph, pw, lh, lw, TF))) return rc;
            // every plane once: blur (only where the resize will sample), resize to the level, polynomial expansion
            if (piped) HIPCHK(c, hipStreamWaitEvent(st, c->fb_ev[k], 0));
            else if ((rc = expand(st, k, g0, planes))) return rc;
#ifdef VQA_AB_VARIANTS
            if (two_kernel) {
                launch_fb_update_first(st, R, coarsest ? nullptr : prev_flow, ph, pw, TF, (float)(1. / pyr_scale), pairs, lh, lw, M);
                for (int i = 0; i < iters; i++) {
                    launch_fb_blur_solve(st, M, pairs, lh, lw, flow);
                    if (i < iters - 1) launch_fb_update(st, R, flow, pairs, lh, lw, M);
                }
                float *t = flow; flow = prev_flow; prev_flow = t; // prev_flow = this level's result
            } else
#endif
            {
                // The coarser level's result (prev_flow) is upsampled and doubled into `flow` by the upsample kernel (8 B/pixel
                // written once per level: forming it inside the first iteration instead cost that iteration 70 % more time
                // than the write - the eight dependent loads per row sit on the march's critical path); the iterations then
                // ping-pong between the two buffers, and prev_flow ends up naming this level's result.
                const float *in = nullptr;
                if (!coarsest) {
                    launch_fb_resize(st, prev_flow, ph, pw, 2, flow, lh, lw, pairs, TF, (float)(1. / pyr_scale), true);
                    float *t = flow; flow = prev_flow; prev_flow = t;
                    in = prev_flow;
                }
                for (int i = 0; i < iters; i++) {
                    // the last iteration of the finest level also leaves the partial sums of |flow| (no magnitude pass)
                    const bool last = k == 0 && i == iters - 1;
                    launch_fb_iter(st, R, in, pairs, lh, lw, flow, last ? (double *)c->fb_part.p : nullptr);
                    float *t = flow; flow = prev_flow; prev_flow = t;
                    in = prev_flow;
                }
            }
            pw = lw; ph = lh;
        }
#ifdef VQA_AB_VARIANTS
        if (two_kernel) launch_fb_mag(st, prev_flow, pairs, h, w, (double *)c->fb_part.p, a > 0 || first_has_prev, res + a);
        else
#endif
        launch_fb_mag_finalize(st, (const double *)c->fb_part.p, fb_iter_blocks(pairs, h, w), pairs, h, w, a > 0 || first_has_prev,
                               res + a);
        if (piped && a + mc < n) HIPCHK(c, hipEventRecord(c->fb_ev[5], st));
        c->last_fb.flow_buf = prev_flow == (float *)c->fb_flow0.p ? 0 : 1;
        c->last_fb.first_pair = a; c->last_fb.pairs = pairs;
    }
    c->last_fb.levels = levels; c->last_fb.h = h; c->last_fb.w = w; c->last_fb.first_valid = first_has_prev;
    for (k = 0; k <= levels; k++) { c->last_fb.lh[k] = lhk[k]; c->last_fb.lw[k] = lwk[k]; c->last_fb.Roff[k] = Roff[k]; }
    c->last_fb.valid = true;
    return VQA_OK;
}

extern "C" {

int vqa_abi_version(void) { return VQA_ABI_VERSION; }

const char *vqa_strerror(int s)
{
    switch (s) {
    case VQA_OK: return "ok";
    case VQA_ERR_INVALID: return "invalid argument";
    case VQA_ERR_NO_DEVICE: return "no HIP device (this engine has no CPU fallback)";
    case VQA_ERR_HIP: return "HIP runtime error";
    case VQA_ERR_OOM: return "out of memory";
    case VQA_ERR_UNSUPPORTED: return "unsupported request";
    case VQA_ERR_STATE: return "call sequence error";
    case VQA_ERR_INCOMPLETE: return "a result would be inexact and is withheld";
    default: return "unknown status";
    }
}

int vqa_device_count(int *count)
{
    if (!count) return VQA_ERR_INVALID;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { *count = 0; return VQA_ERR_NO_DEVICE; }
    *count = n;
    return VQA_OK;
}

void vqa_default_params(vqa_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->canny_low = 100;
    p->canny_high = 200;
    p->sad_range = 7;
    p->dct_mode = VQA_DCT_AUTO;
}

int vqa_create(int device, vqa_ctx **out)
{
    if (!out) return VQA_ERR_INVALID;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return VQA_ERR_NO_DEVICE;
    if (device < 0 || device >= n) return VQA_ERR_NO_DEVICE;
    vqa_ctx *c = new (std::nothrow) vqa_ctx();
    if (!c) return VQA_ERR_OOM;
    c->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return VQA_ERR_HIP;
    }
    c->dct_wave_slots = dct8_wave_slots(); // (the device is current: hipSetDevice above)
    // the one environment variable the shipped library reads (documented in vqa.h): the initial VQA_OPT_OVERLAP
    if (const char *e = getenv("VQA_OVERLAP")) c->opt_overlap = atoi(e) != 0;
#ifdef VQA_TEST_SEAMS
    if (const char *e = getenv("VQA_HYST_MAX_ROUNDS")) c->seam_hyst_max_rounds = atoi(e) > 0 ? atoi(e) : 0;
    if (const char *e = getenv("VQA_HYST_RESCUE_MAX_ROUNDS")) c->seam_hyst_rescue_max_rounds = atoi(e) > 0 ? atoi(e) : 0;
    if (const char *e = getenv("VQA_FAIL_ENSURE_AT")) c->seam_fail_at = atol(e);
    if (const char *e = getenv("VQA_FB_CHUNK_BYTES")) c->seam_fb_chunk_bytes = atoll(e);
    if (const char *e = getenv("VQA_QSLICE")) {
        const long long q = atoll(e);   // 0 (or no number): the shipped slice; otherwise 1 .. 32768 (gridDim.y holds no more)
        if (q != 0 && (q < 1 || q > 32768)) {
            (void)hipStreamDestroy(c->stream);
            delete c;
            return VQA_ERR_INVALID;
        }
        c->seam_qslice = (int)q;
    }
    if (const char *e = getenv("VQA_FSIM_SUBSLICE")) c->seam_fsim_sub = atoi(e) > 0 ? atoi(e) : 0;
    if (const char *e = getenv("VQA_PU21_SUBSLICE")) c->seam_pu21_sub = atoi(e) > 0 ? atoi(e) : 0;
#endif
    *out = c;
    return VQA_OK;
}

int vqa_set_option(vqa_ctx *c, int option, int value)
{
    if (!c) return VQA_ERR_INVALID;
    if (busy(c)) return VQA_ERR_STATE; // options apply to whole submits
    switch (option) {
    case VQA_OPT_OVERLAP: c->opt_overlap = value != 0; return VQA_OK;
    case VQA_OPT_HYST_STATS: c->opt_hyst_stats = value != 0; return VQA_OK;
    default: return VQA_ERR_INVALID;
    }
}

int vqa_get_option(const vqa_ctx *c, int option, int *value)
{
    if (!c || !value) return VQA_ERR_INVALID;
    switch (option) {
    case VQA_OPT_OVERLAP: *value = c->opt_overlap ? 1 : 0; return VQA_OK;
    case VQA_OPT_HYST_STATS: *value = c->opt_hyst_stats ? 1 : 0; return VQA_OK;
    default: return VQA_ERR_INVALID;
    }
}

int vqa_build_flavour(void)
{
    int f = 0;
#ifdef VQA_AB_VARIANTS
    f |= 1;
#endif
#ifdef VQA_TEST_SEAMS
    f |= 2;
#endif
    return f;
}

// every grow-only buffer, the result staging and every cached table of an idle ctx (vqa_trim, vqa_destroy); named here: the complexity batch's buffers, quality's extras, the shared staging and Farneback's - a plane-batch kind's own are in its slot
static void release_scratch(vqa_ctx *c)
{
    dbuf *bufs[] = {&c->gray_full, &c->planeA, &c->planeB, &c->state, &c->res_dev, &c->partials, &c->tile_flags,
                    &c->dirty0, &c->dirty1, &c->again_dev, &c->stage_frames, &c->stage_prev, &c->dct_scratch,
                    &c->dct_pe, &c->dct_pt, &c->qpartials, &c->qms_pyr, &c->qms_dev, &c->qstage_ref, &c->qstage_dist,
                    &c->mot_stage, &c->mot_prev, &c->siti_stage, &c->siti_prev, &c->xpsnr_prev, &c->scale_stage, &c->fb_tmp, &c->fb_blur,
                    &c->fb_img, &c->fb_R, &c->fb_M, &c->fb_flow0, &c->fb_flow1, &c->fb_part};
    for (dbuf *b : bufs) release(*b);
    for (batch_slot &s : c->slot) {   // everything a plane-batch kind owns
        release(s.dev);
        release(s.host);
        for (dbuf &b : s.work) release(b);
    }
    release(c->res_host);
    release(c->qms_host);
    for (auto &kv : c->tabs) free_table(kv.second.v);
    for (auto &kv : c->fb_tabs) free_table(kv.second.v);
    for (auto &kv : c->dct_mats) free_table(kv.second.v);
    for (auto &kv : c->fft_plans) free_table(kv.second.v);
    for (auto &kv : c->fsim_tables) free_table(kv.second.v);
    for (auto &kv : c->scale_tables) free_table(kv.second.v);
    c->scale_tables.clear();
    c->tabs.clear(); c->fb_tabs.clear(); c->dct_mats.clear(); c->fft_plans.clear(); c->fsim_tables.clear();
    // the planes vqa_debug_read_plane would read are gone
    c->last_n = 0; c->last_has_full = c->last_has_state = c->last_has_planes = false;
    c->last_fb.valid = false;
    c->last_u_n = 0;
    c->last_f_n = 0;
}

int vqa_trim(vqa_ctx *c)
{
    if (!c) return VQA_ERR_INVALID;
    if (busy(c)) return VQA_ERR_STATE;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = sync_all(c)) return rc;
    prof_collect(c);
    release_scratch(c);
    (void)hipGetLastError();
    return VQA_OK;
}

int vqa_destroy(vqa_ctx *c)
{
    if (!c) return VQA_ERR_INVALID;
    (void)hipSetDevice(c->device);
    (void)sync_all(c);
    release_scratch(c);
    for (auto &t : c->ev_open) { (void)hipEventDestroy(std::get<1>(t)); (void)hipEventDestroy(std::get<2>(t)); }
    for (hipEvent_t e : c->ev_pool) (void)hipEventDestroy(e);
    for (int i = 0; i < 3; i++) {
        if (c->side[i]) (void)hipStreamDestroy(c->side[i]);
        if (c->ev_join[i]) (void)hipEventDestroy(c->ev_join[i]);
    }
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->ev_xctx) (void)hipEventDestroy(c->ev_xctx);
    for (int i = 0; i < 6; i++)
        if (c->fb_ev[i]) (void)hipEventDestroy(c->fb_ev[i]);
    (void)hipStreamDestroy(c->stream);
    delete c;
    return VQA_OK;
}

const char *vqa_last_hip_error(const vqa_ctx *c) { return c ? c->last_err.c_str() : ""; }

int vqa_alloc_pinned(vqa_ctx *c, size_t bytes, void **out)
{
    if (!c || !out || !bytes) return VQA_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipHostMalloc(out, bytes, hipHostMallocDefault));
    return VQA_OK;
}
int vqa_free_pinned(vqa_ctx *c, void *p)
{
    if (!c || !p) return VQA_ERR_INVALID;
    HIPCHK(c, hipHostFree(p));
    return VQA_OK;
}
static bool host_byte_is_pinned(const void *p)
{
    hipPointerAttribute_t a;
    memset(&a, 0, sizeof a);
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { // ordinary host memory: HIP has never heard of it
        (void)hipGetLastError();
        return false;
    }
    return a.type == hipMemoryTypeHost;
}
int vqa_host_is_pinned(vqa_ctx *c, const void *p, size_t bytes, int *out)
{
    if (!c || !p || !out || !bytes) return VQA_ERR_INVALID;
    // the first AND the last byte: an array that starts inside a registered region and ends outside it (hipHostRegister
    // of part of a buffer) is pageable as far as a DMA of the whole range is concerned
    *out = (host_byte_is_pinned(p) && host_byte_is_pinned((const uint8_t *)p + (bytes - 1))) ? 1 : 0;
    return VQA_OK;
}
int vqa_alloc_device(vqa_ctx *c, size_t bytes, void **out)
{
    if (!c || !out || !bytes) return VQA_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMalloc(out, bytes));
    return VQA_OK;
}
int vqa_free_device(vqa_ctx *c, void *p)
{
    if (!c || !p) return VQA_ERR_INVALID;
    HIPCHK(c, hipFree(p));
    return VQA_OK;
}
int vqa_copy_h2d(vqa_ctx *c, void *dst, const void *src, size_t bytes)
{
    if (!c || !dst || !src) return VQA_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    return VQA_OK;
}
int vqa_stream_wait(vqa_ctx *waiter, vqa_ctx *signaler)
{
    if (!waiter || !signaler || waiter == signaler) return VQA_ERR_INVALID;
    if (waiter->device != signaler->device) return VQA_ERR_INVALID;
    HIPCHK(waiter, hipSetDevice(waiter->device));
    if (!signaler->ev_xctx) HIPCHK(waiter, hipEventCreateWithFlags(&signaler->ev_xctx, hipEventDisableTiming));
    // the record captures the signaler's stream as it stands NOW; re-recording the event later does not move a wait already enqueued
    HIPCHK(waiter, hipEventRecord(signaler->ev_xctx, signaler->stream));
    HIPCHK(waiter, hipStreamWaitEvent(waiter->stream, signaler->ev_xctx, 0));
    return VQA_OK;
}
int vqa_copy_d2h(vqa_ctx *c, void *dst, const void *src, size_t bytes)
{
    if (!c || !dst || !src) return VQA_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    return VQA_OK;
}
int vqa_sync(vqa_ctx *c)
{
    if (!c) return VQA_ERR_INVALID;
    return sync_all(c);
}
void *vqa_stream(vqa_ctx *c) { return c ? (void *)c->stream : nullptr; }
// internal accessors for vqa_comm.hip (not part of the ABI: hidden visibility)
extern "C" __attribute__((visibility("hidden"))) int vqa_ctx_device_(const vqa_ctx *c) { return c->device; }
extern "C" __attribute__((visibility("hidden"))) void *vqa_ctx_stream_(const vqa_ctx *c) { return (void *)c->stream; }

// ---------------------------------------------------------------------------
// A submit that fails after it has started to enqueue must not hand the caller's buffers (and this ctx's scratch) back
// while kernels or copies still use them: whatever the failing step was - a reservation, a copy, a launch, in the first
// slice or a later one, before or after the fork onto the side streams - the public entry points below drain EVERY
// stream of the ctx, drop the submit's timing events and leave the ctx idle and usable (no batch is recorded as pending).  The reference's
// convention for a failed step is log-and-re-raise with nothing left running (video_processing.py:295-297).
static int drain_failed_submit(vqa_ctx *c, int rc, bool touched)
{
    if (rc != VQA_OK && touched) {
        const std::string why = c->last_err; // keep the first error's text
        (void)sync_all(c);
        (void)hipGetLastError();
        prof_discard(c);
        c->last_err = why;
    }
    return rc;
}

static int complexity_submit_body(vqa_ctx *c, const uint8_t *frames, const uint8_t *prev0, int mem_kind, int n, int h, int w,
                                  int64_t frame_stride, int64_t row_stride, uint32_t mask, const vqa_params *params,
                                  bool &touched)
{
    if (!c || !frames || n <= 0 || h <= 0 || w <= 0) return VQA_ERR_INVALID;
    if (mem_kind != VQA_MEM_HOST && mem_kind != VQA_MEM_DEVICE) return VQA_ERR_INVALID;
    if (!mask || (mask & ~VQA_M_ALL)) return VQA_ERR_INVALID;
    if (row_stride < (int64_t)3 * w || frame_stride < row_stride * (h - 1) + (int64_t)3 * w) return VQA_ERR_INVALID;
    if (c->pend_c) return VQA_ERR_STATE;
    vqa_params P;
    if (params) P = *params; else vqa_default_params(&P);
    for (int i = 0; i < 9; i++)
        if (P.reserved[i]) return VQA_ERR_INVALID;
    if (P.motion_mode != VQA_MOTION_SAD && P.motion_mode != VQA_MOTION_FARNEBACK) return VQA_ERR_INVALID;
    if (P.sad_range < 0 || P.sad_range > 7) return VQA_ERR_INVALID;
    if (P.resize_w < 0 || P.resize_h < 0 || ((P.resize_w == 0) != (P.resize_h == 0))) return VQA_ERR_INVALID;
    if (P.dct_mode < VQA_DCT_AUTO || P.dct_mode > VQA_DCT_FULL) return VQA_ERR_INVALID;
    if ((int64_t)h * w > (1ll << 28)) return VQA_ERR_UNSUPPORTED;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    touched = true; // from here on a failure is drained by the caller (drain_failed_submit)

    const int rw = P.resize_w ? P.resize_w : w, rh = P.resize_h ? P.resize_h : h;
    const bool resized = !(rw == w && rh == h);
    const int ph = rh, pw = rw;
    const int pp = align_up(pw, 64), gp = align_up(w, 64);
    const bool want_gh = mask & VQA_M_GRAY_HIST, want_ch = mask & VQA_M_COLOR_HIST, want_dct = mask & VQA_M_DCT;
    const bool want_t = mask & VQA_M_TEMPORAL_DCT, want_e = mask & VQA_M_EDGE, want_m = mask & VQA_M_MOTION;
    const bool want_orb = mask & VQA_M_ORB;
    const bool batch_has_prev0 = prev0 != nullptr;

    // ---- bring frames to the device if they are on the host
    const uint8_t *dframes = frames, *dprev = prev0;
    if (mem_kind == VQA_MEM_HOST) {
        // The device copy is always compact (rows of 3w bytes): padded rows / a region of interest inside
        // larger frames cross PCIe as a 2-D copy, so no byte outside the caller's rows is ever read.
        const size_t rbytes = (size_t)3 * w, fbytes = rbytes * h;
        const bool padded = (size_t)row_stride != rbytes;
        int rc = ensure(c, c->stage_frames, fbytes * n);
        if (rc) return rc;
        if (!padded && (size_t)frame_stride == fbytes) {
            HIPCHK(c, hipMemcpyAsync(c->stage_frames.p, frames, fbytes * n, hipMemcpyHostToDevice, st));
        } else {
            // strided selection (every k-th frame of a clip): only the selected frames cross PCIe
            for (int i = 0; i < n; i++) {
                uint8_t *dst = (uint8_t *)c->stage_frames.p + fbytes * i;
                const uint8_t *src = frames + (int64_t)i * frame_stride;
                if (padded)
                    HIPCHK(c, hipMemcpy2DAsync(dst, rbytes, src, (size_t)row_stride, rbytes, h, hipMemcpyHostToDevice, st));
                else
                    HIPCHK(c, hipMemcpyAsync(dst, src, fbytes, hipMemcpyHostToDevice, st));
            }
        }
        dframes = (const uint8_t *)c->stage_frames.p;
        if (batch_has_prev0) {
            rc = ensure(c, c->stage_prev, fbytes);
            if (rc) return rc;
            if (padded)
                HIPCHK(c, hipMemcpy2DAsync(c->stage_prev.p, rbytes, prev0, (size_t)row_stride, rbytes, h,
                                           hipMemcpyHostToDevice, st));
            else
                HIPCHK(c, hipMemcpyAsync(c->stage_prev.p, prev0, fbytes, hipMemcpyHostToDevice, st));
            dprev = (const uint8_t *)c->stage_prev.p;
        }
        frame_stride = (int64_t)fbytes;
        row_stride = (int64_t)rbytes;
    }

    int rc = ensure(c, c->res_dev, sizeof(vqa_frame_metrics) * (size_t)n);
    if (rc) return rc;
    rc = ensure_pinned(c, c->res_host, sizeof(vqa_frame_metrics) * (size_t)n);
    if (rc) return rc;
    HIPCHK(c, hipMemsetAsync(c->res_dev.p, 0, sizeof(vqa_frame_metrics) * (size_t)n, st));
    vqa_frame_metrics *const res_all = (vqa_frame_metrics *)c->res_dev.p;
    const uint8_t *const dframes_all = dframes, *const dprev_all = dprev;
    const int n_all = n;

    // Frames ride in gridDim.y (<= 65535): larger batches are enqueued as consecutive slices on the same stream.  A
    // slice's "previous frame" is the last frame of the slice before it; scratch planes are reused (stream order).
    const int SLICE = 32768;
    auto run_slice = [&](const int a0) -> int {
    const int n = n_all - a0 < SLICE ? n_all - a0 : SLICE;
    const uint8_t *dframes = dframes_all + (int64_t)a0 * frame_stride;
    const uint8_t *dprev = a0 ? dframes_all + (int64_t)(a0 - 1) * frame_stride : dprev_all;
    const bool has_prev0 = a0 > 0 || batch_has_prev0;
    vqa_frame_metrics *res = res_all + a0;

    // ---- planes
    const bool want_plane = want_gh || want_ch || want_dct || want_t || want_e; // kernels that read the configured plane
    const bool need_full = (!resized && want_plane) || want_m;
    const bool need_planes = resized && want_plane;
    const int64_t full_stride = (int64_t)h * gp, plane_stride = (int64_t)ph * pp;
    uint8_t *gfull = nullptr, *pA = nullptr, *pB = nullptr;
    if (need_full) {
        rc = ensure(c, c->gray_full, (size_t)full_stride * (n + 1));
        if (rc) return rc;
        gfull = (uint8_t *)c->gray_full.p;
        const bool prev_needed = has_prev0 && (want_m || (!resized && want_t));
        prof_scope ps_(c, VQA_K_GRAY_HIST);
        if (prev_needed)
            launch_bgr2gray_hist(st, dprev, 1, h, w, frame_stride, row_stride, gfull, gp, full_stride, nullptr, false,
                                 false, false);
        launch_bgr2gray_hist(st, dframes, n, h, w, frame_stride, row_stride, gfull + full_stride, gp, full_stride, res,
                             !resized && want_gh, !resized && want_ch, !resized && want_dct);
    }
    if (need_planes) {
        resize_tabs T;
        rc = get_tabs(c, h, w, rh, rw, T);
        if (rc) return rc;
        rc = ensure(c, c->planeA, (size_t)plane_stride * (n + 1));
        if (rc) return rc;
        rc = ensure(c, c->planeB, (size_t)plane_stride * n);
        if (rc) return rc;
        pA = (uint8_t *)c->planeA.p;
        pB = (uint8_t *)c->planeB.p;
        prof_scope ps_(c, VQA_K_RESIZE);
        if (has_prev0 && want_t)
            launch_resize_planes(st, dprev, 1, h, w, frame_stride, row_stride, rw, rh, T.xofs, T.xa, T.yofs, T.yb,
                                 T.mode, pA, nullptr, pp, plane_stride, nullptr, false, false, false);
        launch_resize_planes(st, dframes, n, h, w, frame_stride, row_stride, rw, rh, T.xofs, T.xa, T.yofs, T.yb, T.mode,
                             pA + plane_stride, pB, pp, plane_stride, res, want_gh, want_ch, want_dct);
    } else if (!resized) {
        pA = gfull;                // slot 0 = prev0
        pB = gfull + full_stride;  // batch frames only
    }

    // ---- VQA_OPT_OVERLAP (default on): block-SAD, the Canny chain, the DCT metrics and ORB only share the gray planes as
    // input, so they run side by side: SAD, Canny and the full-frame DCT (the long one of the two DCT forms) fork onto their
    // own streams here - the planes exist in stream order - and join before the results are copied (QSAD-bound,
    // scalar-bound and latency-bound kernels next to each other: +3 % on the full suite; the full-frame DCT beside the
    // Farneback pyramid: c3ref +9 %, LAB_NOTES.md)
    int dct_mode_eff = P.dct_mode;
    if (dct_mode_eff == VQA_DCT_AUTO) dct_mode_eff = ((int64_t)ph * pw <= 128 * 128) ? VQA_DCT_FULL : VQA_DCT_BLOCK8;
    const bool use_side[3] = {c->opt_overlap && want_m && P.motion_mode == VQA_MOTION_SAD, c->opt_overlap && want_e,
                              c->opt_overlap && (want_dct || want_t) && dct_mode_eff == VQA_DCT_FULL && (want_m || want_e)};
    const bool overlap = use_side[0] || use_side[1] || use_side[2];
    hipStream_t st_sad = st, st_canny = st, st_dct = st;
    if (overlap) {
        for (int i = 0; i < 3; i++) {
            if (!use_side[i]) continue;
            if (!c->side[i]) HIPCHK(c, hipStreamCreateWithFlags(&c->side[i], hipStreamNonBlocking));
            if (!c->ev_join[i]) HIPCHK(c, hipEventCreateWithFlags(&c->ev_join[i], hipEventDisableTiming));
        }
        if (!c->ev_fork) HIPCHK(c, hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
        HIPCHK(c, hipEventRecord(c->ev_fork, st));
        if (use_side[0]) { st_sad = c->side[0]; HIPCHK(c, hipStreamWaitEvent(st_sad, c->ev_fork, 0)); }
        if (use_side[1]) { st_canny = c->side[1]; HIPCHK(c, hipStreamWaitEvent(st_canny, c->ev_fork, 0)); }
        if (use_side[2]) { st_dct = c->side[2]; HIPCHK(c, hipStreamWaitEvent(st_dct, c->ev_fork, 0)); }
    }

    // ---- DCT energy / temporal DCT (input: plane A)
    if (want_dct || want_t) {
        const int mode = dct_mode_eff;
        if (mode == VQA_DCT_BLOCK8) {
            const int pb = dct8_blocks_per_frame(ph, pw);
            rc = ensure(c, c->partials, sizeof(double) * 2 * (size_t)pb * n);
            if (rc) return rc;
            prof_scope ps_(c, VQA_K_DCT8);
            launch_dct8(st, pA, pp, plane_stride, n, ph, pw, want_dct, want_t, has_prev0, (double *)c->partials.p, res, c->dct_wave_slots);
        } else {
            if (dct_fft_supported(ph, pw)) {
                // both sides factor into 2, 3, 5: FFT-based row / column passes (k_dct_fft.hip)
                dct_fft_plan Pw, Ph;
                rc = get_fft_plan(c, pw, &Pw);
                if (rc) return rc;
                rc = get_fft_plan(c, ph, &Ph);
                if (rc) return rc;
                const size_t tiles = (size_t)dct_fft_tiles(ph, pw);
                rc = ensure(c, c->dct_scratch, sizeof(float) * 2 * (size_t)ph * pw * n);
                if (rc) return rc;
                rc = ensure(c, c->dct_pe, sizeof(double) * tiles * n);
                if (rc) return rc;
                rc = ensure(c, c->dct_pt, sizeof(double) * tiles * n);
                if (rc) return rc;
                prof_scope ps_(c, VQA_K_DCT_FULL, st_dct);
                launch_dct_full_fft(st_dct, pA, pp, plane_stride, n, ph, pw, Pw, Ph, (float *)c->dct_scratch.p, (double *)c->dct_pe.p,
                                    (double *)c->dct_pt.p, want_dct, want_t, has_prev0, res);
            } else {
                float *cw = nullptr, *ch = nullptr;
                rc = get_dct_matrix(c, pw, &cw);
                if (rc) return rc;
                rc = get_dct_matrix(c, ph, &ch);
                if (rc) return rc;
                const size_t tiles = (size_t)((ph + 15) / 16) * ((pw + 15) / 16);
                rc = ensure(c, c->dct_scratch, sizeof(float) * (size_t)ph * pw * n);
                if (rc) return rc;
                rc = ensure(c, c->dct_pe, sizeof(double) * tiles * n);
                if (rc) return rc;
                rc = ensure(c, c->dct_pt, sizeof(double) * tiles * n);
                if (rc) return rc;
                prof_scope ps_(c, VQA_K_DCT_FULL, st_dct);
                launch_dct_full(st_dct, pA, pp, plane_stride, n, ph, pw, cw, ch, (float *)c->dct_scratch.p,
                                (double *)c->dct_pe.p, (double *)c->dct_pt.p, want_dct, want_t, has_prev0, res);
            }
        }
    }

    // ---- motion on the full-resolution gray planes (the reference never resizes for it, :327-328):
    // block-SAD (north_star) or the reference's own Farneback flow
    if (want_m && P.motion_mode == VQA_MOTION_SAD) {
        prof_scope ps_(c, VQA_K_SAD, st_sad);
        launch_block_sad(st_sad, gfull, gp, full_stride, n, h, w, P.sad_range, has_prev0, res);
    } else if (want_m) {
        prof_scope ps_(c, VQA_K_FARNEBACK);
        rc = run_farneback(c, st, gfull, gp, full_stride, n, h, w, has_prev0, res);
        if (rc) return rc;
        c->last_fb.first_pair += a0; c->last_fb.first_valid = batch_has_prev0; // (counted from the submit's first pair, not the slice's)
    }

    // ---- Canny (input: plane B)
    c->last_has_state = false;
    if (want_e) {
        const int ww = (pw + 63) / 64;
        const size_t words = (size_t)n * ((ph + 63) / 64) * ww * 64; // tile-major bit-planes (of the transposed frame: the same count)
        const unsigned ntiles = canny_hyst_tiles(n, ph, pw);
        rc = ensure(c, c->state, sizeof(uint64_t) * words * 2); // strong plane, then weak plane
        if (rc) return rc;
        rc = ensure(c, c->tile_flags, sizeof(uint32_t) * ntiles * 2); // dedup flags, one array per work list
        if (rc) return rc;
        const size_t NS = CANNY_HYST_SEGMENTS; // list segments (and append counters) per frame
        rc = ensure(c, c->dirty0, sizeof(uint32_t) * ntiles * NS); // work list A
        if (rc) return rc;
        rc = ensure(c, c->dirty1, sizeof(uint32_t) * ntiles * NS); // work list B
        if (rc) return rc;
        rc = ensure(c, c->again_dev, sizeof(uint32_t) * 3 * n * NS); // append counters: three buffers, rotated per round (below)
        if (rc) return rc;
        unsigned long long *strong = (unsigned long long *)c->state.p, *weak = strong + words;
        unsigned *queued[2] = {(unsigned *)c->tile_flags.p, (unsigned *)c->tile_flags.p + ntiles};
        unsigned *lists[2] = {(unsigned *)c->dirty0.p, (unsigned *)c->dirty1.p};
        unsigned *counts = (unsigned *)c->again_dev.p;
        HIPCHK(c, hipMemsetAsync(queued[0], 0, sizeof(uint32_t) * ntiles * 2, st_canny));
        HIPCHK(c, hipMemsetAsync(counts, 0, sizeof(uint32_t) * 3 * n * NS, st_canny));
        // The append counters rotate over THREE buffers so that no memset sits between the rounds: round r consumes
        // cnt(r), appends to cnt(r + 1) and zeroes cnt(r + 2) - the buffer round r - 1 consumed (stream order: done)
        // and round r + 1 will append to.  Lists and dedup flags stay double-buffered (index r & 1).
        auto cnt = [&](int r) { return counts + (size_t)(r % 3) * n * NS; };
        int lo = P.canny_low, hi = P.canny_high;
        if (lo > hi) { int t = lo; lo = hi; hi = t; }
        {
            prof_scope ps_(c, VQA_K_CANNY_NMS, st_canny);
            launch_canny_nms(st_canny, pB, pp, plane_stride, n, ph, pw, lo, hi, strong, weak, res);
        }
        // hysteresis to the fixpoint, entirely enqueued (no host readback).  Round 0 relaxes every tile;
        // round r > 0 relaxes the tiles that round r-1 enqueued into lists[r & 1].
        int round = 0;
        {
            prof_scope ps_(c, VQA_K_CANNY_HYST, st_canny);
            launch_canny_hyst_all(st_canny, strong, weak, n, ph, pw, queued[1], lists[1], cnt(1), res, c->opt_hyst_stats);
        }
        {
            // rounds 1..WIDE (still many tiles): wide grid over the per-frame lists; then the tail kernel
            // finishes every frame on its own workgroup with no host round-trip.
            prof_scope ps_(c, VQA_K_CANNY_HYST, st_canny);
            // (a frame's tail runs on ONE workgroup: big frames in small batches get more wide rounds first)
            const canny_geom cg = canny_tiles(ph, pw);
            int WIDE = (cg.tiles_x * cg.tiles_y > 1024 && n < 256) ? 8 : 6; // (measured: 1080p x 256: 4 -> 0.40 ms, 6 -> 0.38 ms of hysteresis)
#ifdef VQA_AB_VARIANTS
            { static const int e = ab_knob("VQA_HYST_WIDE", 0); if (e > 0) WIDE = e; } // lab build: tuning knob
#endif
            for (round = 1; round <= WIDE; round++) {
                const int in = round & 1, out = in ^ 1;
#ifdef VQA_AB_VARIANTS
                static const bool trace = ab_knob("VQA_HYST_TRACE", 0) != 0;
                if (trace) { // lab build, debugging aid: tiles queued for this round, summed over frames (synchronises)
                    std::vector<uint32_t> hc((size_t)n * NS);
                    (void)hipStreamSynchronize(st_canny);
                    (void)hipMemcpy(hc.data(), cnt(round), sizeof(uint32_t) * hc.size(), hipMemcpyDeviceToHost);
                    unsigned long long tot = 0;
                    for (uint32_t v : hc) tot += v;
                    fprintf(stderr, "[hyst] round %d: %llu of %u tiles queued\n", round, tot, ntiles);
                }
#endif
                launch_canny_hyst_list(st_canny, strong, weak, n, ph, pw, queued[in], lists[in], cnt(round), queued[out], lists[out],
                                       cnt(round + 1), cnt(round + 2), res, c->opt_hyst_stats);
            }
            // the tail alternates between the counter the last wide round appended to and the one it zeroed
            unsigned *tc[2];
            tc[round & 1] = cnt(round);
            tc[(round & 1) ^ 1] = cnt(round + 1);
            launch_canny_hyst_tail(st_canny, strong, weak, n, ph, pw, lists[0], tc[0], queued[0], lists[1], tc[1], queued[1],
                                   round & 1, res, c->opt_hyst_stats, c->seam_hyst_max_rounds, c->seam_hyst_rescue_max_rounds);
        }
        launch_canny_finish(st_canny, strong, n, ph, pw, res);
        c->last_has_state = true;
    }

    // ---- ORB keypoint count: always on the 64x64 thumbnail (:385-386), straight from the BGR frames
    if (want_orb) {
        resize_tabs T64;
        rc = get_tabs(c, h, w, 64, 64, T64);
        if (rc) return rc;
        prof_scope ps_(c, VQA_K_ORB);
        launch_orb64(st, dframes, n, h, w, frame_stride, row_stride, T64.xofs, T64.xa, T64.yofs, T64.yb, T64.mode, res);
    }
    if (overlap) {
        hipStream_t ss[3] = {st_sad, st_canny, st_dct};
        for (int i = 0; i < 3; i++) {
            if (!use_side[i]) continue;
            HIPCHK(c, hipEventRecord(c->ev_join[i], ss[i]));
            HIPCHK(c, hipStreamWaitEvent(st, c->ev_join[i], 0));
        }
    }
    c->last_n = n; c->last_has_full = need_full; c->last_has_planes = need_planes; // (debug planes show the last slice)
    return VQA_OK;
    }; // run_slice
    for (int a0 = 0; a0 < n_all; a0 += SLICE)
        if (const int src = run_slice(a0)) return src; // (the caller drains)
    const bool has_prev0 = batch_has_prev0;

    HIPCHK(c, hipGetLastError());
    if (want_gh || want_ch) {
        HIPCHK(c, hipMemcpyAsync(c->res_host.p, c->res_dev.p, sizeof(vqa_frame_metrics) * (size_t)n, hipMemcpyDeviceToHost, st));
        c->pend_c_tail_only = false;
    } else {
        // no histogram was asked for: bring back only the 0.6 KB of scalars behind the 4 KB of bins of each record
        const size_t off = offsetof(vqa_frame_metrics, sum_gray2), tail = sizeof(vqa_frame_metrics) - off;
        HIPCHK(c, hipMemcpy2DAsync((uint8_t *)c->res_host.p + off, sizeof(vqa_frame_metrics), (uint8_t *)c->res_dev.p + off,
                                   sizeof(vqa_frame_metrics), tail, (size_t)n, hipMemcpyDeviceToHost, st));
        c->pend_c_tail_only = true;
    }
    c->pend_c = n;
    c->pend_c_prev0 = has_prev0;
    c->last_h = h; c->last_w = w; c->last_ph = ph; c->last_pw = pw; c->last_pp = pp; c->last_gp = gp;
    c->last_resized = resized;
    return VQA_OK;
}

int vqa_complexity_submit(vqa_ctx *c, const uint8_t *frames, const uint8_t *prev0, int mem_kind, int n, int h, int w,
                          int64_t frame_stride, int64_t row_stride, uint32_t mask, const vqa_params *params)
{
    bool touched = false;
    const int rc = complexity_submit_body(c, frames, prev0, mem_kind, n, h, w, frame_stride, row_stride, mask, params, touched);
    return drain_failed_submit(c, rc, touched);
}

int vqa_complexity_wait(vqa_ctx *c, vqa_frame_metrics *out, int n)
{
    if (!c || !out) return VQA_ERR_INVALID;
    if (!c->pend_c || n != c->pend_c) return VQA_ERR_STATE;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    memcpy(out, c->res_host.p, sizeof(vqa_frame_metrics) * (size_t)n);
    for (int i = 0; i < n; i++) {
        if (c->pend_c_tail_only) memset(&out[i], 0, offsetof(vqa_frame_metrics, sum_gray2)); // bins were not computed
        out[i].has_prev = (i > 0 || c->pend_c_prev0) ? 1u : 0u;
    }
    c->pend_c = 0;
    // north_star: edge counts are bit-exact.  A frame whose hysteresis neither the tail nor the rescue pass brought to
    // the fixpoint (hyst_overflow still 1) has a LOWER BOUND in edge_count: that is never handed out as a count.
    for (int i = 0; i < n; i++)
        if (out[i].hyst_overflow == 1u) {
            c->last_err = "Canny hysteresis of frame " + std::to_string(i) + " of " + std::to_string(n) +
                          " stopped before its fixpoint (edge_count " + std::to_string(out[i].edge_count) +
                          " would be a lower bound): records withheld";
            memset(out, 0, sizeof(vqa_frame_metrics) * (size_t)n);
            return VQA_ERR_INCOMPLETE;
        }
    return VQA_OK;
}

// ---------------------------------------------------------------------------
// What the plane-batch kinds (enum batch_kind) share.  A submit body is: bad_batch_args and the kind's own argument checks;
// check_batch; stage_batch (or stage_pair); the kind's reservations and launches over for_each_slice / for_each_group;
// finish_batch.  A wait is wait_batch around the kind's finalize, or wait_pending and wait_synced around a check of its own.
// Every public submit goes through submit_and_drain.
extern "C++" {   // (templates among them)

// arguments and mem_kind (dist: the second stream; a submit that has none passes `ref` again)
static bool bad_batch_args(const vqa_ctx *c, const void *ref, const void *dist, int mem_kind, int n, const vqa_plane_desc *planes,
                           int n_planes)
{
    return !c || !ref || !dist || n <= 0 || !planes || n_planes <= 0 || n_planes > 4 ||
           (mem_kind != VQA_MEM_HOST && mem_kind != VQA_MEM_DEVICE);
}

struct plane_batch {
    int depth, bps;   // bits and bytes per sample
    int64_t span;     // bytes from a frame's first byte to the end of its last plane
};

// The descriptor rules, per plane in plane order: depth, 16-bit alignment, geometry (VQA_ERR_INVALID), then limits(d) - the
// metric's own VQA_ERR_UNSUPPORTED rules - and only then the next plane.  The order decides the status of a list that breaks
// several rules at once.  The frame strides are checked against B.span after all planes (check_batch).
template <class F> static int check_planes(const vqa_plane_desc *planes, int n_planes, plane_batch &B, F limits)
{
    // sample depth (vqa_plane_desc.bit_depth): 0 / 8 = uint8, 9..16 = little-endian uint16 at even byte offsets, strides and
    // steps; one depth per submit (FFmpeg's filters see one pixel format per frame)
    B.depth = planes[0].bit_depth == 0 ? 8 : planes[0].bit_depth;
    if (B.depth < 8 || B.depth > 16) return VQA_ERR_INVALID;
    B.bps = B.depth > 8 ? 2 : 1;
    B.span = 0;
    for (int p = 0; p < n_planes; p++) {
        const vqa_plane_desc &d = planes[p];
        if ((d.bit_depth == 0 ? 8 : d.bit_depth) != B.depth) return VQA_ERR_INVALID;
        if (B.bps == 2 && ((d.offset | d.row_stride | (int64_t)d.pixel_step) & 1)) return VQA_ERR_INVALID;
        if (d.width <= 0 || d.height <= 0 || d.offset < 0 || d.pixel_step <= 0 ||
            d.row_stride < (int64_t)d.width * d.pixel_step - (d.pixel_step - B.bps))
            return VQA_ERR_INVALID;
        // geometry, still: offset and row_stride are the caller's 64-bit fields, and a plane whose last byte does not fit int64_t is
        // no plane (a wrapped, negative end would shrink the span and pass the frame-stride rule)
        int64_t rows, end;
        if (__builtin_mul_overflow((int64_t)d.height, d.row_stride, &rows) || __builtin_add_overflow(d.offset, rows, &end) ||
            __builtin_add_overflow(end, (int64_t)d.width * d.pixel_step + B.bps, &end))
            return VQA_ERR_INVALID;
        if (int rc = limits(d)) return rc;
        end = d.offset + (int64_t)(d.height - 1) * d.row_stride + (int64_t)(d.width - 1) * d.pixel_step + B.bps;
        B.span = end > B.span ? end : B.span;
    }
    return VQA_OK;
}

// the limits most kinds start from: a smallest side, and the 2^28 samples that bound the 64-bit totals and the sums (vqa.h)
static int side_and_area_limits(const vqa_plane_desc &d, int min_dim)
{
    if (d.width < min_dim || d.height < min_dim) return VQA_ERR_UNSUPPORTED;
    if ((int64_t)d.width * d.height > (1ll << 28)) return VQA_ERR_UNSUPPORTED;
    return VQA_OK;
}

// the limits of a kind that takes the planes of a pixel together: they are plane 0's (the chroma planes of a 16 x 16 4:2:0
// frame are 8 x 8)
static auto plane0_limits(const vqa_plane_desc *planes, int min_dim)
{
    return [=](const vqa_plane_desc &d) { return &d == planes ? side_and_area_limits(d, min_dim) : (int)VQA_OK; };
}

// The three planes of a pixel, taken together: U and V are alike; under a BGR model all three planes are alike; otherwise the
// chroma planes have the luma's size or its ceil-half, in either direction.
enum joint_rule { JOINT_NONE, JOINT_YUV, JOINT_BGR };

static bool joint_planes_ok(const vqa_plane_desc *planes, joint_rule rule)
{
    const vqa_plane_desc &y = planes[0], &u = planes[1], &v = planes[2];
    auto alike = [](const vqa_plane_desc &a, const vqa_plane_desc &b) {
        return a.width == b.width && a.height == b.height && a.row_stride == b.row_stride && a.pixel_step == b.pixel_step;
    };
    if (!alike(u, v)) return false;
    if (rule == JOINT_BGR) return alike(u, y);
    return (u.width == y.width || u.width == (y.width + 1) / 2) && (u.height == y.height || u.height == (y.height + 1) / 2);
}

// The checks of a submit that follow the kind's own argument checks, in the order that decides the status: a pending batch of
// the kind (VQA_ERR_STATE), the planes one by one (check_planes), the joint rule of three planes, the frame strides of the one
// or two streams (a submit that has one passes its stride twice).
template <class F> static int check_batch(const batch_slot &s, int n, int64_t fs_a, int64_t fs_b, const vqa_plane_desc *planes,
                                          int n_planes, plane_batch &B, F limits, joint_rule joint = JOINT_NONE)
{
    if (s.entries) return VQA_ERR_STATE;
    if (int rc = check_planes(planes, n_planes, B, limits)) return rc;
    if (joint != JOINT_NONE && !joint_planes_ok(planes, joint)) return VQA_ERR_INVALID;
    if (n > 1 && (fs_a < B.span || fs_b < B.span)) return VQA_ERR_INVALID;
    return VQA_OK;
}

// host frames brought to the device: `buf` grown to hold them, the copy enqueued on the ctx stream, `frames` moved to the copy
static int stage(vqa_ctx *c, dbuf &buf, const uint8_t *&frames, size_t bytes)
{
    if (int rc = ensure(c, buf, bytes)) return rc;
    HIPCHK(c, hipMemcpyAsync(buf.p, frames, bytes, hipMemcpyHostToDevice, c->stream));
    frames = (const uint8_t *)buf.p;
    return VQA_OK;
}

// one input of a submit - the caller's pointer to its frames, their stride and where host frames are staged - or none
struct batch_input {
    const uint8_t **frames = nullptr;
    int64_t fs = 0;
    dbuf *buf = nullptr;
};

// What follows the checks of a submit: the device is made current, `touched` is set - from here on a failure is drained by the
// caller (drain_failed_submit) - and host frames are staged, in this order: stream a, stream b if the submit has one, the one
// frame prev0 if the submit takes one and the caller gave it.  The staged pointers replace the caller's.
static int stage_batch(vqa_ctx *c, bool &touched, int mem_kind, int n, int64_t span, batch_input a, batch_input b = {},
                       batch_input prev0 = {})
{
    HIPCHK(c, hipSetDevice(c->device));
    touched = true;
    if (mem_kind != VQA_MEM_HOST) return VQA_OK;
    for (const batch_input &s : {a, b})
        if (s.frames)
            if (int rc = stage(c, *s.buf, *s.frames, (size_t)(n - 1) * s.fs + span)) return rc;
    if (prev0.frames && *prev0.frames) return stage(c, *prev0.buf, *prev0.frames, (size_t)span);
    return VQA_OK;
}

// stage_batch for the two host streams of a pair submit.  All pair submits share qstage_*: the stream orders a batch behind
// whatever the ctx already has in flight, so a pending batch of another kind reads its frames before they are overwritten.
static int stage_pair(vqa_ctx *c, bool &touched, int mem_kind, int n, int64_t span, const uint8_t *&ref, int64_t ref_fs,
                      const uint8_t *&dist, int64_t dist_fs, batch_input prev0 = {})
{
    return stage_batch(c, touched, mem_kind, n, span, {&ref, ref_fs, &c->qstage_ref}, {&dist, dist_fs, &c->qstage_dist}, prev0);
}

constexpr int QSLICE = 32768; // frames ride in gridDim.y (<= 65535): larger batches go out as consecutive slices

// the slice length of a ctx: the constant, but for the lab build's VQA_QSLICE seam (every use of QSLICE below goes through here)
static inline int qslice(const vqa_ctx *c)
{
#ifdef VQA_TEST_SEAMS
    if (c->seam_qslice > 0) return c->seam_qslice;
#endif
    (void)c;
    return QSLICE;
}

// the frames of the longest slice of a batch of n: what per-slice scratch is sized for
static inline int slice_frames(const vqa_ctx *c, int n)
{
    return n < qslice(c) ? n : qslice(c);
}

// body(a0, m): frames a0 .. a0 + m - 1 of the batch
template <class F> static void for_each_slice(const vqa_ctx *c, int n, F body)
{
    const int q = qslice(c);
    for (int a0 = 0; a0 < n; a0 += q) body(a0, n - a0 < q ? n - a0 : q);
}

// body(idx, cnt): planes of identical geometry (B,G,R of packed BGR; U,V of 4:2:0) go out as one group
template <class F> static void for_each_group(const vqa_plane_desc *planes, int n_planes, F body)
{
    bool done[4] = {false, false, false, false};
    for (int p = 0; p < n_planes; p++) {
        if (done[p]) continue;
        int idx[4], cnt = 0;
        for (int q = p; q < n_planes; q++) {
            if (!done[q] && planes[q].width == planes[p].width && planes[q].height == planes[p].height &&
                planes[q].row_stride == planes[p].row_stride && planes[q].pixel_step == planes[p].pixel_step) {
                idx[cnt++] = q;
                done[q] = true;
            }
        }
        body(idx, cnt);
    }
}

// Scratch that serves one group of same-geometry planes at a time (the groups follow each other on the stream) is sized by the
// largest group, which no grouping of the planes can exceed when every plane is counted at the largest size: the most bytes(cnt,
// height, width) over the planes, cnt being the planes of that width and height (for_each_group compares strides and steps as
// well: its groups are no larger)
template <class F> static size_t largest_group_bytes(const vqa_plane_desc *planes, int n_planes, F bytes)
{
    size_t most = 0;
    for (int p = 0; p < n_planes; p++) {
        int cnt = 0;
        for (int q = 0; q < n_planes; q++) cnt += planes[q].width == planes[p].width && planes[q].height == planes[p].height;
        const size_t b = bytes(cnt, planes[p].height, planes[p].width);
        most = b > most ? b : most;
    }
    return most;
}

// a public submit: the body, then the drain if it failed after it had started to enqueue
template <class F> static int submit_and_drain(vqa_ctx *c, F body)
{
    bool touched = false;
    const int rc = body(touched);
    return drain_failed_submit(c, rc, touched);
}

// the batch in flight: the last thing a successful submit does (a submit that fails anywhere leaves the slot idle)
static void record_batch(batch_slot &s, int entries, const vqa_plane_desc *planes, int n_planes, int depth)
{
    s.entries = entries;
    s.planes = n_planes;
    s.depth = depth;
    for (int p = 0; p < n_planes; p++) { s.w[p] = planes[p].width; s.h[p] = planes[p].height; }
}

// the tail of a submit: the launches' status, the first `bytes` of the slot's words to its pinned copy, the record
static int finish_batch(vqa_ctx *c, batch_slot &s, size_t bytes, int entries, const vqa_plane_desc *planes, int n_planes, int depth)
{
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(s.host.p, s.dev.p, bytes, hipMemcpyDeviceToHost, c->stream));
    record_batch(s, entries, planes, n_planes, depth);
    return VQA_OK;
}

// The frame of a wait, in two steps.  wait_pending: the arguments, and the kind's batch in flight (`s`) - a wrong n_entries is
// VQA_ERR_STATE and the batch stays pending, whatever else is pending.  A kind with more to check does so between the two, and
// the batch stays pending if it refuses.  wait_synced: the stream synchronised and the timing events folded in; the caller
// then reads s->host and sets s->entries = 0.
static int wait_pending(vqa_ctx *c, batch_kind kind, const void *out, int n_entries, batch_slot *&s)
{
    if (!c || !out) return VQA_ERR_INVALID;
    s = &c->slot[kind];
    if (!s->entries || n_entries != s->entries) return VQA_ERR_STATE;
    return VQA_OK;
}

static int wait_synced(vqa_ctx *c)
{
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    return VQA_OK;
}

// the whole wait of a kind whose pinned copy holds `words` words of T per entry: finalize(the entry's words, the slot, the
// entry's plane index, its record)
template <class T = unsigned long long, class Out, class F>
static int wait_batch(vqa_ctx *c, batch_kind kind, Out *out, int n_entries, int words, F finalize)
{
    batch_slot *s;
    if (int rc = wait_pending(c, kind, out, n_entries, s)) return rc;
    if (int rc = wait_synced(c)) return rc;
    const T *acc = (const T *)s->host.p;
    for (int e = 0; e < n_entries; e++) finalize(acc + (size_t)e * words, *s, e % s->planes, out + e);
    s->entries = 0;
    return VQA_OK;
}

// The marks of a launcher that runs several kernels (cambi_mark, brisque_mark): one prof_scope per kernel id at a time, open
// between its begin and its end.  marks::mark and the address of a marks go to the launcher.
struct marks {
    vqa_ctx *c;
    std::optional<prof_scope> open;
    explicit marks(vqa_ctx *c_) : c(c_) {}
    static void mark(void *p, int id, int begin)
    {
        marks *m = (marks *)p;
        if (begin) m->open.emplace(m->c, id);
        else m->open.reset();
    }
};

} // extern "C++"

// ---------------------------------------------------------------------------
static int quality_submit_body(vqa_ctx *c, const uint8_t *ref, const uint8_t *dist, int mem_kind, int n, int64_t ref_fs,
                               int64_t dist_fs, const vqa_plane_desc *planes, int n_planes, int ssim_mode, bool &touched)
{
    if (bad_batch_args(c, ref, dist, mem_kind, n, planes, n_planes)) return VQA_ERR_INVALID;
    if (ssim_mode != VQA_SSIM_GAUSS && ssim_mode != VQA_SSIM_FFMPEG && ssim_mode != VQA_SSIM_MS) return VQA_ERR_INVALID;
    batch_slot &s = c->slot[KIND_QUALITY];
    const bool ms = ssim_mode == VQA_SSIM_MS, gauss = ms || ssim_mode == VQA_SSIM_GAUSS;   // MS: the Gaussian window on five scales
    int maxblocks = 1;
    plane_batch B;
    int rc = check_batch(s, n, ref_fs, dist_fs, planes, n_planes, B, [&](const vqa_plane_desc &d) -> int {
        // k_ssim_gauss addresses a strip's rows through a 32-bit scalar buffer offset (row * row_stride) plus a 32-bit
        // lane offset: a plane whose rows span 2 GiB (absurd strides / regions of interest only) would wrap silently
        if (gauss &&
            (int64_t)d.height * d.row_stride + (int64_t)d.width * d.pixel_step + B.bps >= ((int64_t)1 << 31)) return VQA_ERR_UNSUPPORTED;
        if (gauss && (d.width < 11 || d.height < 11)) return VQA_ERR_UNSUPPORTED;
        if (ms && (d.width < MS_MIN_DIM || d.height < MS_MIN_DIM)) return VQA_ERR_UNSUPPORTED;   // level 4 must hold a window
        if (ssim_mode == VQA_SSIM_FFMPEG && (d.width < 8 || d.height < 8)) return VQA_ERR_UNSUPPORTED;
        const int b = gauss ? ssim_gauss_blocks(d.height, d.width) : ssim_ffmpeg_blocks(d.height, d.width);
        maxblocks = b > maxblocks ? b : maxblocks;
        return VQA_OK;
    });
    if (rc) return rc;
    if ((rc = stage_pair(c, touched, mem_kind, n, B.span, ref, ref_fs, dist, dist_fs))) return rc;
    hipStream_t st = c->stream;
    const size_t nent = (size_t)n * n_planes;
    if ((rc = ensure(c, s.dev, sizeof(vqa_plane_metrics) * nent))) return rc;
    if ((rc = ensure_pinned(c, s.host, sizeof(vqa_plane_metrics) * nent))) return rc;
    const int nslice = slice_frames(c, n), depth = B.depth;
    // (MS: a second half of the same size for the cs totals; level 0 has the most tiles)
    if ((rc = ensure(c, c->qpartials, sizeof(double) * (size_t)maxblocks * nslice * n_planes * (ms ? 2 : 1)))) return rc;
    if (ms) {
        // the pyramid scratch: levels 1..4 of the largest plane group
        const size_t pyr = largest_group_bytes(planes, n_planes, [&](int cnt, int h, int w) {
            return sizeof(float) * (size_t)ms_levels(nslice, cnt, h, w).total;
        });
        if ((rc = ensure(c, c->qms_pyr, pyr))) return rc;
        if ((rc = ensure(c, c->qms_dev, sizeof(vqa_ms_scales) * nent))) return rc;
        if ((rc = ensure_pinned(c, c->qms_host, sizeof(vqa_ms_scales) * nent))) return rc;
    }
    HIPCHK(c, hipMemsetAsync(s.dev.p, 0, sizeof(vqa_plane_metrics) * nent, st));
    const int64_t pstride = (int64_t)maxblocks * nslice;
    for_each_slice(c, n, [&](int a0, int m) {
        vqa_plane_metrics *res = (vqa_plane_metrics *)s.dev.p + (size_t)a0 * n_planes;
        const uint8_t *sref = ref + (int64_t)a0 * ref_fs, *sdist = dist + (int64_t)a0 * dist_fs;
        for_each_group(planes, n_planes, [&](const int *idx, int cnt) {
            if (ms) {
                // one pyramid launch, then the five scales one after another on the ctx stream (each level's totals leave the
                // partials through its finalize before the next level's kernel overwrites them)
                vqa_ms_scales *msd = (vqa_ms_scales *)c->qms_dev.p + (size_t)a0 * n_planes;
                {
                    prof_scope pp_(c, VQA_K_MS_PYRAMID);
                    launch_ms_pyramid(st, sref, sdist, m, ref_fs, dist_fs, planes, idx, cnt, depth, (float *)c->qms_pyr.p);
                }
                for (int lv = 0; lv < MS_LEVELS; lv++) {
                    prof_scope pl_(c, VQA_K_SSIM_GAUSS);
                    launch_quality_ms_level(st, sref, sdist, m, ref_fs, dist_fs, planes, idx, cnt, n_planes,
                                            (double *)c->qpartials.p, pstride, res, depth, lv, (const float *)c->qms_pyr.p, msd);
                }
                return;
            }
            prof_scope ps_(c, ssim_mode == VQA_SSIM_GAUSS ? VQA_K_SSIM_GAUSS : VQA_K_SSIM_FFMPEG);
            if (ssim_mode == VQA_SSIM_GAUSS)
                launch_quality_gauss(st, sref, sdist, m, ref_fs, dist_fs, planes, idx, cnt, n_planes,
                                     (double *)c->qpartials.p, pstride, res, depth);
            else
                launch_quality_ffmpeg(st, sref, sdist, m, ref_fs, dist_fs, planes, idx, cnt, n_planes,
                                      (double *)c->qpartials.p, pstride, res, depth);
        });
    });
    if (ms) launch_ms_combine(st, (const vqa_ms_scales *)c->qms_dev.p, (int)nent, (vqa_plane_metrics *)s.dev.p);
    // (the tail inline: the scales of an MS batch are copied as well, and the record comes after every copy)
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(s.host.p, s.dev.p, sizeof(vqa_plane_metrics) * nent, hipMemcpyDeviceToHost, st));
    if (ms) HIPCHK(c, hipMemcpyAsync(c->qms_host.p, c->qms_dev.p, sizeof(vqa_ms_scales) * nent, hipMemcpyDeviceToHost, st));
    c->pend_q_ms = ms;
    record_batch(s, (int)nent, planes, n_planes, depth);
    return VQA_OK;
}

int vqa_quality_submit(vqa_ctx *c, const uint8_t *ref, const uint8_t *dist, int mem_kind, int n, int64_t ref_fs,
                       int64_t dist_fs, const vqa_plane_desc *planes, int n_planes, int ssim_mode)
{
    return submit_and_drain(c, [&](bool &touched) {
        return quality_submit_body(c, ref, dist, mem_kind, n, ref_fs, dist_fs, planes, n_planes, ssim_mode, touched);
    });
}

int vqa_quality_wait_ms(vqa_ctx *c, vqa_plane_metrics *out, vqa_ms_scales *scales, int n_entries)
{
    if (!c || !out) return VQA_ERR_INVALID;
    batch_slot &s = c->slot[KIND_QUALITY];
    if (!s.entries || n_entries != s.entries) return VQA_ERR_STATE;
    if (scales && !c->pend_q_ms) return VQA_ERR_STATE;   // (the batch stays pending: vqa_quality_wait collects it)
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    memcpy(out, s.host.p, sizeof(vqa_plane_metrics) * (size_t)n_entries);
    if (scales) memcpy(scales, c->qms_host.p, sizeof(vqa_ms_scales) * (size_t)n_entries);
    s.entries = 0;
    c->pend_q_ms = false;
    return VQA_OK;
}

int vqa_quality_wait(vqa_ctx *c, vqa_plane_metrics *out, int n_entries)
{
    return vqa_quality_wait_ms(c, out, nullptr, n_entries);
}

// ---------------------------------------------------------------------------
// VIF on four scales.  A batch of its own: the stream orders it behind whatever the ctx already has in flight, so the host
// staging (qstage_*) and the caller's device frames are shared with a pending batch of another kind without a hazard.
static int vif_submit_body(vqa_ctx *c, const uint8_t *ref, const uint8_t *dist, int mem_kind, int n, int64_t ref_fs,
                           int64_t dist_fs, const vqa_plane_desc *planes, int n_planes, bool &touched)
{
    if (bad_batch_args(c, ref, dist, mem_kind, n, planes, n_planes)) return VQA_ERR_INVALID;
    batch_slot &s = c->slot[KIND_VIF];
    dbuf &vif_pyr = s.work[0], &vif_acc = s.work[1];
    plane_batch B;
    int rc = check_batch(s, n, ref_fs, dist_fs, planes, n_planes, B,
                         [](const vqa_plane_desc &d) { return side_and_area_limits(d, VIF_MIN_DIM); });
    if (rc) return rc;
    if ((rc = stage_pair(c, touched, mem_kind, n, B.span, ref, ref_fs, dist, dist_fs))) return rc;
    hipStream_t st = c->stream;
    const size_t nent = (size_t)n * n_planes;
    const size_t acc_bytes = sizeof(long long) * 2 * VIF_LEVELS * nent;
    if ((rc = ensure(c, vif_acc, acc_bytes))) return rc;
    if ((rc = ensure(c, s.dev, sizeof(vqa_vif_metrics) * nent))) return rc;
    if ((rc = ensure_pinned(c, s.host, sizeof(vqa_vif_metrics) * nent))) return rc;
    const int nslice = slice_frames(c, n), depth = B.depth;
    // the level scratch: levels 1..3 of the largest plane group
    const size_t pyr = largest_group_bytes(planes, n_planes, [&](int cnt, int h, int w) {
        return sizeof(float) * (size_t)vif_levels(nslice, cnt, h, w).total;
    });
    if ((rc = ensure(c, vif_pyr, pyr))) return rc;
    HIPCHK(c, hipMemsetAsync(vif_acc.p, 0, acc_bytes, st));
    for_each_slice(c, n, [&](int a0, int m) {
        long long *acc = (long long *)vif_acc.p + (size_t)a0 * n_planes * 2 * VIF_LEVELS;
        const uint8_t *sref = ref + (int64_t)a0 * ref_fs, *sdist = dist + (int64_t)a0 * dist_fs;
        for_each_group(planes, n_planes, [&](const int *idx, int cnt) {
            float *scratch = (float *)vif_pyr.p;
            for (int lv = 0; lv < VIF_LEVELS; lv++) {
                if (lv > 0) {
                    prof_scope pd_(c, VQA_K_VIF_DECIMATE);
                    launch_vif_decimate(st, sref, sdist, m, ref_fs, dist_fs, planes, idx, cnt, depth, lv, scratch);
                }
                prof_scope ps_(c, VQA_K_VIF);
                launch_vif_stats(st, sref, sdist, m, ref_fs, dist_fs, planes, idx, cnt, n_planes, depth, lv, scratch, acc);
            }
        });
    });
    launch_vif_finalize(st, (const long long *)vif_acc.p, (int)nent, (vqa_vif_metrics *)s.dev.p);
    return finish_batch(c, s, sizeof(vqa_vif_metrics) * nent, (int)nent, planes, n_planes, depth);
}

int vqa_vif_submit(vqa_ctx *c, const uint8_t *ref, const uint8_t *dist, int mem_kind, int n, int64_t ref_fs,
                   int64_t dist_fs, const vqa_plane_desc *planes, int n_planes)
{
    return submit_and_drain(c, [&](bool &touched) {
        return vif_submit_body(c, ref, dist, mem_kind, n, ref_fs, dist_fs, planes, n_planes, touched);
    });
}

int vqa_vif_wait(vqa_ctx *c, vqa_vif_metrics *out, int n_entries)
{
    // (the device finalizes VIF: the pinned copy holds the records)
    return wait_batch<vqa_vif_metrics>(c, KIND_VIF, out, n_entries, 1,
                                       [](const vqa_vif_metrics *r, const batch_slot &, int, vqa_vif_metrics *o) { *o = *r; });
}

// ---------------------------------------------------------------------------
// ADM on four scales.  A batch of its own, ordered by the stream like a VIF batch.
static int adm_submit_body(vqa_ctx *c, const uint8_t *ref, const uint8_t *dist, int mem_kind, int n, int64_t ref_fs,
                           int64_t dist_fs, const vqa_plane_desc *planes, int n_planes, bool &touched)
{
    if (bad_batch_args(c, ref, dist, mem_kind, n, planes, n_planes)) return VQA_ERR_INVALID;
    batch_slot &s = c->slot[KIND_ADM];
    dbuf &adm_pyr = s.work[0], &adm_part = s.work[1];
    plane_batch B;
    int rc = check_batch(s, n, ref_fs, dist_fs, planes, n_planes, B,
                         [](const vqa_plane_desc &d) { return side_and_area_limits(d, ADM_MIN_DIM); });
    if (rc) return rc;
    if ((rc = stage_pair(c, touched, mem_kind, n, B.span, ref, ref_fs, dist, dist_fs))) return rc;
    hipStream_t st = c->stream;
    const size_t nent = (size_t)n * n_planes;
    const size_t sums_bytes = sizeof(double) * 6 * ADM_LEVELS * nent;
    if ((rc = ensure(c, s.dev, sums_bytes))) return rc;
    if ((rc = ensure_pinned(c, s.host, sums_bytes))) return rc;
    const int nslice = slice_frames(c, n), depth = B.depth;
    // the band scratch and the partials serve one group of same-geometry planes (and one scale) at a time
    const size_t pyr = largest_group_bytes(planes, n_planes, [&](int cnt, int h, int w) {
        return sizeof(float) * (size_t)adm_levels(nslice, cnt, h, w).total;
    });
    const size_t part = largest_group_bytes(planes, n_planes, [&](int cnt, int h, int w) {
        const adm_layout L = adm_levels(nslice, cnt, h, w);
        return sizeof(double) * 6 * (size_t)nslice * cnt * adm_tiles(L.h[1], L.w[1]);
    });
    if ((rc = ensure(c, adm_pyr, pyr))) return rc;
    if ((rc = ensure(c, adm_part, part))) return rc;
    for_each_slice(c, n, [&](int a0, int m) {
        double *sums = (double *)s.dev.p + (size_t)a0 * n_planes * 6 * ADM_LEVELS;
        const uint8_t *sref = ref + (int64_t)a0 * ref_fs, *sdist = dist + (int64_t)a0 * dist_fs;
        for_each_group(planes, n_planes, [&](const int *idx, int cnt) {
            for (int sc = 0; sc < ADM_LEVELS; sc++) {
                {
                    prof_scope ps_(c, VQA_K_ADM);
                    launch_adm_scale(st, sref, sdist, m, ref_fs, dist_fs, planes, idx, cnt, depth, sc, (float *)adm_pyr.p,
                                     (double *)adm_part.p);
                }
                prof_scope pr_(c, VQA_K_ADM_REDUCE);
                launch_adm_reduce(st, (const double *)adm_part.p, m, planes, idx, cnt, n_planes, sc, sums);
            }
        });
    });
    return finish_batch(c, s, sums_bytes, (int)nent, planes, n_planes, depth);
}

int vqa_adm_submit(vqa_ctx *c, const uint8_t *ref, const uint8_t *dist, int mem_kind, int n, int64_t ref_fs,
                   int64_t dist_fs, const vqa_plane_desc *planes, int n_planes)
{
    return submit_and_drain(c, [&](bool &touched) {
        return adm_submit_body(c, ref, dist, mem_kind, n, ref_fs, dist_fs, planes, n_planes, touched);
    });
}

int vqa_adm_wait(vqa_ctx *c, vqa_adm_metrics *out, int n_entries)
{
    return wait_batch<double>(c, KIND_ADM, out, n_entries, 6 * ADM_LEVELS,
                              [](const double *sums, const batch_slot &s, int p, vqa_adm_metrics *o) {
                                  adm_finalize(sums, s.h[p], s.w[p], o);   // (the planes' sizes: the host's cube roots)
                              });
}

// ---------------------------------------------------------------------------
// VMAF's motion feature: the reference stream alone, frame i against frame i - 1.  A batch of its own, ordered by the stream
// like a VIF batch.  Host frames (and prev0) are staged in buffers of their own.
static int motion_submit_body(vqa_ctx *c, const uint8_t *ref, const uint8_t *prev0, int mem_kind, int n, int64_t ref_fs,
                              const vqa_plane_desc *planes, int n_planes, bool &touched)
{
    if (bad_batch_args(c, ref, ref, mem_kind, n, planes, n_planes)) return VQA_ERR_INVALID;
    batch_slot &s = c->slot[KIND_MOTION];
    plane_batch B;
    int rc = check_batch(s, n, ref_fs, ref_fs, planes, n_planes, B,
                         [](const vqa_plane_desc &d) { return side_and_area_limits(d, MOTION_MIN_DIM); });
    if (rc) return rc;
    if ((rc = stage_batch(c, touched, mem_kind, n, B.span, {&ref, ref_fs, &c->mot_stage}, {}, {&prev0, 0, &c->mot_prev}))) return rc;
    hipStream_t st = c->stream;
    const size_t nent = (size_t)n * n_planes;
    const size_t acc_bytes = sizeof(long long) * nent;
    if ((rc = ensure(c, s.dev, acc_bytes))) return rc;
    if ((rc = ensure_pinned(c, s.host, acc_bytes))) return rc;
    HIPCHK(c, hipMemsetAsync(s.dev.p, 0, acc_bytes, st));
    const int depth = B.depth;
    for_each_slice(c, n, [&](int a0, int m) {
        long long *acc = (long long *)s.dev.p + (size_t)a0 * n_planes;
        const uint8_t *sref = ref + (int64_t)a0 * ref_fs;
        const uint8_t *sprev = a0 > 0 ? ref + (int64_t)(a0 - 1) * ref_fs : prev0;
        for_each_group(planes, n_planes, [&](const int *idx, int cnt) {
            prof_scope ps_(c, VQA_K_MOTION);
            launch_motion_sad(st, sref, sprev, m, ref_fs, planes, idx, cnt, n_planes, depth, acc);
        });
    });
    return finish_batch(c, s, acc_bytes, (int)nent, planes, n_planes, depth);
}

int vqa_motion_submit(vqa_ctx *c, const uint8_t *ref, const uint8_t *prev0, int mem_kind, int n, int64_t ref_fs,
                      const vqa_plane_desc *planes, int n_planes)
{
    return submit_and_drain(c, [&](bool &touched) {
        return motion_submit_body(c, ref, prev0, mem_kind, n, ref_fs, planes, n_planes, touched);
    });
}

int vqa_motion_wait(vqa_ctx *c, vqa_motion_metrics *out, int n_entries)
{
    return wait_batch<long long>(c, KIND_MOTION, out, n_entries, 1,
                                 [](const long long *acc, const batch_slot &s, int p, vqa_motion_metrics *o) {
                                     // exact for in-range samples (a total below 2^52); a total above 2^53 is rounded once, to double
                                     o->sad = (double)*acc * (1.0 / 65536.0);
                                     o->motion = o->sad / (double)((int64_t)s.w[p] * s.h[p]);
                                 });
}

// ---------------------------------------------------------------------------
// ITU-T P.910 spatial and temporal information: the reference stream alone, Sobel on frame i and frame i against frame i - 1.
// A batch of its own, ordered by the stream like a motion batch.  Host frames (and prev0) are staged in buffers of their own.
static int siti_submit_body(vqa_ctx *c, const uint8_t *ref, const uint8_t *prev0, int mem_kind, int n, int64_t ref_fs,
                            const vqa_plane_desc *planes, int n_planes, bool &touched)
{
    if (bad_batch_args(c, ref, ref, mem_kind, n, planes, n_planes)) return VQA_ERR_INVALID;
    batch_slot &s = c->slot[KIND_SITI];
    plane_batch B;
    int rc = check_batch(s, n, ref_fs, ref_fs, planes, n_planes, B, [&](const vqa_plane_desc &d) -> int {
        if (int lim = side_and_area_limits(d, SITI_MIN_DIM)) return lim;
        // grad_sq: q < 2^37.01 for arbitrary 16-bit samples, so 2^26 of them stay below 2^64 (vqa.h)
        if (B.depth > 8 && (int64_t)d.width * d.height > (1ll << 26)) return VQA_ERR_UNSUPPORTED;
        return VQA_OK;
    });
    if (rc) return rc;
    if ((rc = stage_batch(c, touched, mem_kind, n, B.span, {&ref, ref_fs, &c->siti_stage}, {}, {&prev0, 0, &c->siti_prev}))) return rc;
    hipStream_t st = c->stream;
    const size_t nent = (size_t)n * n_planes;
    const size_t acc_bytes = sizeof(unsigned long long) * SITI_WORDS * nent;
    if ((rc = ensure(c, s.dev, acc_bytes))) return rc;
    if ((rc = ensure_pinned(c, s.host, acc_bytes))) return rc;
    HIPCHK(c, hipMemsetAsync(s.dev.p, 0, acc_bytes, st));
    const int depth = B.depth;
    for_each_slice(c, n, [&](int a0, int m) {
        unsigned long long *acc = (unsigned long long *)s.dev.p + (size_t)a0 * n_planes * SITI_WORDS;
        const uint8_t *sref = ref + (int64_t)a0 * ref_fs;
        const uint8_t *sprev = a0 > 0 ? ref + (int64_t)(a0 - 1) * ref_fs : prev0;
        for_each_group(planes, n_planes, [&](const int *idx, int cnt) {
            prof_scope ps_(c, VQA_K_SITI);
            launch_siti(st, sref, sprev, m, ref_fs, planes, idx, cnt, n_planes, depth, acc);
        });
    });
    return finish_batch(c, s, acc_bytes, (int)nent, planes, n_planes, depth);
}

int vqa_siti_submit(vqa_ctx *c, const uint8_t *ref, const uint8_t *prev0, int mem_kind, int n, int64_t ref_fs,
                    const vqa_plane_desc *planes, int n_planes)
{
    return submit_and_drain(c, [&](bool &touched) {
        return siti_submit_body(c, ref, prev0, mem_kind, n, ref_fs, planes, n_planes, touched);
    });
}

int vqa_siti_wait(vqa_ctx *c, vqa_siti_metrics *out, int n_entries)
{
    return wait_batch(c, KIND_SITI, out, n_entries, SITI_WORDS,
                      [](const unsigned long long *acc, const batch_slot &s, int p, vqa_siti_metrics *o) {
                          siti_finalize(acc, s.h[p], s.w[p], s.depth, o);
                      });
}

// ---------------------------------------------------------------------------
// PSNR-HVS and PSNR-HVS-M: both streams, the whole 8x8 blocks of every plane.  A batch of its own, ordered by the stream
// like a VIF batch, whose host staging (qstage_*) it shares.
static int psnr_hvs_submit_body(vqa_ctx *c, const uint8_t *ref, const uint8_t *dist, int mem_kind, int n, int64_t ref_fs,
                                int64_t dist_fs, const vqa_plane_desc *planes, int n_planes, bool &touched)
{
    if (bad_batch_args(c, ref, dist, mem_kind, n, planes, n_planes)) return VQA_ERR_INVALID;
    batch_slot &s = c->slot[KIND_PSNR_HVS];
    plane_batch B;
    int rc = check_batch(s, n, ref_fs, dist_fs, planes, n_planes, B,
                         [](const vqa_plane_desc &d) { return side_and_area_limits(d, PSNR_HVS_MIN_DIM); });
    if (rc) return rc;
    if ((rc = stage_pair(c, touched, mem_kind, n, B.span, ref, ref_fs, dist, dist_fs))) return rc;
    hipStream_t st = c->stream;
    const size_t nent = (size_t)n * n_planes;
    const size_t acc_bytes = sizeof(unsigned long long) * PSNR_HVS_WORDS * nent;
    if ((rc = ensure(c, s.dev, acc_bytes))) return rc;
    if ((rc = ensure_pinned(c, s.host, acc_bytes))) return rc;
    HIPCHK(c, hipMemsetAsync(s.dev.p, 0, acc_bytes, st));
    const int depth = B.depth;
    for_each_slice(c, n, [&](int a0, int m) {
        unsigned long long *acc = (unsigned long long *)s.dev.p + (size_t)a0 * n_planes * PSNR_HVS_WORDS;
        const uint8_t *sref = ref + (int64_t)a0 * ref_fs, *sdist = dist + (int64_t)a0 * dist_fs;
        for_each_group(planes, n_planes, [&](const int *idx, int cnt) {
            prof_scope ps_(c, VQA_K_PSNR_HVS);
            launch_psnr_hvs(st, sref, sdist, m, ref_fs, dist_fs, planes, idx, cnt, n_planes, depth, acc);
        });
    });
    return finish_batch(c, s, acc_bytes, (int)nent, planes, n_planes, depth);
}

int vqa_psnr_hvs_submit(vqa_ctx *c, const uint8_t *ref, const uint8_t *dist, int mem_kind, int n, int64_t ref_fs,
                        int64_t dist_fs, const vqa_plane_desc *planes, int n_planes)
{
    return submit_and_drain(c, [&](bool &touched) {
        return psnr_hvs_submit_body(c, ref, dist, mem_kind, n, ref_fs, dist_fs, planes, n_planes, touched);
    });
}

int vqa_psnr_hvs_wait(vqa_ctx *c, vqa_psnr_hvs_metrics *out, int n_entries)
{
    return wait_batch(c, KIND_PSNR_HVS, out, n_entries, PSNR_HVS_WORDS,
                      [](const unsigned long long *acc, const batch_slot &s, int p, vqa_psnr_hvs_metrics *o) {
                          psnr_hvs_finalize(acc, s.h[p], s.w[p], s.depth, o);
                      });
}

// ---------------------------------------------------------------------------
// CIEDE2000: both streams, the three planes of a pixel together, one entry per frame.  A batch of its own, ordered by
// the stream like a PSNR-HVS batch, whose host staging (qstage_*) it shares.
static int ciede_submit_body(vqa_ctx *c, const uint8_t *ref, const uint8_t *dist, int mem_kind, int n, int64_t ref_fs,
                             int64_t dist_fs, const vqa_plane_desc *planes, int n_planes, int model, const double *weights,
                             bool &touched)
{
    if (bad_batch_args(c, ref, dist, mem_kind, n, planes, n_planes)) return VQA_ERR_INVALID;
    if (n_planes != 3 || (model != VQA_CIEDE_YUV709 && model != VQA_CIEDE_BGR)) return VQA_ERR_INVALID;
    double k[3] = {1.0, 1.0, 1.0};
    for (int i = 0; weights && i < 3; i++) {
        if (!std::isfinite(weights[i]) || !(weights[i] > 0.0)) return VQA_ERR_INVALID;
        k[i] = weights[i];
    }
    batch_slot &s = c->slot[KIND_CIEDE];
    plane_batch B;
    int rc = check_batch(s, n, ref_fs, dist_fs, planes, n_planes, B, plane0_limits(planes, CIEDE_MIN_DIM),
                         model == VQA_CIEDE_BGR ? JOINT_BGR : JOINT_YUV);
    if (rc) return rc;
    if ((rc = stage_pair(c, touched, mem_kind, n, B.span, ref, ref_fs, dist, dist_fs))) return rc;
    hipStream_t st = c->stream;
    const size_t acc_bytes = sizeof(unsigned long long) * (size_t)n;
    if ((rc = ensure(c, s.dev, acc_bytes))) return rc;
    if ((rc = ensure_pinned(c, s.host, acc_bytes))) return rc;
    HIPCHK(c, hipMemsetAsync(s.dev.p, 0, acc_bytes, st));
    const int depth = B.depth;
    for_each_slice(c, n, [&](int a0, int m) {
        prof_scope ps_(c, VQA_K_CIEDE);
        launch_ciede(st, ref + (int64_t)a0 * ref_fs, dist + (int64_t)a0 * dist_fs, m, ref_fs, dist_fs, planes, depth, model, k,
                     (unsigned long long *)s.dev.p + a0);
    });
    return finish_batch(c, s, acc_bytes, n, planes, n_planes, depth);
}

int vqa_ciede_submit(vqa_ctx *c, const uint8_t *ref, const uint8_t *dist, int mem_kind, int n, int64_t ref_fs, int64_t dist_fs,
                     const vqa_plane_desc *planes, int n_planes, int model, const double *weights)
{
    return submit_and_drain(c, [&](bool &touched) {
        return ciede_submit_body(c, ref, dist, mem_kind, n, ref_fs, dist_fs, planes, n_planes, model, weights, touched);
    });
}

int vqa_ciede_wait(vqa_ctx *c, vqa_ciede_metrics *out, int n_entries)
{
    // (one entry per frame: the luma grid, for the host's mean)
    return wait_batch(c, KIND_CIEDE, out, n_entries, 1,
                      [](const unsigned long long *acc, const batch_slot &s, int, vqa_ciede_metrics *o) {
                          ciede_finalize(*acc, s.h[0], s.w[0], o);
                      });
}

// ---------------------------------------------------------------------------
// GMSD: both streams, every plane by itself.  A batch of its own, ordered by the stream like a PSNR-HVS batch, whose
// host staging (qstage_*) it shares.
static int gmsd_submit_body(vqa_ctx *c, const uint8_t *ref, const uint8_t *dist, int mem_kind, int n, int64_t ref_fs,
                            int64_t dist_fs, const vqa_plane_desc *planes, int n_planes, bool &touched)
{
    if (bad_batch_args(c, ref, dist, mem_kind, n, planes, n_planes)) return VQA_ERR_INVALID;
    batch_slot &s = c->slot[KIND_GMSD];
    plane_batch B;
    int rc = check_batch(s, n, ref_fs, dist_fs, planes, n_planes, B,
                         [](const vqa_plane_desc &d) { return side_and_area_limits(d, GMSD_MIN_DIM); });
    if (rc) return rc;
    if ((rc = stage_pair(c, touched, mem_kind, n, B.span, ref, ref_fs, dist, dist_fs))) return rc;
    hipStream_t st = c->stream;
    const size_t nent = (size_t)n * n_planes;
    const size_t acc_bytes = sizeof(unsigned long long) * GMSD_WORDS * nent;
    if ((rc = ensure(c, s.dev, acc_bytes))) return rc;
    if ((rc = ensure_pinned(c, s.host, acc_bytes))) return rc;
    HIPCHK(c, hipMemsetAsync(s.dev.p, 0, acc_bytes, st));
    const int depth = B.depth;
    for_each_slice(c, n, [&](int a0, int m) {
        unsigned long long *acc = (unsigned long long *)s.dev.p + (size_t)a0 * n_planes * GMSD_WORDS;
        const uint8_t *sref = ref + (int64_t)a0 * ref_fs, *sdist = dist + (int64_t)a0 * dist_fs;
        for_each_group(planes, n_planes, [&](const int *idx, int cnt) {
            prof_scope ps_(c, VQA_K_GMSD);
            launch_gmsd(st, sref, sdist, m, ref_fs, dist_fs, planes, idx, cnt, n_planes, depth, acc);
        });
    });
    return finish_batch(c, s, acc_bytes, (int)nent, planes, n_planes, depth);
}

int vqa_gmsd_submit(vqa_ctx *c, const uint8_t *ref, const uint8_t *dist, int mem_kind, int n, int64_t ref_fs, int64_t dist_fs,
                    const vqa_plane_desc *planes, int n_planes)
{
    return submit_and_drain(c, [&](bool &touched) {
        return gmsd_submit_body(c, ref, dist, mem_kind, n, ref_fs, dist_fs, planes, n_planes, touched);
    });
}

int vqa_gmsd_wait(vqa_ctx *c, vqa_gmsd_metrics *out, int n_entries)
{
    return wait_batch(c, KIND_GMSD, out, n_entries, GMSD_WORDS,
                      [](const unsigned long long *acc, const batch_slot &s, int p, vqa_gmsd_metrics *o) {
                          gmsd_finalize(acc, s.h[p], s.w[p], o);
                      });
}

// ---------------------------------------------------------------------------
// CAMBI: one stream, every plane by itself.  A batch of its own, ordered by the stream like a GMSD batch; host frames
// are staged in qstage_dist, the buffer of the stream it measures in a one-pass run.
static int cambi_submit_body(vqa_ctx *c, const uint8_t *frames, int mem_kind, int n, int64_t fs, const vqa_plane_desc *planes,
                             int n_planes, bool &touched)
{
    if (bad_batch_args(c, frames, frames, mem_kind, n, planes, n_planes)) return VQA_ERR_INVALID;
    batch_slot &s = c->slot[KIND_CAMBI];
    dbuf &cambi_scratch = s.work[0];
    plane_batch B;
    int rc = check_batch(s, n, fs, fs, planes, n_planes, B,
                         [](const vqa_plane_desc &d) { return side_and_area_limits(d, CAMBI_MIN_DIM); });
    if (rc) return rc;
    if ((rc = stage_batch(c, touched, mem_kind, n, B.span, {&frames, fs, &c->qstage_dist}))) return rc;
    hipStream_t st = c->stream;
    const size_t nent = (size_t)n * n_planes;
    const size_t acc_bytes = sizeof(unsigned long long) * CAMBI_WORDS * nent;
    const size_t per_frame = largest_group_bytes(planes, n_planes, [](int cnt, int h, int w) { return cambi_scratch_bytes(cnt, h, w); });
    if ((rc = ensure(c, s.dev, acc_bytes))) return rc;
    if ((rc = ensure(c, cambi_scratch, per_frame * (size_t)slice_frames(c, n)))) return rc;
    if ((rc = ensure_pinned(c, s.host, acc_bytes))) return rc;
    HIPCHK(c, hipMemsetAsync(s.dev.p, 0, acc_bytes, st));
    const int depth = B.depth;
    marks mk(c);
    for_each_slice(c, n, [&](int a0, int m) {
        unsigned long long *acc = (unsigned long long *)s.dev.p + (size_t)a0 * n_planes * CAMBI_WORDS;
        const uint8_t *sfr = frames + (int64_t)a0 * fs;
        for_each_group(planes, n_planes, [&](const int *idx, int cnt) {
            launch_cambi(st, sfr, m, fs, planes, idx, cnt, n_planes, depth, cambi_scratch.p, acc, marks::mark, &mk);
        });
    });
    return finish_batch(c, s, acc_bytes, (int)nent, planes, n_planes, depth);
}

int vqa_cambi_submit(vqa_ctx *c, const uint8_t *frames, int mem_kind, int n, int64_t fs, const vqa_plane_desc *planes, int n_planes)
{
    return submit_and_drain(c, [&](bool &touched) {
        return cambi_submit_body(c, frames, mem_kind, n, fs, planes, n_planes, touched);
    });
}

int vqa_cambi_wait(vqa_ctx *c, vqa_cambi_metrics *out, int n_entries)
{
    return wait_batch(c, KIND_CAMBI, out, n_entries, CAMBI_WORDS,
                      [](const unsigned long long *acc, const batch_slot &s, int p, vqa_cambi_metrics *o) {
                          cambi_finalize(acc, s.h[p], s.w[p], o);
                      });
}

// ---------------------------------------------------------------------------
// XPSNR: both streams and the reference frame before each pair; the luma plane steers every plane's weights.  A batch of its
// own, ordered by the stream like a GMSD batch, whose host staging (qstage_*) it shares; prev0 is staged by itself.
static int xpsnr_submit_body(vqa_ctx *c, const uint8_t *ref, const uint8_t *dist, const uint8_t *prev0, int mem_kind, int n,
                             int64_t ref_fs, int64_t dist_fs, const vqa_plane_desc *planes, int n_planes, bool &touched)
{
    if (bad_batch_args(c, ref, dist, mem_kind, n, planes, n_planes)) return VQA_ERR_INVALID;
    batch_slot &s = c->slot[KIND_XPSNR];
    plane_batch B;
    int rc = check_batch(s, n, ref_fs, dist_fs, planes, n_planes, B, [&](const vqa_plane_desc &d) -> int {
        if (int lim = side_and_area_limits(d, XPSNR_MIN_DIM)) return lim;
        // sse of the plane: 2^26 squares below 2^32 stay below 2^64 (vqa.h)
        if (B.depth > 8 && (int64_t)d.width * d.height > (1ll << 26)) return VQA_ERR_UNSUPPORTED;
        if (d.pixel_step != B.bps) return VQA_ERR_UNSUPPORTED;   // planar layouts only
        // plane 0 is the luma; every other plane has its size or its ceil-half, in either direction
        const int W = planes[0].width, H = planes[0].height;
        if ((d.width != W && d.width != (W + 1) / 2) || (d.height != H && d.height != (H + 1) / 2)) return VQA_ERR_UNSUPPORTED;
        return VQA_OK;
    });
    if (rc) return rc;
    if ((rc = stage_pair(c, touched, mem_kind, n, B.span, ref, ref_fs, dist, dist_fs, {&prev0, 0, &c->xpsnr_prev}))) return rc;
    hipStream_t st = c->stream;
    const xpsnr_geom g = xpsnr_geometry(planes[0].width, planes[0].height);
    const size_t fw = xpsnr_frame_words(g, n_planes);
    const size_t acc_bytes = sizeof(unsigned long long) * fw * (size_t)n;
    if ((rc = ensure(c, s.dev, acc_bytes))) return rc;
    if ((rc = ensure_pinned(c, s.host, acc_bytes))) return rc;
    HIPCHK(c, hipMemsetAsync(s.dev.p, 0, acc_bytes, st));
    const int depth = B.depth;
    for_each_slice(c, n, [&](int a0, int m) {
        unsigned long long *words = (unsigned long long *)s.dev.p + (size_t)a0 * fw;
        const uint8_t *sref = ref + (int64_t)a0 * ref_fs, *sdist = dist + (int64_t)a0 * dist_fs;
        const uint8_t *sprev = a0 > 0 ? ref + (int64_t)(a0 - 1) * ref_fs : prev0;
        {
            prof_scope ps_(c, VQA_K_XPSNR_ACT);
            launch_xpsnr_act(st, sref, sprev, m, ref_fs, planes[0], g, depth, fw, words);
        }
        for_each_group(planes, n_planes, [&](const int *idx, int cnt) {
            prof_scope ps_(c, VQA_K_XPSNR_SSE);
            launch_xpsnr_sse(st, sref, sdist, m, ref_fs, dist_fs, planes, idx, cnt, g, depth, fw, words);
        });
    });
    return finish_batch(c, s, acc_bytes, n * n_planes, planes, n_planes, depth);
}

int vqa_xpsnr_submit(vqa_ctx *c, const uint8_t *ref, const uint8_t *dist, const uint8_t *prev0, int mem_kind, int n,
                     int64_t ref_fs, int64_t dist_fs, const vqa_plane_desc *planes, int n_planes)
{
    return submit_and_drain(c, [&](bool &touched) {
        return xpsnr_submit_body(c, ref, dist, prev0, mem_kind, n, ref_fs, dist_fs, planes, n_planes, touched);
    });
}

int vqa_xpsnr_wait(vqa_ctx *c, vqa_xpsnr_metrics *out, int n_entries, uint64_t *blocks, int64_t n_block_words)
{
    batch_slot *s;
    if (int rc = wait_pending(c, KIND_XPSNR, out, n_entries, s)) return rc;
    const int npl = s->planes, n = n_entries / npl;
    const xpsnr_geom g = xpsnr_geometry(s->w[0], s->h[0]);
    const size_t fw = xpsnr_frame_words(g, npl), bw = (size_t)g.nbx * g.nby * (3 + npl);
    if (blocks && n_block_words != (int64_t)(bw * (size_t)n)) return VQA_ERR_INVALID;   // (the batch stays pending)
    if (int rc = wait_synced(c)) return rc;
    const unsigned long long *acc = (const unsigned long long *)s->host.p;
    for (int f = 0; f < n; f++)
        xpsnr_finalize(acc + (size_t)f * fw, g, s->depth, npl, s->w, s->h, out + (size_t)f * npl,
                       blocks ? blocks + (size_t)f * bw : nullptr);
    s->entries = 0;
    return VQA_OK;
}

// ---------------------------------------------------------------------------
// HaarPSI: both streams, every plane by itself.  A batch of its own, ordered by the stream like a GMSD batch, whose
// host staging (qstage_*) it shares.
static int haarpsi_submit_body(vqa_ctx *c, const uint8_t *ref, const uint8_t *dist, int mem_kind, int n, int64_t ref_fs,
                               int64_t dist_fs, const vqa_plane_desc *planes, int n_planes, bool &touched)
{
    if (bad_batch_args(c, ref, dist, mem_kind, n, planes, n_planes)) return VQA_ERR_INVALID;
    batch_slot &s = c->slot[KIND_HAARPSI];
    plane_batch B;
    int rc = check_batch(s, n, ref_fs, dist_fs, planes, n_planes, B,
                         [](const vqa_plane_desc &d) { return side_and_area_limits(d, HAARPSI_MIN_DIM); });
    if (rc) return rc;
    if ((rc = stage_pair(c, touched, mem_kind, n, B.span, ref, ref_fs, dist, dist_fs))) return rc;
    hipStream_t st = c->stream;
    const size_t nent = (size_t)n * n_planes;
    const size_t acc_bytes = sizeof(unsigned long long) * HAARPSI_WORDS * nent;
    if ((rc = ensure(c, s.dev, acc_bytes))) return rc;
    if ((rc = ensure_pinned(c, s.host, acc_bytes))) return rc;
    HIPCHK(c, hipMemsetAsync(s.dev.p, 0, acc_bytes, st));
    const int depth = B.depth;
    for_each_slice(c, n, [&](int a0, int m) {
        unsigned long long *acc = (unsigned long long *)s.dev.p + (size_t)a0 * n_planes * HAARPSI_WORDS;
        const uint8_t *sref = ref + (int64_t)a0 * ref_fs, *sdist = dist + (int64_t)a0 * dist_fs;
        for_each_group(planes, n_planes, [&](const int *idx, int cnt) {
            prof_scope ps_(c, VQA_K_HAARPSI);
            launch_haarpsi(st, sref, sdist, m, ref_fs, dist_fs, planes, idx, cnt, n_planes, depth, acc);
        });
    });
    return finish_batch(c, s, acc_bytes, (int)nent, planes, n_planes, depth);
}

int vqa_haarpsi_submit(vqa_ctx *c, const uint8_t *ref, const uint8_t *dist, int mem_kind, int n, int64_t ref_fs,
                       int64_t dist_fs, const vqa_plane_desc *planes, int n_planes)
{
    return submit_and_drain(c, [&](bool &touched) {
        return haarpsi_submit_body(c, ref, dist, mem_kind, n, ref_fs, dist_fs, planes, n_planes, touched);
    });
}

int vqa_haarpsi_wait(vqa_ctx *c, vqa_haarpsi_metrics *out, int n_entries)
{
    return wait_batch(c, KIND_HAARPSI, out, n_entries, HAARPSI_WORDS,
                      [](const unsigned long long *acc, const batch_slot &, int, vqa_haarpsi_metrics *o) { haarpsi_finalize(acc, o); });
}

// ---------------------------------------------------------------------------
// VCA texture features: the reference stream alone and the frame before each frame, every plane by itself.  A batch of its
// own, ordered by the stream like an SI/TI batch, whose host staging (siti_stage, siti_prev) it shares.
static int vca_submit_body(vqa_ctx *c, const uint8_t *ref, const uint8_t *prev0, int mem_kind, int n, int64_t ref_fs,
                           const vqa_plane_desc *planes, int n_planes, bool &touched)
{
    if (bad_batch_args(c, ref, ref, mem_kind, n, planes, n_planes)) return VQA_ERR_INVALID;
    batch_slot &s = c->slot[KIND_VCA];
    dbuf &vca_tabs = s.work[0];
    plane_batch B;
    int rc = check_batch(s, n, ref_fs, ref_fs, planes, n_planes, B, [&](const vqa_plane_desc &d) -> int {
        if (int lim = side_and_area_limits(d, VCA_MIN_DIM)) return lim;
        if (B.depth > 8 && (int64_t)d.width * d.height > (1ll << 26)) return VQA_ERR_UNSUPPORTED;
        if (d.pixel_step != B.bps) return VQA_ERR_UNSUPPORTED;   // planar layouts only
        return VQA_OK;
    });
    if (rc) return rc;
    if ((rc = stage_batch(c, touched, mem_kind, n, B.span, {&ref, ref_fs, &c->siti_stage}, {}, {&prev0, 0, &c->siti_prev}))) return rc;
    hipStream_t st = c->stream;
    int pw[4], ph[4];
    for (int p = 0; p < n_planes; p++) { pw[p] = planes[p].width; ph[p] = planes[p].height; }
    const vca_geom g = vca_geometry(pw, ph, n_planes);
    const size_t acc_words = (size_t)n * n_planes * VCA_WORDS, map_words = g.slot_words * (size_t)n;
    // device: the words, prev0's slot, the frames' slots; host: the same without prev0's slot
    if ((rc = ensure(c, s.dev, sizeof(unsigned long long) * (acc_words + g.slot_words + map_words)))) return rc;
    if ((rc = ensure_pinned(c, s.host, sizeof(unsigned long long) * (acc_words + map_words)))) return rc;
    const bool fresh_tabs = !vca_tabs.p;
    if ((rc = ensure(c, vca_tabs, sizeof(float) * VCA_TABLE_FLOATS))) return rc;
    if (fresh_tabs) {
        static const std::vector<float> tabs = [] { std::vector<float> t(VCA_TABLE_FLOATS); vca_tables(t.data()); return t; }();
        HIPCHK(c, hipMemcpyAsync(vca_tabs.p, tabs.data(), sizeof(float) * VCA_TABLE_FLOATS, hipMemcpyHostToDevice, st));
    }
    unsigned long long *acc = (unsigned long long *)s.dev.p, *map = acc + acc_words + g.slot_words;   // frame 0's slot
    const int depth = B.depth;
    for_each_slice(c, n, [&](int a0, int m) {
        const uint8_t *sref = ref + (int64_t)a0 * ref_fs;
        unsigned long long *smap = map + (size_t)a0 * g.slot_words;
        for_each_group(planes, n_planes, [&](const int *idx, int cnt) {
            prof_scope ps_(c, VQA_K_VCA_BLOCKS);
            // (a later slice's predecessor is the slice before's last frame, whose slot is filled already)
            launch_vca_blocks(st, sref, a0 > 0 ? nullptr : prev0, m, ref_fs, planes, idx, cnt, g, depth,
                              (const float *)vca_tabs.p, smap);
        });
        prof_scope ps_(c, VQA_K_VCA_SUM);
        launch_vca_sum(st, m, n_planes, g, a0 > 0 || prev0 != nullptr, smap, acc + (size_t)a0 * n_planes * VCA_WORDS);
    });
    // (the tail inline: the block map follows the words in the pinned copy, without prev0's slot)
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(s.host.p, acc, sizeof(unsigned long long) * acc_words, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync((unsigned long long *)s.host.p + acc_words, map, sizeof(unsigned long long) * map_words,
                             hipMemcpyDeviceToHost, st));
    record_batch(s, n * n_planes, planes, n_planes, depth);
    return VQA_OK;
}

int vqa_vca_submit(vqa_ctx *c, const uint8_t *ref, const uint8_t *prev0, int mem_kind, int n, int64_t ref_fs,
                   const vqa_plane_desc *planes, int n_planes)
{
    return submit_and_drain(c, [&](bool &touched) {
        return vca_submit_body(c, ref, prev0, mem_kind, n, ref_fs, planes, n_planes, touched);
    });
}

int vqa_vca_wait(vqa_ctx *c, vqa_vca_metrics *out, int n_entries, uint64_t *blocks, int64_t n_block_words)
{
    batch_slot *s;
    if (int rc = wait_pending(c, KIND_VCA, out, n_entries, s)) return rc;
    const int npl = s->planes, n = n_entries / npl;
    const vca_geom g = vca_geometry(s->w, s->h, npl);
    const size_t nb = g.slot_words / 3;
    if (blocks && n_block_words != (int64_t)(2 * nb * (size_t)n)) return VQA_ERR_INVALID;   // (the batch stays pending)
    if (int rc = wait_synced(c)) return rc;
    const unsigned long long *acc = (const unsigned long long *)s->host.p, *map = acc + (size_t)n_entries * VCA_WORDS;
    for (int e = 0; e < n_entries; e++) {
        const int p = e % npl;
        vca_finalize(acc + (size_t)e * VCA_WORDS, g.nbx[p], g.nby[p], s->depth, out + e);
    }
    if (blocks)
        for (size_t i = 0; i < nb * (size_t)n; i++) { blocks[2 * i] = map[3 * i]; blocks[2 * i + 1] = map[3 * i + 1]; }
    s->entries = 0;
    return VQA_OK;
}

// ---------------------------------------------------------------------------
// Blockiness, blur and noise: one stream, every plane by itself.  A batch of its own, ordered by the stream like a
// CAMBI batch, whose host staging (qstage_dist, the buffer of the stream it measures in a one-pass run) it shares.
static int artifacts_submit_body(vqa_ctx *c, const uint8_t *frames, int mem_kind, int n, int64_t fs, const vqa_plane_desc *planes,
                                 int n_planes, bool &touched)
{
    if (bad_batch_args(c, frames, frames, mem_kind, n, planes, n_planes)) return VQA_ERR_INVALID;
    batch_slot &s = c->slot[KIND_ARTIFACTS];
    plane_batch B;
    int rc = check_batch(s, n, fs, fs, planes, n_planes, B,
                         [](const vqa_plane_desc &d) { return side_and_area_limits(d, ARTIFACTS_MIN_DIM); });
    if (rc) return rc;
    if ((rc = stage_batch(c, touched, mem_kind, n, B.span, {&frames, fs, &c->qstage_dist}))) return rc;
    hipStream_t st = c->stream;
    const size_t nent = (size_t)n * n_planes;
    const size_t acc_bytes = sizeof(unsigned long long) * ARTIFACTS_WORDS * nent;
    if ((rc = ensure(c, s.dev, acc_bytes))) return rc;
    if ((rc = ensure_pinned(c, s.host, acc_bytes))) return rc;
    HIPCHK(c, hipMemsetAsync(s.dev.p, 0, acc_bytes, st));
    const int depth = B.depth;
    for_each_slice(c, n, [&](int a0, int m) {
        unsigned long long *acc = (unsigned long long *)s.dev.p + (size_t)a0 * n_planes * ARTIFACTS_WORDS;
        const uint8_t *sfr = frames + (int64_t)a0 * fs;
        for_each_group(planes, n_planes, [&](const int *idx, int cnt) {
            prof_scope ps_(c, VQA_K_ARTIFACTS);
            launch_artifacts(st, sfr, m, fs, planes, idx, cnt, n_planes, depth, acc);
        });
    });
    return finish_batch(c, s, acc_bytes, (int)nent, planes, n_planes, depth);
}

int vqa_artifacts_submit(vqa_ctx *c, const uint8_t *frames, int mem_kind, int n, int64_t fs, const vqa_plane_desc *planes,
                         int n_planes)
{
    return submit_and_drain(c, [&](bool &touched) {
        return artifacts_submit_body(c, frames, mem_kind, n, fs, planes, n_planes, touched);
    });
}

int vqa_artifacts_wait(vqa_ctx *c, vqa_artifacts_metrics *out, int n_entries)
{
    return wait_batch(c, KIND_ARTIFACTS, out, n_entries, ARTIFACTS_WORDS,
                      [](const unsigned long long *acc, const batch_slot &s, int p, vqa_artifacts_metrics *o) {
                          artifacts_finalize(acc, s.h[p], s.w[p], s.depth, o);
                      });
}

// ---------------------------------------------------------------------------
// BRISQUE: one stream, every plane by itself.  A batch of its own, ordered by the stream like a CAMBI batch, whose
// host staging (qstage_dist, the buffer of the stream it measures in a one-pass run) it shares.
static int brisque_submit_body(vqa_ctx *c, const uint8_t *frames, int mem_kind, int n, int64_t fs, const vqa_plane_desc *planes,
                               int n_planes, bool &touched)
{
    if (bad_batch_args(c, frames, frames, mem_kind, n, planes, n_planes)) return VQA_ERR_INVALID;
    batch_slot &s = c->slot[KIND_BRISQUE];
    dbuf &brisque_scratch = s.work[0];
    plane_batch B;
    int rc = check_batch(s, n, fs, fs, planes, n_planes, B,
                         [](const vqa_plane_desc &d) { return side_and_area_limits(d, BRISQUE_MIN_DIM); });
    if (rc) return rc;
    if ((rc = stage_batch(c, touched, mem_kind, n, B.span, {&frames, fs, &c->qstage_dist}))) return rc;
    hipStream_t st = c->stream;
    const size_t nent = (size_t)n * n_planes;
    const size_t acc_bytes = sizeof(unsigned long long) * BRISQUE_WORDS * nent;
    const size_t per_frame = largest_group_bytes(planes, n_planes, [](int cnt, int h, int w) { return brisque_scratch_bytes(cnt, h, w); });
    if ((rc = ensure(c, s.dev, acc_bytes))) return rc;
    if ((rc = ensure(c, brisque_scratch, per_frame * (size_t)slice_frames(c, n)))) return rc;
    if ((rc = ensure_pinned(c, s.host, acc_bytes))) return rc;
    HIPCHK(c, hipMemsetAsync(s.dev.p, 0, acc_bytes, st));
    const int depth = B.depth;
    marks mk(c);
    for_each_slice(c, n, [&](int a0, int m) {
        unsigned long long *acc = (unsigned long long *)s.dev.p + (size_t)a0 * n_planes * BRISQUE_WORDS;
        const uint8_t *sfr = frames + (int64_t)a0 * fs;
        for_each_group(planes, n_planes, [&](const int *idx, int cnt) {
            launch_brisque(st, sfr, m, fs, planes, idx, cnt, n_planes, depth, brisque_scratch.p, acc, marks::mark, &mk);
        });
    });
    return finish_batch(c, s, acc_bytes, (int)nent, planes, n_planes, depth);
}

int vqa_brisque_submit(vqa_ctx *c, const uint8_t *frames, int mem_kind, int n, int64_t fs, const vqa_plane_desc *planes,
                       int n_planes)
{
    return submit_and_drain(c, [&](bool &touched) {
        return brisque_submit_body(c, frames, mem_kind, n, fs, planes, n_planes, touched);
    });
}

int vqa_brisque_wait(vqa_ctx *c, vqa_brisque_metrics *out, int n_entries)
{
    return wait_batch(c, KIND_BRISQUE, out, n_entries, BRISQUE_WORDS,
                      [](const unsigned long long *acc, const batch_slot &s, int p, vqa_brisque_metrics *o) {
                          brisque_finalize(acc, s.h[p], s.w[p], o);
                      });
}

// ---------------------------------------------------------------------------
// MDSI: both streams, the planes of a pixel together, one entry per frame.  A batch of its own, ordered by the stream
// like a CIEDE2000 batch, whose host staging (qstage_*) and geometry rules it shares.
static int mdsi_submit_body(vqa_ctx *c, const uint8_t *ref, const uint8_t *dist, int mem_kind, int n, int64_t ref_fs,
                            int64_t dist_fs, const vqa_plane_desc *planes, int n_planes, int model, bool &touched)
{
    if (bad_batch_args(c, ref, dist, mem_kind, n, planes, n_planes)) return VQA_ERR_INVALID;
    if (n_planes != 1 && n_planes != 3) return VQA_ERR_INVALID;
    if (model != VQA_MDSI_YUV709 && model != VQA_MDSI_BGR && model != VQA_MDSI_GRAY) return VQA_ERR_INVALID;
    if ((n_planes == 1) != (model == VQA_MDSI_GRAY)) return VQA_ERR_INVALID;
    batch_slot &s = c->slot[KIND_MDSI];
    dbuf &mdsi_map = s.work[0];
    plane_batch B;
    int rc = check_batch(s, n, ref_fs, dist_fs, planes, n_planes, B, plane0_limits(planes, MDSI_MIN_DIM),
                         n_planes != 3 ? JOINT_NONE : model == VQA_MDSI_BGR ? JOINT_BGR : JOINT_YUV);
    if (rc) return rc;
    if ((rc = stage_pair(c, touched, mem_kind, n, B.span, ref, ref_fs, dist, dist_fs))) return rc;
    hipStream_t st = c->stream;
    const vqa_plane_desc &y = planes[0];
    const size_t acc_bytes = sizeof(unsigned long long) * MDSI_WORDS * (size_t)n;
    if ((rc = ensure(c, s.dev, acc_bytes))) return rc;
    if ((rc = ensure(c, mdsi_map, mdsi_scratch_bytes(y.height, y.width) * (size_t)slice_frames(c, n)))) return rc;
    if ((rc = ensure_pinned(c, s.host, acc_bytes))) return rc;
    HIPCHK(c, hipMemsetAsync(s.dev.p, 0, acc_bytes, st));
    const int depth = B.depth;
    marks mk(c);
    for_each_slice(c, n, [&](int a0, int m) {
        launch_mdsi(st, ref + (int64_t)a0 * ref_fs, dist + (int64_t)a0 * dist_fs, m, ref_fs, dist_fs, planes, n_planes, depth, model,
                    mdsi_map.p, (unsigned long long *)s.dev.p + (size_t)a0 * MDSI_WORDS, marks::mark, &mk);
    });
    return finish_batch(c, s, acc_bytes, n, planes, n_planes, depth);
}

int vqa_mdsi_submit(vqa_ctx *c, const uint8_t *ref, const uint8_t *dist, int mem_kind, int n, int64_t ref_fs, int64_t dist_fs,
                    const vqa_plane_desc *planes, int n_planes, int model)
{
    return submit_and_drain(c, [&](bool &touched) {
        return mdsi_submit_body(c, ref, dist, mem_kind, n, ref_fs, dist_fs, planes, n_planes, model, touched);
    });
}

int vqa_mdsi_factor(int height, int width) { return height > 0 && width > 0 ? mdsi_factor(height, width) : 0; }

int vqa_mdsi_wait(vqa_ctx *c, vqa_mdsi_metrics *out, int n_entries)
{
    // (one entry per frame: plane 0, for the host's part)
    return wait_batch(c, KIND_MDSI, out, n_entries, MDSI_WORDS,
                      [](const unsigned long long *acc, const batch_slot &s, int, vqa_mdsi_metrics *o) {
                          mdsi_finalize(acc, s.h[0], s.w[0], o);
                      });
}

// ---------------------------------------------------------------------------
// dE_ITP: both streams, the three planes of a pixel together, one entry per frame.  A batch of its own, ordered by the
// stream like a CIEDE2000 batch, whose host staging (qstage_*) and geometry rules it shares.
static int itp_submit_body(vqa_ctx *c, const uint8_t *ref, const uint8_t *dist, int mem_kind, int n, int64_t ref_fs,
                           int64_t dist_fs, const vqa_plane_desc *planes, int n_planes, int model, int transfer, int full_range,
                           bool &touched)
{
    if (bad_batch_args(c, ref, dist, mem_kind, n, planes, n_planes)) return VQA_ERR_INVALID;
    if (n_planes != 3 || (model != VQA_ITP_YUV2020 && model != VQA_ITP_BGR)) return VQA_ERR_INVALID;
    if ((transfer != VQA_ITP_PQ && transfer != VQA_ITP_HLG) || (full_range != 0 && full_range != 1)) return VQA_ERR_INVALID;
    batch_slot &s = c->slot[KIND_ITP];
    plane_batch B;
    int rc = check_batch(s, n, ref_fs, dist_fs, planes, n_planes, B, plane0_limits(planes, ITP_MIN_DIM),
                         model == VQA_ITP_BGR ? JOINT_BGR : JOINT_YUV);
    if (rc) return rc;
    if ((rc = stage_pair(c, touched, mem_kind, n, B.span, ref, ref_fs, dist, dist_fs))) return rc;
    hipStream_t st = c->stream;
    const size_t acc_bytes = sizeof(unsigned long long) * ITP_WORDS * (size_t)n;
    if ((rc = ensure(c, s.dev, acc_bytes))) return rc;
    if ((rc = ensure_pinned(c, s.host, acc_bytes))) return rc;
    HIPCHK(c, hipMemsetAsync(s.dev.p, 0, acc_bytes, st));
    const int depth = B.depth;
    for_each_slice(c, n, [&](int a0, int m) {
        prof_scope ps_(c, VQA_K_ITP);
        launch_itp(st, ref + (int64_t)a0 * ref_fs, dist + (int64_t)a0 * dist_fs, m, ref_fs, dist_fs, planes, depth, model, transfer,
                   full_range, (unsigned long long *)s.dev.p + (size_t)a0 * ITP_WORDS);
    });
    return finish_batch(c, s, acc_bytes, n, planes, n_planes, depth);
}

int vqa_itp_submit(vqa_ctx *c, const uint8_t *ref, const uint8_t *dist, int mem_kind, int n, int64_t ref_fs, int64_t dist_fs,
                   const vqa_plane_desc *planes, int n_planes, int model, int transfer, int full_range)
{
    return submit_and_drain(c, [&](bool &touched) {
        return itp_submit_body(c, ref, dist, mem_kind, n, ref_fs, dist_fs, planes, n_planes, model, transfer, full_range, touched);
    });
}

int vqa_itp_wait(vqa_ctx *c, vqa_itp_metrics *out, int n_entries)
{
    // (one entry per frame: the luma grid, for the host's mean)
    return wait_batch(c, KIND_ITP, out, n_entries, ITP_WORDS,
                      [](const unsigned long long *acc, const batch_slot &s, int, vqa_itp_metrics *o) {
                          itp_finalize(acc, s.h[0], s.w[0], o);
                      });
}

// ---------------------------------------------------------------------------
// PU21-PSNR / PU21-SSIM: both streams, the three planes of a pixel together, one entry per frame.  A batch of its own,
// ordered by the stream like a dE_ITP batch, whose checks, host staging (qstage_*) and geometry rules it shares.

// the frames of one sub-slice: the two q_Y maps of that many frames stay within PU21_MAP_BUDGET (lab build: or what the seam says)
static inline int pu21_subslice(const vqa_ctx *c, int h, int w)
{
#ifdef VQA_TEST_SEAMS
    if (c->seam_pu21_sub > 0) return c->seam_pu21_sub;
#endif
    (void)c;
    const size_t per = PU21_MAP_BUDGET / pu21_map_bytes(h, w);
    return per < 1 ? 1 : per > (size_t)QSLICE ? QSLICE : (int)per;
}

static int pu21_submit_body(vqa_ctx *c, const uint8_t *ref, const uint8_t *dist, int mem_kind, int n, int64_t ref_fs,
                            int64_t dist_fs, const vqa_plane_desc *planes, int n_planes, int model, int transfer, int full_range,
                            bool &touched)
{
    if (bad_batch_args(c, ref, dist, mem_kind, n, planes, n_planes)) return VQA_ERR_INVALID;
    if (n_planes != 3 || (model != VQA_ITP_YUV2020 && model != VQA_ITP_BGR)) return VQA_ERR_INVALID;
    if ((transfer != VQA_ITP_PQ && transfer != VQA_ITP_HLG) || (full_range != 0 && full_range != 1)) return VQA_ERR_INVALID;
    batch_slot &s = c->slot[KIND_PU21];
    dbuf &pu21_map = s.work[0];
    plane_batch B;
    int rc = check_batch(s, n, ref_fs, dist_fs, planes, n_planes, B, plane0_limits(planes, PU21_MIN_DIM),
                         model == VQA_ITP_BGR ? JOINT_BGR : JOINT_YUV);
    if (rc) return rc;
    if ((rc = stage_pair(c, touched, mem_kind, n, B.span, ref, ref_fs, dist, dist_fs))) return rc;
    hipStream_t st = c->stream;
    const vqa_plane_desc &y = planes[0];
    const size_t acc_bytes = sizeof(unsigned long long) * PU21_WORDS * (size_t)n;
    const size_t map_bytes = pu21_map_bytes(y.height, y.width);
    const int sub = pu21_subslice(c, y.height, y.width);
    const int sub_frames = sub < slice_frames(c, n) ? sub : slice_frames(c, n);
    if ((rc = ensure(c, s.dev, acc_bytes))) return rc;
    if ((rc = ensure(c, pu21_map, map_bytes * (size_t)sub_frames))) return rc;
    if ((rc = ensure_pinned(c, s.host, acc_bytes))) return rc;
#ifdef VQA_TEST_SEAMS
    dbuf &pu21_keep = s.work[1];
    c->last_u_n = 0;
    if ((rc = ensure(c, pu21_keep, map_bytes * (size_t)n))) return rc;
#endif
    HIPCHK(c, hipMemsetAsync(s.dev.p, 0, acc_bytes, st));
    const int depth = B.depth;
    hipError_t copy_err = hipSuccess;
    for_each_slice(c, n, [&](int a0, int m) {
        for (int b0 = 0; b0 < m; b0 += sub_frames) {
            const int k = m - b0 < sub_frames ? m - b0 : sub_frames, at = a0 + b0;
            unsigned long long *acc = (unsigned long long *)s.dev.p + (size_t)at * PU21_WORDS;
            {
                prof_scope ps_(c, VQA_K_PU21_ENCODE);
                launch_pu21_encode(st, ref + (int64_t)at * ref_fs, dist + (int64_t)at * dist_fs, k, ref_fs, dist_fs, planes, depth,
                                   model, transfer, full_range, (uint32_t *)pu21_map.p, acc);
            }
            {
                prof_scope ps_(c, VQA_K_PU21_SSIM);
                launch_pu21_ssim(st, (const uint32_t *)pu21_map.p, k, y.height, y.width, acc);
            }
#ifdef VQA_TEST_SEAMS
            const hipError_t e = hipMemcpyAsync((uint8_t *)pu21_keep.p + map_bytes * (size_t)at, pu21_map.p,
                                                map_bytes * (size_t)k, hipMemcpyDeviceToDevice, st);
            if (e != hipSuccess) copy_err = e;
#endif
        }
    });
    HIPCHK(c, copy_err);
    if ((rc = finish_batch(c, s, acc_bytes, n, planes, n_planes, depth))) return rc;
#ifdef VQA_TEST_SEAMS
    c->last_u_n = n; c->last_u_w = y.width; c->last_u_h = y.height;
#endif
    return VQA_OK;
}

int vqa_pu21_submit(vqa_ctx *c, const uint8_t *ref, const uint8_t *dist, int mem_kind, int n, int64_t ref_fs, int64_t dist_fs,
                    const vqa_plane_desc *planes, int n_planes, int model, int transfer, int full_range)
{
    return submit_and_drain(c, [&](bool &touched) {
        return pu21_submit_body(c, ref, dist, mem_kind, n, ref_fs, dist_fs, planes, n_planes, model, transfer, full_range, touched);
    });
}

int vqa_pu21_wait(vqa_ctx *c, vqa_pu21_metrics *out, int n_entries)
{
    // (one entry per frame: the luma grid, for the host's divisions)
    return wait_batch(c, KIND_PU21, out, n_entries, PU21_WORDS,
                      [](const unsigned long long *acc, const batch_slot &s, int, vqa_pu21_metrics *o) {
                          pu21_finalize(acc, s.h[0], s.w[0], o);
                      });
}

double vqa_pu21_encode(double cd_m2) { return pu21_encode_host(cd_m2); }

#ifdef VQA_TEST_SEAMS
int vqa_pu21_lab_read_maps(vqa_ctx *c, uint32_t *dst, int64_t n_values)
{
    if (!c || !dst) return VQA_ERR_INVALID;
    if (c->slot[KIND_PU21].entries || !c->last_u_n) return VQA_ERR_STATE;
    if (n_values != (int64_t)c->last_u_n * 2 * c->last_u_h * c->last_u_w) return VQA_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(dst, c->slot[KIND_PU21].work[1].p, sizeof(uint32_t) * (size_t)n_values, hipMemcpyDeviceToHost));
    return VQA_OK;
}
#endif

// ---------------------------------------------------------------------------
// FSIM / FSIMc: both streams, the planes of a pixel together, one entry per frame.  A batch of its own, ordered by the
// stream like an MDSI batch, whose checks, host staging (qstage_*) and geometry rules it shares.

// the frames of one sub-slice: the intermediates of that many frames stay within FSIM_SCRATCH_BUDGET (lab build: or what the seam says)
static inline int fsim_subslice(const vqa_ctx *c, int h, int w)
{
#ifdef VQA_TEST_SEAMS
    if (c->seam_fsim_sub > 0) return c->seam_fsim_sub < FSIM_MAX_SUBSLICE ? c->seam_fsim_sub : FSIM_MAX_SUBSLICE;
#endif
    (void)c;
    const size_t per = FSIM_SCRATCH_BUDGET / fsim_scratch_bytes(h, w);
    return per < 1 ? 1 : per > (size_t)FSIM_MAX_SUBSLICE ? FSIM_MAX_SUBSLICE : (int)per;
}

static int fsim_submit_body(vqa_ctx *c, const uint8_t *ref, const uint8_t *dist, int mem_kind, int n, int64_t ref_fs,
                            int64_t dist_fs, const vqa_plane_desc *planes, int n_planes, int model, bool &touched)
{
    if (bad_batch_args(c, ref, dist, mem_kind, n, planes, n_planes)) return VQA_ERR_INVALID;
    if (n_planes != 1 && n_planes != 3) return VQA_ERR_INVALID;
    if (model != VQA_FSIM_YUV709 && model != VQA_FSIM_BGR && model != VQA_FSIM_GRAY) return VQA_ERR_INVALID;
    if ((n_planes == 1) != (model == VQA_FSIM_GRAY)) return VQA_ERR_INVALID;
    batch_slot &s = c->slot[KIND_FSIM];
    dbuf &fsim_scratch = s.work[0], &fsim_map = s.work[1];
    plane_batch B;
    int rc = check_batch(s, n, ref_fs, dist_fs, planes, n_planes, B, plane0_limits(planes, FSIM_MIN_DIM),
                         n_planes != 3 ? JOINT_NONE : model == VQA_FSIM_BGR ? JOINT_BGR : JOINT_YUV);
    if (rc) return rc;
    const vqa_plane_desc &y = planes[0];
    int f, hd, wd;
    fsim_grid(y.height, y.width, &f, &hd, &wd);
    if (hd > FSIM_MAX_GRID || wd > FSIM_MAX_GRID) return VQA_ERR_UNSUPPORTED;   // (the last refusal, after every check the kinds share)
    if ((rc = stage_pair(c, touched, mem_kind, n, B.span, ref, ref_fs, dist, dist_fs))) return rc;
    hipStream_t st = c->stream;
    fsim_tabs tabs;
    if ((rc = get_fsim_tabs(c, hd, wd, &tabs))) return rc;
    const size_t acc_bytes = sizeof(unsigned long long) * FSIM_WORDS * (size_t)n;
    const size_t map_bytes = 2 * sizeof(uint32_t) * (size_t)hd * (size_t)wd;   // the two p maps of a frame
    const int sub = fsim_subslice(c, y.height, y.width);
    const int sub_frames = sub < slice_frames(c, n) ? sub : slice_frames(c, n);
    if ((rc = ensure(c, s.dev, acc_bytes))) return rc;
    if ((rc = ensure(c, fsim_scratch, fsim_scratch_bytes(y.height, y.width) * (size_t)sub_frames))) return rc;
    if ((rc = ensure(c, fsim_map, map_bytes * (size_t)sub_frames))) return rc;
    if ((rc = ensure_pinned(c, s.host, acc_bytes))) return rc;
#ifdef VQA_TEST_SEAMS
    dbuf &fsim_keep = s.work[2];
    c->last_f_n = 0;
    if ((rc = ensure(c, fsim_keep, map_bytes * (size_t)n))) return rc;
#endif
    HIPCHK(c, hipMemsetAsync(s.dev.p, 0, acc_bytes, st));
    const int depth = B.depth;
    marks mk(c);
    hipError_t copy_err = hipSuccess;
    for_each_slice(c, n, [&](int a0, int m) {
        for (int b0 = 0; b0 < m; b0 += sub_frames) {
            const int k = m - b0 < sub_frames ? m - b0 : sub_frames, at = a0 + b0;
            launch_fsim(st, ref + (int64_t)at * ref_fs, dist + (int64_t)at * dist_fs, k, ref_fs, dist_fs, planes, n_planes, depth,
                        model, tabs, fsim_scratch.p, (uint32_t *)fsim_map.p,
                        (unsigned long long *)s.dev.p + (size_t)at * FSIM_WORDS, marks::mark, &mk);
#ifdef VQA_TEST_SEAMS
            const hipError_t e = hipMemcpyAsync((uint8_t *)fsim_keep.p + map_bytes * (size_t)at, fsim_map.p,
                                                map_bytes * (size_t)k, hipMemcpyDeviceToDevice, st);
            if (e != hipSuccess) copy_err = e;
#endif
        }
    });
    HIPCHK(c, copy_err);
    if ((rc = finish_batch(c, s, acc_bytes, n, planes, n_planes, depth))) return rc;
#ifdef VQA_TEST_SEAMS
    c->last_f_n = n; c->last_f_w = wd; c->last_f_h = hd;
#endif
    return VQA_OK;
}

int vqa_fsim_submit(vqa_ctx *c, const uint8_t *ref, const uint8_t *dist, int mem_kind, int n, int64_t ref_fs, int64_t dist_fs,
                    const vqa_plane_desc *planes, int n_planes, int model)
{
    return submit_and_drain(c, [&](bool &touched) {
        return fsim_submit_body(c, ref, dist, mem_kind, n, ref_fs, dist_fs, planes, n_planes, model, touched);
    });
}

int vqa_fsim_wait(vqa_ctx *c, vqa_fsim_metrics *out, int n_entries)
{
    // (one entry per frame: plane 0, for the host's part)
    return wait_batch(c, KIND_FSIM, out, n_entries, FSIM_WORDS,
                      [](const unsigned long long *acc, const batch_slot &s, int, vqa_fsim_metrics *o) {
                          fsim_finalize(acc, s.h[0], s.w[0], o);
                      });
}

static inline bool fsim_bad_grid(int hd, int wd, int orient)
{
    return hd < 2 || wd < 2 || hd > FSIM_MAX_GRID || wd > FSIM_MAX_GRID || orient < 0 || orient > 3;
}

double vqa_fsim_noise_factor(int hd, int wd, int orient)
{
    return fsim_bad_grid(hd, wd, orient) ? (double)NAN : fsim_noise_factor_host(hd, wd, orient);
}

int vqa_fsim_filter(int hd, int wd, int scale, int orient, double *dst)
{
    if (fsim_bad_grid(hd, wd, orient) || scale < 0 || scale > 3 || !dst) return VQA_ERR_INVALID;
    fsim_filter_host(hd, wd, scale, orient, dst);
    return VQA_OK;
}

#ifdef VQA_TEST_SEAMS
int vqa_fsim_lab_read_maps(vqa_ctx *c, uint32_t *dst, int64_t n_values)
{
    if (!c || !dst) return VQA_ERR_INVALID;
    if (c->slot[KIND_FSIM].entries || !c->last_f_n) return VQA_ERR_STATE;
    if (n_values != (int64_t)c->last_f_n * 2 * c->last_f_h * c->last_f_w) return VQA_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(dst, c->slot[KIND_FSIM].work[2].p, sizeof(uint32_t) * (size_t)n_values, hipMemcpyDeviceToHost));
    return VQA_OK;
}
#endif

// ---------------------------------------------------------------------------
// Signal statistics: one stream alone and the frame before each frame, every plane by itself.  A batch of its own, ordered by
// the stream like an SI/TI batch, whose host staging (siti_stage, siti_prev) it shares.

// the words of a frame's profile (the row sums, then the column sums, of every plane in order) and where each plane's start
static int sigstats_profile(const int *w, const int *h, int n_planes, int off[4])
{
    int at = 0;
    for (int p = 0; p < 4; p++) {
        off[p] = at;
        if (p < n_planes) at += h[p] + w[p];
    }
    return at;
}

static int sigstats_submit_body(vqa_ctx *c, const uint8_t *ref, const uint8_t *prev0, int mem_kind, int n, int64_t ref_fs,
                                const vqa_plane_desc *planes, int n_planes, int black_level, int crop_level, bool &touched)
{
    if (bad_batch_args(c, ref, ref, mem_kind, n, planes, n_planes)) return VQA_ERR_INVALID;
    if (black_level > 65535 || crop_level > 65535) return VQA_ERR_INVALID;
    batch_slot &s = c->slot[KIND_SIGSTATS];
    dbuf &sig_hist = s.work[0];
    plane_batch B;
    int rc = check_batch(s, n, ref_fs, ref_fs, planes, n_planes, B, [&](const vqa_plane_desc &d) -> int {
        if (int lim = side_and_area_limits(d, SIGSTATS_MIN_DIM)) return lim;
        // sum_sq: 2^26 squares of 16-bit samples stay below 2^58 (vqa.h)
        if (B.depth > 8 && (int64_t)d.width * d.height > (1ll << 26)) return VQA_ERR_UNSUPPORTED;
        return VQA_OK;
    });
    if (rc) return rc;
    if ((rc = stage_batch(c, touched, mem_kind, n, B.span, {&ref, ref_fs, &c->siti_stage}, {}, {&prev0, 0, &c->siti_prev}))) return rc;
    hipStream_t st = c->stream;
    const int depth = B.depth, bins = sigstats_bins(depth);
    const int black = black_level < 0 ? 32 << (depth - 8) : black_level, crop = crop_level < 0 ? 24 << (depth - 8) : crop_level;
    int pw[4], ph[4], prof_off[4];
    for (int p = 0; p < n_planes; p++) { pw[p] = planes[p].width; ph[p] = planes[p].height; }
    const int prof_words = sigstats_profile(pw, ph, n_planes, prof_off);
    const size_t nent = (size_t)n * n_planes;
    const size_t acc_words = SIGSTATS_WORDS * nent, out_bytes = sizeof(unsigned long long) * (acc_words + (size_t)prof_words * n);
    // the frames of one sub-slice: their histograms stay within SIGSTATS_HIST_BUDGET
    const size_t frame_hist = sizeof(uint32_t) * (size_t)bins * n_planes, fit = SIGSTATS_HIST_BUDGET / frame_hist;
    const int sub_frames = fit < (size_t)slice_frames(c, n) ? (int)fit : slice_frames(c, n);
    if ((rc = ensure(c, s.dev, out_bytes))) return rc;
    if ((rc = ensure(c, sig_hist, frame_hist * (size_t)sub_frames))) return rc;
    if ((rc = ensure_pinned(c, s.host, out_bytes))) return rc;
    HIPCHK(c, hipMemsetAsync(s.dev.p, 0, out_bytes, st));
    unsigned long long *acc = (unsigned long long *)s.dev.p, *prof = acc + acc_words;
    hipError_t set_err = hipSuccess;
    for_each_slice(c, n, [&](int a0, int m) {
        for (int b0 = 0; b0 < m; b0 += sub_frames) {
            const int k = m - b0 < sub_frames ? m - b0 : sub_frames, at = a0 + b0;
            const hipError_t e = hipMemsetAsync(sig_hist.p, 0, frame_hist * (size_t)k, st);
            if (e != hipSuccess) set_err = e;
            const uint8_t *sref = ref + (int64_t)at * ref_fs;
            const uint8_t *sprev = at > 0 ? ref + (int64_t)(at - 1) * ref_fs : prev0;
            unsigned long long *sacc = acc + (size_t)at * n_planes * SIGSTATS_WORDS, *sprof = prof + (size_t)at * prof_words;
            for_each_group(planes, n_planes, [&](const int *idx, int cnt) {
                prof_scope ps_(c, VQA_K_SIGSTATS_ACCUM);
                launch_sigstats_accum(st, sref, sprev, k, ref_fs, planes, idx, cnt, n_planes, depth, prof_off, prof_words,
                                      (uint32_t *)sig_hist.p, sacc, sprof);
            });
            prof_scope ps_(c, VQA_K_SIGSTATS_SCAN);
            launch_sigstats_scan(st, k, planes, n_planes, depth, black, crop, prof_off, prof_words, (const uint32_t *)sig_hist.p,
                                 sprof, sacc);
        }
    });
    HIPCHK(c, set_err);
    return finish_batch(c, s, out_bytes, (int)nent, planes, n_planes, depth);
}

int vqa_sigstats_submit(vqa_ctx *c, const uint8_t *frames, const uint8_t *prev0, int mem_kind, int n, int64_t frame_stride,
                        const vqa_plane_desc *planes, int n_planes, int black_level, int crop_level)
{
    return submit_and_drain(c, [&](bool &touched) {
        return sigstats_submit_body(c, frames, prev0, mem_kind, n, frame_stride, planes, n_planes, black_level, crop_level, touched);
    });
}

int vqa_sigstats_wait(vqa_ctx *c, vqa_sigstats_metrics *out, int n_entries, int profiles, uint64_t *profile_words,
                      int64_t n_profile_words)
{
    batch_slot *s;
    if (int rc = wait_pending(c, KIND_SIGSTATS, out, n_entries, s)) return rc;
    int off[4];
    const int n = n_entries / s->planes, prof_words = sigstats_profile(s->w, s->h, s->planes, off);
    if (profiles && (!profile_words || n_profile_words != (int64_t)prof_words * n)) return VQA_ERR_INVALID;   // (the batch stays pending)
    if (int rc = wait_synced(c)) return rc;
    const unsigned long long *acc = (const unsigned long long *)s->host.p, *prof = acc + (size_t)n_entries * SIGSTATS_WORDS;
    for (int e = 0; e < n_entries; e++) sigstats_finalize(acc + (size_t)e * SIGSTATS_WORDS, s->depth, out + e);
    if (profiles) memcpy(profile_words, prof, sizeof(uint64_t) * (size_t)prof_words * n);
    s->entries = 0;
    return VQA_OK;
}

// ---------------------------------------------------------------------------
// The resampler: one stream, plane i of the source list into plane i of the destination list in the caller's device memory.
// A batch of its own with no result words, ordered by the stream like every other kind - so whatever the ctx is handed next
// reads dst after it has been written.  Host frames are staged in scale_stage.

// the memory `p` points into is device memory of the ctx's device
static bool byte_is_on_device(const vqa_ctx *c, const void *p)
{
    hipPointerAttribute_t a;
    memset(&a, 0, sizeof a);
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return a.type == hipMemoryTypeDevice && a.device == c->device;
}

static int scale_submit_body(vqa_ctx *c, const uint8_t *frames, int mem_kind, int n, int64_t fs, const vqa_plane_desc *planes,
                             uint8_t *dst, int64_t dst_fs, const vqa_plane_desc *dplanes, int n_planes, int filter, bool &touched)
{
    if (bad_batch_args(c, frames, dst, mem_kind, n, planes, n_planes) || !dplanes) return VQA_ERR_INVALID;
    if (!scale_filter_known(filter)) return VQA_ERR_INVALID;
    batch_slot &s = c->slot[KIND_SCALE];
    plane_batch B, D;
    auto limits = [](const vqa_plane_desc &d) { return side_and_area_limits(d, SCALE_MIN_DIM); };
    int rc = check_batch(s, n, fs, fs, planes, n_planes, B, limits);
    if (rc) return rc;
    if ((rc = check_planes(dplanes, n_planes, D, limits))) return rc;
    if (D.depth != B.depth) return VQA_ERR_UNSUPPORTED;
    if (n > 1 && dst_fs < D.span) return VQA_ERR_INVALID;
    for (int p = 0; p < n_planes; p++)
        if (!scale_ratio_ok(planes[p].width, dplanes[p].width) || !scale_ratio_ok(planes[p].height, dplanes[p].height))
            return VQA_ERR_UNSUPPORTED;
    const int64_t dst_bytes = (int64_t)(n - 1) * dst_fs + D.span, src_bytes = (int64_t)(n - 1) * fs + B.span;
    if (!byte_is_on_device(c, dst) || !byte_is_on_device(c, dst + (dst_bytes - 1))) return VQA_ERR_INVALID;
    if (mem_kind == VQA_MEM_DEVICE && (uintptr_t)frames < (uintptr_t)dst + (uint64_t)dst_bytes &&
        (uintptr_t)dst < (uintptr_t)frames + (uint64_t)src_bytes)
        return VQA_ERR_INVALID;
    if ((rc = stage_batch(c, touched, mem_kind, n, B.span, {&frames, fs, &c->scale_stage}))) return rc;
    hipStream_t st = c->stream;
    const int depth = B.depth;
    // the groups: planes alike on BOTH sides go out as one launch
    bool done[4] = {false, false, false, false};
    auto alike = [](const vqa_plane_desc &a, const vqa_plane_desc &b) {
        return a.width == b.width && a.height == b.height && a.row_stride == b.row_stride && a.pixel_step == b.pixel_step;
    };
    for (int p = 0; p < n_planes; p++) {
        if (done[p]) continue;
        scale_job job;
        int cnt = 0;
        for (int q = p; q < n_planes; q++)
            if (!done[q] && alike(planes[q], planes[p]) && alike(dplanes[q], dplanes[p])) {
                job.src_off[cnt] = planes[q].offset;
                job.dst_off[cnt] = dplanes[q].offset;
                cnt++;
                done[q] = true;
            }
        for (int i = cnt; i < 4; i++) { job.src_off[i] = job.src_off[0]; job.dst_off[i] = job.dst_off[0]; }
        const vqa_plane_desc &a = planes[p], &b = dplanes[p];
        scale_tabs tx, ty;
        if ((rc = get_scale_tabs(c, filter, a.width, b.width, tx))) return rc;
        if ((rc = get_scale_tabs(c, filter, a.height, b.height, ty))) return rc;
        // what k_scale's shared memory holds (vqa_kernels.hpp): inside the ratio limits no tile's footprint is larger
        if (tx.span_w > SCALE_FW || ty.span_h > SCALE_FH || tx.ksize > SCALE_KSIZE_MAX || ty.ksize > SCALE_KSIZE_MAX)
            return VQA_ERR_UNSUPPORTED;
        // uint8 samples are summed in 32 bits: 255 sum |k| + 2^21 < 2^31 holds for every table seen (sum |w| stays below 2 even
        // where a window is cut and renormalised); a table that broke it would be refused, not summed wrong
        const int64_t worst = tx.abs_sum > ty.abs_sum ? tx.abs_sum : ty.abs_sum;
        if (depth == 8 && 255 * worst + (1ll << (SCALE_BITS - 1)) >= (1ll << 31)) return VQA_ERR_UNSUPPORTED;
        job.src_fs = fs; job.dst_fs = dst_fs;
        job.src_rs = a.row_stride; job.dst_rs = b.row_stride;
        job.src_step = a.pixel_step; job.dst_step = b.pixel_step;
        job.sw = a.width; job.sh = a.height; job.dw = b.width; job.dh = b.height;
        job.peak = (1 << depth) - 1;
        job.peak_x = a.width == b.width ? (depth > 8 ? 65535 : 255) : job.peak;
        job.kx = tx.k; job.xmin = tx.xmin; job.xcount = tx.count; job.ksx = tx.ksize;
        job.ky = ty.k; job.ymin = ty.xmin; job.ycount = ty.count; job.ksy = ty.ksize;
        for_each_slice(c, n, [&](int a0, int m) {
            job.src = frames + (int64_t)a0 * fs;
            job.dst = dst + (int64_t)a0 * dst_fs;
            prof_scope ps_(c, VQA_K_SCALE);
            launch_scale(st, job, m, cnt, depth);
        });
    }
    HIPCHK(c, hipGetLastError());
    record_batch(s, n, dplanes, n_planes, depth);
    return VQA_OK;
}

int vqa_scale_submit(vqa_ctx *c, const uint8_t *frames, int mem_kind, int n, int64_t frame_stride, const vqa_plane_desc *src_planes,
                     uint8_t *dst, int64_t dst_frame_stride, const vqa_plane_desc *dst_planes, int n_planes, int filter)
{
    return submit_and_drain(c, [&](bool &touched) {
        return scale_submit_body(c, frames, mem_kind, n, frame_stride, src_planes, dst, dst_frame_stride, dst_planes, n_planes,
                                 filter, touched);
    });
}

int vqa_scale_wait(vqa_ctx *c)
{
    if (!c) return VQA_ERR_INVALID;
    batch_slot &s = c->slot[KIND_SCALE];
    if (!s.entries) return VQA_ERR_STATE;
    if (int rc = wait_synced(c)) return rc;
    s.entries = 0;
    return VQA_OK;
}

int vqa_scale_tables(int filter, int in, int out, int32_t *k, int32_t *xmin, int32_t *count, int *ksize)
{
    const int given = (k != nullptr) + (xmin != nullptr) + (count != nullptr);
    if (!scale_filter_known(filter) || in <= 0 || out <= 0 || !ksize || (given != 0 && given != 3)) return VQA_ERR_INVALID;
    if (!scale_ratio_ok(in, out)) return VQA_ERR_UNSUPPORTED;
    *ksize = scale_ksize(filter, in, out);
    if (given) scale_build_axis(filter, in, out, k, xmin, count);
    return VQA_OK;
}

// The planes of a copy (conform, weave) sorted into those a granule copy can take - a contiguous pixel step on both sides; `k`
// planes that interleave on both sides with one window go as one plane of k times the samples - and the others, which the gather
// takes.  odd: 16-bit samples at odd addresses would straddle a granule's dwords: the gather takes them all.  fill(p, P): plane p
// of the submit.
extern "C++" template <class Fill>
static void copy_plan(int n_planes, int bps, bool odd, Fill fill, conform_plane *fast, int &n_fast, conform_plane *slow, int &n_slow)
{
    bool done[4] = {false, false, false, false};
    for (int p = 0; p < n_planes; p++) {
        if (done[p]) continue;
        conform_plane P;
        fill(p, P);
        done[p] = true;
        const int k = P.src_step / bps;
        if (!odd && P.src_step == P.dst_step && P.src_step == bps) {
            fast[n_fast++] = P;
            continue;
        }
        // planes p .. p + k - 1 interleave: the same geometry and window, offsets one sample apart on both sides
        bool inter = !odd && P.src_step == P.dst_step && P.src_step == k * bps && k >= 2 && k <= 3 && p + k <= n_planes;
        for (int q = 1; inter && q < k; q++) {
            conform_plane Q;
            fill(p + q, Q);
            inter = !done[p + q] && Q.src_off == P.src_off + (int64_t)q * bps && Q.dst_off == P.dst_off + (int64_t)q * bps &&
                    Q.src_rs == P.src_rs && Q.dst_rs == P.dst_rs && Q.src_step == P.src_step && Q.dst_step == P.dst_step &&
                    Q.w == P.w && Q.h == P.h && Q.y0 == P.y0 && Q.x0 == P.x0;
        }
        if (inter) {
            for (int q = 1; q < k; q++) done[p + q] = true;
            P.inter = k; P.w *= k; P.x0 *= k;
            fast[n_fast++] = P;
        } else {
            slow[n_slow++] = P;
        }
    }
}

// ---------------------------------------------------------------------------
// Conform: a registered copy of one stream - window, frame gather, table, matrix - into the caller's device memory.  A batch of
// its own with no result words and the resampler's slot semantics.  The frame index and the tables reach the device through the
// slot's pinned copy, so the caller's arrays are free when the submit returns.
static int conform_submit_body(vqa_ctx *c, const uint8_t *frames, int mem_kind, int n_in, int64_t fs, const vqa_plane_desc *planes,
                               uint8_t *dst, int64_t dst_fs, const vqa_plane_desc *dplanes, int n_planes, const int32_t *origin,
                               const int32_t *index, int n_out, const void *lut, const int64_t *matrix, bool &touched)
{
    if (bad_batch_args(c, frames, dst, mem_kind, n_in, planes, n_planes) || !dplanes) return VQA_ERR_INVALID;
    if (!index) n_out = n_in;
    if (n_out <= 0 || (matrix && n_planes != 3)) return VQA_ERR_INVALID;
    if (n_out > CONFORM_MAX_OUT) return VQA_ERR_UNSUPPORTED;
    batch_slot &s = c->slot[KIND_CONFORM];
    plane_batch B, D;
    auto src_limits = [](const vqa_plane_desc &d) { return side_and_area_limits(d, 1); };
    auto dst_limits = [=](const vqa_plane_desc &d) { return side_and_area_limits(d, &d == dplanes ? CONFORM_MIN_DIM : CONFORM_MIN_DIM / 2); };
    int rc = check_batch(s, n_in, fs, fs, planes, n_planes, B, src_limits, matrix ? JOINT_YUV : JOINT_NONE);
    if (rc) return rc;
    if ((rc = check_planes(dplanes, n_planes, D, dst_limits))) return rc;
    if (D.depth != B.depth) return VQA_ERR_UNSUPPORTED;
    if (n_out > 1 && dst_fs < D.span) return VQA_ERR_INVALID;
    const int depth = B.depth, bps = B.bps, bins = 1 << depth, peak = bins - 1;
    for (int p = 0; p < n_planes; p++) {
        const int64_t y0 = origin ? origin[2 * p] : 0, x0 = origin ? origin[2 * p + 1] : 0;
        if (y0 < 0 || x0 < 0 || y0 + dplanes[p].height > planes[p].height || x0 + dplanes[p].width > planes[p].width)
            return VQA_ERR_INVALID;
    }
    if (index)
        for (int j = 0; j < n_out; j++)
            if (index[j] < 0 || index[j] >= n_in) return VQA_ERR_INVALID;
    if (lut)
        for (size_t i = 0; i < (size_t)n_planes * bins; i++)
            if ((bps == 2 ? (int)((const uint16_t *)lut)[i] : (int)((const uint8_t *)lut)[i]) > peak) return VQA_ERR_INVALID;
    if (matrix)
        for (int k = 0; k < 3; k++)
            for (int i = 0; i < 4; i++) {
                const int64_t v = matrix[4 * k + i], lim = i < 3 ? CONFORM_MAX_COEF : CONFORM_MAX_BIAS;
                if (v > lim || v < -lim) return VQA_ERR_INVALID;
            }
    const int64_t dst_bytes = (int64_t)(n_out - 1) * dst_fs + D.span, src_bytes = (int64_t)(n_in - 1) * fs + B.span;
    if (!byte_is_on_device(c, dst) || !byte_is_on_device(c, dst + (dst_bytes - 1))) return VQA_ERR_INVALID;
    if (mem_kind == VQA_MEM_DEVICE && (uintptr_t)frames < (uintptr_t)dst + (uint64_t)dst_bytes &&
        (uintptr_t)dst < (uintptr_t)frames + (uint64_t)src_bytes)
        return VQA_ERR_INVALID;
    if ((rc = stage_batch(c, touched, mem_kind, n_in, B.span, {&frames, fs, &s.work[0]}))) return rc;
    hipStream_t st = c->stream;

    conform_job job;
    memset(&job, 0, sizeof job);
    job.src = frames; job.dst = dst;
    job.src_fs = fs; job.dst_fs = dst_fs;
    job.peak = peak;
    // the index and the tables: the caller's -> the pinned copy -> the device, the tables 16-byte aligned behind the index
    const size_t index_bytes = index ? ((size_t)n_out * sizeof(int32_t) + 15) / 16 * 16 : 0;
    const size_t lut_bytes = lut ? (size_t)n_planes * bins * bps : 0;
    if (index_bytes + lut_bytes) {
        if ((rc = ensure(c, s.work[1], index_bytes + lut_bytes))) return rc;
        if ((rc = ensure_pinned(c, s.host, index_bytes + lut_bytes))) return rc;
        if (index) memcpy(s.host.p, index, (size_t)n_out * sizeof(int32_t));
        if (lut) memcpy((uint8_t *)s.host.p + index_bytes, lut, lut_bytes);
        HIPCHK(c, hipMemcpyAsync(s.work[1].p, s.host.p, index_bytes + lut_bytes, hipMemcpyHostToDevice, st));
        if (index) job.index = (const int32_t *)s.work[1].p;
        if (lut) job.lut = (const uint8_t *)s.work[1].p + index_bytes;
    }
    auto fill = [&](int p, conform_plane &P) {
        const vqa_plane_desc &a = planes[p], &b = dplanes[p];
        P.src_off = a.offset; P.dst_off = b.offset;
        P.src_rs = a.row_stride; P.dst_rs = b.row_stride;
        P.src_step = a.pixel_step; P.dst_step = b.pixel_step;
        P.w = b.width; P.h = b.height;
        P.y0 = origin ? origin[2 * p] : 0; P.x0 = origin ? origin[2 * p + 1] : 0;
        P.inter = 1; P.lut0 = p;
    };
    if (matrix) {
        for (int k = 0; k < 3; k++)
            for (int i = 0; i < 4; i++) job.m[k][i] = matrix[4 * k + i];
        for (int p = 0; p < 3; p++) fill(p, job.plane[p]);
        launch_conform_matrix(st, job, planes[0].height, planes[0].width, planes[1].height, planes[1].width, n_out, depth);
    } else {
        // three launches at most: the granule copy's planes, then the others by the gather (copy_plan)
        const bool odd = bps == 2 && (((uintptr_t)frames | (uintptr_t)dst | (uintptr_t)fs | (uintptr_t)dst_fs) & 1);
        conform_job fast = job, slow = job;
        int n_fast = 0, n_slow = 0;
        copy_plan(n_planes, bps, odd, fill, fast.plane, n_fast, slow.plane, n_slow);
        launch_conform_copy(st, fast, n_out, n_fast, depth, false);
        launch_conform_copy(st, slow, n_out, n_slow, depth, true);
    }
    HIPCHK(c, hipGetLastError());
    record_batch(s, n_out, dplanes, n_planes, depth);
    return VQA_OK;
}

int vqa_conform_submit(vqa_ctx *c, const uint8_t *frames, int mem_kind, int n_in, int64_t frame_stride,
                       const vqa_plane_desc *src_planes, uint8_t *dst, int64_t dst_frame_stride, const vqa_plane_desc *dst_planes,
                       int n_planes, const int32_t *origin, const int32_t *index, int n_out, const void *lut, const int64_t *matrix)
{
    return submit_and_drain(c, [&](bool &touched) {
        return conform_submit_body(c, frames, mem_kind, n_in, frame_stride, src_planes, dst, dst_frame_stride, dst_planes, n_planes,
                                   origin, index, n_out, lut, matrix, touched);
    });
}

int vqa_conform_wait(vqa_ctx *c)
{
    if (!c) return VQA_ERR_INVALID;
    batch_slot &s = c->slot[KIND_CONFORM];
    if (!s.entries) return VQA_ERR_STATE;
    if (int rc = wait_synced(c)) return rc;
    s.entries = 0;
    return VQA_OK;
}

// ---------------------------------------------------------------------------
// Convert: one stream at another sample depth and / or chroma layout, into the caller's device memory.  A batch of its own with
// no result words and conform's slot semantics.  Host frames are staged in the slot's own work buffer (vqa_trim releases it with
// the slot).
static int convert_submit_body(vqa_ctx *c, const uint8_t *frames, int mem_kind, int n, int64_t fs, const vqa_plane_desc *planes,
                               uint8_t *dst, int64_t dst_fs, const vqa_plane_desc *dplanes, int n_planes, int chroma, int siting,
                               int range, bool &touched)
{
    if (bad_batch_args(c, frames, dst, mem_kind, n, planes, n_planes) || !dplanes) return VQA_ERR_INVALID;
    if ((chroma != VQA_CHROMA_BOX && chroma != VQA_CHROMA_LINEAR) || (siting != VQA_SITING_CENTER && siting != VQA_SITING_LEFT) ||
        (range != VQA_RANGE_LIMITED && range != VQA_RANGE_FULL))
        return VQA_ERR_INVALID;
    if (n > CONVERT_MAX_FRAMES) return VQA_ERR_UNSUPPORTED;
    batch_slot &s = c->slot[KIND_CONVERT];
    plane_batch B, D;
    auto src_limits = [=](const vqa_plane_desc &d) { return side_and_area_limits(d, &d == planes ? CONVERT_MIN_DIM : CONVERT_MIN_DIM / 2); };
    auto dst_limits = [=](const vqa_plane_desc &d) { return side_and_area_limits(d, &d == dplanes ? CONVERT_MIN_DIM : CONVERT_MIN_DIM / 2); };
    int rc = check_batch(s, n, fs, fs, planes, n_planes, B, src_limits);
    if (rc) return rc;
    if ((rc = check_planes(dplanes, n_planes, D, dst_limits))) return rc;
    for (int p = 0; p < n_planes; p++)
        if (convert_relation_of(planes[p].width, dplanes[p].width) < 0 || convert_relation_of(planes[p].height, dplanes[p].height) < 0)
            return VQA_ERR_UNSUPPORTED;
    if (n > 1 && dst_fs < D.span) return VQA_ERR_INVALID;
    const int64_t dst_bytes = (int64_t)(n - 1) * dst_fs + D.span, src_bytes = (int64_t)(n - 1) * fs + B.span;
    if (!byte_is_on_device(c, dst) || !byte_is_on_device(c, dst + (dst_bytes - 1))) return VQA_ERR_INVALID;
    if (mem_kind == VQA_MEM_DEVICE && (uintptr_t)frames < (uintptr_t)dst + (uint64_t)dst_bytes &&
        (uintptr_t)dst < (uintptr_t)frames + (uint64_t)src_bytes)
        return VQA_ERR_INVALID;
    if ((rc = stage_batch(c, touched, mem_kind, n, B.span, {&frames, fs, &s.work[0]}))) return rc;

    convert_job job;
    memset(&job, 0, sizeof job);
    job.src = frames; job.dst = dst;
    job.src_fs = fs; job.dst_fs = dst_fs;
    job.chroma = chroma; job.siting = siting; job.range = range;
    job.ds = B.depth; job.dd = D.depth;
    job.inv_ps = 1.0f / (float)((1 << B.depth) - 1);
    // four launches at most: the planes the rows kernel can take (a contiguous pixel step on both sides), one launch per
    // horizontal relation, then the others by the gather.  16-bit samples at odd addresses would straddle a granule's dwords: the
    // gather takes them.
    const bool odd = (B.bps == 2 && (((uintptr_t)frames | (uintptr_t)fs) & 1)) || (D.bps == 2 && (((uintptr_t)dst | (uintptr_t)dst_fs) & 1));
    convert_job group[4] = {job, job, job, job};   // same, up, down; the gather
    int count[4] = {0, 0, 0, 0};
    for (int p = 0; p < n_planes; p++) {
        const vqa_plane_desc &a = planes[p], &b = dplanes[p];
        convert_plane P;
        P.src_off = a.offset; P.dst_off = b.offset;
        P.src_rs = a.row_stride; P.dst_rs = b.row_stride;
        P.src_step = a.pixel_step; P.dst_step = b.pixel_step;
        P.sw = a.width; P.sh = a.height; P.dw = b.width; P.dh = b.height;
        P.rx = convert_relation_of(a.width, b.width); P.ry = convert_relation_of(a.height, b.height);
        const bool rows = !odd && a.pixel_step == B.bps && b.pixel_step == D.bps;
        P.pair = rows && P.ry == CONVERT_UP && b.row_stride % 16 == 0;
        const int g = rows ? P.rx : 3;
        group[g].plane[count[g]++] = P;
    }
    for (int g = 0; g < 4; g++) launch_convert(c->stream, group[g], n, count[g], g, g == 3);
    HIPCHK(c, hipGetLastError());
    record_batch(s, n, dplanes, n_planes, D.depth);
    return VQA_OK;
}

int vqa_convert_submit(vqa_ctx *c, const uint8_t *frames, int mem_kind, int n, int64_t frame_stride, const vqa_plane_desc *src_planes,
                       uint8_t *dst, int64_t dst_frame_stride, const vqa_plane_desc *dst_planes, int n_planes, int chroma, int siting,
                       int range)
{
    return submit_and_drain(c, [&](bool &touched) {
        return convert_submit_body(c, frames, mem_kind, n, frame_stride, src_planes, dst, dst_frame_stride, dst_planes, n_planes,
                                   chroma, siting, range, touched);
    });
}

int vqa_convert_wait(vqa_ctx *c)
{
    if (!c) return VQA_ERR_INVALID;
    batch_slot &s = c->slot[KIND_CONVERT];
    if (!s.entries) return VQA_ERR_STATE;
    if (int rc = wait_synced(c)) return rc;
    s.entries = 0;
    return VQA_OK;
}

// ---------------------------------------------------------------------------
// Fields: the field statistics of one plane of one stream, frame i against frame i - 1.  A batch of its own, ordered by the
// stream like an SI/TI batch.  Host frames and prev0 are staged in the slot's own work buffers.
static int fields_submit_body(vqa_ctx *c, const uint8_t *frames, const uint8_t *prev0, int mem_kind, int n, int64_t fs,
                              const vqa_plane_desc *plane, bool &touched)
{
    if (bad_batch_args(c, frames, frames, mem_kind, n, plane, 1)) return VQA_ERR_INVALID;
    if (n > FIELDS_MAX_FRAMES) return VQA_ERR_UNSUPPORTED;
    batch_slot &s = c->slot[KIND_FIELDS];
    plane_batch B;
    int rc = check_batch(s, n, fs, fs, plane, 1, B, [](const vqa_plane_desc &d) { return side_and_area_limits(d, FIELDS_MIN_DIM); });
    if (rc) return rc;
    if ((rc = stage_batch(c, touched, mem_kind, n, B.span, {&frames, fs, &s.work[0]}, {}, {&prev0, 0, &s.work[1]}))) return rc;
    const size_t bytes = sizeof(unsigned long long) * FIELDS_WORDS * (size_t)n;
    if ((rc = ensure(c, s.dev, bytes))) return rc;
    if ((rc = ensure_pinned(c, s.host, bytes))) return rc;
    HIPCHK(c, hipMemsetAsync(s.dev.p, 0, bytes, c->stream));
    launch_fields_accum(c->stream, frames, prev0, n, fs, plane[0], B.depth, (unsigned long long *)s.dev.p);
    c->fields_prev0 = prev0 != nullptr;
    return finish_batch(c, s, bytes, n, plane, 1, B.depth);
}

int vqa_fields_submit(vqa_ctx *c, const uint8_t *frames, const uint8_t *prev0, int mem_kind, int n, int64_t frame_stride,
                      const vqa_plane_desc *plane)
{
    return submit_and_drain(c, [&](bool &touched) { return fields_submit_body(c, frames, prev0, mem_kind, n, frame_stride, plane, touched); });
}

int vqa_fields_wait(vqa_ctx *c, vqa_fields_metrics *out, int n)
{
    batch_slot *s;
    if (int rc = wait_pending(c, KIND_FIELDS, out, n, s)) return rc;
    if (int rc = wait_synced(c)) return rc;
    const unsigned long long *acc = (const unsigned long long *)s->host.p;
    for (int i = 0; i < n; i++, acc += FIELDS_WORDS) {
        vqa_fields_metrics &o = out[i];
        for (int f = 0; f < 2; f++) {
            o.comb[f] = acc[f]; o.fwd[f] = acc[2 + f]; o.bwd[f] = acc[4 + f]; o.sad[f] = acc[6 + f]; o.changed[f] = acc[8 + f];
        }
        o.count = (uint64_t)(s->h[0] - 4) * (uint64_t)s->w[0];
        o.has_prev = i > 0 || c->fields_prev0;
    }
    s->entries = 0;
    return VQA_OK;
}

// ---------------------------------------------------------------------------
// Weave: frames out of the fields of other frames, into the caller's device memory.  A batch of its own with no result words
// and conform's slot semantics.  The two frame indices reach the device through the slot's pinned copy, so the caller's arrays
// are free when the submit returns.
static int weave_submit_body(vqa_ctx *c, const uint8_t *frames, int mem_kind, int n_in, int64_t fs, const vqa_plane_desc *planes,
                             uint8_t *dst, int64_t dst_fs, const vqa_plane_desc *dplanes, int n_planes, const int32_t *top,
                             const int32_t *bottom, int n_out, bool &touched)
{
    if (bad_batch_args(c, frames, dst, mem_kind, n_in, planes, n_planes) || !dplanes || !top || !bottom || n_out <= 0)
        return VQA_ERR_INVALID;
    if (n_out > WEAVE_MAX_OUT) return VQA_ERR_UNSUPPORTED;
    batch_slot &s = c->slot[KIND_WEAVE];
    plane_batch B, D;
    auto src_limits = [=](const vqa_plane_desc &d) { return side_and_area_limits(d, &d == planes ? WEAVE_MIN_DIM : WEAVE_MIN_DIM / 2); };
    auto dst_limits = [=](const vqa_plane_desc &d) { return side_and_area_limits(d, &d == dplanes ? WEAVE_MIN_DIM : WEAVE_MIN_DIM / 2); };
    int rc = check_batch(s, n_in, fs, fs, planes, n_planes, B, src_limits);
    if (rc) return rc;
    if ((rc = check_planes(dplanes, n_planes, D, dst_limits))) return rc;
    if (D.depth != B.depth) return VQA_ERR_INVALID;
    for (int p = 0; p < n_planes; p++)
        if (planes[p].width != dplanes[p].width || planes[p].height != dplanes[p].height) return VQA_ERR_INVALID;
    if (n_out > 1 && dst_fs < D.span) return VQA_ERR_INVALID;
    for (int j = 0; j < n_out; j++)
        if (top[j] < 0 || top[j] >= n_in || bottom[j] < 0 || bottom[j] >= n_in) return VQA_ERR_INVALID;
    const int64_t dst_bytes = (int64_t)(n_out - 1) * dst_fs + D.span, src_bytes = (int64_t)(n_in - 1) * fs + B.span;
    if (!byte_is_on_device(c, dst) || !byte_is_on_device(c, dst + (dst_bytes - 1))) return VQA_ERR_INVALID;
    if (mem_kind == VQA_MEM_DEVICE && (uintptr_t)frames < (uintptr_t)dst + (uint64_t)dst_bytes &&
        (uintptr_t)dst < (uintptr_t)frames + (uint64_t)src_bytes)
        return VQA_ERR_INVALID;
    if ((rc = stage_batch(c, touched, mem_kind, n_in, B.span, {&frames, fs, &s.work[0]}))) return rc;
    hipStream_t st = c->stream;

    // the indices: the caller's -> the pinned copy -> the device, top then bottom
    const size_t index_bytes = (size_t)n_out * sizeof(int32_t);
    if ((rc = ensure(c, s.work[1], 2 * index_bytes))) return rc;
    if ((rc = ensure_pinned(c, s.host, 2 * index_bytes))) return rc;
    memcpy(s.host.p, top, index_bytes);
    memcpy((uint8_t *)s.host.p + index_bytes, bottom, index_bytes);
    HIPCHK(c, hipMemcpyAsync(s.work[1].p, s.host.p, 2 * index_bytes, hipMemcpyHostToDevice, st));

    weave_job job;
    memset(&job, 0, sizeof job);
    job.src = frames; job.dst = dst;
    job.src_fs = fs; job.dst_fs = dst_fs;
    job.top = (const int32_t *)s.work[1].p; job.bottom = job.top + n_out;
    auto fill = [&](int p, conform_plane &P) {
        const vqa_plane_desc &a = planes[p], &b = dplanes[p];
        P.src_off = a.offset; P.dst_off = b.offset;
        P.src_rs = a.row_stride; P.dst_rs = b.row_stride;
        P.src_step = a.pixel_step; P.dst_step = b.pixel_step;
        P.w = b.width; P.h = b.height;
        P.y0 = 0; P.x0 = 0;
        P.inter = 1; P.lut0 = 0;
    };
    const bool odd = B.bps == 2 && (((uintptr_t)frames | (uintptr_t)dst | (uintptr_t)fs | (uintptr_t)dst_fs) & 1);
    weave_job fast = job, slow = job;
    int n_fast = 0, n_slow = 0;
    copy_plan(n_planes, B.bps, odd, fill, fast.plane, n_fast, slow.plane, n_slow);
    launch_fields_weave(st, fast, n_out, n_fast, B.depth, false);
    launch_fields_weave(st, slow, n_out, n_slow, B.depth, true);
    HIPCHK(c, hipGetLastError());
    record_batch(s, n_out, dplanes, n_planes, B.depth);
    return VQA_OK;
}

int vqa_weave_submit(vqa_ctx *c, const uint8_t *frames, int mem_kind, int n_in, int64_t frame_stride, const vqa_plane_desc *src_planes,
                     uint8_t *dst, int64_t dst_frame_stride, const vqa_plane_desc *dst_planes, int n_planes, const int32_t *top_index,
                     const int32_t *bottom_index, int n_out)
{
    return submit_and_drain(c, [&](bool &touched) {
        return weave_submit_body(c, frames, mem_kind, n_in, frame_stride, src_planes, dst, dst_frame_stride, dst_planes, n_planes,
                                 top_index, bottom_index, n_out, touched);
    });
}

int vqa_weave_wait(vqa_ctx *c)
{
    if (!c) return VQA_ERR_INVALID;
    batch_slot &s = c->slot[KIND_WEAVE];
    if (!s.entries) return VQA_ERR_STATE;
    if (int rc = wait_synced(c)) return rc;
    s.entries = 0;
    return VQA_OK;
}

// ---------------------------------------------------------------------------
// Temporal alignment: plane 0 of both streams, every distorted frame against a band of reference frames.  A batch of its own,
// ordered by the stream like a GMSD batch, whose host staging (qstage_*) it shares; the two streams have their own frame counts,
// which is the one thing the shared frame does not carry: they are staged one by one.
static int align_submit_body(vqa_ctx *c, const uint8_t *ref, int n_ref, const uint8_t *dist, int n_dist, int mem_kind, int64_t ref_fs,
                             int64_t dist_fs, const vqa_plane_desc *plane, int offset, int radius, bool &touched)
{
    if (bad_batch_args(c, ref, dist, mem_kind, n_ref < n_dist ? n_ref : n_dist, plane, 1)) return VQA_ERR_INVALID;
    if (radius < 0 || radius > VQA_ALIGN_MAX_RADIUS) return VQA_ERR_INVALID;
    if (n_dist > ALIGN_MAX_DIST || n_ref > ALIGN_MAX_REF) return VQA_ERR_UNSUPPORTED;
    batch_slot &s = c->slot[KIND_ALIGN];
    plane_batch B;
    int rc = check_batch(s, n_ref, ref_fs, ref_fs, plane, 1, B, [](const vqa_plane_desc &d) { return side_and_area_limits(d, 1); });
    if (rc) return rc;
    if (n_dist > 1 && dist_fs < B.span) return VQA_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    touched = true;
    if (mem_kind == VQA_MEM_HOST) {
        if ((rc = stage(c, c->qstage_ref, ref, (size_t)(n_ref - 1) * ref_fs + B.span))) return rc;
        if ((rc = stage(c, c->qstage_dist, dist, (size_t)(n_dist - 1) * dist_fs + B.span))) return rc;
    }
    hipStream_t st = c->stream;
    const size_t band = 2 * (size_t)radius + 1, words = (size_t)n_dist * band, bytes = sizeof(unsigned long long) * (words + n_dist + n_ref);
    if ((rc = ensure(c, s.dev, bytes))) return rc;
    if ((rc = ensure_pinned(c, s.host, bytes))) return rc;
    HIPCHK(c, hipMemsetAsync(s.dev.p, 0, bytes, st));
    // a pair (j, k) with 0 <= j + offset + k < n_ref exists: only then is anything launched (and offset is small)
    const int64_t lo = (int64_t)offset - radius, hi = (int64_t)n_dist - 1 + offset + radius;
    if (hi >= 0 && lo < n_ref) {
        unsigned long long *cross = (unsigned long long *)s.dev.p;
        prof_scope ps_(c, VQA_K_ALIGN_CROSS);
        launch_align_cross(st, ref, n_ref, dist, n_dist, ref_fs, dist_fs, plane[0], B.depth, offset, radius, cross, cross + words,
                           cross + words + n_dist);
    }
    c->align_n_ref = n_ref; c->align_n_dist = n_dist; c->align_offset = offset; c->align_radius = radius;
    return finish_batch(c, s, bytes, (int)words, plane, 1, B.depth);
}

int vqa_align_submit(vqa_ctx *c, const uint8_t *ref, int n_ref, const uint8_t *dist, int n_dist, int mem_kind, int64_t ref_frame_stride,
                     int64_t dist_frame_stride, const vqa_plane_desc *plane, int offset, int radius)
{
    return submit_and_drain(c, [&](bool &touched) {
        return align_submit_body(c, ref, n_ref, dist, n_dist, mem_kind, ref_frame_stride, dist_frame_stride, plane, offset, radius,
                                 touched);
    });
}

// sse = E_d[j] + E_r[i] - 2 C[j][i] in 64-bit words (the true value is below 2^60, so the wrap-around arithmetic is exact)
int vqa_align_wait(vqa_ctx *c, uint64_t *sse, int64_t n_words)
{
    batch_slot *s;
    if (!c || !sse) return VQA_ERR_INVALID;
    if (n_words != (int64_t)c->slot[KIND_ALIGN].entries) return VQA_ERR_STATE;
    if (int rc = wait_pending(c, KIND_ALIGN, sse, (int)n_words, s)) return rc;
    if (int rc = wait_synced(c)) return rc;
    const int n_dist = c->align_n_dist, n_ref = c->align_n_ref, band = 2 * c->align_radius + 1;
    const unsigned long long *cross = (const unsigned long long *)s->host.p, *ed = cross + (size_t)n_dist * band, *er = ed + n_dist;
    for (int j = 0; j < n_dist; j++)
        for (int k = 0; k < band; k++) {
            const int64_t i = (int64_t)j + c->align_offset + k - c->align_radius;
            const size_t at = (size_t)j * band + k;
            sse[at] = i >= 0 && i < n_ref ? (uint64_t)(ed[j] + er[i] - 2 * cross[at]) : VQA_ALIGN_NONE;
        }
    s->entries = 0;
    return VQA_OK;
}

// ---------------------------------------------------------------------------
// Spatial registration: plane 0 of both streams, every distorted frame against its reference frame at every shift of the band.  A
// batch of its own, ordered by the stream like an alignment batch, whose host staging (qstage_*) it shares.
static int shift_submit_body(vqa_ctx *c, const uint8_t *ref, const uint8_t *dist, int n, int mem_kind, int64_t ref_fs, int64_t dist_fs,
                             const vqa_plane_desc *plane, int radius, int margin, bool &touched)
{
    if (bad_batch_args(c, ref, dist, mem_kind, n, plane, 1)) return VQA_ERR_INVALID;
    if (radius < 1 || radius > VQA_SHIFT_MAX_RADIUS || margin < radius) return VQA_ERR_INVALID;
    if (n > SHIFT_MAX_FRAMES) return VQA_ERR_UNSUPPORTED;
    batch_slot &s = c->slot[KIND_SHIFT];
    plane_batch B;
    // (a margin of half the int range or more leaves no core in any plane: the comparison is made without forming 2M + 1)
    int rc = check_batch(s, n, ref_fs, dist_fs, plane, 1, B, [margin](const vqa_plane_desc &d) {
        if ((d.width - 1) / 2 < margin || (d.height - 1) / 2 < margin) return (int)VQA_ERR_UNSUPPORTED;
        return side_and_area_limits(d, 1);
    });
    if (rc) return rc;
    if ((rc = stage_pair(c, touched, mem_kind, n, B.span, ref, ref_fs, dist, dist_fs))) return rc;
    hipStream_t st = c->stream;
    const size_t grid = (size_t)(2 * radius + 1) * (2 * radius + 1), words = (size_t)n * grid, bytes = sizeof(unsigned long long) * (words + n);
    if ((rc = ensure(c, s.dev, bytes))) return rc;
    if ((rc = ensure_pinned(c, s.host, bytes))) return rc;
    HIPCHK(c, hipMemsetAsync(s.dev.p, 0, bytes, st));
    {
        unsigned long long *out = (unsigned long long *)s.dev.p;
        prof_scope ps_(c, VQA_K_SHIFT);
        launch_shift(st, ref, dist, n, ref_fs, dist_fs, plane[0], B.depth, radius, margin, out, out + words);
    }
    c->shift_n = n; c->shift_radius = radius;
    return finish_batch(c, s, bytes, (int)words, plane, 1, B.depth);
}

int vqa_shift_submit(vqa_ctx *c, const uint8_t *ref, const uint8_t *dist, int n, int mem_kind, int64_t ref_frame_stride,
                     int64_t dist_frame_stride, const vqa_plane_desc *plane, int radius, int margin)
{
    return submit_and_drain(c, [&](bool &touched) {
        return shift_submit_body(c, ref, dist, n, mem_kind, ref_frame_stride, dist_frame_stride, plane, radius, margin, touched);
    });
}

// sse = E_d[j] + (E_r - 2 C)[j][a][b] in 64-bit words (the true value is below 2^60, so the wrap-around arithmetic is exact)
int vqa_shift_wait(vqa_ctx *c, uint64_t *sse, int64_t n_words)
{
    batch_slot *s;
    if (!c || !sse) return VQA_ERR_INVALID;
    if (n_words != (int64_t)c->slot[KIND_SHIFT].entries) return VQA_ERR_STATE;
    if (int rc = wait_pending(c, KIND_SHIFT, sse, (int)n_words, s)) return rc;
    if (int rc = wait_synced(c)) return rc;
    const size_t grid = (size_t)(2 * c->shift_radius + 1) * (2 * c->shift_radius + 1);
    const unsigned long long *acc = (const unsigned long long *)s->host.p, *ed = acc + (size_t)c->shift_n * grid;
    for (int j = 0; j < c->shift_n; j++)
        for (size_t k = 0; k < grid; k++) sse[j * grid + k] = (uint64_t)(ed[j] + acc[j * grid + k]);
    s->entries = 0;
    return VQA_OK;
}

// ---------------------------------------------------------------------------
// HDR light levels and gamut QC: one stream alone, the three planes of a pixel together, one entry per frame.  A batch of its
// own, ordered by the stream like a dE_ITP batch, whose checks and geometry rules it shares; host frames are staged in qstage_dist.
static int light_submit_body(vqa_ctx *c, const uint8_t *frames, int mem_kind, int n, int64_t fs, const vqa_plane_desc *planes,
                             int n_planes, int model, int full_range, const uint64_t *table, int want_histogram, bool &touched)
{
    if (bad_batch_args(c, frames, frames, mem_kind, n, planes, n_planes) || !table) return VQA_ERR_INVALID;
    if (n_planes != 3 || (model != VQA_ITP_YUV2020 && model != VQA_ITP_BGR)) return VQA_ERR_INVALID;
    if (full_range != 0 && full_range != 1) return VQA_ERR_INVALID;
    if (table[65535] >= VQA_LIGHT_TABLE_LIMIT) return VQA_ERR_INVALID;
    for (int i = 1; i < 65536; i++)
        if (table[i] < table[i - 1]) return VQA_ERR_INVALID;
    batch_slot &s = c->slot[KIND_LIGHT];
    dbuf &tab_dev = s.work[0], &hist_dev = s.work[1];
    plane_batch B;
    int rc = check_batch(s, n, fs, fs, planes, n_planes, B, plane0_limits(planes, LIGHT_MIN_DIM),
                         model == VQA_ITP_BGR ? JOINT_BGR : JOINT_YUV);
    if (rc) return rc;
    if ((rc = stage_batch(c, touched, mem_kind, n, B.span, {&frames, fs, &c->qstage_dist}))) return rc;
    hipStream_t st = c->stream;
    const bool hist = want_histogram != 0;
    const size_t tab_bytes = sizeof(uint64_t) * 65536, frame_hist = sizeof(uint32_t) * LIGHT_BINS;
    const size_t acc_bytes = sizeof(unsigned long long) * LIGHT_WORDS * (size_t)n;
    const int sub_frames = slice_frames(c, n) < LIGHT_SUB_FRAMES ? slice_frames(c, n) : LIGHT_SUB_FRAMES;
    // the table: no light batch is in flight (check_batch) and nothing else reads it, so the copy needs no ordering; it is
    // skipped when the device still holds this very table
    const bool same = tab_dev.p && c->light_table.size() == 65536 && !memcmp(c->light_table.data(), table, tab_bytes);
    if (!same) {
        c->light_table.clear();
        if ((rc = ensure(c, tab_dev, tab_bytes))) return rc;
        HIPCHK(c, hipMemcpy(tab_dev.p, table, tab_bytes, hipMemcpyHostToDevice));
        c->light_table.assign(table, table + 65536);
    }
    if ((rc = ensure(c, s.dev, acc_bytes))) return rc;
    if ((rc = ensure(c, hist_dev, frame_hist * (size_t)sub_frames))) return rc;
    if ((rc = ensure_pinned(c, s.host, acc_bytes + (hist ? frame_hist * (size_t)n : 0)))) return rc;
    HIPCHK(c, hipMemsetAsync(s.dev.p, 0, acc_bytes, st));
    const int depth = B.depth;
    hipError_t err = hipSuccess;
    for_each_slice(c, n, [&](int a0, int m) {
        for (int b0 = 0; b0 < m; b0 += sub_frames) {
            const int k = m - b0 < sub_frames ? m - b0 : sub_frames, at = a0 + b0;
            hipError_t e = hipMemsetAsync(hist_dev.p, 0, frame_hist * (size_t)k, st);
            if (e != hipSuccess) err = e;
            unsigned long long *sacc = (unsigned long long *)s.dev.p + (size_t)at * LIGHT_WORDS;
            {
                prof_scope ps_(c, VQA_K_LIGHT_ACCUM);
                launch_light_accum(st, frames + (int64_t)at * fs, k, fs, planes, depth, model, full_range,
                                   (const unsigned long long *)tab_dev.p, (uint32_t *)hist_dev.p, sacc);
            }
            {
                prof_scope ps_(c, VQA_K_LIGHT_SCAN);
                launch_light_scan(st, k, planes[0].height, planes[0].width, (const uint32_t *)hist_dev.p, sacc);
            }
            if (hist) {   // the sub-slice's histograms leave before the next sub-slice zeroes them (the stream orders the three)
                e = hipMemcpyAsync((uint8_t *)s.host.p + acc_bytes + frame_hist * (size_t)at, hist_dev.p, frame_hist * (size_t)k,
                                   hipMemcpyDeviceToHost, st);
                if (e != hipSuccess) err = e;
            }
        }
    });
    HIPCHK(c, err);
    c->light_hist = hist;
    return finish_batch(c, s, acc_bytes, n, planes, n_planes, depth);
}

int vqa_light_submit(vqa_ctx *c, const uint8_t *frames, int mem_kind, int n, int64_t frame_stride, const vqa_plane_desc *planes,
                     int n_planes, int model, int full_range, const uint64_t *table, int want_histogram)
{
    return submit_and_drain(c, [&](bool &touched) {
        return light_submit_body(c, frames, mem_kind, n, frame_stride, planes, n_planes, model, full_range, table, want_histogram,
                                 touched);
    });
}

int vqa_light_wait(vqa_ctx *c, vqa_light_metrics *out, int n_entries, uint32_t *hist)
{
    batch_slot *s;
    if (int rc = wait_pending(c, KIND_LIGHT, out, n_entries, s)) return rc;
    if (hist && !c->light_hist) return VQA_ERR_INVALID;   // (the batch stays pending)
    if (int rc = wait_synced(c)) return rc;
    const unsigned long long *acc = (const unsigned long long *)s->host.p;
    for (int e = 0; e < n_entries; e++)
        light_finalize(acc + (size_t)e * LIGHT_WORDS, s->h[0], s->w[0], c->light_table.data(), out + e);
    if (hist) memcpy(hist, acc + (size_t)n_entries * LIGHT_WORDS, sizeof(uint32_t) * LIGHT_BINS * (size_t)n_entries);
    s->entries = 0;
    return VQA_OK;
}

int vqa_light_table(int transfer, uint64_t *table)
{
    if (!table) return VQA_ERR_INVALID;
    if (transfer == VQA_ITP_HLG) return VQA_ERR_UNSUPPORTED;   // HLG's display light is not a per-channel function
    if (transfer != VQA_ITP_PQ) return VQA_ERR_INVALID;
    light_table_host(table);
    return VQA_OK;
}

int vqa_light_gamut(int gamut, int64_t m[9])
{
    if (!m) return VQA_ERR_INVALID;
    return light_gamut_host(gamut, m) ? VQA_OK : VQA_ERR_INVALID;
}

// ---------------------------------------------------------------------------
// Colour registration: both streams, the planes of a pixel together, one entry per frame and ONE set of tables per submit.  A
// batch of its own, ordered by the stream like a CIEDE2000 batch, whose checks, geometry rules and host staging (qstage_*) it
// shares.  No kernel id: the kernel carries no prof_scope.
static int colorfit_submit_body(vqa_ctx *c, const uint8_t *ref, const uint8_t *dist, int mem_kind, int n, int64_t ref_fs,
                                int64_t dist_fs, const vqa_plane_desc *planes, int n_planes, int want_tables, bool &touched)
{
    if (bad_batch_args(c, ref, dist, mem_kind, n, planes, n_planes)) return VQA_ERR_INVALID;
    if ((n_planes != 1 && n_planes != 3) || (want_tables != 0 && want_tables != 1)) return VQA_ERR_INVALID;
    batch_slot &s = c->slot[KIND_COLORFIT];
    plane_batch B;
    int rc = check_batch(s, n, ref_fs, dist_fs, planes, n_planes, B, plane0_limits(planes, COLORFIT_MIN_DIM),
                         n_planes == 3 ? JOINT_YUV : JOINT_NONE);
    if (rc) return rc;
    if (n > VQA_COLORFIT_MAX_FRAMES) return VQA_ERR_UNSUPPORTED;
    // (n h w <= 2^31 keeps a table's sum_dd below 2^63; no byte has been read so far)
    if (want_tables && (int64_t)n * planes[0].width * planes[0].height > VQA_COLORFIT_TABLE_POSITIONS) return VQA_ERR_UNSUPPORTED;
    if ((rc = stage_pair(c, touched, mem_kind, n, B.span, ref, ref_fs, dist, dist_fs))) return rc;
    const int depth = B.depth;
    const size_t acc_words = (size_t)COLORFIT_WORDS * (size_t)n;
    const size_t tab_words = want_tables ? (size_t)n_planes * colorfit_bins(depth) * 3 : 0;
    const size_t bytes = sizeof(unsigned long long) * (acc_words + tab_words);
    if ((rc = ensure(c, s.dev, bytes))) return rc;
    if ((rc = ensure_pinned(c, s.host, bytes))) return rc;
    HIPCHK(c, hipMemsetAsync(s.dev.p, 0, bytes, c->stream));
    unsigned long long *acc = (unsigned long long *)s.dev.p;
    launch_colorfit(c->stream, ref, dist, n, ref_fs, dist_fs, planes, n_planes, depth, acc, want_tables ? acc + acc_words : nullptr);
    c->colorfit_table_words = (int64_t)tab_words;
    return finish_batch(c, s, bytes, n, planes, n_planes, depth);
}

int vqa_colorfit_submit(vqa_ctx *c, const uint8_t *ref, const uint8_t *dist, int mem_kind, int n, int64_t ref_fs, int64_t dist_fs,
                        const vqa_plane_desc *planes, int n_planes, int want_tables)
{
    return submit_and_drain(c, [&](bool &touched) {
        return colorfit_submit_body(c, ref, dist, mem_kind, n, ref_fs, dist_fs, planes, n_planes, want_tables, touched);
    });
}

int vqa_colorfit_wait(vqa_ctx *c, vqa_colorfit_metrics *out, int n_entries, uint64_t *tables, int64_t n_table_words)
{
    batch_slot *s;
    if (int rc = wait_pending(c, KIND_COLORFIT, out, n_entries, s)) return rc;
    // (either refusal leaves the batch pending)
    if (tables && !c->colorfit_table_words) return VQA_ERR_INVALID;
    if (tables && n_table_words != c->colorfit_table_words) return VQA_ERR_STATE;
    if (int rc = wait_synced(c)) return rc;
    const unsigned long long *acc = (const unsigned long long *)s->host.p;
    for (int e = 0; e < n_entries; e++) colorfit_finalize(acc + (size_t)e * COLORFIT_WORDS, s->h[0], s->w[0], s->planes, out + e);
    if (tables) memcpy(tables, acc + (size_t)n_entries * COLORFIT_WORDS, sizeof(uint64_t) * (size_t)n_table_words);
    s->entries = 0;
    return VQA_OK;
}

// ---------------------------------------------------------------------------
// Clip-wide sync, first half: the signature of one plane of every frame of one stream.  A batch of its own, ordered by the
// stream like a CAMBI batch, whose host staging (qstage_dist) it shares.
static int sig_submit_body(vqa_ctx *c, const uint8_t *frames, int mem_kind, int n, int64_t fs, const vqa_plane_desc *plane,
                           bool &touched)
{
    if (bad_batch_args(c, frames, frames, mem_kind, n, plane, 1)) return VQA_ERR_INVALID;
    if (n > VQA_SIG_MAX_BATCH) return VQA_ERR_UNSUPPORTED;
    batch_slot &s = c->slot[KIND_SIG];
    plane_batch B;
    int rc = check_batch(s, n, fs, fs, plane, 1, B, [](const vqa_plane_desc &d) { return side_and_area_limits(d, VQA_SIG_GRID); });
    if (rc) return rc;
    if ((rc = stage_batch(c, touched, mem_kind, n, B.span, {&frames, fs, &c->qstage_dist}))) return rc;
    const size_t bytes = (size_t)VQA_SIG_BYTES * n;
    if ((rc = ensure(c, s.dev, bytes))) return rc;
    if ((rc = ensure_pinned(c, s.host, bytes))) return rc;
    {
        prof_scope ps_(c, VQA_K_SIG);
        launch_sig(c->stream, frames, n, fs, plane[0], B.depth, (uint8_t *)s.dev.p);
    }
    return finish_batch(c, s, bytes, n, plane, 1, B.depth);
}

int vqa_sig_submit(vqa_ctx *c, const uint8_t *frames, int mem_kind, int n, int64_t frame_stride, const vqa_plane_desc *plane)
{
    return submit_and_drain(c, [&](bool &touched) { return sig_submit_body(c, frames, mem_kind, n, frame_stride, plane, touched); });
}

int vqa_sig_wait(vqa_ctx *c, uint8_t *sig, int n)
{
    batch_slot *s;
    if (int rc = wait_pending(c, KIND_SIG, sig, n, s)) return rc;
    if (int rc = wait_synced(c)) return rc;
    memcpy(sig, s->host.p, (size_t)VQA_SIG_BYTES * n);
    s->entries = 0;
    return VQA_OK;
}

// Clip-wide sync, second half: every distorted signature against every reference signature.  A batch of its own; the two host
// arrays are staged in the slot's own work buffers (they are no frames, and nothing else reads them).
static int sig_cross_submit_body(vqa_ctx *c, const uint8_t *dist_sig, int n_dist, const uint8_t *ref_sig, int n_ref, bool &touched)
{
    if (!c || !dist_sig || !ref_sig || n_dist < 1 || n_ref < 1) return VQA_ERR_INVALID;
    if (n_dist > VQA_SIG_MAX_FRAMES || n_ref > VQA_SIG_MAX_FRAMES) return VQA_ERR_UNSUPPORTED;
    batch_slot &s = c->slot[KIND_SIGX];
    if (s.entries) return VQA_ERR_STATE;
    HIPCHK(c, hipSetDevice(c->device));
    touched = true;
    int rc;
    if ((rc = stage(c, s.work[0], dist_sig, (size_t)VQA_SIG_BYTES * n_dist))) return rc;
    if ((rc = stage(c, s.work[1], ref_sig, (size_t)VQA_SIG_BYTES * n_ref))) return rc;
    const size_t n_diag = (size_t)n_dist + n_ref - 1, bytes = sizeof(unsigned long long) * (n_diag + n_dist);
    if ((rc = ensure(c, s.dev, bytes))) return rc;
    if ((rc = ensure_pinned(c, s.host, bytes))) return rc;
    hipStream_t st = c->stream;
    unsigned long long *diag = (unsigned long long *)s.dev.p;
    HIPCHK(c, hipMemsetAsync(diag, 0, sizeof(unsigned long long) * n_diag, st));
    {
        prof_scope ps_(c, VQA_K_SIG_DIAG);
        launch_sig_diag(st, dist_sig, n_dist, ref_sig, n_ref, diag);
    }
    {
        prof_scope ps_(c, VQA_K_SIG_BEST);
        launch_sig_best(st, dist_sig, n_dist, ref_sig, n_ref, diag + n_diag);
    }
    c->sigx_n_dist = n_dist; c->sigx_n_ref = n_ref;
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(s.host.p, s.dev.p, bytes, hipMemcpyDeviceToHost, st));
    s.entries = n_dist;
    s.planes = 0;
    return VQA_OK;
}

int vqa_sig_cross_submit(vqa_ctx *c, const uint8_t *dist_sig, int n_dist, const uint8_t *ref_sig, int n_ref)
{
    return submit_and_drain(c, [&](bool &touched) { return sig_cross_submit_body(c, dist_sig, n_dist, ref_sig, n_ref, touched); });
}

int vqa_sig_cross_wait(vqa_ctx *c, uint64_t *diag, int64_t n_diag, uint64_t *best, int64_t n_best)
{
    if (!c || !diag || !best) return VQA_ERR_INVALID;
    batch_slot *s = &c->slot[KIND_SIGX];
    if (!s->entries || n_best != c->sigx_n_dist || n_diag != (int64_t)c->sigx_n_dist + c->sigx_n_ref - 1) return VQA_ERR_STATE;
    if (int rc = wait_synced(c)) return rc;
    const unsigned long long *words = (const unsigned long long *)s->host.p;
    memcpy(diag, words, sizeof(uint64_t) * (size_t)n_diag);
    memcpy(best, words + n_diag, sizeof(uint64_t) * (size_t)n_best);
    s->entries = 0;
    return VQA_OK;
}

// ---------------------------------------------------------------------------
int vqa_profile_enable(vqa_ctx *c, int on)
{
    if (!c) return VQA_ERR_INVALID;
    c->prof_on = on != 0;
    return VQA_OK;
}

// The kernel ids, written once: a row per id that exists, ascending, a line per feature.  vqa_kernel_name and vqa_profile_read
// know exactly these rows; every other id below VQA_K_EAVE is a gap and stays unknown.  A new kernel takes the next id after the
// last and adds its row here and in _native.py's K_TABLE ("Kernel ids").
namespace {
struct kernel_row { int id; const char *name; };
constexpr kernel_row KERNELS[] = {
    {VQA_K_GRAY_HIST, "k_bgr2gray_hist"}, {VQA_K_RESIZE, "k_resize_planes"}, {VQA_K_DCT8, "k_dct8"}, {VQA_K_DCT_FULL, "k_dct_full"},
    {VQA_K_CANNY_NMS, "k_canny_nms"}, {VQA_K_CANNY_HYST, "k_canny_hyst"}, {VQA_K_SAD, "k_block_sad"},
    {VQA_K_SSIM_GAUSS, "k_ssim_gauss"}, {VQA_K_SSIM_FFMPEG, "k_ssim_ffmpeg"}, {VQA_K_ORB, "k_orb64"},
    {VQA_K_FARNEBACK, "farneback(pyramid)"}, {VQA_K_MS_PYRAMID, "k_ms_pyramid"},
    {VQA_K_VIF, "k_vif_stats"}, {VQA_K_VIF_DECIMATE, "k_vif_decimate"},
    {VQA_K_ADM, "k_adm_scale"}, {VQA_K_ADM_REDUCE, "k_adm_reduce"},
    {VQA_K_MOTION, "k_motion_sad"},
    {VQA_K_SITI, "k_siti"},
    {VQA_K_PSNR_HVS, "k_psnr_hvs"},
    {VQA_K_CIEDE, "k_ciede"},
    {VQA_K_GMSD, "k_gmsd"},
    {VQA_K_CAMBI_MASK, "k_cambi_mask"}, {VQA_K_CAMBI_DECIMATE, "k_cambi_decimate"}, {VQA_K_CAMBI_CONTRAST, "k_cambi_contrast"},
    {VQA_K_CAMBI_TOPK, "k_cambi_topk"},
    {VQA_K_XPSNR_ACT, "k_xpsnr_act"}, {VQA_K_XPSNR_SSE, "k_xpsnr_sse"},
    {VQA_K_HAARPSI, "k_haarpsi"},
    {VQA_K_VCA_BLOCKS, "k_vca_blocks"}, {VQA_K_VCA_SUM, "k_vca_sum"},
    {VQA_K_ARTIFACTS, "k_artifacts"},
    {VQA_K_BRISQUE_HALF, "k_brisque_half"}, {VQA_K_BRISQUE_MSCN, "k_brisque_mscn"}, {VQA_K_BRISQUE_SEAM, "k_brisque_seam"},
    {VQA_K_MDSI_MAP, "k_mdsi_map"}, {VQA_K_MDSI_DEV, "k_mdsi_dev"},
    {VQA_K_ITP, "k_itp"},
    {VQA_K_PU21_ENCODE, "k_pu21_encode"}, {VQA_K_PU21_SSIM, "k_pu21_ssim"},
    {VQA_K_FSIM_LUMA, "k_fsim_luma"}, {VQA_K_FSIM_DFT, "k_fsim_dft"}, {VQA_K_FSIM_ENERGY, "k_fsim_energy"},
    {VQA_K_FSIM_MEDIAN, "k_fsim_median"}, {VQA_K_FSIM_PC, "k_fsim_pc"}, {VQA_K_FSIM_POOL, "k_fsim_pool"},
    {VQA_K_SIGSTATS_ACCUM, "k_sigstats_accum"}, {VQA_K_SIGSTATS_SCAN, "k_sigstats_scan"},
    {VQA_K_SCALE, "k_scale"},
    {VQA_K_ALIGN_CROSS, "k_align_cross"},
    {VQA_K_SHIFT, "k_shift"},
    {VQA_K_LIGHT_ACCUM, "k_light_accum"}, {VQA_K_LIGHT_SCAN, "k_light_scan"},
    {VQA_K_SIG, "k_sig"}, {VQA_K_SIG_DIAG, "k_sig_diag"}, {VQA_K_SIG_BEST, "k_sig_best"},
};
constexpr int N_KERNELS = sizeof(KERNELS) / sizeof(KERNELS[0]);

constexpr bool kernels_ascending()
{
    for (int i = 1; i < N_KERNELS; i++)
        if (KERNELS[i - 1].id >= KERNELS[i].id) return false;
    return KERNELS[0].id >= 0;
}
static_assert(kernels_ascending(), "KERNELS: the rows are in strictly ascending id order");
static_assert(KERNELS[N_KERNELS - 1].id == VQA_K_EAVE - 1, "KERNELS: the last row is the last id, and VQA_K_EAVE sizes prof_ms / prof_n");
static_assert(N_KERNELS == 55, "KERNELS: a kernel id was added or removed without its row");

// id -> name, null for a gap
struct kernel_names { const char *of[VQA_K_EAVE]; };
constexpr kernel_names kernel_names_by_id()
{
    kernel_names t{};
    for (const kernel_row &r : KERNELS) t.of[r.id] = r.name;
    return t;
}
constexpr kernel_names KERNEL_NAME = kernel_names_by_id();
} // namespace

int vqa_profile_read(vqa_ctx *c, int id, double *total_ms, int64_t *launches, int reset)
{
    if (!c || id < 0 || id >= VQA_K_EAVE || !KERNEL_NAME.of[id]) return VQA_ERR_INVALID;
    if (!busy(c)) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        prof_collect(c);
    }
    if (total_ms) *total_ms = c->prof_ms[id];
    if (launches) *launches = c->prof_n[id];
    if (reset) { c->prof_ms[id] = 0; c->prof_n[id] = 0; }
    return VQA_OK;
}

const char *vqa_kernel_name(int id)
{
    const char *name = (id >= 0 && id < VQA_K_EAVE) ? KERNEL_NAME.of[id] : nullptr;
    return name ? name : "?";
}

// ---------------------------------------------------------------------------
int vqa_debug_read_plane(vqa_ctx *c, int which, int frame, uint8_t *dst, int dst_h, int dst_w)
{
    if (!c || !dst || frame < 0 || frame >= c->last_n) return VQA_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    const uint8_t *src = nullptr;
    int h = 0, w = 0, pitch = 0;
    if (which == 3) {
        if (!c->last_has_full) return VQA_ERR_STATE;
        h = c->last_h; w = c->last_w; pitch = c->last_gp;
        src = (const uint8_t *)c->gray_full.p + (int64_t)(frame + 1) * h * pitch;
    } else if (which == 0 || which == 1) {
        h = c->last_ph; w = c->last_pw; pitch = c->last_pp;
        if (c->last_resized) {
            if (!c->last_has_planes) return VQA_ERR_STATE;
            src = which == 0 ? (const uint8_t *)c->planeA.p + (int64_t)(frame + 1) * h * pitch
                             : (const uint8_t *)c->planeB.p + (int64_t)frame * h * pitch;
        } else {
            if (!c->last_has_full) return VQA_ERR_STATE;
            src = (const uint8_t *)c->gray_full.p + (int64_t)(frame + 1) * h * pitch;
        }
    } else if (which == 2) {
        if (!c->last_has_state) return VQA_ERR_STATE;
        h = c->last_ph; w = c->last_pw;
        if (dst_h != h || dst_w != w) return VQA_ERR_INVALID;
        const int ww = (w + 63) / 64, ty_n = (h + 63) / 64;
        std::vector<uint64_t> bits((size_t)ty_n * ww * 64);
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipMemcpy(bits.data(), (const uint64_t *)c->state.p + (size_t)frame * bits.size(),
                            sizeof(uint64_t) * bits.size(), hipMemcpyDeviceToHost));
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) {
                // the planes hold the transposed frame, one word per column and 64 rows: unpacked into the row-major map
                const uint64_t wd = bits[(size_t)canny_plane_word(h, w, y, x)];
                dst[(size_t)y * w + x] = ((wd >> (y & 63)) & 1ull) ? 255 : 0;
            }
        return VQA_OK;
    } else {
        return VQA_ERR_INVALID;
    }
    if (dst_h != h || dst_w != w) return VQA_ERR_INVALID;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy2D(dst, (size_t)w, src, (size_t)pitch, (size_t)w, (size_t)h, hipMemcpyDeviceToHost));
    return VQA_OK;
}

int vqa_debug_read_farneback(vqa_ctx *c, int which, int index, int level, float *dst, int dst_h, int dst_w)
{
    if (!c || !dst || (which != 0 && which != 1)) return VQA_ERR_INVALID;
    const auto &F = c->last_fb;
    if (!F.valid) return VQA_ERR_STATE;
    if (level < 0 || level > F.levels || (which == 0 && level != 0)) return VQA_ERR_INVALID;
    if (dst_h != F.lh[level] || dst_w != F.lw[level]) return VQA_ERR_INVALID;
    // pairs first_pair .. first_pair + pairs - 1 and their planes first_pair .. first_pair + pairs are resident
    const int local = index - F.first_pair;
    if (local < 0 || local >= F.pairs + which) return VQA_ERR_INVALID;
    if (index == 0 && !F.first_valid) return VQA_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = sync_all(c)) return rc; // the piped mode's expansions are written on the side stream
    const size_t L = (size_t)F.lh[level] * F.lw[level];
    if (which == 0) {
        const float *flow = (const float *)(F.flow_buf ? c->fb_flow1.p : c->fb_flow0.p);
        HIPCHK(c, hipMemcpy(dst, flow + (size_t)local * L * 2, sizeof(float) * L * 2, hipMemcpyDeviceToHost));
    } else {
        const float *R = (const float *)c->fb_R.p + F.Roff[level];
        HIPCHK(c, hipMemcpy(dst, R + (size_t)local * L * 5, sizeof(float) * L * 5, hipMemcpyDeviceToHost));
    }
    return VQA_OK;
}

} // extern "C"
