"""CPU: the probe matrix of tests/probe_cases.py is sound before a GPU sees it.

  the geometry     the planes cross the seams probe_cases says they cross (the launch arithmetic of csrc/k_quality.hip restated)
  the reference    probe_reference's maps are the references' own numbers; D does not depend on the crop
  stability        r = max_k |D_32(k) - D_64(k)| / |D_64(k)| per (kind, level, content, depth); the GPU's bar is 4 r, floored at 1e-5
  the cap          no bar above 1e-3; what would push one past it is excluded by name, at most 1 in 16 (probe, level) items of a
                   kind, and no seam loses all of its probes
  teeth            eight mutations of the float64 reference, each at one seam: a probe beside the seam moves by more than twice
                   its group's bar while the plane mean of an ordinary pair moves by less than 1e-4 - what the suite's bars
                   could not see
  ADM and motion   the same on their planes (ADM: "adm" is plane A, "adm-b" plane B): the seams from the kernels' constants, the
                   scales a patch reaches, the unsure items of the angle test and their intervals, motion's linearity, and eight
                   more mutations, each at 10 bars or more on a probe
"""
import contextlib

import numpy as np
import pytest

import adm_reference as A
import hbd_reference as R
import layout_cases as LC
import motion_reference as MO
import msssim_reference as M
import probe_cases as PC
import probe_reference as PR
import vif_reference as V

MEAN_BAR = 1e-4     # the suite's bar on a plane mean (tests/test_gpu_parity.py's RTOL, tests/test_gpu_vif.py's BAR)
ADM_BAR = 1e-4               # tests/test_gpu_adm.py's bar on a scale, absolute
MOTION_BAR = 26 * 2.0 ** -17 # tests/test_gpu_motion.py's bar on the plane mean, absolute
KINDS = ("gauss", "ffmpeg", "vif", "ms-cs", "ms-ssim", "adm", "adm-b", "motion")
GROUPS = [(k, n, d) for k in KINDS for n in PC.CONTENTS for d in PC.DEPTHS[PR.base_kind(k)]]


def _levels(kind):
    return {"vif": PC.VIF_LEVELS, "ms-cs": PC.MS_LEVELS, "ms-ssim": PC.MS_LEVELS, "adm": PC.ADM_LEVELS, "adm-b": PC.ADM_LEVELS}.get(kind, 1)


# ---- the geometry ----------------------------------------------------------------------------------------------------------------
def _gauss_geometry(h, w, groups_per_strip_row):
    """csrc/k_quality.hip: 246 map columns per workgroup; ssim_strips() and ssim_strip_rows() -> (column blocks, strips, rows)"""
    ncb = (w - 10 + 245) // 246
    cap = max((h - 10) // 64, 1)
    ns = max((h - 10 + 1099) // 1100, min(-(-6144 // (groups_per_strip_row * ncb)), 4096))
    ns = min(ns, cap)
    return ncb, ns, (-(-(h - 10) // ns) + 23) // 24 * 24


def test_the_planes_cross_the_seams_the_probes_are_placed_at():
    h, w = PC.PLANE
    n = 1 + len(PC.probes("gauss"))
    assert _gauss_geometry(h, w, n) == (2, 2, 72)                      # seams at map column 246 and map row 72
    assert _gauss_geometry(h, w, 3072) == (2, 1, 144)                  # 3072 * 1 * 2 = 6144 workgroups: one long strip per plane
    assert _gauss_geometry(h, w, 3071)[1] == 2
    bw, bh = w >> 2, h >> 2
    assert ((bw - 1 + 62) // 63, (bh - 1 + 31) // 32) == (2, 2) and bw - 1 == 65 and bh - 1 == 34      # vf_ssim: waves, strips
    for s, (lh, lw) in enumerate(V.level_dims(h, w)):                  # VIF: 64 x 16 tiles on every level
        assert lh > 128 >> s and (128 >> s) % 16 == 0, s
        assert (lw > 256 >> s and (256 >> s) % 64 == 0) if s < 3 else (lw, 256 >> s) == (33, 32), s
    mh, mw = PC.MS_PLANE
    nm = 1 + len(PC.probes("ms"))
    dims = [(mh >> s, mw >> s) for s in range(5)]
    assert all(d[0] % 2 == 0 and d[1] % 2 == 0 for d in dims[:4]) and dims[4] == (22, 33)
    assert [_gauss_geometry(lh, lw, nm) for lh, lw in dims] == [(3, 5, 72), (2, 2, 96), (1, 1, 96), (1, 1, 48), (1, 1, 24)]
    # every probe lies in its plane and its patch never clips a sample
    for kind in ("gauss", "ffmpeg", "vif", "ms"):
        ph, pw = PC.plane_of(kind)
        for name in PC.CONTENTS:
            for depth in PC.DEPTHS[kind]:
                a = PC.ref_plane(kind, name, depth)
                assert a.shape == (ph, pw) and a.min() >= 0 and a.max() <= (1 << depth) - 1
        for p in PC.probes(kind):
            y0, y1, x0, x1 = PC.patch_box(p, (ph, pw), PC.patch_size(kind))
            assert 0 <= y0 < y1 <= ph and 0 <= x0 < x1 <= pw, (kind, p)


def test_every_vf_ssim_kernel_is_reached_by_its_descriptor():
    h, w = PC.PLANE
    for (lay, depth), want in PC.FFMPEG_PATHS.items():
        planes, probed, size = PC.layout(lay, h, w, depth)
        fs = size * (2 if depth > 8 else 1)
        assert fs % 8 == 0
        got = LC.ffmpeg_kernels(0, 0, fs, fs, planes, depth)
        assert got[probed] == want and set(got) == {want}, (lay, depth, got)
    assert set(PC.FFMPEG_PATHS.values()) == {"fast<1>", "fast<3>", "ffmpeg", "ffmpeg16<true>", "ffmpeg16<false>"}


def test_a_batch_is_frame_zero_plus_one_patch_per_frame():
    for kind, lay, depth in (("gauss", "bgr24", 8), ("gauss", "yuv420-u", 10), ("ffmpeg", "gray-off1", 8), ("ffmpeg", "gray-off2", 10)):
        ref, dist, planes, probed = PC.batch(kind, "smooth", depth, lay)
        pr = PC.probes(kind)
        assert ref.shape == dist.shape and ref.shape[0] == 1 + len(pr) and (ref == ref[0]).all() and (dist[0] == ref[0]).all()
        a = R.plane(ref[0], planes[probed])
        assert np.array_equal(a, PC.ref_plane(kind, "smooth", depth))
        for k in (1, 37, len(pr)):
            for i, p in enumerate(planes):
                d = R.plane(dist[k], p)
                if i != probed:
                    assert np.array_equal(d, R.plane(ref[0], p))
                else:
                    assert R.sse(a, d) == PC.sse_of(pr[k - 1], a.shape, depth)
                    y0, y1, x0, x1 = PC.patch_box(pr[k - 1], a.shape)
                    m = np.zeros(a.shape, bool)
                    m[y0:y1, x0:x1] = True
                    assert (np.abs(a - d) == np.where(m, 64 << (depth - 8), 0)).all()


# ---- the reference side is the references' own ---------------------------------------------------------------------------------
def test_the_maps_are_the_references_own_numbers():
    a = PC.ref_plane("gauss", "smooth", 10)
    d = PC.dist_plane("gauss", "smooth", 10, (72, 246))
    for dt in (np.float64, np.float32):
        cs, S = PR.gauss_maps(a.astype(np.float64), d.astype(np.float64), 1023, dt)
        assert S.mean() == R.ssim_gauss(a, d, 1023, dt)
    cs, S = PR.gauss_maps(a.astype(np.float64), d.astype(np.float64), 1023)
    c, s = M.window_means(a.astype(np.float64), d.astype(np.float64), 1023)
    assert abs(cs.mean() - c) <= 1e-14 and abs(S.mean() - s) <= 1e-14
    assert PR.ffmpeg_map(a, d, 10).sum() / PR.map_samples("ffmpeg") == R.ssim_ffmpeg(a, d, 1023)
    a8, d8 = PC.ref_plane("ffmpeg", "noise", 8), PC.dist_plane("ffmpeg", "noise", 8, (128, 256))
    assert abs(PR.ffmpeg_map(a8, d8, 8).mean() - R.ssim_ffmpeg(a8, d8, 255)) <= 1e-6      # (416 against 416.16: DESIGN.md section 3)
    av, dv = PC.ref_plane("vif", "smooth", 10), PC.dist_plane("vif", "smooth", 10, (128, 256))
    for dt in (np.float64, np.float32):
        num, den, _scale, _vif = V.vif(av, dv, 10, dt)
        maps = PR.vif_maps(av, dv, 10, dt)
        assert [float(m[0].sum(dtype=np.float64)) for m in maps] == list(num) and [float(m[1].sum(dtype=np.float64)) for m in maps] == list(den)


def test_d_is_the_sum_over_the_touched_windows():
    """the crop gives what the whole plane gives, and both are N times the difference of the two plane means"""
    for name in PC.CONTENTS:
        a = PC.ref_plane("gauss", name, 8)
        pr = PC.probes("gauss")
        for k in (0, 9, 35, 44, 89):
            d = PC.dist_plane("gauss", name, 8, pr[k])
            x, y = a.astype(np.float64), d.astype(np.float64)
            for dt in (np.float64, np.float32):
                crop, whole = PR.gauss_level_D(x, y, 255, dt), PR.gauss_level_D(x, y, 255, dt, crop=False)
                assert np.allclose(crop, whole, rtol=1e-10, atol=0), (name, pr[k], crop, whole)
            n = PR.map_samples("gauss")
            means = n * (R.ssim_gauss(a, a, 255) - R.ssim_gauss(a, d, 255))
            assert abs(means - PR.D64("gauss", name, 8)[k, 0]) <= 1e-9 * abs(means), (name, pr[k])
    a = PC.ref_plane("ms", "noise", 8)
    pr = PC.probes("ms")
    k = len(pr) - 13                                           # a tier-4 probe in the middle of the plane
    cs0, s0, _ = M.msssim(a, a, 255)
    cs1, s1, _ = M.msssim(a, PC.dist_plane("ms", "noise", 8, pr[k]), 255)
    for lv in range(5):
        n = PR.map_samples("ms", lv)
        assert abs(n * (cs0[lv] - cs1[lv]) - PR.D64("ms-cs", "noise", 8)[k, lv]) <= 1e-9 * n
        assert abs(n * (s0[lv] - s1[lv]) - PR.D64("ms-ssim", "noise", 8)[k, lv]) <= 1e-9 * n


# ---- stability, the cap, the exclusions ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,name,depth", GROUPS, ids=["%s-%s-%d" % g for g in GROUPS])
def test_the_reference_alone_is_stable_and_the_bar_is_inside_the_cap(kind, name, depth):
    r, d64 = PR.ratios(kind, name, depth), PR.D64(kind, name, depth)
    pr = PC.probes(PR.base_kind(kind))
    for lv in range(_levels(kind)):
        keep = PR.kept(kind, lv)
        k = keep[int(np.argmax(r[keep, lv]))]
        bar = PR.bar(kind, lv, name, depth)
        print("%s %s %d bits level %d: r %.2e at %s (D_64 %.3e), bar %.2e, %d probes, |D_64| %.2e .. %.2e" % (
            kind, name, depth, lv, r[k, lv], pr[k], d64[k, lv], bar, len(keep), np.abs(d64[keep, lv]).min(), np.abs(d64[keep, lv]).max()))
        assert np.isfinite(r[keep, lv]).all() and (np.abs(d64[keep, lv]) > 0).all()
        assert PC.FLOOR <= bar <= PC.CAP, (kind, name, depth, lv, bar, pr[k])


def test_the_exclusions_are_few_named_and_leave_every_seam_probed():
    for kind in ("gauss", "ffmpeg", "vif", "ms"):
        pr = PC.probes(kind)
        items = [(lv, p) for p in pr for lv in PC.levels_of(kind, p)]
        ex = PC.EXCLUDED[kind]
        assert all(key in items and isinstance(reason, str) and reason for key, reason in ex.items()), kind
        assert len(ex) <= PC.MAX_EXCLUDED_SHARE * len(items), (kind, len(ex), len(items))
        if kind == "ms":       # every tier keeps all of its probes
            assert not ex
            continue
        for lv in range(_levels(kind)):
            for seam, (axis, at) in PC.SEAMS[kind].items():
                left = [p for p in pr if p[0 if axis == "row" else 1] in at and not PC.excluded(kind, lv, p)]
                assert left, (kind, lv, seam)
    for (kind, lv, name, depth), margin in PC.MARGIN_OF.items():     # a wider margin names a group that exists and stays inside the cap
        assert (kind, name, depth) in GROUPS and lv < _levels(kind) and margin > PC.MARGIN
        assert margin * PR.group_ratio(kind, lv, name, depth) <= PC.CAP / 10
    # an exclusion is needed: the excluded item's own ratio, times the margin, is beyond what the kept ones give the group
    worst = np.max([PR.ratios("vif", n, d) for n in PC.CONTENTS for d in PC.DEPTHS["vif"]], axis=0)
    pr = PC.probes("vif")
    for lv, p in PC.EXCLUDED["vif"]:
        kept_worst = worst[PR.kept("vif", lv), lv].max()
        print("excluded VIF level %d probe %s: ratio %.2e (the worst kept one: %.2e)" % (lv, p, worst[pr.index(p), lv], kept_worst))
        assert worst[pr.index(p), lv] > kept_worst


# ---- teeth ---------------------------------------------------------------------------------------------------------------------------
def _ordinary(a, depth):
    """an ordinary distorted pair of the plane, the kind the parity tests feed: one level of noise on every sample (hostile_cases'
    distortion).  Its plane mean is what the suite's 1e-4 judges; the mutation moves it by 3.3e-5 at the most.  Two things were
    measured and are not asserted: with three levels of noise the smooth field's SSIM falls to 0.75 and vf_ssim's column mutation and
    VIF's clamp move the mean by 1.9e-4 and 2.1e-4, just visible; and the probe's own frame, whose distortion is the patch alone and
    sits on the seam, moves its mean by up to 1.3e-3 (printed below) - a mean sees a seam only when the test's content is on it"""
    rng = np.random.default_rng(5)
    return np.clip(a + rng.integers(-1, 2, a.shape) * (1 << (depth - 8)), 0, (1 << depth) - 1)


def _filt_without_the_last_tap(x):
    g = R._gauss11(x.dtype)
    h, w = x.shape
    v = sum(g[k] * x[k:k + h - 10, :] for k in range(11))
    return sum(g[k] * v[:, k:k + w - 10] for k in range(10))


def _gauss_mutations(L):
    def last_tap(a, b, maps):
        bad = PR.gauss_maps(a, b, L, filt=_filt_without_the_last_tap)
        out = [m.copy() for m in maps]
        for o, m in zip(out, bad):
            o[:, 246] = m[:, 246]
        return out

    def moved(src, dst, axis):
        def f(a, b, maps):
            out = [m.copy() for m in maps]
            for o in out:
                if axis == 0:
                    o[dst] = o[src]
                else:
                    o[:, dst] = o[:, src]
            return out
        return f
    cols, rows = (240, 246, 251), (66, 72, 77, 83)
    return [("map column 246 loses its last tap", last_tap, 1, cols), ("map column 246 reads one column to the right", moved(247, 246, 1), 1, cols),
            ("map row 72 repeats row 71", moved(71, 72, 0), 0, rows), ("map column 245 repeats column 244", moved(244, 245, 1), 1, cols)]


def _beside(kind, axis, at):
    return [k for k, p in enumerate(PC.probes(kind)) if p[axis] in at]


@pytest.mark.parametrize("name", PC.CONTENTS)
def test_teeth_gaussian_ssim(name):
    depth, L = 8, 255
    a = PC.ref_plane("gauss", name, depth).astype(np.float64)
    bar = PR.bar("gauss", 0, name, depth)
    d64 = PR.D64("gauss", name, depth)[:, 0]
    o = _ordinary(a.astype(np.int64), depth).astype(np.float64)
    plain = PR.gauss_maps(a, o, L)
    for what, mutate, axis, at in _gauss_mutations(L):
        moves = []
        for k in _beside("gauss", axis, at):
            d = PC.dist_plane("gauss", name, depth, PC.probes("gauss")[k]).astype(np.float64)
            got = PR.gauss_level_D(a, d, L, crop=False, mutate=mutate)[1]
            moves.append(abs(got - d64[k]) / abs(d64[k]))
        best = PC.dist_plane("gauss", name, depth, PC.probes("gauss")[_beside("gauss", axis, at)[int(np.argmax(moves))]]).astype(np.float64)
        own = PR.gauss_maps(a, best, L)
        own_move = abs(mutate(a, best, own)[1].mean() - own[1].mean()) / own[1].mean()
        mean_move = abs(mutate(a, o, plain)[1].mean() - plain[1].mean()) / plain[1].mean()
        print("gauss %s, %s: a probe moves by %.2e (bar %.2e), its plane mean by %.2e, the mean of an ordinary pair by %.2e" % (
            name, what, max(moves), bar, own_move, mean_move))
        assert max(moves) > 2 * bar, (what, moves, bar)
        assert mean_move < MEAN_BAR, (what, mean_move)


def _ffmpeg_mutations(depth):
    def wrong_block_column(a, b, m):
        a2, b2 = a.copy(), b.copy()
        a2[:, 256:260], b2[:, 256:260] = a[:, 252:256], b[:, 252:256]      # lane 63 has no right-hand lane: its own block column twice
        out = m.copy()
        out[:, 63] = PR.ffmpeg_map(a2, b2, depth)[:, 63]
        return out

    def repeated_row(a, b, m):
        out = m.copy()
        out[32] = out[31]
        return out
    return [("sample column 63 pools the wrong right-hand block column", wrong_block_column, 1, (251, 256, 258)),
            ("sample row 32 repeats row 31", repeated_row, 0, (128, 134))]


@pytest.mark.parametrize("name", PC.CONTENTS)
@pytest.mark.parametrize("depth", PC.DEPTHS["ffmpeg"])
def test_teeth_vf_ssim(name, depth):
    a = PC.ref_plane("ffmpeg", name, depth)
    bar = PR.bar("ffmpeg", 0, name, depth)
    d64 = PR.D64("ffmpeg", name, depth)[:, 0]
    o = _ordinary(a, depth)
    plain = PR.ffmpeg_map(a, o, depth)
    for what, mutate, axis, at in _ffmpeg_mutations(depth):
        moves = []
        for k in _beside("ffmpeg", axis, at):
            got = PR.ffmpeg_probe_D(a, PC.dist_plane("ffmpeg", name, depth, PC.probes("ffmpeg")[k]), depth, mutate=mutate)
            moves.append(abs(got - d64[k]) / abs(d64[k]))
        best = PC.dist_plane("ffmpeg", name, depth, PC.probes("ffmpeg")[_beside("ffmpeg", axis, at)[int(np.argmax(moves))]])
        own = PR.ffmpeg_map(a, best, depth)
        own_move = abs(mutate(a, best, own).mean() - own.mean()) / own.mean()
        mean_move = abs(mutate(a, o, plain).mean() - plain.mean()) / plain.mean()
        print("vf_ssim %s %d bits, %s: a probe moves by %.2e (bar %.2e), its plane mean by %.2e, the mean of an ordinary pair by %.2e" % (
            name, depth, what, max(moves), bar, own_move, mean_move))
        assert max(moves) > 2 * bar, (what, moves, bar)
        assert mean_move < MEAN_BAR, (what, mean_move)


def _scale(maps):
    return float(maps[0].sum(dtype=np.float64) / maps[1].sum(dtype=np.float64))


@contextlib.contextmanager
def _clamped_borders():
    keep = V.border_index
    V.border_index = lambda i, n: min(max(i, 0), n - 1)
    try:
        yield
    finally:
        V.border_index = keep


@pytest.mark.parametrize("name", PC.CONTENTS)
def test_teeth_vif(name):
    """both on level 0: the border rule of its filter, and num's column 256 (the seam of tile columns 3 | 4) read at 257"""
    depth, lv = 8, 0
    a = PC.ref_plane("vif", name, depth)
    pr = PC.probes("vif")
    bar = PR.bar("vif", lv, name, depth)
    d64 = PR.D64("vif", name, depth)[:, lv]
    o = _ordinary(a, depth)

    def clamp(x, y):
        with _clamped_borders():
            return PR.vif_maps(x, y, depth)[lv]

    def off_by_one(x, y):
        num, den = (m.copy() for m in PR.vif_maps(x, y, depth)[lv])
        num[:, 256] = num[:, 257]
        return num, den
    edges = [k for k, p in enumerate(pr) if p[0] in (0, 139) or p[1] in (0, 263)]
    for what, mutated, ks in (("the reflecting border replaced by a clamp", clamp, edges),
                              ("tile-seam column 256 read one sample off", off_by_one, _beside("vif", 1, (251, 256, 258)))):
        rr = mutated(a, a)[0].sum(dtype=np.float64)
        moves, own = [], []
        for k in ks:
            d = PC.dist_plane("vif", name, depth, pr[k])
            bad = mutated(a, d)
            got = float(rr - bad[0].sum(dtype=np.float64))
            moves.append(abs(got - d64[k]) / abs(d64[k]))
            own.append(abs(_scale(bad) - _scale(PR.vif_maps(a, d, depth)[lv])))
        move = abs(_scale(mutated(a, o)) - _scale(PR.vif_maps(a, o, depth)[lv]))
        print("VIF %s, %s: a probe moves by %.2e (bar %.2e), its scale%d by %.2e, scale%d of an ordinary pair by %.2e" % (
            name, what, max(moves), bar, lv, own[int(np.argmax(moves))], lv, move))
        assert max(moves) > 2 * bar, (what, moves, bar)
        assert move < MEAN_BAR, (what, move)


# ---- ADM and motion: the geometry ----------------------------------------------------------------------------------------------------
def _adm_tiles(bh, bw):
    """csrc/vqa_kernels.hpp, adm_tiles: workgroups of 32 x 16 band samples -> (tile rows, tile columns)"""
    return (bh + 15) // 16, (bw + 31) // 32


def _adm_region_of(bh, bw):
    """csrc/vqa_kernels.hpp, adm_region_of: the (int) casts truncate towards 0"""
    left, top = int(bw * 0.1 - 0.5), int(bh * 0.1 - 0.5)
    return top, bh - top, left, bw - left


def _motion_tiles(h, w):
    """csrc/k_motion.hip, launch_motion_sad: 64 x 32 tiles -> (tile rows, tile columns)"""
    return (h + 31) // 32, (w + 63) // 64


def test_adm_and_motion_planes_cross_the_seams_the_probes_are_placed_at():
    assert all(PC.adm_region(bh, bw) == _adm_region_of(bh, bw) == A.region(bh, bw)[:4] for bh in range(1, 200) for bw in (1, 7, 33, 40, 320))
    assert all(PC.adm_dwt_index(i, n) == A.dwt_index(i, n) for n in (3, 6, 7, 48, 112) for i in range((n + 1) // 2))
    # plane A: every scale's pooled region has samples on both sides of a tile seam, both ways
    dims = A.level_dims(*PC.ADM_PLANE_A)
    assert dims == [(160, 320), (80, 160), (40, 80), (20, 40)]
    assert [_adm_region_of(*d) for d in dims] == [(15, 145, 31, 289), (7, 73, 15, 145), (3, 37, 7, 73), (1, 19, 3, 37)]
    assert [_adm_tiles(*d) for d in dims] == [(10, 10), (5, 5), (3, 3), (2, 2)]
    for s, d in enumerate(dims):
        top, bottom, left, right = _adm_region_of(*d)
        assert top < 16 < bottom and left < 32 < right, s
        # pixel row 256 and pixel column 512 are tile seams of this scale, inside its region
        assert (256 >> (s + 1)) % 16 == 0 and top < 256 >> (s + 1) < bottom and (512 >> (s + 1)) % 32 == 0 and left < 512 >> (s + 1) < right
    top, bottom, left, right = _adm_region_of(17, 33)                   # the scale-3 band of a 272 x 528 plane: two tiles each way,
    assert bottom <= 16 and right <= 32                                  # but the second ones are not pooled
    for seam, (axis, at, scales) in PC.SEAMS["adm"].items():
        if seam.startswith("tile"):                                      # the probes are P - 3, P, P + 3 around pixel P
            P, unit = at[1], (32 if axis == "row" else 64)
            assert at == (P - 3, P, P + 3) and scales == tuple(s for s in range(4) if P % (unit << s) == 0), seam
        elif seam.startswith("rows r"):                                  # band row 8 of a tile: between a thread's two samples
            s = scales[0]
            assert any((p >> (s + 1)) % 16 == 8 for p in at), seam
    top, bottom, left, right = _adm_region_of(*dims[0])
    assert (30 >> 1, 288 >> 1, 62 >> 1, 576 >> 1) == (top, bottom - 1, left, right - 1)
    # plane B: the region reaches the band's edge on scales 1 .. 3 and one seam each way is left on scale 0
    dims = A.level_dims(*PC.ADM_PLANE_B)
    assert dims == [(24, 56), (12, 28), (6, 14), (3, 7)]
    assert [_adm_region_of(*d) for d in dims] == [(1, 23, 5, 51), (0, 12, 2, 26), (0, 6, 0, 14), (0, 3, 0, 7)]
    assert [_adm_tiles(*d) for d in dims] == [(2, 2), (1, 1), (1, 1), (1, 1)]
    # motion: 5 x 5 tiles, every probed seam is one
    h, w = PC.plane_of("motion")
    assert _motion_tiles(h, w) == (5, 5)
    for seam, (axis, at, _scales) in PC.SEAMS["motion"].items():
        if seam.startswith("tile"):
            P, unit, n = at[1], (32 if axis == "row" else 64), (h if axis == "row" else w)
            assert at == (P - 2, P, P + 2) and P % unit == 0 and 0 < P < n, seam
    assert 16 in PC.MOTION_ROWS and 99 % 4 == 3 and 100 % 4 == 0
    # every probe lies in its plane, no patch clips a sample, and every seam's probes exist
    for kind in ("adm", "adm-b", "motion"):
        ph, pw = PC.plane_of(kind)
        pr = PC.probes(kind)
        assert len(set(pr)) == len(pr) and 2 * len(pr) + 1 <= 100
        for name in PC.CONTENTS:
            for depth in PC.DEPTHS[kind]:
                a = PC.ref_plane(kind, name, depth)
                assert a.shape == (ph, pw) and a.min() >= 0 and a.max() <= (1 << depth) - 1
        for p in pr:
            y0, y1, x0, x1 = PC.patch_box(p, (ph, pw), PC.patch_size(kind))
            assert 0 <= y0 < y1 <= ph and 0 <= x0 < x1 <= pw, (kind, p)
        for seam, (axis, at, _scales) in PC.SEAMS[kind].items():
            assert all(any(p[0 if axis == "row" else 1] == v for p in pr) for v in at), (kind, seam)


def test_adm_reaches_the_scales_it_is_judged_on_and_is_exactly_zero_elsewhere():
    """probe_cases.adm_reach, from the index rules alone, against the reference: D is exactly 0, in float64 and in float32, on every
    scale the patch reaches no pooled sample of, and nowhere else"""
    assert PC.levels_of("adm", PC.ADM_OUTSIDE) == []
    assert all(PC.levels_of("adm", p) == [0, 1, 2, 3] for p in PC.probes("adm") if p != PC.ADM_OUTSIDE)
    assert [p for p in PC.probes("adm-b") if PC.levels_of("adm-b", p) != [0, 1, 2, 3]] == [(24, 0), (24, 111)]      # region columns 5 .. 50
    for kind in ("adm", "adm-b"):
        reach = np.array([[s in PC.levels_of(kind, p) for s in range(4)] for p in PC.probes(kind)])
        for name in PC.CONTENTS:
            for depth in PC.DEPTHS[kind]:
                assert ((PR.D64(kind, name, depth) != 0) == reach).all() and ((PR.D32(kind, name, depth) != 0) == reach).all()


def test_adm_and_motion_batches():
    for kind, lay, depth in (("adm", "bgr24", 8), ("adm-b", "gray", 10)):
        ref, dist, planes, probed = PC.batch(kind, "noise", depth, lay)
        pr = PC.probes(kind)
        assert ref.shape == dist.shape and ref.shape[0] == 1 + len(pr) and (ref == ref[0]).all() and (dist[0] == ref[0]).all()
        assert np.array_equal(R.plane(ref[0], planes[probed]), PC.ref_plane(kind, "noise", depth))
        for k in (1, len(pr)):
            for i, p in enumerate(planes):
                want = PC.dist_plane(kind, "noise", depth, pr[k - 1]) if i == probed else R.plane(ref[0], p)
                assert np.array_equal(R.plane(dist[k], p), want)
    pr = PC.probes("motion")
    for lay, depth in (("bgr24", 8), ("gray", 16)):
        f, planes, probed = PC.motion_batch("smooth", depth, lay)
        assert f.shape[0] == 2 * len(pr) + 1 and (f[0::2] == f[0]).all()
        for k in (1, len(pr)):
            for i, p in enumerate(planes):
                want = PC.dist_plane("motion", "smooth", depth, pr[k - 1]) if i == probed else R.plane(f[0], p)
                assert np.array_equal(R.plane(f[2 * k - 1], p), want)
    assert PC.motion_touched((50, 150)) == 81 and PC.motion_touched((0, 0)) == 100 and PC.motion_touched((0, 150)) == 5 * 9


def test_the_adm_and_motion_sides_are_the_references_own_numbers():
    a, d = PC.ref_plane("adm-b", "noise", 10), PC.dist_plane("adm-b", "noise", 10, (24, 64))
    for dt in (np.float64, np.float32):
        num, den, _scale, _adm2 = A.adm(a, d, 10, dt)
        got = PR.adm_sums(a, d, 10, dt)
        assert np.array_equal(got[0], num) and np.array_equal(got[1], den)
    a, d = PC.ref_plane("motion", "smooth", 10), PC.dist_plane("motion", "smooth", 10, (64, 64))
    assert PR.motion_sad(d, a, 10) == MO.sad(d, a, 10) and np.array_equal(PR.motion_blur(MO.samples(d, 10)), MO.blur(MO.samples(d, 10)))
    assert abs(PR.motion_sad(d, a, 10, np.float32) - MO.sad(d, a, 10)) <= 1e-6 * MO.sad(d, a, 10)


def test_motion_is_linear_so_the_touched_outputs_alone_carry_d():
    """sad(base + delta, base) = sum |blur(delta)|: the blur is linear and the samples are exact, so the pair's sad is the patch's
    own blur - 81 output samples for a whole 5 x 5 patch - whatever the base holds"""
    for name in PC.CONTENTS:
        for depth in PC.DEPTHS["motion"]:
            a = PC.ref_plane("motion", name, depth)
            d64 = PR.D64("motion", name, depth)[:, 0]
            for k, p in enumerate(PC.probes("motion")):
                delta = (PC.dist_plane("motion", name, depth, p) - a) / float(1 << (depth - 8))
                b = np.abs(MO.blur(delta))
                assert abs(b.sum() - d64[k]) <= 1e-12 * d64[k], (name, depth, p)
                assert np.count_nonzero(b) == PC.motion_touched(p), p


# ---- ADM and motion: the exclusions, the unsure items ---------------------------------------------------------------------------------
def test_adm_and_motion_exclusions_are_few_named_and_leave_every_seam_probed():
    items = {kind: [(lv, p) for p in PC.probes(kind) for lv in PC.levels_of(kind, p)] for kind in ("adm", "adm-b", "motion")}
    for kind, it in items.items():
        assert all(key in it and isinstance(reason, str) and reason for key, reason in PC.EXCLUDED[kind].items()), kind
        for seam, (axis, at, scales) in PC.SEAMS[kind].items():
            for lv in scales:
                left = [PC.probes(kind)[k] for k in PR.kept(kind, lv) if PC.probes(kind)[k][0 if axis == "row" else 1] in at]
                assert left, (kind, lv, seam)
    n_adm = len(items["adm"]) + len(items["adm-b"])                    # one kind on two planes
    assert len(PC.EXCLUDED["adm"]) + len(PC.EXCLUDED["adm-b"]) <= PC.MAX_EXCLUDED_SHARE * n_adm and not PC.EXCLUDED["motion"]
    print("ADM: %d (probe, scale) items, %d excluded" % (n_adm, len(PC.EXCLUDED["adm"]) + len(PC.EXCLUDED["adm-b"])))
    # an exclusion is needed: the item's own ratio is beyond what the kept ones of its scale give, and 4 times it is beyond the cap
    worst = np.max([PR.ratios("adm-b", n, d) for n in PC.CONTENTS for d in PC.DEPTHS["adm-b"]], axis=0)
    pr = PC.probes("adm-b")
    for lv, p in PC.EXCLUDED["adm-b"]:
        kept_worst = worst[PR.kept("adm-b", lv), lv].max()
        print("excluded ADM plane B scale %d probe %s: ratio %.2e (the worst kept one: %.2e)" % (lv, p, worst[pr.index(p), lv], kept_worst))
        assert worst[pr.index(p), lv] > kept_worst and PC.MARGIN * worst[pr.index(p), lv] > PC.CAP


def test_adm_unsure_items_are_judged_against_the_interval_of_their_forced_flags():
    """the angle test is a discontinuity.  An item whose touched region holds a sample within 2^-20 of it (tests/test_gpu_adm.py's
    margin, adm_reference's machinery) is not excluded: it is held to the interval of the runs with those flags forced off and on,
    widened by the bar.  They are listed here; every other item has an interval of one point"""
    n = 0
    for kind in ("adm", "adm-b"):
        pr = PC.probes(kind)
        for name in PC.CONTENTS:
            for depth in PC.DEPTHS[kind]:
                d64, d32 = PR.D64(kind, name, depth), PR.D32(kind, name, depth)
                lo, hi = PR.interval(kind, name, depth)
                un = PR.adm_unsure(kind, name, depth)
                sure = np.ones(d64.shape, bool)
                for (s, p), (a, b) in sorted(un.items()):
                    k = pr.index(p)
                    sure[k, s] = False
                    n += 1
                    print("unsure: %s %s %d bits scale %d probe %s: D_64 %.6e in [%.6e, %.6e] (%.1e of D_64), D_32 %.6e" % (
                        kind, name, depth, s, p, d64[k, s], a, b, (b - a) / abs(d64[k, s]), d32[k, s]))
                    assert a <= d64[k, s] <= b and s in PC.levels_of(kind, p)
                assert np.array_equal(lo[sure], d64[sure]) and np.array_equal(hi[sure], d64[sure])
    assert 0 < n <= 24        # 744 (probe, scale) items over the eight cases


def test_the_derived_margin_of_adm_plane_b_scale_3_is_its_arithmetic():
    """probe_cases.MARGIN_OF, ("adm-b", 3, "noise", 8): the figures of its comment, recomputed from the reference alone"""
    key = ("adm-b", 3, "noise", 8)
    kind, s, name, depth = key
    pr = PC.probes(kind)
    d64, d32 = PR.D64(kind, name, depth)[:, s], PR.D32(kind, name, depth)[:, s]
    r, bar = PR.group_ratio(*key), PR.bar(*key)
    assert bar == PC.MARGIN_OF[key] * r and abs(r - 4.29e-6) < 1e-8
    sig = {}
    for k in PR.kept(kind, s):
        sig[pr[k]], e, n = PR.adm_sigma(kind, name, depth, pr[k], s)
        print("%s: D_64 %.3e, sigma_D %.2e over %d touched samples (e %.2e), the float32 run is %.2e = %.2f sigma off, the bar is %.1f sigma" % (
            pr[k], d64[k], sig[pr[k]], n, e, abs(d32[k] - d64[k]), abs(d32[k] - d64[k]) / sig[pr[k]], bar * abs(d64[k]) / sig[pr[k]]))
        assert 1.0e-5 < e < 1.4e-5 and 4 <= n <= 12 and 2.5e-7 < sig[pr[k]] < 8.5e-7
        assert abs(d32[k] - d64[k]) <= 2 * sig[pr[k]]                        # the reference's own draws are the model's
    k = pr.index((0, 56))
    assert abs(d64[k]) == np.abs(d64[PR.kept(kind, s)]).min()              # the smallest D of the group sets the margin
    assert PC.MARGIN * r * abs(d64[k]) < 0.6 * sig[(0, 56)]                # 4 r is half a sigma there
    assert 3.0 * sig[(0, 56)] <= bar * abs(d64[k]) <= 4.5 * sig[(0, 56)]   # the margin: 3 .. 4.5 sigma


# ---- ADM and motion: teeth -------------------------------------------------------------------------------------------------------------
TEETH = 10          # a mutation moves a probe beside its seam by at least this many bars


class _AdmMutation:
    """what adm_sums' `mutate` wants; a mutation overrides one of the two"""
    def bands(self, s, x, b):
        return b

    def patched(self, s):
        return contextlib.nullcontext()


@contextlib.contextmanager
def _patched(module, name, value):
    keep = getattr(module, name)
    setattr(module, name, value)
    try:
        yield
    finally:
        setattr(module, name, keep)


class _ColumnFromShiftedInputs(_AdmMutation):
    what = "scale-0 band column 32 is computed from inputs one sample off"

    def bands(self, s, x, b):
        if s:
            return b
        bad = A.dwt(np.roll(x, -1, axis=1))
        out = [m.copy() for m in b]
        for o, m in zip(out, bad):
            o[:, 32] = m[:, 32]
        return out


class _MaskNeighbourZero(_AdmMutation):
    what = "scale 0: the mask's neighbours across the seam (column 31, seen from column 32) read as 0"

    def patched(self, s):
        if s:
            return contextlib.nullcontext()
        orig = A._neighbour_sum

        def f(m):
            out = orig(m).copy()
            bh = m.shape[0]
            e = m[[A.border_index(i, bh) for i in range(-1, bh + 1)], 31]
            out[:, 32] -= (e[0:bh] + e[1:bh + 1] + e[2:bh + 2]) * m.dtype.type(1.0 / 30.0)
            return out
        return _patched(A, "_neighbour_sum", f)


class _ABandColumnCopied(_AdmMutation):
    what = "the a band handed to scale 1 has column 32 copied from column 31"

    def bands(self, s, x, b):
        if s:
            return b
        a = b[0].copy()
        a[:, 32] = a[:, 31]
        return [a] + list(b[1:])


class _RegionLeftOffByOne(_AdmMutation):
    what = "scale 0: the region's left bound is 32, not 31"

    def patched(self, s):
        if s:
            return contextlib.nullcontext()
        orig = A.region

        def f(bh, bw):
            top, bottom, left, right, area = orig(bh, bw)
            return top, bottom, left + 1, right, area
        return _patched(A, "region", f)


class _MinusOneReadsZero(_AdmMutation):
    what = "the mask's band index -1 reads 0 instead of 1"

    def patched(self, s):
        orig = A.border_index
        return _patched(A, "border_index", lambda i, n: 0 if i < 0 else orig(i, n))


# (plane, mutation, the scales it shows on, the probes beside its seam)
_COL64 = [(PC.ADM_ROW, c) for c in (61, 62, 64, 67)] + [(32, 64)]
ADM_TEETH = [
    ("adm", _ColumnFromShiftedInputs(), (0, 1, 2, 3), _COL64),
    ("adm", _MaskNeighbourZero(), (0,), _COL64),
    ("adm", _ABandColumnCopied(), (1, 2, 3), _COL64),
    ("adm", _RegionLeftOffByOne(), (0,), _COL64),
    ("adm-b", _MinusOneReadsZero(), (1, 2, 3), [(0, 0), (0, 56), (0, 111), (24, 0), (47, 0)]),
]


@pytest.mark.parametrize("name", PC.CONTENTS)
@pytest.mark.parametrize("kind,mutation,scales,beside", ADM_TEETH, ids=[type(t[1]).__name__.strip("_") for t in ADM_TEETH])
def test_teeth_adm(kind, mutation, scales, beside, name):
    depth = 8
    a = PC.ref_plane(kind, name, depth)
    pr = PC.probes(kind)
    d64 = PR.D64(kind, name, depth)
    num0 = PR.adm_sums(a, a, depth, mutate=mutation)[0]
    best = (-1.0, None)
    for p in beside:
        k = pr.index(p)
        D = num0 - PR.adm_sums(a, PC.dist_plane(kind, name, depth, p), depth, mutate=mutation)[0]
        for s in scales:
            if k in PR.kept(kind, s) and (s, p) not in PR.adm_unsure(kind, name, depth):
                move, bar = abs(D[s] - d64[k, s]) / abs(d64[k, s]), PR.bar(kind, s, name, depth)
                best = max(best, (move / bar, (p, s, move, bar)), key=lambda b: b[0])
    o = _ordinary(a, depth)
    plain, bad = PR.adm_sums(a, o, depth), PR.adm_sums(a, o, depth, mutate=mutation)
    scale_move = float(np.abs(bad[0] / bad[1] - plain[0] / plain[1]).max())
    p, s, move, bar = best[1]
    print("ADM %s %s, %s: probe %s scale %d moves by %.2e = %.0f bars (bar %.2e); a scale of an ordinary pair moves by %.2e: %s its 1e-4" % (
        "plane A" if kind == "adm" else "plane B", name, mutation.what, p, s, move, best[0], bar, scale_move,
        "under" if scale_move < ADM_BAR else "ABOVE"))
    assert best[0] >= TEETH, (mutation.what, best)


def _apron_of_one(v, out):
    """the tile that begins at column 64 holds one apron column, not two: its first output's outermost tap reads 0, not column 62"""
    out = out.copy()
    out[:, 64] -= v.dtype.type(MO.TAPS[0]) * v[:, 62]
    return out


def _column_63_dropped(d):
    d = d.copy()
    d[:, 63] = 0
    return d


_EDGES = [(0, PC.MOTION_COL), (139, PC.MOTION_COL), (PC.MOTION_ROW, 0), (PC.MOTION_ROW, 263), (0, 0), (139, 263)]
_SEAM64 = [(PC.MOTION_ROW, 62), (PC.MOTION_ROW, 64), (PC.MOTION_ROW, 66), (64, 64)]
MOTION_TEETH = [("an apron of 1 at tile column 64", dict(hmutate=_apron_of_one), False, _SEAM64),
                ("a clamped border instead of a reflecting one", {}, True, _EDGES),
                ("the output of column 63 is dropped", dict(omutate=_column_63_dropped), False, _SEAM64)]


@pytest.mark.parametrize("name", PC.CONTENTS)
@pytest.mark.parametrize("what,how,clamp,beside", MOTION_TEETH, ids=["apron", "clamp", "dropped"])
def test_teeth_motion(what, how, clamp, beside, name):
    depth = 8
    a = PC.ref_plane("motion", name, depth)
    h, w = a.shape
    pr = PC.probes("motion")
    d64 = PR.D64("motion", name, depth)[:, 0]
    fixed = PR.motion_fixed_point()
    rel = PR.bar("motion", 0, name, depth)
    o = _ordinary(a, depth)
    with (_patched(MO, "border_index", lambda i, n: min(max(i, 0), n - 1)) if clamp else contextlib.nullcontext()):
        got = {p: PR.motion_sad(PC.dist_plane("motion", name, depth, p), a, depth, **how) for p in beside}
        bad = PR.motion_sad(o, a, depth, **how)
    best = (-1.0, None)
    for p in beside:
        k = pr.index(p)
        bar = rel + fixed[k] / d64[k]
        move = abs(got[p] - d64[k]) / d64[k]
        best = max(best, (move / bar, (p, move, bar)), key=lambda b: b[0])
    mean_move = abs(bad - MO.sad(o, a, depth)) / (h * w)
    p, move, bar = best[1]
    print("motion %s, %s: probe %s moves by %.2e = %.0f bars (bar %.2e); the motion of an ordinary pair moves by %.2e: %s its %.2e" % (
        name, what, p, move, best[0], bar, mean_move, "under" if mean_move < MOTION_BAR else "ABOVE", MOTION_BAR))
    assert best[0] >= TEETH, (what, best)
