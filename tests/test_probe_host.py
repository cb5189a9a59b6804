"""CPU: the probe matrix of tests/probe_cases.py is sound before a GPU sees it.

  the geometry     the planes cross the seams probe_cases says they cross (the launch arithmetic of csrc/k_quality.hip restated)
  the reference    probe_reference's maps are the references' own numbers; D does not depend on the crop
  stability        r = max_k |D_32(k) - D_64(k)| / |D_64(k)| per (kind, level, content, depth); the GPU's bar is 4 r, floored at 1e-5
  the cap          no bar above 1e-3; what would push one past it is excluded by name, at most 1 in 16 (probe, level) items of a
                   kind, and no seam loses all of its probes
  teeth            eight mutations of the float64 reference, each at one seam: a probe beside the seam moves by more than twice
                   its group's bar while the plane mean of an ordinary pair moves by less than 1e-4 - what the suite's bars
                   could not see
"""
import contextlib

import numpy as np
import pytest

import hbd_reference as R
import layout_cases as LC
import msssim_reference as M
import probe_cases as PC
import probe_reference as PR
import vif_reference as V

MEAN_BAR = 1e-4     # the suite's bar on a plane mean (tests/test_gpu_parity.py's RTOL, tests/test_gpu_vif.py's BAR)
KINDS = ("gauss", "ffmpeg", "vif", "ms-cs", "ms-ssim")
GROUPS = [(k, n, d) for k in KINDS for n in PC.CONTENTS for d in PC.DEPTHS[PR.base_kind(k)]]


def _levels(kind):
    return {"vif": PC.VIF_LEVELS, "ms-cs": PC.MS_LEVELS, "ms-ssim": PC.MS_LEVELS}.get(kind, 1)


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
