"""CPU: the clips tests/test_gpu_depths.py submits at 9, 11, 12, 13, 14 and 15 bits are fair inputs - inside the depth's range, with
content in the bits below the 8-bit level, of uint16 samples, the range-end clips at the ends they are named for - and fair tests
of the kernels, not of fp32 itself: where a kind's reference can run in the precision the kernel uses, that run stays inside the
kind's existing admission figure on every plane of every frame, of the natural clips and of the range-end clips alike
(hostile_cases' half bar for SSIM, VIF and ADM, ciede_cases.ADMIT, psnr_hvs_cases.ADMIT, mdsi_reference.derived_bar under
mdsi_cases.BAR_LIMIT).  A (kind, content, depth) that does not is left out by name in depth_cases.EXCLUDED, within its cap, and is
shown here to leave the figure; depth_cases.FLOAT_ENDS was chosen so that the list is empty.  BRISQUE admits fit by fit inside
its own checker (brisque_reference.alpha_spans), dE_ITP and PU21 have no reduced-precision restatement.  Also the hand pins of
cambi_reference.to10 at the depths where it rounds and clamps."""
import numpy as np
import pytest

import cambi_reference as CB
import ciede_cases as CC
import ciede_reference as CR
import depth_cases as DC
import hostile_cases as HK
import mdsi_cases as MC
import mdsi_reference as MR
import motion_cases as K
import psnr_hvs_cases as PC
import psnr_hvs_reference as PR
import test_hostile_host as THH

_JOBS = {}


def _job(kind, depth, which="natural"):
    if (kind, depth, which) not in _JOBS:
        _JOBS[kind, depth, which] = {"natural": DC.job, "ends": DC.float_end_job, "words": DC.range_end_job}[which](kind, depth)
    return _JOBS[kind, depth, which]


def _streams(kind, depth):
    """every host array of a kind's natural clip at a depth"""
    if kind == "pu21":
        return list(DC.pu21_clip("natural", depth)[:2])
    return [a for a in _job(kind, depth).host if a is not None]


@pytest.mark.parametrize("depth", DC.DEPTHS)
def test_every_clip_is_in_range_uses_its_low_bits_and_is_uint16(depth):
    peak, low = (1 << depth) - 1, (1 << (depth - 8)) - 1
    for kind in DC.KINDS:
        for a in _streams(kind, depth):
            assert a.dtype == np.uint16, (kind, depth)
            assert int(a.max()) <= peak and int(a.max()) > peak // 4, (kind, depth, int(a.max()))
            assert (a & low).any(), (kind, depth, "nothing below the 8-bit level")
    for kind in DC.SHIFT_KINDS:                   # the shifted clips: the 8-bit samples, nothing below the 8-bit level
        lo, hi = DC.shifted_jobs(kind, depth)
        for a8, a in zip(lo.host, hi.host):
            if a8 is None:
                continue
            assert a.dtype == np.uint16 and int(a.max()) <= peak and not (a & low).any() and np.array_equal(a >> (depth - 8), a8)


def _range_end_clips(depth):
    """(kind, content, the host arrays that hold it) of every range-end clip at a depth: frame i of a clip is content i"""
    for kind, names in DC.RANGE_ENDS.items():
        j = _job(kind, depth, "words")
        for i in range(j.n):
            yield kind, names[i % len(names)], [a[i] for a in j.host[:2]]
    for kind in DC.FLOAT_ENDS:
        for i, name in enumerate(DC.float_ends(kind, depth)):
            if kind == "pu21":
                yield kind, name, list(DC.pu21_clip(name, depth)[:2])
            else:
                yield kind, name, [a[i] for a in _job(kind, depth, "ends").host[:2]]


# the end of the range a content is named for: every other range-end content holds both 0 and the maximum
ONE_END = {"bright_flat": "peak", "dark_flat": "zero", "flat_peak": "peak", "flatpeak": "peak", "sparse": "under peak", "flat": "near peak",
           "top_ramp": "10-bit peak", "staircase": "none", "top_ramp_peak": "peak"}


@pytest.mark.parametrize("depth", DC.DEPTHS)
def test_the_range_end_clips_reach_the_ends_of_the_range(depth):
    """every range-end clip is uint16, inside the range and AT the end it is named for: the maximum 2^depth - 1, 0, or both
    (CAMBI's staircase is its banded mid-range companion; its top_ramp ends at the 10-bit maximum brought to the depth, which is
    the peak at 9 bits, and top_ramp_peak ends at the peak; BRISQUE's flat is peak - 3 .. peak - 1 by definition, VCA's sparse a
    flat field one or two codes under the peak with single samples a few codes lower)"""
    peak = (1 << depth) - 1
    seen = 0
    for kind, name, arrays in _range_end_clips(depth):
        a = np.concatenate([x.reshape(-1) for x in arrays])
        assert a.dtype == np.uint16 and int(a.max()) <= peak, (kind, name, depth)
        lo, hi = int(a.min()), int(a.max())
        end = ONE_END.get(name, "both")
        if end == "both":
            assert (lo, hi) == (0, peak), (kind, name, depth, lo, hi)
        elif end == "peak":
            assert hi == peak, (kind, name, depth, hi)
        elif end == "zero":
            assert lo == 0, (kind, name, depth, lo)
        elif end == "near peak":
            assert (lo, hi) == (peak - 3, peak - 1), (kind, name, depth, lo, hi)
        elif end == "under peak":
            assert peak - 8 <= lo < hi < peak, (kind, name, depth, lo, hi)
        elif end == "10-bit peak":
            assert hi == (1023 << (depth - 10) if depth >= 10 else 1023 >> (10 - depth)), (kind, name, depth, hi)
            assert CB.to10(np.array([[hi]], np.int64), depth)[0, 0] == (1023 if depth >= 10 else 1022)
        else:
            assert 0 < lo and hi < peak and lo != hi, (kind, name, depth, lo, hi)
        seen += 1
    assert seen == sum(max(DC.RANGE_END_FRAMES, len(v)) for v in DC.RANGE_ENDS.values()) + sum(len(DC.float_ends(k, depth)) for k in DC.FLOAT_ENDS)
    if depth >= 11:                              # top_ramp_peak's last band rounds up to 1024: what the clamp of to10 is for
        half = 1 << (depth - 11)
        assert (peak + half) >> (depth - 10) == 1024 and CB.to10(np.array([[peak]], np.int64), depth)[0, 0] == 1023


def test_the_kinds_the_jobs_and_the_exclusions():
    import test_gpu_all_kinds as TAK
    assert set(DC.KINDS) == (set(TAK.KINDS) - {"complexity"}) | {"ffmpeg", "ms", "pu21"} and len(DC.KINDS) == 19
    assert DC.DEPTHS == (9, 11, 12, 13, 14, 15) and set(DC.SHIFT) == set(DC.KINDS)
    assert {"vif", "adm", "motion", "siti", "vca", "cambi", "ciede"} == set(DC.SHIFT_KINDS) and not {"gauss", "ffmpeg", "ms", "gmsd", "haarpsi"} & set(DC.SHIFT_KINDS)
    # the integer kinds and the float-bar kinds of the issue, each with range-end contents
    assert set(DC.RANGE_ENDS) == {"cambi", "artifacts", "xpsnr", "vca", "siti", "gmsd", "haarpsi", "psnr_hvs"}
    assert set(DC.FLOAT_ENDS) == {"gauss", "ms", "vif", "adm", "ciede", "mdsi", "brisque", "itp", "pu21"}
    for kind in DC.KINDS:
        if kind != "pu21":
            j = _job(kind, 9)
            assert (j.h, j.w) == (DC.MS_GEOMETRY if kind == "ms" else DC.GEOMETRY) and j.n in DC.FRAMES
            assert len(j.planes) == (1 if kind == "ms" else 3)
    with pytest.raises(KeyError):
        DC.job("pu21", 9)
    per = {}
    for kind, content, depth in DC.EXCLUDED:
        assert content != "natural" and content in DC.FLOAT_ENDS[kind] and depth in DC.DEPTHS
        per.setdefault((kind, depth), set()).add(content)
    assert all(len(v) <= DC.MAX_EXCLUDED_PER_KIND_AND_DEPTH for v in per.values())
    for kind in DC.FLOAT_ENDS:
        for depth in DC.DEPTHS:
            assert len(DC.float_ends(kind, depth)) >= len(DC.FLOAT_ENDS[kind]) - DC.MAX_EXCLUDED_PER_KIND_AND_DEPTH >= 0
            assert DC.float_ends(kind, depth), (kind, depth)


def _pairs(kind, depth, which="natural"):
    """(tag, ref plane, dist plane) of every plane of every frame of a kind's job"""
    j = _job(kind, depth, which)
    r, d, _p0 = j.host
    for jx, p in enumerate(j.planes):
        sr, sd = K.plane_series(r, p), K.plane_series(d, p)
        for i in range(j.n):
            yield "%s %s %d bits frame %d plane %d" % (kind, which, depth, i, jx), sr[i], sd[i]


@pytest.mark.parametrize("depth", DC.DEPTHS)
@pytest.mark.parametrize("kind", ["gauss", "ms", "vif", "adm"])
def test_float32_stays_within_half_the_bar(kind, depth):
    """tests/test_hostile_host.py's rule and figure, on the planes test_gpu_depths.py submits: the natural clip and the range-end
    clip (vf_ssim's reference sums integers).  SSIM's bar is relative: its value stays far from 0"""
    metric = "ssim" if kind in ("gauss", "ms") else kind
    for which in ("natural", "ends"):
        worst = 0.0
        for tag, r, d in _pairs(kind, depth, which):
            e, ref = THH.DEV[metric](r, d, depth)
            worst = max(worst, e)
            assert e <= THH.HALF, (tag, e)
            if metric == "ssim":
                assert abs(ref) >= 0.1, (tag, ref)
        print("depths, admission:", kind, which, depth, "bits, float32 deviation at most %.2e" % worst)


def test_what_is_excluded_does_leave_its_figure():
    """an exclusion is a finding, not a convenience: the float32 run of every excluded (kind, content, depth) is outside the figure
    on some plane of the clip's geometry"""
    for kind, content, depth in DC.EXCLUDED:
        metric = "ssim" if kind in ("gauss", "ms") else kind
        sizes = [DC.MS_GEOMETRY] if kind == "ms" else [DC.GEOMETRY, ((DC.GEOMETRY[0] + 1) // 2, (DC.GEOMETRY[1] + 1) // 2)]
        worst = max(THH.DEV[metric](*HK.pair(content, h, w, depth), depth)[0] for h, w in sizes)
        print("depths, excluded:", kind, content, depth, "bits, float32 deviation %.2e" % worst)
        assert worst > THH.HALF, (kind, content, depth, worst)


def _vif_deviation(j):
    r, d, _p0 = j.host
    return max(THH.DEV["vif"](K.plane_series(r, p)[i], K.plane_series(d, p)[i], j.depth)[0] for p in j.planes for i in range(j.n))


def test_vifs_job_is_the_first_admitted_one():
    """depth_cases.INDEX_STEPS: VIF's natural job at a depth is the FIRST index k + 19 m whose clip the figure admits with
    depth_cases.INDEX_SPARE to spare - every earlier one is shown not to (DESIGN.md section 3 has this as an open item: the
    float32 run of VIF's reference reaches the GPU bar itself on natural content at 35 x 37)"""
    import test_gpu_all_kinds as TAK
    k = DC.KINDS.index("vif")
    h, w = DC.GEOMETRY
    assert {key[0] for key in DC.INDEX_STEPS} == {"vif"}
    for depth in DC.DEPTHS:
        steps = DC.INDEX_STEPS.get(("vif", depth), 0)
        assert _job("vif", depth).index == k + len(DC.KINDS) * steps
        dev = _vif_deviation(_job("vif", depth))
        print("depths, vif: %d bits, job index step %d, float32 deviation %.2e" % (depth, steps, dev))
        assert dev <= DC.INDEX_SPARE * THH.HALF, (depth, steps, dev)
        for m in range(steps):
            earlier = TAK.Job(k + len(DC.KINDS) * m, "vif", DC.FRAMES[(k + len(DC.KINDS) * m) % 4], "yuv420p", h, w, depth)
            dev = _vif_deviation(earlier)
            print("depths, vif: %d bits, job index step %d passed over, float32 deviation %.2e" % (depth, m, dev))
            assert dev > DC.INDEX_SPARE * THH.HALF, (depth, m, dev)


@pytest.mark.parametrize("depth", DC.DEPTHS)
def test_ciede_psnr_hvs_and_mdsi_are_admitted(depth):
    for which in ("natural", "ends"):
        j = _job("ciede", depth, which)
        fr, fd = CR.split_planes(j.host[0], j.planes), CR.split_planes(j.host[1], j.planes)
        for i in range(j.n):
            a = CR.de_mean(fr[i], fd[i], depth, CR.YUV709, (1.0, 1.0, 1.0))
            b = CR.de_mean(fr[i], fd[i], depth, CR.YUV709, (1.0, 1.0, 1.0), np.float32)
            assert np.isfinite(b) and a > 0.0 and abs(b - a) / a <= CC.ADMIT, ("ciede", which, depth, i, a, b)
        j = _job("mdsi", depth, which)
        for i in range(j.n):
            r, d = j.lists[0][i], j.lists[1][i]
            gcs = MR.gcs_float(r, d, MC.MODEL["yuv420p"], depth)
            dev, _ = MR.pool_float(gcs)
            bar = MR.derived_bar(gcs)
            got, _ = MR.pool_words(MR.mdsi_quantised(r, d, MC.MODEL["yuv420p"], depth), gcs.size)
            assert bar <= MC.BAR_LIMIT and abs(got - dev) <= bar, ("mdsi", which, depth, i, got, dev, bar)
    for tag, r, d in _pairs("psnr_hvs", depth):
        a, b = PR.psnr_hvs(r, d, depth), PR.psnr_hvs(r, d, depth, np.float32)
        assert max(abs(b[k] - a[k]) / a[k] for k in (0, 1)) <= PC.ADMIT, tag


def test_to10_by_hand():
    """below 10 bits a shift up; from 11 bits (x + half) >> (depth - 10), clamped: (2047 + 1) >> 1 is 1024"""
    def one(x, depth):
        return int(CB.to10(np.array([[x]], np.int64), depth)[0, 0])
    assert one(511, 9) == 1022
    assert one(2047, 11) == 1023 and one(2045, 11) == 1023
    assert one(32767, 15) == 1023 and one(16, 15) == 1
    assert one(2044, 11) == 1022 and one(0, 13) == 0 and one(3, 13) == 0 and one(4, 13) == 1
