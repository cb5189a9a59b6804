"""GPU: localised probes at the tile seams of Gaussian SSIM, vf_ssim, MS-SSIM, VIF, ADM and motion (tests/probe_cases.py has the planes, the probe
centres and the patch; tests/probe_reference.py the float64 / float32 side; tests/test_probe_host.py shows the matrix sound and
with teeth on the CPU).

One batch per case: frame 0 is (ref, ref), frame k is (ref, dist_k) with one small patch beside a seam of the work decomposition.
The kernels sum integers (2^-27 fixed point) or doubles of exact terms, so every window the patch does not touch gives frame k
what it gives frame 0, bit for bit, and

    D_gpu(k) = N (value(frame 0) - value(frame k))

is the sum over the touched windows alone: an error in one map column at a seam, which a plane mean hides under 1e-4, is 1e-3 ..
1e-1 of it.  D_gpu is held to the float64 D within the group's bar - 4 times the reference's own float32-to-float64 ratio, floored
at 1e-5, never above 1e-3 - and the exact consequences are asserted as they are: SSE is the closed form, the planes without a
patch return frame 0's bits, VIF's den is a function of ref alone, MS-SSIM's level 0 is Gaussian SSIM.

Largest |D_gpu - D_64| / |D_64| on an MI355X, with the bar of that group (test_the_worst_gaps prints them; DESIGN.md section 3,
"probe parity"):
    Gaussian SSIM   2.69e-5 (5.4e-5)   noise, 10 bits, probe (5, 0); gray, the G plane of bgr24 and the U plane of 4:2:0 alike;
                                       4.9e-6 on the smooth field
    vf_ssim         7.87e-7 (1e-5)     8 bits, all three kernels: the float32 restatement of FFmpeg's ssim_end1 to every digit;
                                       1.3e-12 at 10 bits on both 16-bit kernels
    MS-SSIM cs      4.21e-5 (7.2e-5)   level 0, noise, 10 bits, probe (5, 527): the one group with a margin of 7, derived in
                                       probe_cases.MARGIN_OF; levels 1 .. 4: 2.6e-5, 1.1e-7, 1.0e-6, 3.8e-5
    MS-SSIM ssim    8.83e-5 (4.2e-4)   level 4, noise, 8 bits; levels 0 .. 3: 1.9e-5, 3.0e-5, 1.3e-7, 7.7e-7
    VIF             1.42e-4 (1.7e-4)   level 3, noise, 8 bits, probe (139, 258); levels 0 .. 2: 1.1e-6, 2.5e-6, 8.1e-6
Every equality holds: SSE, the planes without a patch, den, MS-SSIM's level 0, and the 3072-frame batch's bits.

ADM and motion (kinds "adm": plane A, 320 x 640, 37 probes; "adm-b": plane B, 48 x 112, 11 probes; "motion": the 140 x 264 plane, 25
probes in 51 frames).  ADM: D_gpu = num[s](frame 0) - num[s](frame k), the float32 cubes are summed per thread and as doubles in a
fixed order per tile from there on; an item whose touched region holds a sample within 2^-20 of the angle test's discontinuity is
held to the interval of its forced-flag runs, widened by the bar (18 items, listed by tests/test_probe_host.py and DESIGN.md).
Motion: D_gpu is sad of the pair (p_k, base); the bar adds the derived fixed-point term, 2^-17 per output the blur reaches.
    ADM plane A     4.56e-7 (1e-5), 3.20e-6 (1e-5), 3.81e-6 (1e-5), 3.17e-5 (8.8e-5) on scales 0 .. 3; nearest to its bar: scale 3,
                    noise, 8 bits, probe (100, 128), 1.51e-5 (2.75e-5)
    ADM plane B     5.40e-6 (1.6e-5), 2.44e-5 (1.0e-4), 1.24e-4 (7.7e-4), 3.61e-5 (9.9e-5): scale 3, noise, 8 bits, probe (0, 56) is
                    the one group of these kinds with a derived margin (23, probe_cases.MARGIN_OF: the float32 noise on D is
                    7e-7 absolute for every probe of the 3 x 7 band and this probe's D is the smallest, 2.3e-2)
    motion          2.69e-7 (1.2e-5)   noise, 16 bits, probe (128, 256); 7.4e-8 on the smooth field
Every equality holds: frame 0 has num = den bit for bit, scale = 1 and adm2 = 1; den[s] is frame 0's on every frame; num[s] is frame
0's bits exactly where D_64 is 0; the planes without a patch return every field of frame 0; sad[2 k] = sad[2 k - 1] bit for bit,
sad[0] = 0 without prev0 and the last probe's bits with it, and the unprobed planes give 0.
"""
import numpy as np
import pytest

import probe_cases as PC
import probe_reference as PR

pytestmark = pytest.mark.gpu

WORST = {}   # (kind, level, content, depth) -> (gap, bar, probe, layout)


def _judge(kind, name, depth, got, lay):
    """got: D_gpu [probes, levels] of a case; every probe the level keeps within the group's bar of D_64 (one of ADM's unsure items:
    of the interval of its forced-flag runs; motion: the bar plus the derived fixed-point term)"""
    want = PR.D64(kind, name, depth)
    pr = PC.probes(PR.base_kind(kind))
    assert got.shape == want.shape, (got.shape, want.shape)
    failed = []
    gaps = PR.gap(kind, name, depth, got)
    slack = np.broadcast_to(PR.slack(kind), want.shape)
    for lv in range(want.shape[1]):
        keep = PR.kept(kind, lv)
        bar = PR.bar(kind, lv, name, depth) + slack[keep, lv] / np.abs(want[keep, lv])
        gap = gaps[keep, lv]
        k = int(np.argmax(gap))
        bar = np.broadcast_to(bar, gap.shape)
        print("%s %s %d bits %s level %d: largest gap %.3e at %s (D_gpu %.6e, D_64 %.6e), bar %.2e" % (
            kind, name, depth, lay, lv, gap[k], pr[keep[k]], got[keep[k], lv], want[keep[k], lv], bar[k]))
        key = (kind, lv, name, depth)
        if key not in WORST or gap[k] > WORST[key][0]:
            WORST[key] = (float(gap[k]), float(bar[k]), pr[keep[k]], lay)
        failed += [(lv, pr[keep[i]], float(gap[i]), float(bar[i])) for i in range(len(keep)) if not gap[i] <= bar[i]]
    assert not failed, failed


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _mode(name):
    from rtvqa_amd import _native as N
    return {"gauss": N.SSIM_GAUSS, "ffmpeg": N.SSIM_FFMPEG, "ms": N.SSIM_MS}[name]


def _check_exact(res, kind, depth, probed):
    """SSE: 0 on frame 0 and on every plane without a patch, the closed form on the probed plane of frame k; the planes without a
    patch return frame 0's SSIM bits"""
    pr = PC.probes(kind)
    shape = PC.plane_of(kind)
    assert (res[0]["sse"] == 0).all()
    want = [PC.sse_of(p, shape, depth) for p in pr]
    assert [int(v) for v in res[1:, probed]["sse"]] == want
    for p in range(res.shape[1]):
        if p != probed:
            assert (res[1:, p]["sse"] == 0).all(), p
            assert (_bits(res[1:, p]["ssim"]) == _bits(res[0, p]["ssim"])).all(), p


def _d_of(values, n):
    """N (value(frame 0) - value(frame k)) for k = 1 ..: values [frames] or [frames, levels], n a scalar or [levels]"""
    return (values[0] - values[1:]) * n


SSIM_CASES = [("gauss",) + c for c in PC.GAUSS_CASES] + [("ffmpeg",) + c for c in PC.FFMPEG_CASES]


@pytest.mark.parametrize("name", PC.CONTENTS)
@pytest.mark.parametrize("kind,lay,depth", SSIM_CASES, ids=["%s-%s-%d" % c for c in SSIM_CASES])
def test_gaussian_ssim_and_vf_ssim(engine, kind, lay, depth, name):
    """Gaussian SSIM: gray at 8, 10, 16 bits; packed BGR24 with the patch in G (three planes in one launch); 4:2:0 at 10 bits with
    the patch in U.  vf_ssim: the five kernels launch_quality_ffmpeg selects, each by its descriptor (probe_cases.FFMPEG_PATHS)"""
    ref, dist, planes, probed = PC.batch(kind, name, depth, lay)
    res = engine.quality(ref, dist, planes, _mode(kind))
    assert res.shape == (ref.shape[0], len(planes))
    _check_exact(res, kind, depth, probed)
    _judge(kind, name, depth, _d_of(res[:, probed]["ssim"], PR.map_samples(kind))[:, None], lay)


@pytest.mark.parametrize("name", PC.CONTENTS)
@pytest.mark.parametrize("depth", PC.DEPTHS["ms"])
def test_msssim_levels(engine, depth, name):
    """every level's cs and ssim mean of the 352 x 528 plane; level 0 is Gaussian SSIM's value bit for bit"""
    ref, dist, planes, probed = PC.batch("ms", name, depth)
    res, cs, ssim = engine.quality(ref, dist, planes, _mode("ms"), scales=True)
    assert cs.shape == ssim.shape == (ref.shape[0], 1, PC.MS_LEVELS)
    _check_exact(res, "ms", depth, probed)
    single = engine.quality(ref, dist, planes, _mode("gauss"))
    assert np.ascontiguousarray(ssim[:, :, 0]).tobytes() == np.ascontiguousarray(single["ssim"]).tobytes()
    assert np.ascontiguousarray(res["sse"]).tobytes() == np.ascontiguousarray(single["sse"]).tobytes()
    n = np.array([PR.map_samples("ms", lv) for lv in range(PC.MS_LEVELS)], np.float64)
    _judge("ms-cs", name, depth, _d_of(cs[:, 0], n), "gray")
    _judge("ms-ssim", name, depth, _d_of(ssim[:, 0], n), "gray")


@pytest.mark.parametrize("name", PC.CONTENTS)
@pytest.mark.parametrize("depth", PC.DEPTHS["vif"])
def test_vif_levels(engine, depth, name):
    """num[s] of all four levels; den[s] is a function of ref alone: frame 0's bits on every frame"""
    ref, dist, planes, probed = PC.batch("vif", name, depth)
    got = engine.vif(ref, dist, planes)
    assert got.shape == (ref.shape[0], 1)
    den = _bits(got[:, 0]["den"])
    assert den.shape == (ref.shape[0], PC.VIF_LEVELS) and (den == den[0]).all(), np.nonzero(den != den[0])
    _judge("vif", name, depth, _d_of(np.ascontiguousarray(got[:, 0]["num"]), 1.0), "gray")


def test_one_long_strip_gives_the_probe_frames_the_same_bits(engine):
    """the Gaussian gray 8-bit batch again with frame 0 repeated until n * planes * column blocks reaches 6144: ssim_strips stops
    taking the cap of two strips and gives one strip of 144 rows per plane - the geometry a 1080p batch runs and no small test
    reaches.  The 2^-27 sums are associative: every record of the small batch comes back bit for bit"""
    ref, dist, planes, _probed = PC.batch("gauss", "noise", 8)
    small = engine.quality(ref, dist, planes, _mode("gauss"))
    n = 6144 // 2
    pad = np.repeat(ref[:1], n - ref.shape[0], axis=0)
    big = engine.quality(np.concatenate([ref, pad]), np.concatenate([dist, pad]), planes, _mode("gauss"))
    assert big.shape == (n, 1)
    assert big[:ref.shape[0]].tobytes() == small.tobytes()
    assert (_bits(big[ref.shape[0]:]["ssim"]) == _bits(small[0, 0]["ssim"])).all() and (big[ref.shape[0]:]["sse"] == 0).all()


ADM_CASES = [(plane,) + c for plane in ("adm", "adm-b") for c in PC.ADM_CASES]


@pytest.mark.parametrize("name", PC.CONTENTS)
@pytest.mark.parametrize("plane,lay,depth", ADM_CASES, ids=["%s-%s-%d" % c for c in ADM_CASES])
def test_adm_scales(engine, plane, lay, depth, name):
    """num[s] of all four scales on plane A (320 x 640: tile seams inside every scale's pooled region) and plane B (48 x 112: the
    band's edge is pooled); gray at 8 and 10 bits - k_adm_scale<uint8_t> and <uint16_t>, <float> above scale 0 - and packed BGR24
    with the patch in G, three planes in one group.  What follows exactly from the kernel's fixed orders is asserted as it is"""
    ref, dist, planes, probed = PC.batch(plane, name, depth, lay)
    got = engine.adm(ref, dist, planes)
    assert got.shape == (ref.shape[0], len(planes))
    want = PR.D64(plane, name, depth)
    for p in range(len(planes)):
        g = got[:, p]
        # identical planes: num = den bit for bit; den is a function of ref alone
        assert (_bits(g[0]["num"]) == _bits(g[0]["den"])).all() and (g[0]["scale"] == 1.0).all() and g[0]["adm2"] == 1.0, p
        assert (_bits(g["den"]) == _bits(g[0]["den"])).all(), (p, np.nonzero(_bits(g["den"]) != _bits(g[0]["den"])))
        if p != probed:       # the planes without a patch: every field of frame 0
            assert all(g[k].tobytes() == g[0].tobytes() for k in range(1, g.shape[0])), p
    num = np.ascontiguousarray(got[:, probed]["num"])
    same = _bits(num[1:]) == _bits(num[0])
    assert same[want == 0].all(), np.nonzero(~same & (want == 0))       # the patch reaches no pooled sample of the scale
    assert not same[want != 0].any()
    _judge(plane, name, depth, num[0] - num[1:], lay)


@pytest.mark.parametrize("name", PC.CONTENTS)
@pytest.mark.parametrize("lay,depth", PC.MOTION_CASES, ids=["%s-%d" % c for c in PC.MOTION_CASES])
def test_motion_pairs(engine, lay, depth, name):
    """base, p_1, base, p_2, .., base: sad[2 k - 1] is the pair (p_k, base) and sad[2 k] the same pair reversed - the same |d| per
    sample, the same integers; the outputs the blur of the patch does not reach add 0 to both"""
    frames, planes, probed = PC.motion_batch(name, depth, lay)
    got = engine.motion(frames, planes)
    assert got.shape == (frames.shape[0], len(planes))
    sad = np.ascontiguousarray(got[:, probed]["sad"])
    assert (got[0]["sad"] == 0.0).all() and (got[0]["motion"] == 0.0).all()      # no predecessor
    assert (_bits(sad[2::2]) == _bits(sad[1::2])).all(), np.nonzero(sad[2::2] != sad[1::2])
    for p in range(len(planes)):
        if p != probed:       # every frame of the planes without a patch is the same frame
            assert (got[:, p]["sad"] == 0.0).all(), p
    first = engine.motion(frames[:1], planes, prev0=frames[-2])                  # base after the last probe's frame
    assert _bits(first[0, probed]["sad"]) == _bits(sad[-1]) and first[0, probed]["sad"] > 0.0
    _judge("motion", name, depth, sad[1::2][:, None], lay)


def test_the_worst_gaps():
    """the figures DESIGN.md section 3 records: the largest gap of every kind and level over contents, depths and layouts"""
    for kind in ("gauss", "ffmpeg", "ms-cs", "ms-ssim", "vif", "adm", "adm-b", "motion"):
        for lv in sorted({k[1] for k in WORST if k[0] == kind}):
            key = max((k for k in WORST if k[0] == kind and k[1] == lv), key=lambda k: WORST[k][0] / WORST[k][1])
            gap, bar, probe, lay = WORST[key]
            print("probe parity: %s level %d largest gap %.3e (bar %.2e) at %s, %s %d bits %s" % (kind, lv, gap, bar, probe, key[2], key[3], lay))
            assert gap <= bar
