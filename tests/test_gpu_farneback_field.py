"""Farneback on the device, judged per pixel (cases, bars, seam table and checks: tests/farneback_field_cases.py; the reference's own
distance and the teeth of the checks: tests/test_farneback_field_host.py).

  expansions   every level, every plane, all five coefficients: the oracle's BITS (k_fb_level3<1> / <2>, k_fb_level<2,64>,
               k_fb_level<2,16> and k_fb_polyexp_march at every seam; the three-kernel fallback in a child process);
  flow         every pair, pixel and component within bar(case) = 4 e(case) of the C oracle, no pixel excluded;
  consistency  flow_mag_mean is the fixed-point sum of the field read back, exactly; the field is the same bytes with the overlap
               option on and off, and alone or inside a larger batch that is cut into other strips."""
import os
import subprocess
import sys

import numpy as np
import pytest

import farneback_field_cases as fc

pytestmark = pytest.mark.gpu
REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = fc.cases()
FLOW_CASES = [c for c in CASES if fc.judged_on_flow(c)]


def _levels(shape):
    return range(fc.levels_of(*shape) + 1)


def _submit(eng, frames):
    from rtvqa_amd import _native as N
    return eng.complexity(frames[1:], prev0=frames[0], mask=N.M_MOTION, motion_mode=N.MOTION_FARNEBACK)


def _read_all(eng, shape, pairs):
    flows = np.stack([eng.debug_farneback_flow(p, *shape) for p in range(pairs)])
    exps = {(q, k): eng.debug_farneback_expansion(q, k, *fc.level_size(shape[0], shape[1], k)) for q in range(pairs + 1) for k in _levels(shape)}
    return flows, exps


_RUNS = {}


@pytest.fixture
def run(engine):
    """one submit per case for the whole module: -> (records, flow [pairs][h][w][2], {(plane, level): expansion [lh][lw][5]})"""
    def get(case):
        if case not in _RUNS:
            rec = _submit(engine, fc.bgr_frames(case))
            _RUNS[case] = (rec,) + _read_all(engine, case[0], fc.PAIRS)
        return _RUNS[case]
    return get


@pytest.mark.parametrize("case", CASES, ids=fc.case_id)
def test_expansions_are_the_oracles_bits(run, case):
    """'the float planes (blurred images, expansions, products) are bit-identical to the oracle's' (k_farneback.hip): every level,
    each of the three planes, all five coefficient planes, bit for bit"""
    shape = case[0]
    exps = run(case)[2]
    for k in _levels(shape):
        kernels = (fc.level_kernel(fc.PLANES, shape[0], shape[1], k)[0], "k_fb_polyexp_march")
        for q in range(fc.PLANES):
            got, want = exps[(q, k)], fc.expansion_c(case, q, k)
            d = fc.first_difference(got, want)
            if d is not None:
                y, x, c = d
                n = int((got.view(np.uint32) != want.view(np.uint32)).sum())
                pytest.fail("%s: level %d (%s), plane %d, coefficient %d: first of %d differing values at %s: device %r, oracle %r"
                            % (fc.case_id(case), k, kernels[0], q, c, n, fc.describe(shape, k, y, x, kernels), got[y, x, c], want[y, x, c]))


@pytest.mark.parametrize("case", FLOW_CASES, ids=fc.case_id)
def test_flow_field_is_within_the_references_own_distance(run, case):
    """|flow_gpu - flow_C| <= bar = 4 e at every pixel of every pair, both components (floored at the float32 spacing of the case's
    largest component, never above 1e-4): the device's known deviations - column sums restarted every 16 rows, the horizontal order -
    are far below the reference's float32-to-float64 distance e, and a wrong seam column is 1e-2."""
    shape = case[0]
    flows = run(case)[1]
    want = fc.flow_c(case)[0]
    bar = fc.bar_of(case)
    worst = max((fc.flow_gap(flows[p], want[p]) + (p,) for p in range(fc.PAIRS)), key=lambda t: t[0])
    gap, (y, x, comp), p = worst
    over = int((np.abs(flows.astype(np.float64) - want) > bar).sum())
    print("\n%s: largest |gpu - C| = %.3g (bar %.3g, e %.3g) at pair %d, component %d, %s" % (fc.case_id(case), gap, bar, fc.e_of(case), p, comp,
                                                                                        fc.describe(shape, 0, y, x, ("k_fb_iter", "k_fb_upflow"))))
    assert np.isfinite(flows).all()
    assert gap <= bar, "%d values over the bar; the largest, %.3g against %.3g, at pair %d component %d, %s" % (
        over, gap, bar, p, comp, fc.describe(shape, 0, y, x, ("k_fb_iter", "k_fb_upflow")))


@pytest.mark.parametrize("case", CASES, ids=fc.case_id)
def test_flow_mag_mean_is_the_fixed_point_sum_of_the_field(run, case):
    """EXACT: the record's flow_mag_mean equals the mean of the field read back when formed as k_fb_iter and k_fb_mag_finalize form
    it - float32 magnitudes, each rounded to 2^-28 fixed point, summed as integers (tests/farneback_field_cases.fixed_point_mean)"""
    rec, flows, _ = run(case)
    for p in range(fc.PAIRS):
        want, total = fc.fixed_point_mean(flows[p])
        got = float(rec[p]["flow_mag_mean"])
        assert got == want, (fc.case_id(case), p, got, want, round((got - want) * flows[p].shape[0] * flows[p].shape[1] * 2.0 ** 28))
        assert got > 0


@pytest.mark.parametrize("case", [((264, 520), "pan"), ((263, 519), "noise"), ((70, 500), "pan2"), ((9, 9), "noise")], ids=fc.case_id)
def test_field_is_the_same_bytes_with_the_overlap_option_on_and_off(engine, run, case):
    """the piped mode forms the expansions on a side stream; the read-back waits for it.  Flow and expansions: the same bytes"""
    from rtvqa_amd import _native as N
    keep = engine.get_option(N.OPT_OVERLAP)
    got = {}
    try:
        for on in (True, False):
            engine.set_overlap(on)
            rec = _submit(engine, fc.bgr_frames(case))
            got[on] = (rec["flow_mag_mean"].tobytes(),) + _read_all(engine, case[0], fc.PAIRS)
    finally:
        engine.set_overlap(bool(keep))
    base = run(case)
    for on in (True, False):
        assert got[on][0] == base[0]["flow_mag_mean"].tobytes(), on
        assert got[on][1].tobytes() == base[1].tobytes(), on
        for key, r in base[2].items():
            assert got[on][2][key].tobytes() == r.tobytes(), (on, key)


@pytest.mark.parametrize("pairs", [fc.NINE_PAIRS, fc.MANY_PAIRS])
def test_field_of_a_pair_does_not_depend_on_the_batch(engine, run, pairs):
    """the same pair alone, in the 2-pair case and inside a larger batch: the same bytes.  The frames of the larger batch cycle
    through the case's three, so its pair i is the case's pair i % 3 for i % 3 < 2.  With 44 pairs k_fb_iter marches 5 strips of
    64 rows where the small batches march 6 of 48 (tests/test_farneback_field_host.py asserts the geometry)."""
    case = ((264, 520), "pan")
    shape = case[0]
    fr = fc.bgr_frames(case)
    base_rec, base_flows, base_exps = run(case)
    rec = _submit(engine, fr[:2])
    assert rec["flow_mag_mean"].tobytes() == base_rec["flow_mag_mean"][:1].tobytes()
    assert engine.debug_farneback_flow(0, *shape).tobytes() == base_flows[0].tobytes()
    big = np.stack([fr[i % 3] for i in range(pairs + 1)])
    rec = _submit(engine, big)
    for i in (0, 1, 3, pairs - 2, pairs - 1):
        if i % 3 == 2:
            continue
        assert float(rec[i]["flow_mag_mean"]) == float(base_rec[i % 3]["flow_mag_mean"]), i
        assert engine.debug_farneback_flow(i, *shape).tobytes() == base_flows[i % 3].tobytes(), i
    for q in (0, 4, pairs):
        for k in _levels(shape):
            got = engine.debug_farneback_expansion(q, k, *fc.level_size(shape[0], shape[1], k))
            assert got.tobytes() == base_exps[(q % 3, k)].tobytes(), (q, k)


_FALLBACK_CODE = (
    "import sys, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
    "import rtvqa_amd\n"
    "from rtvqa_amd import _native as N\n"
    "import farneback_field_cases as fc\n"
    "case = ((263, 519), 'pan')\n"
    "shape = case[0]\n"
    "fr = fc.bgr_frames(case)\n"
    "with rtvqa_amd.Engine(0) as eng:\n"
    "    assert eng.lib.vqa_build_flavour() & N.FLAVOUR_AB_VARIANTS\n"
    "    rec = eng.complexity(fr[1:], prev0=fr[0], mask=N.M_MOTION, motion_mode=N.MOTION_FARNEBACK)\n"
    "    out = {'mean': rec['flow_mag_mean'], 'flow': np.stack([eng.debug_farneback_flow(p, *shape) for p in range(fc.PAIRS)])}\n"
    "    for q in range(fc.PLANES):\n"
    "        for k in range(fc.levels_of(*shape) + 1):\n"
    "            out['R%%d_%%d' %% (q, k)] = eng.debug_farneback_expansion(q, k, *fc.level_size(shape[0], shape[1], k))\n"
    "np.savez(sys.argv[1], **out)\n"
    "print('FALLBACK-OK')\n"
)


def test_three_kernel_fallback_expansions_are_the_oracles_bits(run, tmp_path):
    """k_fb_blur_h, k_fb_blur_v and k_fb_resize<1> ship, but are reached only when a level's patch overflows the LDS budget.  The
    lab build takes them at every level with VQA_FB_LEVEL_VARIANT=1 (a fresh child process: the knob is read there): on 263 x 519,
    whose level 1 is bilinear, the expansions are the oracle's bits and the flow field the fused path's bytes."""
    from rtvqa_amd import _native as N
    case = ((263, 519), "pan")
    env = dict(os.environ, VQA_LIB_PATH=N.LAB_LIB_PATH, VQA_FB_LEVEL_VARIANT="1")
    out = str(tmp_path / "fallback.npz")
    r = subprocess.run([sys.executable, "-c", _FALLBACK_CODE % (REPO_ROOT, os.path.join(REPO_ROOT, "tests")), out], env=env,
                       capture_output=True, text=True, timeout=300, cwd=REPO_ROOT)
    assert r.returncode == 0 and "FALLBACK-OK" in r.stdout, (r.stdout[-300:], r.stderr[-1500:])
    got = np.load(out)
    for q in range(fc.PLANES):
        for k in _levels(case[0]):
            d = fc.first_difference(got["R%d_%d" % (q, k)], fc.expansion_c(case, q, k))
            assert d is None, "level %d, plane %d, coefficient %d: first difference at %s" % (k, q, d[2], fc.describe(case[0], k, d[0], d[1]))
    base = run(case)
    assert got["flow"].tobytes() == base[1].tobytes() and got["mean"].tobytes() == base[0]["flow_mag_mean"].tobytes()


def test_read_back_states_and_arguments():
    """VQA_ERR_STATE while nothing valid is resident (before the first Farneback submit, after vqa_trim), VQA_ERR_INVALID on wrong
    dimensions and indices; a block-SAD submit in between leaves the record alone"""
    import rtvqa_amd
    from rtvqa_amd import _native as N
    case = ((97, 131), "pan")
    (h, w), fr = case[0], fc.bgr_frames(case)
    lh, lw = fc.level_size(h, w, 1)

    def status(eng, which, index, level, dh, dw):
        buf = np.zeros(5 * h * w, np.float32)
        return eng.lib.vqa_debug_read_farneback(eng.ctx, which, index, level, buf.ctypes.data, dh, dw)

    with rtvqa_amd.Engine(0) as eng:
        assert status(eng, 0, 0, 0, h, w) == N.VQA_ERR_STATE
        eng.complexity(fr[1:], prev0=fr[0], mask=N.M_MOTION)                       # block-SAD: still nothing
        assert status(eng, 0, 0, 0, h, w) == N.VQA_ERR_STATE
        _submit(eng, fr)
        assert status(eng, 0, 0, 0, h, w) == status(eng, 0, 1, 0, h, w) == N.VQA_OK
        assert status(eng, 1, 2, 1, lh, lw) == status(eng, 1, 0, 0, h, w) == N.VQA_OK
        for args in ((0, 2, 0, h, w), (0, -1, 0, h, w), (1, 3, 0, h, w), (1, -1, 0, h, w),     # a pair / plane the chunk does not hold
                     (0, 0, 0, w, h), (0, 0, 0, h, w + 1), (1, 0, 1, h, w), (1, 0, 1, lh + 1, lw),  # dimensions that are not the level's
                     (1, 0, 2, lh // 2, lw // 2), (1, 0, -1, h, w), (0, 0, 1, lh, lw),          # a level the pyramid (or the flow) lacks
                     (2, 0, 0, h, w), (-1, 0, 0, h, w)):
            assert status(eng, *args) == N.VQA_ERR_INVALID, args
        assert eng.lib.vqa_debug_read_farneback(eng.ctx, 0, 0, 0, None, h, w) == N.VQA_ERR_INVALID
        flow = eng.debug_farneback_flow(1, h, w)
        eng.complexity(fr[1:], prev0=fr[0], mask=N.M_MOTION)                       # block-SAD does not touch Farneback's buffers
        assert eng.debug_farneback_flow(1, h, w).tobytes() == flow.tobytes()
        eng.complexity(fr[1:], mask=N.M_MOTION, motion_mode=N.MOTION_FARNEBACK)    # no prev0: pair 0 and plane 0 do not exist
        assert status(eng, 0, 0, 0, h, w) == status(eng, 1, 0, 0, h, w) == N.VQA_ERR_INVALID
        assert status(eng, 0, 1, 0, h, w) == status(eng, 1, 1, 0, h, w) == N.VQA_OK
        assert eng.debug_farneback_flow(1, h, w).tobytes() == flow.tobytes()
        eng.trim()
        assert status(eng, 0, 1, 0, h, w) == N.VQA_ERR_STATE
