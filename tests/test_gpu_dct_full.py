"""GPU: full-frame DCT parity at every size class of its three implementations (tests/dct_full_cases.py has the planes, the
contents, the probe frames and path_of(), the restated dispatch; tests/test_dct_full_host.py shows on the CPU that every class has
a case, that the float64 reference is stable and that each probe has teeth).

dct_energy and temporal_dct_l1 of every frame against scipy.fft.dctn(norm="ortho") in float64 on the same gray plane, at the
project's bar of 1e-4 relative, through engine.complexity:
  * the vector-ALU products with a side of 128 or more (64 x 1920, 1080 x 64, 100 x 500) and on either side of
    h >= 128 && w >= 128 (127 x 128, 128 x 127 | 128 x 129);
  * the MFMA products on odd sides: an odd lda (three rows in four off load8's 16-byte alignment), K % 16 = 1, last tiles one
    sample wide (257 x 385), and 255 x 129 as the frame's own size;
  * the FFT passes on either side of w = 2048 (256 | 512 threads), of h = 1152 | 1200 (the two slab classes) and of
    h = 2000 | 2048 (the last slab, the pair kernel's first), at the longest transform (4000 points) both ways, at the plans
    without a radix-8 or radix-4 pass (1458 = 2 * 3^6, seven passes; 1250 = 2 * 5^4) and at ragged work splits.
Energy alone, temporal alone and both return the same bits; a batch without prev0 returns 0.0 and has_prev = 0 first and the
same bits after; AUTO is FULL at 64 x 256 and the 8 x 8 metric at 64 x 258; device frames give the host frames' bits.

dct_energy equals sum gray^2 for any orthogonal transform, right or wrong, and L1 on natural frames spreads over all coefficients,
so one plane of each path and class also runs probe frames on a noise base: single pixels (a dense spectrum: how each input
sample is weighted; also against the closed form 40 S_h(y) S_w(x)) and quantised cosines (a nearly single coefficient: that
frequency's twiddles).  The pair (p_k, base) and its reverse give the same bits.

test_the_worst_gaps prints the largest gap per path and class; DESIGN.md section 3, "full-frame DCT parity", records them."""
import numpy as np
import pytest

import dct_full_cases as DC

pytestmark = pytest.mark.gpu

WORST = {}      # (class, what) -> (gap, where)
_RUNS = {}


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _classes(path):
    return [path] if isinstance(path, str) else ["fft " + path[1], "fft " + path[2]]


def _note(path, what, gap, where):
    for cls in _classes(path):
        if (cls, what) not in WORST or gap > WORST[(cls, what)][0]:
            WORST[(cls, what)] = (float(gap), where)


def _kw(c):
    from rtvqa_amd import _native as N
    return dict(dct_mode=N.DCT_FULL) if c.native else dict(dct_mode=N.DCT_FULL, resize=(c.w, c.h))


def _run(engine, c):
    """the runs of a case, once: both metrics with the histogram's sum_gray2, each metric alone, both, and the four frames
    without prev0"""
    from rtvqa_amd import _native as N
    key = DC.case_id(c)
    if key not in _RUNS:
        fr = DC.clip(c.h, c.w, c.native)
        kw = _kw(c)
        both = N.M_DCT | N.M_TEMPORAL_DCT
        _RUNS[key] = {
            "hist": engine.complexity(fr[1:], prev0=fr[0], mask=both | N.M_GRAY_HIST, **kw),
            "energy": engine.complexity(fr[1:], prev0=fr[0], mask=N.M_DCT, **kw),
            "temporal": engine.complexity(fr[1:], prev0=fr[0], mask=N.M_TEMPORAL_DCT, **kw),
            "both": engine.complexity(fr[1:], prev0=fr[0], mask=both, **kw),
            "no_prev0": engine.complexity(fr, mask=both, **kw),
        }
    return _RUNS[key]


@pytest.mark.parametrize("case", DC.CASES, ids=DC.case_id)
def test_parity_on_the_natural_content(engine, case):
    assert DC.path_of(case.h, case.w) == case.path
    run = _run(engine, case)
    rec = run["hist"]
    g = DC.planes_of(case)
    failed = []
    for i in range(DC.FRAMES):
        e, l1 = DC.energy(g[i + 1]), DC.l1(g[i], g[i + 1])
        ge, gl = DC.rel(float(rec[i]["dct_energy"]), e), DC.rel(float(rec[i]["temporal_dct_l1"]), l1)
        gp = DC.rel(float(rec[i]["dct_energy"]), float(rec[i]["sum_gray2"]))
        print("%s (%s) frame %d: energy gap %.3e, Parseval %.3e, L1 gap %.3e" % (DC.case_id(case), case.path, i, ge, gp, gl))
        _note(case.path, "energy", ge, DC.case_id(case))
        _note(case.path, "L1, natural", gl, DC.case_id(case))
        assert int(rec[i]["sum_gray2"]) == int((g[i + 1].astype(np.int64) ** 2).sum())
        assert rec[i]["has_prev"] == 1
        failed += [(i, what, gap) for what, gap in (("energy", ge), ("Parseval", gp), ("L1", gl)) if not gap < DC.RTOL]
    assert not failed, failed
    # without prev0: the first temporal sample is 0 and flagged, every later one and every energy has the first batch's bits
    nop, both = run["no_prev0"], run["both"]
    assert float(nop[0]["temporal_dct_l1"]) == 0.0 and nop[0]["has_prev"] == 0
    assert DC.rel(float(nop[0]["dct_energy"]), DC.energy(g[0])) < DC.RTOL
    assert (nop[1:]["has_prev"] == 1).all()
    assert (_bits(nop[1:]["dct_energy"]) == _bits(both["dct_energy"])).all()
    assert (_bits(nop[1:]["temporal_dct_l1"]) == _bits(both["temporal_dct_l1"])).all()


@pytest.mark.parametrize("case", DC.CASES, ids=DC.case_id)
def test_a_metric_alone_returns_the_bits_it_has_beside_the_other(engine, case):
    """which[] / the grid's z / plane_b of the FFT kernels and the two launch pairs of the products: the partials and their
    reduction order do not depend on the mask"""
    run = _run(engine, case)
    both = run["both"]
    assert (_bits(run["energy"]["dct_energy"]) == _bits(both["dct_energy"])).all()
    assert (_bits(run["temporal"]["temporal_dct_l1"]) == _bits(both["temporal_dct_l1"])).all()
    assert (_bits(run["hist"]["dct_energy"]) == _bits(both["dct_energy"])).all()
    assert (_bits(run["hist"]["temporal_dct_l1"]) == _bits(both["temporal_dct_l1"])).all()
    # the metric that was not asked for stays 0
    assert (run["energy"]["temporal_dct_l1"] == 0.0).all() and (run["temporal"]["dct_energy"] == 0.0).all()
    assert (both["dct_energy"] > 0).all() and (both["temporal_dct_l1"] > 0).all()


@pytest.mark.parametrize("h,w", DC.PROBED, ids=lambda v: str(v))
def test_probe_frames(engine, h, w):
    from rtvqa_amd import _native as N
    path = DC.path_of(h, w)
    pr = DC.probes(h, w)
    fr = DC.probe_batch(h, w)
    rec = engine.complexity(fr[1:], prev0=fr[0], mask=N.M_DCT | N.M_TEMPORAL_DCT | N.M_GRAY_HIST, dct_mode=N.DCT_FULL)
    alone = engine.complexity(fr[1:], prev0=fr[0], mask=N.M_TEMPORAL_DCT, dct_mode=N.DCT_FULL)
    assert (_bits(alone["temporal_dct_l1"]) == _bits(rec["temporal_dct_l1"])).all()
    base = DC.base_plane(h, w)
    e_base = DC.energy(base)
    failed = []
    for k, probe in enumerate(pr):
        p = DC.probe_plane(h, w, probe)
        want = float(np.abs(DC.dct2(p - base)).sum())
        got, back = float(rec[2 * k]["temporal_dct_l1"]), float(rec[2 * k + 1]["temporal_dct_l1"])
        gap = DC.rel(got, want)
        _note(path, "L1, %s" % probe[0], gap, "%dx%d %s" % (h, w, probe[1]))
        line = "%d x %d (%s) %s %s: L1 %.6e, float64 %.6e, gap %.3e" % (h, w, path, probe[0], probe[1], got, want, gap)
        if not gap < DC.RTOL:
            failed.append(("L1", probe, gap))
        if _bits(got) != _bits(back):
            failed.append(("the reversed pair", probe, got, back))
        if probe[0] == "impulse":
            closed = DC.IMPULSE * DC.basis_l1(h)[probe[1][0]] * DC.basis_l1(w)[probe[1][1]]
            line += ", closed form %.6e (%.3e)" % (closed, DC.rel(got, closed))
            if not DC.rel(got, closed) < DC.RTOL:
                failed.append(("closed form", probe, got, closed))
        print(line)
        # the energies: the probe frame's, and the base's after it
        ge = DC.rel(float(rec[2 * k]["dct_energy"]), DC.energy(p))
        gb = DC.rel(float(rec[2 * k + 1]["dct_energy"]), e_base)
        _note(path, "energy", max(ge, gb), "%dx%d %s" % (h, w, probe[1]))
        if not (ge < DC.RTOL and gb < DC.RTOL):
            failed.append(("energy", probe, ge, gb))
        if not DC.rel(float(rec[2 * k]["dct_energy"]), float(rec[2 * k]["sum_gray2"])) < DC.RTOL:
            failed.append(("Parseval", probe))
        assert int(rec[2 * k]["sum_gray2"]) == int((p ** 2).sum())
    assert not failed, failed
    # every base frame is the same plane: one energy, bit for bit
    assert len({int(b) for b in _bits(rec[1::2]["dct_energy"])}) == 1


def test_auto_picks_full_up_to_128_x_128_samples_and_the_block_metric_above(engine):
    from rtvqa_amd import _native as N
    mask = N.M_DCT | N.M_TEMPORAL_DCT
    for (h, w), full in (((64, 256), True), ((64, 258), False)):
        assert DC.auto_is_full(h, w) == full
        fr = DC.clip(h, w)
        rec = {m: engine.complexity(fr[1:], prev0=fr[0], mask=mask, resize=(w, h), dct_mode=m) for m in (N.DCT_AUTO, N.DCT_FULL, N.DCT_BLOCK8)}
        same = N.DCT_FULL if full else N.DCT_BLOCK8
        other = N.DCT_BLOCK8 if full else N.DCT_FULL
        assert (_bits(rec[N.DCT_AUTO]["temporal_dct_l1"]) == _bits(rec[same]["temporal_dct_l1"])).all(), (h, w)
        assert (_bits(rec[N.DCT_AUTO]["dct_energy"]) == _bits(rec[same]["dct_energy"])).all(), (h, w)
        assert (rec[N.DCT_AUTO]["temporal_dct_l1"] != rec[other]["temporal_dct_l1"]).all(), (h, w)     # a different metric


@pytest.mark.parametrize("h,w", [(135, 241), (150, 162)], ids=lambda v: str(v))
def test_device_frames_give_the_host_frames_bits(engine, h, w):
    """one odd MFMA plane and one FFT plane"""
    from rtvqa_amd import _native as N
    c = next(c for c in DC.CASES if (c.h, c.w) == (h, w))
    assert c.path == ("mfma" if h == 135 else ("fft", "rows<2048,256>", "cols8<1152>"))
    fr = DC.clip(h, w)
    host = _run(engine, c)["both"]
    dev, prev = engine.upload(fr[1:]), engine.upload(fr[:1])
    got = engine.complexity(dev, prev0=prev, mask=N.M_DCT | N.M_TEMPORAL_DCT, **_kw(c))
    assert (_bits(got["dct_energy"]) == _bits(host["dct_energy"])).all()
    assert (_bits(got["temporal_dct_l1"]) == _bits(host["temporal_dct_l1"])).all()


def test_the_worst_gaps():
    """runs after the parity tests of this module (pytest keeps the file's order): the figures DESIGN.md section 3 records"""
    classes = ["valu", "mfma", "fft rows<2048,256>", "fft rows<4096,512>", "fft cols8<1152>", "fft cols8<2048>", "fft cols<false>"]
    for cls in classes:
        for what in ("energy", "L1, natural", "L1, impulse", "L1, cosine"):
            assert (cls, what) in WORST, (cls, what)
            gap, where = WORST[(cls, what)]
            print("full-frame DCT parity: %-18s %-12s largest gap %.3e at %s" % (cls, what, gap, where))
            assert gap < DC.RTOL
