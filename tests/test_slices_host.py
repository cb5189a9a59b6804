"""The slice-seam content on the host side (no GPU): tests/slice_cases.py's pool and index maps against a brute-force
restatement; the shipped library has no VQA_QSLICE seam, so far as that shows without a GPU; and every pool entry at every layout
is a fair test of the kernels and not of fp32 itself - for every (entry, depth, metric) tests/test_gpu_slices.py compares with a
reference that has a float32 run of its own, that run stays within half the GPU bar of the float64 run (the method of
tests/test_hostile_host.py).  What fails is left out by name in slice_cases.EXCLUDED, at most two of the seven entries per metric
and depth; the five natural entries pass for every metric."""
import os
import subprocess
import sys

import numpy as np
import pytest

import adm_reference as A
import ciede_reference as CR
import hbd_reference as H
import hostile_cases as K
import msssim_reference as M
import psnr_hvs_reference as P
import slice_cases as SC
import vif_reference as V

HALF = 5e-5
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_pool_is_seven_entries_per_plane_at_the_planes_own_size():
    assert SC.POOL[5:] == ("checker_inv", K.ENDS) and all(n.startswith("natural") for n in SC.POOL[:5]) and len(set(SC.POOL)) == 7
    for chroma, h, w, depth in SC.SMALL + SC.BIG + (SC.SMALL_BGR, SC.BIG_CIEDE):
        r, d, planes = SC.pool(chroma, h, w, depth)
        r2, d2, _ = SC.pool(chroma, h, w, depth)
        assert r.tobytes() == r2.tobytes() and d.tobytes() == d2.tobytes()            # seeded
        assert r.shape[0] == 7 and r.dtype == (np.uint16 if depth > 8 else np.uint8) and r.max() <= (1 << depth) - 1
        assert len({r[e].tobytes() for e in range(7)}) == 7 and len({d[e].tobytes() for e in range(7)}) == 7
        for e, name in enumerate(SC.POOL):
            for k, p in enumerate(planes):
                want = SC.entry_pair(name, p[1], p[0], depth, k)
                assert (K.plane_of(r[e], p) == want[0]).all() and (K.plane_of(d[e], p) == want[1]).all(), (chroma, name, k)
    r, d, planes = SC.pool("420", 67, 99, 8)
    assert [(p[0], p[1]) for p in planes] == [(99, 67), (50, 34), (50, 34)]
    L = 255
    assert (K.plane_of(r[5], planes[0]) + K.plane_of(d[5], planes[0]) == L).all()       # the checkerboard against its inverse
    assert (r[6] == L).all() and (d[6] == 0).all()                                   # the ends of the range


def test_the_index_maps_against_a_brute_force_restatement():
    """which records of a batch must be equal, from the frames' own bytes: a pair record is a function of (ref i, dist i), a
    temporal record of (frame i - 1 or prev0 or nothing, frame i)"""
    r, d, _ = SC.pool("mono", 16, 16, 8)
    for n in SC.SMALL_NS + (30, 71):
        br, bd = SC.batch(r, n), SC.batch(d, n)
        assert br.shape[0] == n and br.flags["C_CONTIGUOUS"]
        key = [(br[i].tobytes(), bd[i].tobytes()) for i in range(n)]
        first = {}
        for i in range(n):
            first.setdefault(key[i], i)
            assert first[key[i]] == SC.pair_source(i) == SC.pair_map(n)[i], i
        for e0 in (None, 6, 2):           # prev0: none, pool entry 6, another entry
            p0 = None if e0 is None else r[e0].tobytes()
            tkey = [((br[i - 1].tobytes() if i else p0), br[i].tobytes()) for i in range(n)]
            first = {}
            for i in range(n):
                first.setdefault(tkey[i], i)
                src = SC.temporal_source(i)
                assert src == SC.temporal_map(n)[i] and tkey[src] == tkey[i], i
                if i >= 8:
                    assert src == SC.temporal_source(i - 7) and tkey[i] == tkey[i - 7]
                # the map merges everything that is equal, but for record 7 (and its repeats) when prev0 is pool entry 6
                if first[tkey[i]] != src:
                    assert e0 == 6 and src == 7 and first[tkey[i]] == 0, (i, src)
            if n > 7:
                assert (tkey[7] == tkey[0]) == (e0 == 6)
    # the seam falls inside a period, at the shipped constant and at the lab value
    assert 32768 % SC.PERIOD == 1 and 3 % SC.PERIOD == 3 and SC.BIG_N == 32768 + 3
    assert SC.pair_source(32768) == 1 and SC.temporal_source(32768) == 1 == SC.temporal_source(32768 - 7)


def test_the_shipped_library_has_no_slice_seam():
    """VQA_QSLICE is read by the lab build alone: the shipped library does not hold the name, the lab library does; and a child
    process loads the shipped library with an absurd VQA_QSLICE in its environment as it does without one (without a GPU
    vqa_create fails for want of a device either way - tests/test_gpu_slices.py runs the shipped library with the variable set)."""
    from rtvqa_amd import _native as N
    assert b"VQA_QSLICE" not in open(N.LIB_PATH, "rb").read()
    assert b"VQA_QSLICE" in open(N.LAB_LIB_PATH, "rb").read()
    code = ("import sys, ctypes as C; sys.path.insert(0, %r)\n"
            "from rtvqa_amd import _native as N\n"
            "lib = N.load()\n"
            "ctx = C.c_void_p()\n"
            "print('FLAVOUR', lib.vqa_build_flavour(), 'CREATE', lib.vqa_create(0, C.byref(ctx)))\n" % REPO)
    outs = []
    for q in (None, "-5", "99999"):
        env = {k: v for k, v in os.environ.items() if k not in ("VQA_LIB_PATH", "VQA_QSLICE")}
        if q is not None:
            env["VQA_QSLICE"] = q
        res = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120, cwd=REPO)
        assert res.returncode == 0 and "FLAVOUR 0" in res.stdout, (res.stdout[-300:], res.stderr[-800:])
        outs.append(res.stdout)
    assert outs[0] == outs[1] == outs[2], outs


def _dev(metric, chroma, depth, r, d, planes, e):
    """the float32 run of the metric's reference against its float64 run on pool entry e -> [(deviation, reference value)] per
    plane (CIEDE2000: per frame)"""
    L = (1 << depth) - 1
    if metric == "ciede":
        fr, fd = CR.split_planes(r[e:e + 1], planes)[0], CR.split_planes(d[e:e + 1], planes)[0]
        model = CR.BGR if chroma == "bgr" else CR.YUV709
        a, b = CR.de_mean(fr, fd, depth, model), CR.de_mean(fr, fd, depth, model, (1.0, 1.0, 1.0), np.float32)
        return [(abs(a - b) / a if a > 0 else abs(b), a)]
    out = []
    for p in planes:
        rp, dp = K.plane_of(r[e], p), K.plane_of(d[e], p)
        if metric == "gauss":
            a, b = H.ssim_gauss(rp, dp, L), H.ssim_gauss(rp, dp, L, dtype=np.float32)
            out.append((abs(a - b) / abs(a), a))
        elif metric == "ms":             # the bar is absolute, on every level's mean
            gaps = [abs(H.ssim_gauss(x, y, L) - H.ssim_gauss(x, y, L, dtype=np.float32)) for x, y in zip(M.pyramid(rp), M.pyramid(dp))]
            out.append((max(gaps), 1.0))
        elif metric in ("vif", "adm"):
            f = V.vif if metric == "vif" else A.adm
            a, b = f(rp, dp, depth), f(rp, dp, depth, dtype=np.float32)
            out.append((max(np.abs(a[2] - b[2]).max(), abs(a[3] - b[3])), 1.0))
        elif metric == "psnr_hvs":
            a, b = P.psnr_hvs(rp, dp, depth), P.psnr_hvs(rp, dp, depth, np.float32)
            out.append((max(abs(a[j] - b[j]) / a[j] if a[j] > 0 else abs(b[j]) for j in (0, 1)), 1.0))
        else:
            raise KeyError(metric)
    return out


@pytest.mark.parametrize("metric", SC.FLOAT32_CHECKED)
def test_float32_stays_within_half_the_bar_on_every_entry_compared_with_a_reference(metric):
    worst = (0.0, "")
    for chroma, h, w, depth in SC.layouts_of(metric):
        r, d, planes = SC.pool(chroma, h, w, depth)
        for e in SC.ref_entries(metric, depth):
            for k, (dev, ref) in enumerate(_dev(metric, chroma, depth, r, d, planes, e)):
                tag = "%s %s %dx%d %d bits %s plane %d" % (metric, chroma, h, w, depth, SC.POOL[e], k)
                print(tag, "float32 deviation %.2e" % dev)
                worst = max(worst, (dev, tag))
                assert dev <= HALF, (tag, dev)
                if metric == "gauss":
                    assert abs(ref) >= 0.1, (tag, ref)          # the relative bar is well defined
    print(metric, "worst float32 deviation: %.2e (%s)" % worst)


def test_the_exclusions_are_few_never_natural_and_their_deviations():
    assert set(SC.EXCLUDED) == set(SC.FLOAT32_CHECKED) and SC.MAX_EXCLUDED == 2
    for metric, excl in SC.EXCLUDED.items():
        for depth in (8, 10):
            out = {n for n, dp in excl if dp == depth}
            assert len(out) <= SC.MAX_EXCLUDED and out <= set(SC.POOL[5:]), (metric, depth, out)
            assert len(SC.ref_entries(metric, depth)) == 7 - len(out) and SC.ref_entries(metric, depth)[:5] == [0, 1, 2, 3, 4]
        for name, depth in excl:
            for chroma, h, w, dp in SC.layouts_of(metric):
                if dp == depth:
                    r, d, planes = SC.pool(chroma, h, w, depth)
                    for k, (dev, ref) in enumerate(_dev(metric, chroma, depth, r, d, planes, SC.POOL.index(name))):
                        print("excluded from", metric, ":", name, depth, "bits", chroma, "%dx%d" % (h, w), "plane", k,
                              "float32 deviation %.2e, reference value %.3e" % (dev, ref))
    for m in SC.METRICS:
        if m not in SC.FLOAT32_CHECKED:
            assert SC.ref_entries(m, 8) == SC.ref_entries(m, 10) == list(range(7))
