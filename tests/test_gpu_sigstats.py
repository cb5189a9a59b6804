"""GPU: the signal statistics (vqa_sigstats_submit / vqa_sigstats_wait) through the C ABI and the engine against the NumPy
restatement of tests/sigstats_reference.py (written from the definition in include/vqa.h; its order statistics come from a sort,
not from a histogram).

Every word of the family is an integer function of the samples, so every word is held to EQUALITY; the three doubles follow from
the record's own words by the stated host formula within 2 ulp.  The geometries are test_gpu_siti.py's grid."""
import ctypes as C

import numpy as np
import pytest

import motion_cases as K
import sigstats_cases as SC
import sigstats_reference as R
import test_sigstats_host as H

pytestmark = pytest.mark.gpu


def _check(got, f, planes, depth, tag, prev0=None, black=None, crop=None, sums=None):
    assert got.shape == (len(f), len(planes))
    for j, p in enumerate(planes):
        pl = K.plane_series(f, p)
        p0 = K.plane_series(prev0[None], p)[0] if prev0 is not None else None
        want = R.series(pl, depth, p0, black, crop)
        for i in range(len(pl)):
            diff = R.same_words(got[i, j], want[i])
            assert not diff, (tag, i, j, {k: (int(got[i, j][k]), want[i][k]) for k in diff})
            for name, v in zip(("mean", "stdev", "dif"), R.doubles(got[i, j])):
                assert R.ulp_close(float(got[i, j][name]), v), (tag, i, j, name, got[i, j][name], v)
            if sums is not None:
                rows, cols = R.profile(pl[i])
                assert np.array_equal(sums[j]["rows"][i], rows) and np.array_equal(sums[j]["cols"][i], cols), (tag, i, j)


@pytest.mark.parametrize("geom,depth,layout", SC.GRID, ids=SC.IDS)
def test_parity_with_the_restatement(engine, geom, depth, layout):
    """noise over the sample type's full range (above the peak at 10 and 12 bits), a boxed picture whose bars sit exactly at
    crop_level, a frame equal to its predecessor; without and with prev0, default and other levels, with the profiles"""
    h, w = geom
    tag = "%dx%d %s" % (h, w, layout)
    f, planes = SC.clip(layout, h, w, depth, seed=h + w)
    got = engine.sigstats(f, planes)
    assert (got[0]["sad"] == 0).all() and (got[0]["changed"] == 0).all() and (got[0]["dif"] == 0.0).all()   # no predecessor
    assert (got[3]["sad"] == 0).all() and (got[3]["changed"] == 0).all() and (got[1]["changed"] > 0).all()
    if 8 < depth < 16:
        assert (got[0]["above_peak"] > 0).all()
    for j, p in enumerate(planes):                      # the bars exactly at the default level are dark
        t, b, l, r = SC.BARS
        assert tuple(int(got[2, j][k]) for k in ("top", "bottom", "left", "right")) == (t, p[1] - b - 1, l, p[0] - r - 1)
    _check(got, f, planes, depth, tag)
    tail, sums = engine.sigstats(f[1:], planes, prev0=f[0], profiles=True)
    assert tail.tobytes() == got[1:].tobytes()          # frame 0 with prev0 is frame 1 of the clip prefixed by it
    _check(tail, f[1:], planes, depth, tag + " prev0", prev0=f[0], sums=sums)
    # other levels: black_level below the default, crop_level where this clip's bars sit
    s = 1 << (depth - 8)
    black, crop = 20 * s + 1, 29 * s + 1
    f2, _ = SC.clip(layout, h, w, depth, seed=h + w + 1, crop_level=crop)
    got2, sums2 = engine.sigstats(f2[1:], planes, prev0=f2[0], black_level=black, crop_level=crop, profiles=True)
    _check(got2, f2[1:], planes, depth, tag + " levels", prev0=f2[0], black=black, crop=crop, sums=sums2)
    one_less = engine.sigstats(f2[2:3], planes, crop_level=crop - 1)
    assert (one_less["top"] == 0).all() and (one_less["left"] == 0).all()       # one below the bars: nothing is dark
    assert (got2[1]["top"] == SC.BARS[0]).all() and (got2[1]["left"] == SC.BARS[2]).all()


@pytest.mark.parametrize("depth,value", [(8, 255), (8, 200), (16, 65535)])
def test_the_counter_width_case(engine, depth, value):
    """a flat plane of 258 x 256 = 66048 samples puts them all into ONE bin: the smallest shape that breaks a 16-bit counter or a
    saturating add"""
    h, w = 258, 256
    f, planes = SC.mono(np.full((2, h, w), value), depth)
    got = engine.sigstats(f, planes)
    n = h * w
    for i in range(2):
        g = got[i, 0]
        assert int(g["count"]) == n == 66048 and int(g["sum"]) == n * value and int(g["sum_sq"]) == n * value * value
        assert [int(g[k]) for k in ("min", "low", "median", "high", "max", "or_mask", "and_mask")] == [value] * 7
        assert int(g["over_luma"]) == int(g["over_chroma"]) == (n if value > 240 << (depth - 8) else 0)
        assert int(g["below_black"]) == int(g["under"]) == int(g["above_peak"]) == 0
        assert (int(g["top"]), int(g["bottom"]), int(g["left"]), int(g["right"])) == (0, h - 1, 0, w - 1)
        assert int(g["sad"]) == 0 and int(g["changed"]) == 0
        assert float(g["mean"]) == float(value) and float(g["stdev"]) == 0.0
    _check(got, f, planes, depth, "flat %d" % depth)


@pytest.mark.parametrize("case", H.hand_cases(), ids=[c[0] for c in H.hand_cases()])
def test_known_answers_on_the_device(engine, case):
    _name, x, depth, levels, known = case
    black, crop = levels or (None, None)
    f, planes = SC.mono(x[None], depth)
    got = engine.sigstats(f, planes, black_level=black, crop_level=crop)
    assert {k: int(got[0, 0][k]) for k in known} == known
    _check(got, f, planes, depth, _name, black=black, crop=crop)


def test_batches_positions_and_memory_kinds_give_the_same_bytes(engine):
    h, w, layout, n = 66, 98, "yuv420p", 9
    f, planes = K.clip(layout, h, w, 8, "natural", seed=11, n=n)
    whole, wsums = engine.sigstats(f, planes, profiles=True)
    assert engine.sigstats(f, planes).tobytes() == whole.tobytes()             # run to run
    F = np.concatenate([f[4:6], f[:3], f[4:6], f[7:9], f[4:6]])                 # the pair (4, 5) at places 1, 6 and 10
    got, sums = engine.sigstats(F, planes, profiles=True)
    dF = engine.upload(F)
    dgot, dsums = engine.sigstats(dF, planes, profiles=True)
    assert dgot.tobytes() == got.tobytes()
    for pos in (1, 6, 10):
        assert got[pos].tobytes() == whole[5].tobytes(), pos
        for j in range(len(planes)):
            for key in ("rows", "cols"):
                assert sums[j][key][pos].tobytes() == dsums[j][key][pos].tobytes() == wsums[j][key][5].tobytes(), (pos, j, key)
    assert engine.sigstats(f[5:6], planes, prev0=f[4]).tobytes() == whole[5:6].tobytes()
    df = engine.upload(f)
    assert engine.sigstats(df, planes).tobytes() == whole.tobytes()
    assert engine.sigstats(df.slice(5, 6), planes, prev0=df.frame(4)).tobytes() == whole[5:6].tobytes()
    pinned = engine.alloc_pinned(f.shape)
    pinned[...] = f
    assert engine.is_pinned(pinned) and engine.sigstats(pinned, planes).tobytes() == whole.tobytes()
    engine.free_pinned(pinned)
    dF._owner.free()
    df._owner.free()
    _check(whole, f, planes, 8, "natural", sums=wsums)


def test_pending_next_to_other_kinds(engine):
    """one context with an SSE / SSIM, an SI/TI and a VCA batch pending too: sigstats among them is sigstats alone, byte for byte,
    and each wait collects its own kind"""
    from rtvqa_amd import _native as N
    h, w, layout, n = 66, 98, "yuv420p", 4
    f, planes = K.clip(layout, h, w, 8, "natural", seed=21, n=n)
    d, _ = K.clip(layout, h, w, 8, "noise", seed=22, n=n)
    alone, asums = engine.sigstats(f[1:], planes, prev0=f[0], profiles=True)
    siti, vca, quality = engine.siti(f[1:], planes, prev0=f[0]), engine.vca(f[1:], planes, prev0=f[0]), engine.quality(f[1:], d[1:], planes)
    for order in (("quality", "siti", "vca", "sigstats"), ("sigstats", "vca", "quality", "siti")):
        engine.quality_submit(f[1:], d[1:], planes)
        engine.siti_submit(f[1:], planes, prev0=f[0])
        engine.sigstats_submit(f[1:], planes, prev0=f[0])
        engine.vca_submit(f[1:], planes, prev0=f[0])
        with pytest.raises(N.VqaError) as e:                 # a second batch of the kind: refused, the first stays pending
            engine.sigstats_submit(f[:1], planes)
        assert e.value.status == N.VQA_ERR_STATE
        got = {}
        for kind in order:
            got[kind] = engine.sigstats_wait(profiles=True) if kind == "sigstats" else getattr(engine, kind + "_wait")()
        assert got["sigstats"][0].tobytes() == alone.tobytes(), order
        for j in range(len(planes)):
            assert got["sigstats"][1][j]["rows"].tobytes() == asums[j]["rows"].tobytes()
            assert got["sigstats"][1][j]["cols"].tobytes() == asums[j]["cols"].tobytes()
        assert got["siti"].tobytes() == siti.tobytes() and got["vca"].tobytes() == vca.tobytes()
        assert got["quality"].tobytes() == quality.tobytes()
    # a wait with nothing of the kind pending, and another kind's wait with only this kind pending
    out = np.zeros(3 * len(planes), alone.dtype)
    assert engine.lib.vqa_sigstats_wait(engine.ctx, out.ctypes.data_as(C.POINTER(N.VqaSigstatsMetrics)), out.size, 0, None, 0) == N.VQA_ERR_STATE
    engine.sigstats_submit(f[1:], planes, prev0=f[0])
    sout = np.zeros(3 * len(planes), siti.dtype)
    assert engine.lib.vqa_siti_wait(engine.ctx, sout.ctypes.data_as(C.POINTER(N.VqaSitiMetrics)), sout.size) == N.VQA_ERR_STATE
    assert engine.sigstats_wait().tobytes() == alone.tobytes()


def E_planes(planes):
    from rtvqa_amd.engine import plane_descs
    return plane_descs(planes)


def test_errors(engine):
    from rtvqa_amd import _native as N
    from rtvqa_amd.engine import gray_planes, mono_planes
    h, w = 20, 24
    f, planes = SC.mono(np.random.default_rng(5).integers(0, 256, (3, h, w)), 8)
    want = engine.sigstats(f, planes, profiles=True)
    # planes below 16 x 16
    for hh, ww in ((15, 16), (16, 15)):
        with pytest.raises(N.VqaError) as e:
            engine.sigstats(np.zeros((1, hh * ww), np.uint8), gray_planes(hh, ww))
        assert e.value.status == N.VQA_ERR_UNSUPPORTED
    # a level above 65535: the engine's ValueError, the library's VQA_ERR_INVALID; a negative one is the default
    for kw in (dict(black_level=65536), dict(crop_level=65536), dict(black_level=-1), dict(crop_level=1.5)):
        with pytest.raises(ValueError):
            engine.sigstats(f, planes, **kw)
    lib, ctx = engine.lib, engine.ctx
    for levels in ((65536, -1), (-1, 65536)):
        assert lib.vqa_sigstats_submit(ctx, f.ctypes.data, None, N.VQA_MEM_HOST, 3, f.shape[1], E_planes(planes), 1, *levels) == N.VQA_ERR_INVALID
    assert lib.vqa_sigstats_submit(ctx, f.ctypes.data, None, N.VQA_MEM_HOST, 3, f.shape[1], E_planes(planes), 1, -7, -1) == N.VQA_OK
    out = np.zeros(3, want[0].dtype)
    assert lib.vqa_sigstats_wait(ctx, out.ctypes.data_as(C.POINTER(N.VqaSigstatsMetrics)), 3, 0, None, 0) == N.VQA_OK
    assert out.tobytes() == want[0].tobytes()
    assert engine.sigstats(f, planes, black_level=65535, crop_level=0)[0, 0]["below_black"] == h * w
    # a dtype that does not match the depth
    with pytest.raises(ValueError):
        engine.sigstats(f.astype(np.uint16), planes)
    with pytest.raises(ValueError):
        engine.sigstats(f, mono_planes(h, w, 10))
    with pytest.raises(ValueError):
        engine.sigstats(f, planes, prev0=f[0].astype(np.uint16))
    # a wrong n_profile_words (or no buffer) leaves the batch pending
    engine.sigstats_submit(f, planes)
    words = np.zeros(3 * (h + w), np.uint64)
    wp = words.ctypes.data_as(C.POINTER(C.c_uint64))
    rp = out.ctypes.data_as(C.POINTER(N.VqaSigstatsMetrics))
    for bad in (words.size - 1, words.size + 1, 0):
        assert lib.vqa_sigstats_wait(ctx, rp, 3, 1, wp, bad) == N.VQA_ERR_INVALID
    assert lib.vqa_sigstats_wait(ctx, rp, 3, 1, None, words.size) == N.VQA_ERR_INVALID
    assert lib.vqa_sigstats_wait(ctx, rp, 2, 1, wp, words.size) == N.VQA_ERR_STATE
    with pytest.raises(N.VqaError) as e:                         # still pending: a second submit is refused
        engine.sigstats_submit(f, planes)
    assert e.value.status == N.VQA_ERR_STATE
    rec, sums = engine.sigstats_wait(profiles=True)
    assert rec.tobytes() == want[0].tobytes() and sums[0]["rows"].tobytes() == want[1][0]["rows"].tobytes()
    assert sums[0]["cols"].tobytes() == want[1][0]["cols"].tobytes()


def test_the_kernels_are_timed_under_their_ids(engine):
    f, planes = SC.clip("yuv420p", 66, 98, 8, seed=3)
    engine.profile(True)
    engine.profile_read(reset=True)
    engine.sigstats(f, planes)
    got = engine.profile_read(reset=True)
    engine.profile(False)
    assert sorted(got) == ["k_sigstats_accum", "k_sigstats_scan"]
    assert got["k_sigstats_accum"][1] == 2 and got["k_sigstats_scan"][1] == 1      # two geometry groups, one sub-slice
