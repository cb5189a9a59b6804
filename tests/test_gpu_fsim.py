"""GPU: FSIM / FSIMc (vqa_fsim_submit / vqa_fsim_wait) through the C ABI, the engine, the one-pass stream and the reference-shaped
entry points, against the NumPy restatement of tests/fsim_reference.py (written from the definition in include/vqa.h).

What is asserted was fixed before the kernels first ran.  One child process on the lab library runs every case of
fsim_cases.matrix() and reads the p maps back: every sample of both maps must be within 1 unit of rint(PC 2^24) of the float64
restatement (np.fft); sum_pc and sum_sim must EQUAL the integer pooling over the GPU's own maps, sum_simc lie within
P 2^-24 + N of it (one unit of gc per sample, for the device's pow); fsim and fsimc must lie within the case's own bar
4 N 2^-24 / sum PC_m of the unquantised restatement, which tests/test_fsim_host.py admits case by case.  The same child runs the
slice pool uncut and with VQA_QSLICE=3 and VQA_FSIM_SUBSLICE=2.  Everything else runs on the shipped library.  Seen on an MI355X: the
largest map difference 0 units, the largest score gap 2.61e-8 against its bar 4.14e-6 (noise, bgr24, 16 x 16)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path[:0] = [REPO, os.path.dirname(os.path.abspath(__file__))]

import fsim_cases as FC
import fsim_reference as R

pytestmark = pytest.mark.gpu

FIELDS = ("sum_pc", "sum_sim", "sum_simc", "count", "factor", "flags", "fsim", "fsimc")
WORST = {"gap": 0.0, "bar": 0.0, "tag": "", "map": 0}
MATRIX = FC.matrix()
SEAMS = ("VQA_QSLICE", "VQA_FSIM_SUBSLICE")


def _child(out_path):
    import rtvqa_amd
    for k in SEAMS:
        os.environ.pop(k, None)
    plain = rtvqa_amd.Engine(0)
    os.environ["VQA_QSLICE"], os.environ["VQA_FSIM_SUBSLICE"] = "3", "2"   # read once, in vqa_create
    cut = rtvqa_amd.Engine(0)
    for k in SEAMS:
        os.environ.pop(k)
    assert plain.lib.vqa_build_flavour() == 3
    got = {}
    for case in MATRIX:
        c, l, (h, w), dp = case
        r, d = FC.pair(c, l, h, w, dp)
        rec, maps = plain.fsim(FC.pack([r], l, dp), FC.pack([d], l, dp), FC.engine_planes(l, h, w, dp), maps=True)
        got[FC.case_id(case)] = np.frombuffer(rec.tobytes(), np.uint8)
        got[FC.case_id(case) + "|maps"] = maps[0]
    for layout, h, w, dp in FC.SLICE_LAYOUTS:
        rs, ds = FC.slice_pool(layout, h, w, dp)
        r, d, planes = FC.pack(rs, layout, dp), FC.pack(ds, layout, dp), FC.engine_planes(layout, h, w, dp)
        for name, eng in (("plain", plain), ("cut", cut)):
            dr, dd = eng.upload(r), eng.upload(d)
            eng.profile(True)
            for mem, (a, b) in (("host", (r, d)), ("device", (dr, dd))):
                rec, maps = eng.fsim(a, b, planes, maps=True)
                got["%s|%s|%s" % (name, layout, mem)] = np.frombuffer(rec.tobytes(), np.uint8)
                got["%s|%s|%s|maps" % (name, layout, mem)] = maps
            prof = eng.profile_read(reset=True)
            got["%s|%s|launches" % (name, layout)] = np.array([prof[k][1] for k in ("k_fsim_luma", "k_fsim_dft", "k_fsim_energy",
                                                                                    "k_fsim_median", "k_fsim_pc", "k_fsim_pool")], np.int64)
            eng.profile(False)
            for buf in (dr, dd):
                buf._owner.free()
    plain.close()
    cut.close()
    np.savez(out_path, **got)
    print("FSIM-LAB-OK", len(got))


@pytest.fixture(scope="module")
def lab(tmp_path_factory):
    from rtvqa_amd import _native as N
    out = str(tmp_path_factory.mktemp("fsimlab") / "lab.npz")
    env = dict(os.environ, VQA_LIB_PATH=N.LAB_LIB_PATH)
    for k in SEAMS:
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True, timeout=600, cwd=REPO)
    assert r.returncode == 0 and "FSIM-LAB-OK" in r.stdout, (r.stdout[-300:], r.stderr[-2000:])
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


def _words(g):
    b = int(g["sum_simc"])
    return int(g["sum_pc"]), int(g["sum_sim"]), b - (1 << 64) if b >= 1 << 63 else b   # (B is signed, in two's complement)


def _one(engine, r, d, layout, h, w, depth):
    return engine.fsim(FC.pack([r], layout, depth), FC.pack([d], layout, depth), FC.engine_planes(layout, h, w, depth))[0]


def _check_words(g, maps, r, d, layout, depth, tag):
    """the record against the integer pooling over the GPU's OWN maps"""
    h, w = r[0].shape
    f, hd, wd = R.grid(h, w)
    n = hd * wd
    assert int(g["count"]) == n and int(g["factor"]) == f and maps.shape == (2, hd, wd)
    p, a, b = R.pool_words(list(r), list(d), FC.MODEL[layout], depth, maps[0].astype(np.int64), maps[1].astype(np.int64))
    gp, ga, gb = _words(g)
    print(tag, "words", (gp, ga, gb), "pooling over the maps", (p, a, b))
    assert (gp, ga) == (p, a), tag
    assert abs(gb - b) <= p * 2.0 ** -24 + n, (tag, gb, b)
    assert int(g["flags"]) == (1 if p == 0 else 0)
    if p:
        assert float(g["fsim"]) == float(ga) / float(gp) and float(g["fsimc"]) == float(gb) / float(gp)
    else:
        assert float(g["fsim"]) == 1.0 and float(g["fsimc"]) == 1.0


@pytest.mark.parametrize("case", MATRIX, ids=[FC.case_id(c) for c in MATRIX])
def test_parity_on_every_content_layout_shape_and_depth(lab, case):
    from rtvqa_amd.engine import FSIM_DTYPE
    name, layout, (h, w), depth = case
    tag = FC.case_id(case)
    r, d = FC.pair(name, layout, h, w, depth)
    g = np.frombuffer(lab[tag].tobytes(), FSIM_DTYPE)[0]
    maps = lab[tag + "|maps"]
    assert g.dtype.names == FIELDS and int(g["factor"]) == FC.FACTORS[(h, w)]
    e = FC.expected(case)
    # the maps: every sample of both within 1 unit of the restatement's
    gap_map = max(int(np.abs(maps[0].astype(np.int64) - R.quantise(e["pc_r"])).max()),
                  int(np.abs(maps[1].astype(np.int64) - R.quantise(e["pc_d"])).max()))
    WORST["map"] = max(WORST["map"], gap_map)
    print(tag, "largest map gap %d units of 2^-24" % gap_map)
    assert gap_map <= 1, (tag, gap_map)
    _check_words(g, maps, r, d, layout, depth, tag)
    # the scores against the unquantised float64 restatement
    gap = max(abs(float(g["fsim"]) - e["fsim"]), abs(float(g["fsimc"]) - e["fsimc"]))
    print(tag, "fsim %.10f (float64 %.10f) fsimc %.10f (float64 %.10f) gap %.2e bar %.2e" %
          (g["fsim"], e["fsim"], g["fsimc"], e["fsimc"], gap, e["bar"]))
    if name in FC.STRUCTURELESS:
        assert _words(g) == (0, 0, 0) and int(g["flags"]) == 1 and g["fsim"] == 1.0 and g["fsimc"] == 1.0
        assert not maps.any()
    else:
        if gap > WORST["gap"]:
            WORST.update(gap=gap, bar=e["bar"], tag=tag)
        assert e["bar"] <= FC.BAR_LIMIT and gap <= e["bar"], (tag, gap, e["bar"])
        assert int(g["flags"]) == 0
    if name == "identical":
        assert _words(g) == (int(g["sum_pc"]),) * 3 and g["fsim"] == 1.0 and g["fsimc"] == 1.0 and int(g["sum_pc"]) > 0
        assert (maps[0] == maps[1]).all()
    if layout == "gray":
        assert g["fsimc"] == g["fsim"] and int(g["sum_simc"]) == int(g["sum_sim"])


def test_the_worst_gap_of_the_parity_matrix():
    """runs after the parity tests of this module (pytest keeps the file's order): the figures DESIGN.md 4t and the README quote"""
    print("parity matrix: largest score gap %.3e against its bar %.3e (%s); largest map gap %d unit(s)" %
          (WORST["gap"], WORST["bar"], WORST["tag"], WORST["map"]))


def test_slices_and_sub_slices_give_the_bytes_of_one(lab):
    from rtvqa_amd.engine import FSIM_DTYPE
    for layout, h, w, dp in FC.SLICE_LAYOUTS:
        plain, pmaps = lab["plain|%s|host" % layout].tobytes(), lab["plain|%s|host|maps" % layout]
        f, hd, wd = R.grid(h, w)
        assert len(plain) == 56 * FC.SLICE_FRAMES and pmaps.shape == (FC.SLICE_FRAMES, 2, hd, wd)
        for mem in ("host", "device"):
            for name in ("plain", "cut"):
                assert lab["%s|%s|%s" % (name, layout, mem)].tobytes() == plain, (name, layout, mem)
                assert (lab["%s|%s|%s|maps" % (name, layout, mem)] == pmaps).all(), (name, layout, mem)
        # one profile entry per kernel id per sub-slice (five for the DFTs, four for the energies): 2 submits of 1 sub-slice;
        # 2 submits of 2 + 1, 2 + 1, 1 = 5 sub-slices
        assert list(lab["plain|%s|launches" % layout]) == [2, 10, 8, 2, 2, 2]
        assert list(lab["cut|%s|launches" % layout]) == [10, 50, 40, 10, 10, 10]
        # every frame of the batch is its own: frame i is pool entry i
        rec = np.frombuffer(plain, FSIM_DTYPE)
        assert len({x.tobytes() for x in rec}) == FC.SLICE_FRAMES
        rs, ds = FC.slice_pool(layout, h, w, dp)
        for i in range(FC.SLICE_FRAMES):
            _check_words(rec[i], pmaps[i], rs[i], ds[i], layout, dp, "slice pool %s frame %d" % (layout, i))
            want = R.fsim_float(list(rs[i]), list(ds[i]), FC.MODEL[layout], dp)
            assert np.abs(pmaps[i, 0].astype(np.int64) - R.quantise(want[2])).max() <= 1
            assert np.abs(pmaps[i, 1].astype(np.int64) - R.quantise(want[3])).max() <= 1


def test_exactness_on_the_device(engine):
    for layout, depth in (("bgr24", 8), ("yuv420p", 10), ("gray", 16)):
        for h, w in FC.SMALL + ((385, 391),):
            r, _ = FC.pair("noise", layout, h, w, depth)
            g = _one(engine, r, r, layout, h, w, depth)
            p = int(g["sum_pc"])
            assert p > 0 and _words(g) == (p, p, p) and g["fsim"] == 1.0 and g["fsimc"] == 1.0 and int(g["flags"]) == 0, (layout, h, w)
    for name in FC.STRUCTURELESS:
        r, d = FC.pair(name, "yuv420p", 33, 67)
        g = _one(engine, r, d, "yuv420p", 33, 67, 8)
        assert _words(g) == (0, 0, 0) and int(g["flags"]) == 1 and g["fsim"] == 1.0 and g["fsimc"] == 1.0, name
    # a gray YUV clip: the same bytes at 4:4:4, 4:2:2 and 4:2:0
    (y, _, _), (yd, _, _) = FC.pair("natural", "yuv444p", 33, 67)
    got = []
    for layout in ("yuv444p", "yuv422p", "yuv420p"):
        sizes = FC.plane_sizes(layout, 33, 67)
        r = [y] + [np.full(s, 128, np.int64) for s in sizes[1:]]
        d = [yd] + [np.full(s, 128, np.int64) for s in sizes[1:]]
        got.append(_one(engine, r, d, layout, 33, 67, 8).tobytes())
    assert got[0] == got[1] == got[2]


def test_the_depths_between_the_matrix_depths(engine):
    """9, 12 and 15 bits (uint16 samples): the scale s = 2^(depth - 8) and the peak enter the 3 x 4 matrix only"""
    for layout, depth in (("yuv420p", 9), ("bgr24", 12), ("gray", 15), ("yuv422p", 15)):
        r, d = FC.pair("natural", layout, 33, 67, depth)
        g = _one(engine, r, d, layout, 33, 67, depth)
        want = R.fsim_float(list(r), list(d), FC.MODEL[layout], depth)
        bar = R.derived_bar(want[2], want[3])
        assert bar <= FC.BAR_LIMIT and abs(g["fsim"] - want[0]) <= bar and abs(g["fsimc"] - want[1]) <= bar, (layout, depth)
        same = _one(engine, r, r, layout, 33, 67, depth)
        assert same["fsim"] == 1.0 and same["fsimc"] == 1.0 and int(same["sum_pc"]) > 0


def _clip(layout, h, w, depth, n):
    """n distinct frame pairs -> (ref, dist, planes, the frames as plane tuples)"""
    names = ("natural", "noise", "texture_flat", "half", "natural", "noise", "half", "noise")
    pairs = [FC.pair(names[k % 8], layout, h, w, depth, seed=11 + k) for k in range(n)]
    rs, ds = [p[0] for p in pairs], [p[1] for p in pairs]
    return FC.pack(rs, layout, depth), FC.pack(ds, layout, depth), FC.engine_planes(layout, h, w, depth), rs, ds


def test_batches_positions_and_memory_kinds_give_the_same_bytes(engine):
    """the same pair at several places of batches of 1, 3 and 8, from host, pinned and device memory; frame_fsim in chunks of 1, 3
    and 64; a strided view and an unaligned region of interest of resident frames"""
    from rtvqa_amd import video_processing as vp
    from rtvqa_amd.engine import DeviceFrames
    h, w, layout, n = 33, 67, "yuv420p", 8
    r, d, planes, rs, ds = _clip(layout, h, w, 8, n)
    whole = engine.fsim(r, d, planes)
    assert whole.shape == (n,) and len({x.tobytes() for x in whole}) == n
    for i in range(n):
        want = R.fsim_float(list(rs[i]), list(ds[i]), "yuv709")
        bar = R.derived_bar(want[2], want[3])
        assert abs(whole["fsim"][i] - want[0]) <= bar and abs(whole["fsimc"][i] - want[1]) <= bar, i
    assert engine.fsim(r, d, planes).tobytes() == whole.tobytes()             # run to run
    one = whole[5:6].tobytes()
    assert engine.fsim(r[5:6], d[5:6], planes).tobytes() == one               # a batch of 1
    for order in ([5, 0, 5], [1, 5, 2], [5, 1, 2, 3, 5, 6, 7, 5]):            # batches of 3 and 8
        got = engine.fsim(r[order], d[order], planes)
        for pos, k in enumerate(order):
            assert got[pos].tobytes() == whole[k].tobytes(), (order, pos)
    dr, dd = engine.upload(r), engine.upload(d)
    assert engine.fsim(dr, dd, planes).tobytes() == whole.tobytes()
    assert engine.fsim(dr.slice(5, 6), dd.slice(5, 6), planes).tobytes() == one
    pr, pd = engine.alloc_pinned(r.shape), engine.alloc_pinned(d.shape)
    pr[...], pd[...] = r, d
    assert engine.is_pinned(pr)
    assert engine.fsim(pr, pd, planes).tobytes() == whole.tobytes()
    for src in ((r, d), (pr, pd), (dr, dd)):
        for bs in (1, 3, 64):
            fs, fc = vp.frame_fsim(src[0], src[1], layout, h, w, batch_size=bs)
            assert fs.shape == (n,)
            assert fs.tobytes() == np.ascontiguousarray(whole["fsim"]).tobytes(), (type(src[0]), bs)
            assert fc.tobytes() == np.ascontiguousarray(whole["fsimc"]).tobytes(), (type(src[0]), bs)
    engine.free_pinned(pr)
    engine.free_pinned(pd)
    # every second frame of the resident clips: frame_stride does the stepping
    odd = [DeviceFrames(x.ptr + x.frame_stride, 4, x.h, x.w, frame_stride=2 * x.frame_stride, row_stride=x.row_stride, owner=x,
                        channels=x.channels) for x in (dr, dd)]
    assert engine.fsim(odd[0], odd[1], planes).tobytes() == whole[1::2].tobytes()
    # a window of resident 60 x 80 4:4:4 frames (uploaded as [n, 3 * 60, 80]; the window's plane k starts k * 60 rows further
    # down) at (9, 13), 35 x 45: odd origin, odd size; against the same samples as frames of their own
    H, W, (y0, x0, hh, ww) = 60, 80, (9, 13, 35, 45)
    g, gd, _, grs, gds = _clip("yuv444p", H, W, 8, 3)
    cut_r = [tuple(p[y0:y0 + hh, x0:x0 + ww] for p in f) for f in grs]
    cut_d = [tuple(p[y0:y0 + hh, x0:x0 + ww] for p in f) for f in gds]
    own = FC.engine_planes("yuv444p", hh, ww)
    alone = engine.fsim(FC.pack(cut_r, "yuv444p"), FC.pack(cut_d, "yuv444p"), own)
    dg, dgd = engine.upload(g.reshape(3, 3 * H, W)), engine.upload(gd.reshape(3, 3 * H, W))
    roi = [(ww, hh, k * H * W, W, 1) for k in range(3)]
    a, b = dg.roi(y0, y0 + hh, x0, x0 + ww), dgd.roi(y0, y0 + hh, x0, x0 + ww)
    assert engine.fsim(a, b, roi).tobytes() == alone.tobytes()
    assert engine.fsim(g, gd, [(ww, hh, k * H * W + y0 * W + x0, W, 1) for k in range(3)]).tobytes() == alone.tobytes()


def test_in_flight_next_to_an_mdsi_and_a_pu21_batch(engine):
    f, d, planes, _, _ = _clip("yuv420p", 33, 67, 8, 3)
    want, mwant, uwant = engine.fsim(f, d, planes), engine.mdsi(f, d, planes), engine.pu21(f, d, planes)
    df, dd = engine.upload(f), engine.upload(d)
    for order in (("fsim", "mdsi", "pu21"), ("pu21", "fsim", "mdsi")):
        engine.mdsi_submit(df, dd, planes)
        engine.fsim_submit(df, dd, planes)
        engine.pu21_submit(df, dd, planes)
        wants = {"fsim": want, "mdsi": mwant, "pu21": uwant}
        for kind in order:
            assert getattr(engine, kind + "_wait")().tobytes() == wants[kind].tobytes(), (order, kind)
    engine.mdsi_submit(f, d, planes)             # host frames share the staging of a pending MDSI batch
    engine.fsim_submit(f, d, planes)
    assert engine.fsim_wait().tobytes() == want.tobytes() and engine.mdsi_wait().tobytes() == mwant.tobytes()


def _submit(engine, f, d, planes, n=None, model=0):
    from rtvqa_amd import _native as N
    from rtvqa_amd.engine import plane_descs
    fb = f.shape[1] * f.dtype.itemsize
    return engine.lib.vqa_fsim_submit(engine.ctx, f.ctypes.data, d.ctypes.data, N.VQA_MEM_HOST, f.shape[0] if n is None else n,
                                      fb, fb, plane_descs(planes), len(planes), model)


def test_the_state_machine_and_the_refusals(engine):
    from rtvqa_amd import _native as N
    from rtvqa_amd.engine import plane_descs, yuv_planes
    f, d, planes, _, _ = _clip("yuv420p", 64, 96, 8, 2)
    want = engine.fsim(f, d, planes)
    mwant = engine.mdsi(f, d, planes)
    fout, mout = (N.VqaFsimMetrics * 2)(), (N.VqaMdsiMetrics * 2)()
    lib, ctx = engine.lib, engine.ctx

    def idle():
        return lib.vqa_fsim_wait(ctx, fout, 2) == N.VQA_ERR_STATE
    assert idle()                                                         # wait without submit
    assert _submit(engine, f, d, planes) == N.VQA_OK
    assert _submit(engine, f, d, planes) == N.VQA_ERR_STATE               # a second submit while pending
    assert lib.vqa_mdsi_wait(ctx, mout, 2) == N.VQA_ERR_STATE             # another kind's wait: the batch survives
    assert lib.vqa_trim(ctx) == N.VQA_ERR_STATE
    assert lib.vqa_fsim_wait(ctx, fout, 6) == N.VQA_ERR_STATE             # a wrong entry count: one entry per FRAME
    assert lib.vqa_fsim_wait(ctx, fout, 2) == N.VQA_OK
    assert bytes(fout) == want.tobytes()
    Y, U, V = planes
    z16 = np.zeros((2, 64 * 96 * 3), np.uint16)
    p10 = yuv_planes(64, 96, "420", 10)
    wide = np.zeros((1, 16 * 1030), np.uint8)
    refused = [
        (f, planes[:1], {"model": N.FSIM_YUV709}, N.VQA_ERR_INVALID),                       # one plane with the wrong model
        (f, planes, {"model": N.FSIM_GRAY}, N.VQA_ERR_INVALID),                             # three planes with the gray model
        (f, planes[:2], {}, N.VQA_ERR_INVALID),                                             # two planes
        (f, [Y, U, (V[0] - 1,) + V[1:]], {}, N.VQA_ERR_INVALID),                            # U and V geometries differ
        (f, planes, {"model": N.FSIM_BGR}, N.VQA_ERR_INVALID),                              # B, G, R must share one geometry
        (f, planes, {"model": 3}, N.VQA_ERR_INVALID),                                       # an unknown model
        (f, planes, {"model": -1}, N.VQA_ERR_INVALID),
        (z16, p10[:1] + [p[:5] for p in p10[1:]], {}, N.VQA_ERR_INVALID),                   # mixed depths
        (f, [(16, 15, 0, 16, 1), (8, 8, 240, 8, 1), (8, 8, 304, 8, 1)], {}, N.VQA_ERR_UNSUPPORTED),   # luma 15 rows x 16
        (f, [(15, 16, 0, 15, 1)], {"model": N.FSIM_GRAY}, N.VQA_ERR_UNSUPPORTED),                     # too small
        (wide, [(1030, 16, 0, 1030, 1)], {"model": N.FSIM_GRAY}, N.VQA_ERR_UNSUPPORTED),              # f = 1 and wd = 1030 > 1024
        (f, [(16385, 16384, 0, 16385, 1)] * 3, {"model": N.FSIM_BGR}, N.VQA_ERR_UNSUPPORTED),         # more than 2^28 samples
    ]
    for k, (buf, pl, kw, status) in enumerate(refused):
        assert _submit(engine, buf, buf, pl, n=1, **kw) == status, k
        assert idle(), k                                                  # a failed submit leaves nothing in flight
    fb, pd = f.shape[1], plane_descs(planes)
    assert lib.vqa_fsim_submit(ctx, f.ctypes.data, d.ctypes.data, N.VQA_MEM_HOST, 2, fb - 1, fb, pd, 3, 0) == N.VQA_ERR_INVALID
    assert lib.vqa_fsim_submit(ctx, f.ctypes.data, None, N.VQA_MEM_HOST, 2, fb, fb, pd, 3, 0) == N.VQA_ERR_INVALID
    assert idle()
    # a 16 x 16 4:2:0 frame is measured: its 8 x 8 chroma planes are no limit
    z = np.zeros((1, 16 * 16 * 3 // 2), np.uint8)
    assert _submit(engine, z, z, yuv_planes(16, 16, "420", 8)) == N.VQA_OK and lib.vqa_fsim_wait(ctx, fout, 1) == N.VQA_OK
    assert fout[0].sum_pc == 0 and fout[0].flags == 1 and fout[0].fsim == 1.0 and fout[0].count == 256
    assert engine.fsim(f, d, planes).tobytes() == want.tobytes()
    engine.trim()                                                         # the tables of the geometry go and come back
    assert engine.fsim(f, d, planes).tobytes() == want.tobytes()
    assert engine.mdsi(f, d, planes).tobytes() == mwant.tobytes()


def test_one_pass_entry_points(engine, tmp_path):
    """run_ffmpeg_metrics(.., fsim=True) and config "fsim": true on a 4-frame 72 x 88 .y4m pair: the psnr / ssim logs are byte for
    byte those of a plain run, the log's values are Engine.fsim's and follow pu_ssim, and the row gains FSIM, FSIMC after PU_SSIM
    with every other column as without the key"""
    from rtvqa_amd import frames, synth
    from rtvqa_amd import video_processing as vp
    h, w, n = 72, 88, 4
    r, d, planes, _, _ = _clip("yuv420p", h, w, 8, n)
    d[2] = r[2]                                                  # one identical frame: exactly 1 in the record and the log
    pr, pd = str(tmp_path / "ref.y4m"), str(tmp_path / "enc.y4m")
    frames.write_y4m(pr, r, h, w)
    frames.write_y4m(pd, d, h, w)
    logs = {k: [str(tmp_path / ("%s_%s.log" % (k, t))) for t in ("psnr", "ssim", "vmaf")] for k in ("plain", "fsim", "feat", "both")}
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["plain"], batch_size=4) is None
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["fsim"], batch_size=4, fsim=True) is None
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["feat"], batch_size=4, mdsi=True, pu21=True) is None
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["both"], batch_size=3, mdsi=True, pu21=True, fsim=True) is None
    assert not os.path.exists(logs["plain"][2])
    for k in (0, 1):
        for kind in ("fsim", "feat", "both"):
            assert open(logs["plain"][k], "rb").read() == open(logs[kind][k], "rb").read(), (kind, k)
    want = engine.fsim(r, d, planes)
    assert want["fsim"][2] == 1.0 and want["fsimc"][2] == 1.0 and (want["fsim"][[0, 1, 3]] < 1.0).all()
    doc, feat, both = (json.load(open(logs[k][2])) for k in ("fsim", "feat", "both"))
    assert list(doc["frames"][0]["metrics"]) == ["fsim", "fsimc"] == list(doc["pooled_metrics"])
    names = list(feat["frames"][0]["metrics"])
    assert names[-1] == "pu_ssim" and "fsim" not in json.dumps(feat)
    assert list(both["frames"][0]["metrics"]) == names + ["fsim", "fsimc"]
    for i in range(n):
        for dc in (doc, both):
            assert dc["frames"][i]["metrics"]["fsim"] == float(want["fsim"][i])
            assert dc["frames"][i]["metrics"]["fsimc"] == float(want["fsimc"][i])
        assert {k: both["frames"][i]["metrics"][k] for k in names} == feat["frames"][i]["metrics"]
    bgr = synth.s_natural(n, h, w, seed=12)
    cfg = {"crf": 23, "resize_width": 64, "resize_height": 64, "frame_interval": 1, "batch_size": 4}

    def row(name, **kw):
        return vp.process_video_and_extract_metrics(pr, pd, dict(cfg, **kw), csv_file=str(tmp_path / (name + ".csv")),
                                                    column_order="fixed", encoded_bgr=bgr)

    def same(a, b):
        return a == b or (a != a and b != b)

    row0, row1 = row("row0"), row("row1", fsim=True)
    k0 = list(row0)
    at = k0.index("SSIM") + 1
    assert list(row1) == k0[:at] + ["FSIM", "FSIMC"] + k0[at:] and all(same(row0[k], row1[k]) for k in k0)
    assert abs(row1["FSIM"] - want["fsim"].mean()) <= 1e-15 and abs(row1["FSIMC"] - want["fsimc"].mean()) <= 1e-15
    row2, row3 = row("row2", pu21=True, batch_size=2), row("row3", pu21=True, fsim=True, batch_size=2)
    k2 = list(row2)
    at = k2.index("PU_SSIM") + 1
    assert list(row3) == k2[:at] + ["FSIM", "FSIMC"] + k2[at:] and all(same(row2[k], row3[k]) for k in k2)
    assert row3["FSIM"] == row1["FSIM"]
    # the same call without the key, and with it false: the same file, byte for byte, with no new column
    row("row0b", fsim=False)
    assert open(str(tmp_path / "row0.csv"), "rb").read() == open(str(tmp_path / "row0b.csv"), "rb").read()
    assert b"FSIM" not in open(str(tmp_path / "row0.csv"), "rb").read()
    assert b"PU_SSIM,FSIM,FSIMC" in open(str(tmp_path / "row3.csv"), "rb").read()


def test_profile_names_the_kernels(engine):
    from rtvqa_amd import _native as N
    f, d, planes, _, _ = _clip("yuv420p", 33, 67, 8, 2)
    engine.profile(True)
    try:
        engine.profile_read(reset=True)
        engine.fsim(f, d, planes)
        prof = engine.profile_read(reset=True)
        assert [prof[k][1] for k in ("k_fsim_luma", "k_fsim_dft", "k_fsim_energy", "k_fsim_median", "k_fsim_pc", "k_fsim_pool")] == \
            [1, 5, 4, 1, 1, 1], prof
        assert "k_mdsi_map" not in prof
        ms, cnt = C.c_double(0), C.c_int64(0)
        for bad in (N.K_RIM, N.K_HEM, N.K_VERGE):                          # ids 55, 62 and 52 are unknown
            assert engine.lib.vqa_profile_read(engine.ctx, bad, C.byref(ms), C.byref(cnt), 0) == N.VQA_ERR_INVALID
    finally:
        engine.profile(False)


if __name__ == "__main__":
    _child(sys.argv[1])
