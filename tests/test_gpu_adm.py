"""GPU: ADM on four scales (vqa_adm_submit / vqa_adm_wait) through the C ABI, the engine, the one-pass stream and the
reference-shaped entry point, against the float64 reference of tests/adm_reference.py (written from the definition in
include/vqa.h).  Bar: 1e-4 absolute on every scale and on adm2.  The decoupling's angle test is a discontinuity: where a
(case, scale) misses that bar, the bar becomes 1e-4 plus the spread the reference reports when the flags of the samples within
2^-20 of the boundary are forced either way, never more than 2e-3, and on at most a quarter of the (case, scale) entries
(include/vqa.h, vqa_adm_submit).  tests/test_adm_host.py checks on the CPU that the reference's own float32 run of every pair
compared here stays within 5e-5 of its float64 run."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import adm_cases as K
import adm_reference as A

pytestmark = pytest.mark.gpu

BAR = 1e-4
BAR_MAX = 2e-3
MARGIN = 2.0 ** -20
ENTRIES = {"all": 0, "widened": []}   # (case, scale) entries of the parity tests; entry 4 of a case is adm2


def _check(got, r, d, planes, depth, tag, count=True):
    """got: [n, p] ADM records; every scale and adm2 within the bar of the reference"""
    isz = r.dtype.itemsize
    worst = 0.0
    for i in range(got.shape[0]):
        for p, pl in enumerate(planes):
            rp, dp = K.plane_of(K.flat(r)[i], pl, isz), K.plane_of(K.flat(d)[i], pl, isz)
            num, den, scale, adm2 = A.adm(rp, dp, depth)
            err = np.append(np.abs(got[i, p]["scale"] - scale), abs(float(got[i, p]["adm2"]) - adm2))
            print(tag, "frame", i, "plane", p, "scale", np.round(scale, 6), "adm2 %.6f" % adm2, "err", " ".join("%.2e" % e for e in err))
            worst = max(worst, err.max())
            if count:
                ENTRIES["all"] += 5
            bars = np.full(5, BAR)
            if (err > BAR).any():
                _n, _d, _s, _a, unsure, lo, hi = A.adm(rp, dp, depth, margin=MARGIN)
                for s in np.nonzero(err > BAR)[0]:
                    bar = min(BAR + (hi[s] - lo[s]), BAR_MAX)
                    print(tag, "frame", i, "plane", p, "entry", s, "unsure samples", unsure[s], "spread %.2e" % (hi[s] - lo[s]),
                          "bar %.2e" % bar)
                    assert unsure[s] > 0 and err[s] <= bar, (tag, i, p, s, err[s], bar, unsure[s])
                    assert count, "the widened bar belongs to the parity matrix alone"
                    ENTRIES["widened"].append((tag, i, p, int(s), float(err[s]), float(bar)))
                    bars[s] = bar
            assert (np.abs(got[i, p]["den"] - den) <= BAR * den).all(), (tag, i, p, got[i, p]["den"], den)
            assert (np.abs(got[i, p]["num"] - num) <= (bars[:4] + BAR) * den).all(), (tag, i, p, got[i, p]["num"], num)
    print(tag, "worst", "%.2e" % worst)


@pytest.mark.parametrize("kind", K.KINDS)
@pytest.mark.parametrize("geom,depth,layout,seed", K.GRID, ids=K.IDS)
def test_parity_with_the_reference(engine, geom, depth, layout, seed, kind):
    h, w = geom
    r, d, planes = K.frames(layout, h, w, depth, kind, seed)
    got = engine.adm(r, d, planes)
    assert got.shape == (1, len(planes))
    _check(got, r, d, planes, depth, "%dx%d %s %s" % (h, w, layout, kind))
    # the record is consistent with itself: quotients of its own sums, in double
    for p in range(len(planes)):
        g = got[0, p]
        assert np.array_equal(g["scale"], g["num"] / g["den"])
        assert abs(float(g["adm2"]) - g["num"].sum() / g["den"].sum()) <= 1e-15


@pytest.mark.parametrize("kind", K.KINDS)
def test_a_region_of_interest_of_padded_device_frames(engine, kind):
    """a 75 x 93 window at (9, 13) of resident 120 x 160 frames: rows are 160 bytes apart, nothing outside the window is read
    (the DWT mirrors inside the window)"""
    r, d, roi, rr, dc = K.roi_frames(kind)
    dr, dd = engine.upload(r), engine.upload(d)
    got = engine.adm(dr, dd, roi)
    from rtvqa_amd.engine import gray_planes
    win = gray_planes(K.ROI["h"], K.ROI["w"])
    _check(got, rr, dc, win, 8, "roi " + kind)
    assert got.tobytes() == engine.adm(rr, dc, win).tobytes()      # the window alone gives the same bits
    assert got.tobytes() == engine.adm(r, d, roi).tobytes()        # and so does host memory


def test_the_widened_bar_serves_at_most_a_quarter_of_the_entries():
    """runs after the parity tests of this module (pytest keeps the file's order)"""
    print("entries", ENTRIES["all"], "widened", ENTRIES["widened"])
    assert 4 * len(ENTRIES["widened"]) <= ENTRIES["all"], ENTRIES


def test_identical_inputs_give_num_equal_to_den_bit_for_bit(engine):
    for (h, w), depth, layout, seed in K.GRID:
        r, _d, planes = K.frames(layout, h, w, depth, "noise", seed=3)
        got = engine.adm(r, r, planes)
        assert got["num"].tobytes() == got["den"].tobytes(), (layout, got["num"], got["den"])
        assert (got["scale"] == 1.0).all() and (got["adm2"] == 1.0).all()
    # a constant against a constant: no detail but the fp32 taps' rounding (hi sums to 1e-8, not 0: bands of 1e-6, whose cube
    # roots reach 1e-7), num_s = den_s = 3 cbrt(area_s / 32)
    from rtvqa_amd.engine import gray_planes
    a, b = np.full((1, 47 * 35), 100, np.uint8), np.full((1, 47 * 35), 140, np.uint8)
    got = engine.adm(a, b, gray_planes(47, 35))[0, 0]
    want = [3.0 * np.cbrt(A.region(bh, bw)[4] / 32.0) for bh, bw in A.level_dims(47, 35)]
    assert np.allclose(got["den"], want, rtol=0, atol=1e-5) and np.allclose(got["num"], want, rtol=0, atol=1e-5)
    assert abs(float(got["adm2"]) - 1.0) <= 1e-6


def test_batches_and_positions_give_the_same_bits(engine):
    """the same pair at positions 0, 3 and 63 of batches of 1, 7 and 64, and frame_adm in chunks of 3 and 7"""
    from rtvqa_amd import video_processing as vp
    h, w, layout = 98, 130, "yuv420p"
    r, d, planes = K.frames(layout, h, w, 8, "noise", seed=11, n=8)
    R, D = np.repeat(r, 8, axis=0), np.repeat(d, 8, axis=0)       # 64 frames: frame i is pair i // 8
    R[[0, 3, 63]], D[[0, 3, 63]] = r[5], d[5]
    one = engine.adm(r[5:6], d[5:6], planes)
    want = (one["num"].tobytes(), one["den"].tobytes())
    whole = engine.adm(R, D, planes)
    for pos in (0, 3, 63):
        assert (whole[pos:pos + 1]["num"].tobytes(), whole[pos:pos + 1]["den"].tobytes()) == want, pos
    seven = engine.adm(R[:7], D[:7], planes)
    for pos in (0, 3):
        assert (seven[pos:pos + 1]["num"].tobytes(), seven[pos:pos + 1]["den"].tobytes()) == want, pos
    assert seven.tobytes() == whole[:7].tobytes()
    assert engine.adm(R, D, planes).tobytes() == whole.tobytes()   # run to run
    assert engine.adm(engine.upload(R), engine.upload(D), planes).tobytes() == whole.tobytes()   # device memory
    for src_r, src_d in ((R[:17], D[:17]), (engine.upload(R[:17]), engine.upload(D[:17]))):
        for bs in (3, 7):
            scale, adm2, sizes = vp.frame_adm(src_r, src_d, layout, h, w, batch_size=bs)
            assert scale.shape == (17, 3, 4) and adm2.shape == (17, 3) and sizes == [(p[0], p[1]) for p in planes]
            assert scale.tobytes() == np.ascontiguousarray(whole[:17]["scale"]).tobytes(), bs
            assert adm2.tobytes() == np.ascontiguousarray(whole[:17]["adm2"]).tobytes(), bs


def _submit(engine, r, d, planes):
    from rtvqa_amd import _native as N
    from rtvqa_amd.engine import plane_descs
    fb = K.flat(r).shape[1] * r.dtype.itemsize
    return engine.lib.vqa_adm_submit(engine.ctx, r.ctypes.data, d.ctypes.data, N.VQA_MEM_HOST, r.shape[0], fb, fb,
                                     plane_descs(planes), len(planes))


def test_the_state_machine_and_the_refusals(engine):
    from rtvqa_amd import _native as N
    from rtvqa_amd.engine import gray_planes, plane_descs, yuv420p_planes, yuv_planes
    r, d, planes = K.frames("yuv420p", 64, 96, 8, "noise", seed=8)
    want = engine.adm(r, d, planes)
    vwant = engine.vif(r, d, planes)
    qwant = engine.quality(r, d, planes)
    aout, vout, qout = (N.VqaAdmMetrics * 3)(), (N.VqaVifMetrics * 3)(), (N.VqaPlaneMetrics * 3)()
    # wait without submit
    assert engine.lib.vqa_adm_wait(engine.ctx, aout, 3) == N.VQA_ERR_STATE
    # submit while pending; the other kinds' waits on an ADM batch; the batch survives all of them
    assert _submit(engine, r, d, planes) == N.VQA_OK
    assert _submit(engine, r, d, planes) == N.VQA_ERR_STATE
    assert engine.lib.vqa_quality_wait(engine.ctx, qout, 3) == N.VQA_ERR_STATE
    assert engine.lib.vqa_quality_wait_ms(engine.ctx, qout, None, 3) == N.VQA_ERR_STATE
    assert engine.lib.vqa_vif_wait(engine.ctx, vout, 3) == N.VQA_ERR_STATE
    assert engine.lib.vqa_trim(engine.ctx) == N.VQA_ERR_STATE
    assert engine.lib.vqa_set_option(engine.ctx, N.OPT_HYST_STATS, 0) == N.VQA_ERR_STATE
    assert engine.lib.vqa_adm_wait(engine.ctx, aout, 2) == N.VQA_ERR_STATE      # a wrong entry count
    assert engine.lib.vqa_adm_wait(engine.ctx, aout, 3) == N.VQA_OK
    assert bytes(aout) == want.tobytes()
    # an ADM wait on a quality batch and on a VIF batch; each survives
    fb = K.flat(r).shape[1]
    assert engine.lib.vqa_quality_submit(engine.ctx, r.ctypes.data, d.ctypes.data, N.VQA_MEM_HOST, 1, fb, fb, plane_descs(planes), 3,
                                         N.SSIM_GAUSS) == N.VQA_OK
    assert engine.lib.vqa_adm_wait(engine.ctx, aout, 3) == N.VQA_ERR_STATE
    assert engine.lib.vqa_quality_wait(engine.ctx, qout, 3) == N.VQA_OK
    assert bytes(qout) == qwant.tobytes()
    assert engine.lib.vqa_vif_submit(engine.ctx, r.ctypes.data, d.ctypes.data, N.VQA_MEM_HOST, 1, fb, fb, plane_descs(planes), 3) == N.VQA_OK
    assert engine.lib.vqa_adm_wait(engine.ctx, aout, 3) == N.VQA_ERR_STATE
    assert engine.lib.vqa_vif_wait(engine.ctx, vout, 3) == N.VQA_OK
    assert bytes(vout) == vwant.tobytes()
    # all three in flight on one upload (what the stream does): each wait collects its own, in any order
    dr, dd = engine.upload(r), engine.upload(d)
    engine.quality_submit(dr, dd, planes)
    engine.vif_submit(dr, dd, planes)
    engine.adm_submit(dr, dd, planes)
    assert engine.adm_wait().tobytes() == want.tobytes()
    assert engine.quality_wait().tobytes() == qwant.tobytes()
    assert engine.vif_wait().tobytes() == vwant.tobytes()
    # planes below 16
    for h, w in ((15, 40), (40, 15)):
        z = np.zeros((1, h * w), np.uint8)
        assert _submit(engine, z, z, gray_planes(h, w)) == N.VQA_ERR_UNSUPPORTED, (h, w)
    z = np.zeros((1, 16 * 16), np.uint8)
    assert _submit(engine, z, z, gray_planes(16, 16)) == N.VQA_OK
    assert engine.lib.vqa_adm_wait(engine.ctx, aout, 1) == N.VQA_OK
    z = np.zeros((1, 30 * 30 * 3 // 2), np.uint8)                      # 4:2:0 at 30: the chroma planes are 15
    assert _submit(engine, z, z, yuv420p_planes(30, 30)) == N.VQA_ERR_UNSUPPORTED
    # what vqa_quality_submit refuses is refused the same way: mixed depths, bad depths, odd 16-bit strides
    z16 = np.zeros((1, 64 * 64 * 3 // 2), np.uint16)
    p10 = yuv_planes(64, 64, "420", 10)
    assert _submit(engine, z16, z16, p10) == N.VQA_OK
    assert engine.lib.vqa_adm_wait(engine.ctx, aout, 3) == N.VQA_OK
    assert _submit(engine, z16, z16, p10[:1] + [p[:5] for p in p10[1:]]) == N.VQA_ERR_INVALID
    assert _submit(engine, z16, z16, [p[:5] + (17,) for p in p10]) == N.VQA_ERR_INVALID
    assert _submit(engine, z16, z16, [(p[0], p[1], p[2], p[3] + 1, p[4], p[5]) for p in p10]) == N.VQA_ERR_INVALID
    assert engine.lib.vqa_adm_submit(engine.ctx, None, d.ctypes.data, N.VQA_MEM_HOST, 1, fb, fb, plane_descs(planes), 3) == N.VQA_ERR_INVALID
    assert engine.lib.vqa_adm_submit(engine.ctx, r.ctypes.data, d.ctypes.data, 7, 1, fb, fb, plane_descs(planes), 3) == N.VQA_ERR_INVALID
    # nothing is pending and the ctx computes as before
    assert engine.lib.vqa_adm_wait(engine.ctx, aout, 3) == N.VQA_ERR_STATE
    assert engine.adm(r, d, planes).tobytes() == want.tobytes()


def _free_bytes():
    import torch
    return torch.cuda.mem_get_info(0)[0]


def test_trim_returns_the_band_scratch():
    import rtvqa_amd
    h, w, n = 1080, 1920, 48
    r, d, planes = K.frames("yuv420p", h, w, 8, "noise", seed=2)
    r, d = np.repeat(r, n, axis=0), np.repeat(d, n, axis=0)
    with rtvqa_amd.Engine(0) as eng:
        small = eng.adm(r[:1], d[:1], planes)
        eng.trim()
        base = _free_bytes()
        dr, dd = eng.upload(r), eng.upload(d)
        held = _free_bytes()
        eng.adm_submit(dr, dd, planes)
        from rtvqa_amd import _native as N
        assert eng.lib.vqa_trim(eng.ctx) == N.VQA_ERR_STATE
        big = eng.adm_wait()
        grown = _free_bytes()
        assert held - grown > (200 << 20), (held, grown)      # 48 x 1080p: 2.6 B per luma pixel = 261 MiB of a bands
        eng.trim()
        dr._owner.free()
        dd._owner.free()
        after = _free_bytes()
        assert abs(after - base) <= (64 << 20), (base, held, grown, after)
        again = eng.adm(r[:1], d[:1], planes)
        assert small.tobytes() == again.tobytes() == big[:1].tobytes()


def test_the_other_modes_keep_their_results_next_to_adm():
    """PSNR / Gaussian SSIM, MS-SSIM, VIF and a complexity batch before and after ADM batches on one ctx: the same bits"""
    import rtvqa_amd
    from rtvqa_amd import _native as N
    from rtvqa_amd import synth
    r, d, planes = K.frames("yuv420p", 322, 386, 8, "noise", seed=4, n=3)
    bgr = synth.s_natural(5, 96, 128, seed=3)
    with rtvqa_amd.Engine(0) as eng:
        def others():
            g = eng.quality(r, d, planes, N.SSIM_GAUSS)
            ms = eng.quality(r, d, planes, N.SSIM_MS, scales=True)
            v = eng.vif(r, d, planes)
            c = eng.complexity(bgr[1:], bgr[0])
            return [g.tobytes()] + [np.ascontiguousarray(x).tobytes() for x in ms] + [v.tobytes(), c.tobytes()]
        before = others()
        a1 = eng.adm(r, d, planes)
        after = others()
        assert before == after
        assert eng.adm(r, d, planes).tobytes() == a1.tobytes()
        _check(a1[:1], r[:1], d[:1], planes, 8, "next to the other modes", count=False)


def test_one_pass_entry_points(tmp_path):
    """run_ffmpeg_metrics(.., adm=True): the psnr / ssim logs are byte for byte those of the run without, plus the JSON;
    with vif=True as well the VIF part of the JSON is what vif=True alone writes; process_video_and_extract_metrics with
    "adm": true: the row gains ADM2 and ADM_scale0..3 after the VIF columns and nothing else moves"""
    import rtvqa_amd
    from rtvqa_amd import frames, synth
    from rtvqa_amd import video_processing as vp
    h, w, n = 96, 128, 7
    r, d, planes = K.frames("yuv420p", h, w, 8, "noise", seed=6, n=n)
    pr, pd = str(tmp_path / "ref.y4m"), str(tmp_path / "enc.y4m")
    frames.write_y4m(pr, r, h, w)
    frames.write_y4m(pd, d, h, w)
    logs = {k: [str(tmp_path / ("%s_%s.log" % (k, t))) for t in ("psnr", "ssim", "vmaf")] for k in ("plain", "vif", "adm", "both")}
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["plain"], batch_size=3) is None
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["vif"], batch_size=3, vif=True) is None
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["adm"], batch_size=3, adm=True) is None
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["both"], batch_size=3, vif=True, adm=True) is None
    assert not os.path.exists(logs["plain"][2])
    for k in (0, 1):
        for kind in ("vif", "adm", "both"):
            assert open(logs["plain"][k], "rb").read() == open(logs[kind][k], "rb").read()
    doc = json.load(open(logs["adm"][2]))
    both, vdoc = json.load(open(logs["both"][2])), json.load(open(logs["vif"][2]))
    names = ["adm2"] + ["adm_scale%d" % s for s in range(4)]
    assert "vmaf" not in json.dumps(both) and len(doc["frames"]) == n
    assert sorted(doc["frames"][0]["metrics"]) == sorted(names) and sorted(doc["pooled_metrics"]) == sorted(names)
    assert list(both["frames"][0]["metrics"]) == ["vif_scale%d" % s for s in range(4)] + names
    for i in range(n):
        assert {k: v for k, v in both["frames"][i]["metrics"].items() if k.startswith("vif")} == vdoc["frames"][i]["metrics"]
        assert {k: v for k, v in both["frames"][i]["metrics"].items() if k.startswith("adm")} == doc["frames"][i]["metrics"]
    assert {k: v for k, v in both["pooled_metrics"].items() if k.startswith("vif")} == vdoc["pooled_metrics"]
    with rtvqa_amd.Engine(0) as eng:
        want = eng.adm(r, d, planes)
    for i in range(n):
        m = doc["frames"][i]["metrics"]
        assert [m["adm_scale%d" % s] for s in range(4)] == [float(x) for x in want[i, 0]["scale"]]
        assert m["adm2"] == float(want[i, 0]["adm2"])
    x = want[:, 0]["adm2"]
    p = doc["pooled_metrics"]["adm2"]
    assert sorted(p) == ["harmonic_mean", "max", "mean", "min"]
    assert abs(p["mean"] - x.mean()) <= 1e-15 and p["min"] == x.min() and p["max"] == x.max()
    assert abs(p["harmonic_mean"] - (n / (1.0 / (x + 1.0)).sum() - 1.0)) <= 1e-15
    _check(want[:2], r[:2], d[:2], planes, 8, "entry point", count=False)
    bgr = synth.s_natural(n, h, w, seed=12)
    cfg = {"crf": 23, "resize_width": 64, "resize_height": 64, "frame_interval": 1, "batch_size": 2}
    row0 = vp.process_video_and_extract_metrics(pr, pd, dict(cfg, vif=True), csv_file=str(tmp_path / "row0.csv"), column_order="fixed",
                                                encoded_bgr=bgr)
    row1 = vp.process_video_and_extract_metrics(pr, pd, dict(cfg, vif=True, adm=True), csv_file=str(tmp_path / "row1.csv"),
                                                column_order="fixed", encoded_bgr=bgr)
    row2 = vp.process_video_and_extract_metrics(pr, pd, dict(cfg, adm=True), csv_file=str(tmp_path / "row2.csv"), column_order="fixed",
                                                encoded_bgr=bgr)
    assert "VMAF" not in row1
    added = [k for k in row1 if k not in row0]
    assert added == ["ADM2", "ADM_scale0", "ADM_scale1", "ADM_scale2", "ADM_scale3"]
    assert list(row1)[:10] == list(row0)[:10] and list(row1)[10:15] == added and list(row1)[15:] == list(row0)[10:]
    assert list(row2) == [k for k in row1 if not k.startswith("VIF_")]
    for k in row0:
        assert row0[k] == row1[k] or (row0[k] != row0[k] and row1[k] != row1[k]), k
    assert abs(row1["ADM2"] - want[:, 0]["adm2"].mean()) <= 1e-15 and row2["ADM2"] == row1["ADM2"]
    for s in range(4):
        assert abs(row1["ADM_scale%d" % s] - want[:, 0]["scale"][:, s].mean()) <= 1e-15


def test_profile_shows_four_scales_and_four_reductions_per_plane_group():
    import rtvqa_amd
    from rtvqa_amd import _native as N
    r, d, planes = K.frames("yuv420p", 96, 128, 8, "noise", seed=9, n=3)
    with rtvqa_amd.Engine(0) as eng:
        eng.lib.vqa_kernel_name.restype = C.c_char_p
        assert eng.lib.vqa_kernel_name(N.K_ADM) == b"k_adm_scale" and eng.lib.vqa_kernel_name(N.K_ADM_REDUCE) == b"k_adm_reduce"
        eng.profile(True)
        eng.adm(r, d, planes)
        prof = eng.profile_read(reset=True)
        assert prof["k_adm_scale"][1] == 8 and prof["k_adm_reduce"][1] == 8, prof       # luma; the two chroma planes together
        assert prof["k_adm_scale"][0] > 0 and prof["k_adm_reduce"][0] > 0
        assert "k_vif_stats" not in prof
        rb, db, pb = K.frames("bgr24", 40, 56, 8, "noise", seed=9, n=2)
        eng.adm(rb, db, pb)
        prof = eng.profile_read(reset=True)
        assert prof["k_adm_scale"][1] == 4 and prof["k_adm_reduce"][1] == 4, prof       # B, G, R are one group
        eng.quality(r, d, planes, N.SSIM_GAUSS)
        eng.vif(r, d, planes)
        prof = eng.profile_read(reset=True)
        assert "k_adm_scale" not in prof and "k_adm_reduce" not in prof, prof
        ms, cnt = C.c_double(0), C.c_int64(0)
        for bad in (14, 15, N.K_COUNT_EXT):
            assert eng.lib.vqa_profile_read(eng.ctx, bad, C.byref(ms), C.byref(cnt), 0) == N.VQA_ERR_INVALID
