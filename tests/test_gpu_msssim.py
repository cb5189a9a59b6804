"""GPU: multi-scale SSIM (VQA_SSIM_MS) through the C ABI, the engine and the reference-shaped entry point, against the
float64 reference of tests/msssim_reference.py (written from the definition in include/vqa.h)."""
import ctypes as C
import re

import numpy as np
import pytest

import hbd_reference as R
import msssim_reference as M

pytestmark = pytest.mark.gpu

BAR = 1e-4   # absolute, on every per-level mean: the project's bar for this window (tests/test_gpu_quality_hbd.py)

# geometry (h, w), depth, layout
GRID = [((161, 161), 8, "gray"), ((177, 263), 8, "bgr24"), ((270, 480), 8, "yuv444p"), ((322, 386), 10, "yuv420p10le"),
        ((333, 200), 16, "gray16le"), ((1080, 1920), 8, "yuv420p")]
STRUCTURED = ("noise3", "noise20", "blur")
CONTENTS = STRUCTURED + ("random",)


def _planes(layout, h, w):
    from rtvqa_amd import video_processing as vp
    return vp.LAYOUTS[layout][0](h, w)


def _texture(h, w, depth, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    ph = rng.uniform(0, 6.28, 4)
    v = (0.5 + 0.16 * np.sin(x / 2.3 + ph[0]) * np.cos(y / 3.1 + ph[1]) + 0.14 * np.sin((x + 2 * y) / 5.7 + ph[2])
         + 0.12 * np.cos((2 * x - y) / 17.0 + ph[3]))
    return np.clip(np.rint(v * ((1 << depth) - 1)), 0, (1 << depth) - 1).astype(np.int64)


def _plane_pair(h, w, depth, content, seed):
    mx = (1 << depth) - 1
    rng = np.random.default_rng(seed + 1000)
    if content == "random":
        return rng.integers(0, mx + 1, (h, w)), rng.integers(0, mx + 1, (h, w))
    a = _texture(h, w, depth, seed)
    if content == "blur":   # a half-pixel shift: the mean of horizontal neighbours, the last column kept
        b = np.concatenate([(a[:, :-1] + a[:, 1:] + 1) >> 1, a[:, -1:]], axis=1)
    else:
        k = 3 if content == "noise3" else 20
        b = np.clip(a + rng.integers(-k, k + 1, a.shape) * (1 << (depth - 8)), 0, mx)
    return a, b


def _frames(layout, h, w, depth, content, seed, n=1):
    """n frame pairs in `layout`: -> (ref, dist, planes) with [n, samples] arrays ([n, h, w, 3] for bgr24)"""
    planes = _planes(layout, h, w)
    dt = np.uint16 if depth > 8 else np.uint8
    isz = np.dtype(dt).itemsize
    size = max(p[2] + (p[1] - 1) * p[3] + (p[0] - 1) * p[4] + isz for p in planes) // isz
    out = [np.zeros((n, size), dt), np.zeros((n, size), dt)]
    for i in range(n):
        for k, p in enumerate(planes):
            pw, ph, off, rs, step = p[:5]
            pair = _plane_pair(ph, pw, depth, content, seed * 131 + i * 7 + k)
            for o, v in zip(out, pair):
                view = np.lib.stride_tricks.as_strided(o[i, off // isz:], shape=(ph, pw), strides=(rs, step))
                view[...] = v
    if layout == "bgr24":
        out = [o.reshape(n, h, w, 3) for o in out]
    return out[0], out[1], planes


def _flat(a):
    return a.reshape(a.shape[0], -1)


def _ms(engine, r, d, planes):
    from rtvqa_amd import _native as N
    return engine.quality(r, d, planes, N.SSIM_MS, scales=True)


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("geom,depth,layout", GRID, ids=["%dx%d-%s" % (g[0][0], g[0][1], g[2]) for g in GRID])
def test_parity_with_the_reference(engine, geom, depth, layout, content):
    """per-level cs_s and ssim_s within 1e-4 absolute of the float64 reference; sse exact; the value is the definition's
    product of the engine's own ten means (1e-12 relative) and within the propagated per-level bar of the reference's;
    ssim[0] is bit for bit what VQA_SSIM_GAUSS returns for the pair"""
    from rtvqa_amd import _native as N
    h, w = geom
    r, d, planes = _frames(layout, h, w, depth, content, seed=h + depth)
    res, cs, ssim = _ms(engine, r, d, planes)
    assert res.shape == (1, len(planes)) and cs.shape == ssim.shape == (1, len(planes), 5)
    sse_w, cs_w, ssim_w, ms_w = M.frame_msssim(_flat(r)[0], _flat(d)[0], planes, depth)
    for p in range(len(planes)):
        print(layout, content, "plane", p, "cs err", np.abs(cs[0, p] - cs_w[p]).max(), "ssim err", np.abs(ssim[0, p] - ssim_w[p]).max(),
              "ms", float(res[0, p]["ssim"]), "ref", ms_w[p])
    for p in range(len(planes)):
        assert int(res[0, p]["sse"]) == sse_w[p], (p, int(res[0, p]["sse"]), sse_w[p])
        assert np.abs(cs[0, p] - cs_w[p]).max() <= BAR, (p, cs[0, p], cs_w[p])
        assert np.abs(ssim[0, p] - ssim_w[p]).max() <= BAR, (p, ssim[0, p], ssim_w[p])
        got = float(res[0, p]["ssim"])
        own = M.combine(cs[0, p], ssim[0, p])                                  # (a)
        assert abs(got - own) <= 1e-12 * own, (p, got, own)
        bound = M.value_bound(cs_w[p], ssim_w[p], BAR)                          # (b)
        if content in STRUCTURED:
            assert bound is not None, (p, M.terms(cs_w[p], ssim_w[p]))          # no structured case sits near the clamp
        if bound is not None:
            assert abs(got - ms_w[p]) <= bound, (p, got, ms_w[p], bound)
        if min(list(cs_w[p][:4]) + [ssim_w[p][4]]) < -1e-3:
            assert got == 0.0, (p, got)
    single = engine.quality(r, d, planes, N.SSIM_GAUSS)
    assert np.ascontiguousarray(ssim[:, :, 0]).tobytes() == np.ascontiguousarray(single["ssim"]).tobytes()
    assert np.ascontiguousarray(res["sse"]).tobytes() == np.ascontiguousarray(single["sse"]).tobytes()


def test_a_negative_cs_mean_gives_exactly_zero(engine):
    from rtvqa_amd.engine import gray_planes
    from test_msssim_host import negative_cs_pair
    a, b = negative_cs_pair()
    cs_w, ssim_w, ms_w = M.msssim(a, b, 255)
    assert cs_w[1] < -1e-3 and ms_w == 0.0
    res, cs, ssim = _ms(engine, a.astype(np.uint8)[None].reshape(1, -1), b.astype(np.uint8)[None].reshape(1, -1), gray_planes(177, 263))
    assert np.abs(cs[0, 0] - cs_w).max() <= BAR and np.abs(ssim[0, 0] - ssim_w).max() <= BAR
    assert cs[0, 0, 1] < 0 and float(res[0, 0]["ssim"]) == 0.0


@pytest.mark.parametrize("depth,layout", [(8, "yuv420p"), (10, "yuv420p10le"), (8, "bgr24")])
def test_batches_positions_and_residences_give_the_same_bits(engine, depth, layout):
    """the same pair gives the same bits in batches of 1, 3 and 17, wherever it sits in a batch, from host, pinned and
    device-resident memory, and run to run (k_quality.hip: what the single-buffer barrier discipline protects)"""
    from rtvqa_amd import _native as N
    from rtvqa_amd import video_processing as vp
    h, w = 322, 386
    r, d, planes = _frames(layout, h, w, depth, "noise3", seed=21, n=17)
    dt = r.dtype
    whole = _ms(engine, r, d, planes)
    want = [np.ascontiguousarray(x).tobytes() for x in whole]

    def same(got, sel=slice(None)):
        return [np.ascontiguousarray(x).tobytes() for x in got] == [np.ascontiguousarray(x[sel]).tobytes() for x in whole]
    assert [np.ascontiguousarray(x).tobytes() for x in _ms(engine, r, d, planes)] == want              # run to run
    for bs in (1, 3):
        parts = [_ms(engine, r[a:a + bs], d[a:a + bs], planes) for a in range(0, 17, bs)]
        assert same([np.concatenate([p[k] for p in parts]) for k in range(3)]), bs
    order = np.arange(17)[::-1].copy()                                                                   # other positions
    assert same(_ms(engine, r[order], d[order], planes), order)
    dr, dd = engine.upload(r), engine.upload(d)
    assert same(_ms(engine, dr, dd, planes))
    pr, pd = engine.alloc_pinned(r.shape, dt), engine.alloc_pinned(d.shape, dt)
    pr[:], pd[:] = r, d
    assert engine.is_pinned(pr)
    assert same(_ms(engine, pr, pd, planes))
    # the one-pass stream: pinned ring, two alternating engines, per-scale series handed to the caller
    for src_r, src_d in ((r, d), (pr, pd), (dr, dd)):
        for bs in (3, 17):
            sse, ms, _sizes, sc = vp.frame_quality(src_r, src_d, layout, "msssim", h, w, batch_size=bs, scales=True)
            assert sse.tobytes() == np.ascontiguousarray(whole[0]["sse"]).tobytes(), bs
            assert ms.tobytes() == np.ascontiguousarray(whole[0]["ssim"]).tobytes(), bs
            assert sc["cs"].tobytes() == want[1] and sc["ssim"].tobytes() == want[2], bs
    chunks = []
    sse, ms, _sizes = vp.frame_quality(r, d, layout, "msssim", h, w, batch_size=5, on_chunk=lambda f0, a, b: chunks.append((f0, a, b)))
    assert [c[0] for c in chunks] == [0, 5, 10, 15]
    assert np.concatenate([c[2] for c in chunks]).tobytes() == np.ascontiguousarray(whole[0]["ssim"]).tobytes() == ms.tobytes()
    engine.free_pinned(pr)
    engine.free_pinned(pd)


def test_known_answers(engine):
    """identical frames: exactly 1.0 per plane; a constant against a constant: cs_s = 1 and MS-SSIM = l(level 4)^w_4"""
    h, w = 322, 386
    for depth, layout in ((8, "yuv420p"), (10, "yuv420p10le"), (8, "bgr24")):
        r, _d, planes = _frames(layout, h, w, depth, "noise3", seed=4, n=2)
        res, cs, ssim = _ms(engine, r, r, planes)
        print(layout, "identical: 1 - ms", 1.0 - res["ssim"].ravel(), "1 - cs", (1.0 - cs).max(), "1 - ssim", (1.0 - ssim).max())
        assert (res["sse"] == 0).all()
        assert (res["ssim"] == 1.0).all(), 1.0 - res["ssim"]
    for depth, layout, a, b in ((8, "gray", 100, 140), (10, "gray10le", 400, 560), (16, "gray16le", 65535, 40000), (8, "gray", 255, 128)):
        mx = (1 << depth) - 1
        dt = np.uint16 if depth > 8 else np.uint8
        planes = _planes(layout, 170, 161)
        r, d = np.full((1, 170 * 161), a, dt), np.full((1, 170 * 161), b, dt)
        res, cs, ssim = _ms(engine, r, d, planes)
        c1 = (.01 * mx) ** 2
        lum = (2.0 * a * b + c1) / (float(a) ** 2 + float(b) ** 2 + c1)
        print(layout, a, b, "cs", cs[0, 0], "ssim", ssim[0, 0], "lum", lum, "ms", float(res[0, 0]["ssim"]), lum ** M.WEIGHTS[4])
        assert np.abs(cs[0, 0] - 1.0).max() <= BAR
        assert np.abs(ssim[0, 0] - lum).max() <= BAR
        want = lum ** M.WEIGHTS[4]
        assert abs(float(res[0, 0]["ssim"]) - want) <= M.value_bound([1.0] * 5, [lum] * 5, BAR)
        assert int(res[0, 0]["sse"]) == 170 * 161 * (a - b) ** 2


def _submit(engine, r, d, planes, mode):
    from rtvqa_amd import _native as N
    from rtvqa_amd.engine import plane_descs
    fb = _flat(r).shape[1] * r.dtype.itemsize
    return engine.lib.vqa_quality_submit(engine.ctx, r.ctypes.data, d.ctypes.data, N.VQA_MEM_HOST, r.shape[0], fb, fb,
                                         plane_descs(planes), len(planes), mode)


def test_refusals_leave_the_context_usable(engine):
    from rtvqa_amd import _native as N
    from rtvqa_amd.engine import gray_planes, yuv420p_planes, yuv_planes
    for h, w in ((160, 400), (400, 160)):
        z = np.zeros((1, h * w), np.uint8)
        assert _submit(engine, z, z, gray_planes(h, w), N.SSIM_MS) == N.VQA_ERR_UNSUPPORTED, (h, w)
        assert _submit(engine, z, z, gray_planes(h, w), N.SSIM_GAUSS) == N.VQA_OK
        engine._pending_q = (1, 1, (z,))
        engine.quality_wait()
    z = np.zeros((1, 320 * 320 * 3 // 2), np.uint8)                      # 4:2:0 at 320: the chroma planes are 160
    assert _submit(engine, z, z, yuv420p_planes(320, 320), N.SSIM_MS) == N.VQA_ERR_UNSUPPORTED
    z16 = np.zeros((1, 322 * 322 * 3 // 2), np.uint16)
    p10 = yuv_planes(322, 322, "420", 10)
    # what VQA_SSIM_GAUSS refuses is refused the same way: mixed depths, bad depths, odd 16-bit strides
    assert _submit(engine, z16, z16, p10[:1] + [p[:5] for p in p10[1:]], N.SSIM_MS) == N.VQA_ERR_INVALID
    assert _submit(engine, z16, z16, [p[:5] + (17,) for p in p10], N.SSIM_MS) == N.VQA_ERR_INVALID
    assert _submit(engine, z16, z16, [(p[0], p[1], p[2], p[3] + 1, p[4], p[5]) for p in p10], N.SSIM_MS) == N.VQA_ERR_INVALID
    assert _submit(engine, z16, z16, p10, 3) == N.VQA_ERR_INVALID
    # vqa_quality_wait_ms with scales after a Gaussian submit: VQA_ERR_STATE, and the batch is still there for vqa_quality_wait
    r, d, planes = _frames("yuv420p", 322, 386, 8, "noise3", seed=8)
    assert _submit(engine, r, d, planes, N.SSIM_GAUSS) == N.VQA_OK
    out = (N.VqaPlaneMetrics * 3)()
    sc = (N.VqaMsScales * 3)()
    assert engine.lib.vqa_quality_wait_ms(engine.ctx, out, sc, 3) == N.VQA_ERR_STATE
    assert engine.lib.vqa_quality_wait_ms(engine.ctx, out, None, 3) == N.VQA_OK
    gauss = [out[i].ssim for i in range(3)]
    # plain vqa_quality_wait after an MS submit; the ctx computes as before
    assert _submit(engine, r, d, planes, N.SSIM_MS) == N.VQA_OK
    assert engine.lib.vqa_quality_wait(engine.ctx, out, 3) == N.VQA_OK
    res, cs, ssim = _ms(engine, r, d, planes)
    assert [out[i].ssim for i in range(3)] == [float(v) for v in res[0]["ssim"]]
    assert [float(v) for v in ssim[0, :, 0]] == gauss


def _free_bytes():
    import torch
    return torch.cuda.mem_get_info(0)[0]


def test_trim_returns_the_pyramid_scratch():
    """vqa_trim after a multi-scale batch: the device's free memory is back within 64 MiB (the existing trim test's margin)
    of what it was, a pending batch refuses the trim, and a following batch gives the same bits"""
    import rtvqa_amd
    from rtvqa_amd import _native as N
    h, w, n = 1080, 1920, 48
    r, d, planes = _frames("yuv420p", h, w, 8, "noise3", seed=2)
    r, d = np.repeat(r, n, axis=0), np.repeat(d, n, axis=0)
    with rtvqa_amd.Engine(0) as eng:
        small = eng.quality(r[:1], d[:1], planes, N.SSIM_MS, scales=True)
        eng.trim()
        base = _free_bytes()
        dr, dd = eng.upload(r), eng.upload(d)
        held = _free_bytes()
        eng.quality_submit(dr, dd, planes, N.SSIM_MS)
        assert eng.lib.vqa_trim(eng.ctx) == N.VQA_ERR_STATE
        big = eng.quality_wait(scales=True)
        grown = _free_bytes()
        assert held - grown > (200 << 20), (held, grown)      # 48 x 1080p: 2.7 B per luma pixel = 265 MiB of levels
        eng.trim()
        dr._owner.free()
        dd._owner.free()
        after = _free_bytes()
        assert abs(after - base) <= (64 << 20), (base, held, grown, after)
        again = eng.quality(r[:1], d[:1], planes, N.SSIM_MS, scales=True)
        for a, b, c in zip(small, again, big):
            assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes() == np.ascontiguousarray(c[:1]).tobytes()


def test_entry_point_on_a_10bit_y4m_pair(tmp_path):
    """run_ffmpeg_metrics(.., ssim_mode="msssim") on a 10-bit 4:2:0 .y4m pair: the ssim stats file keeps FFmpeg's line
    format, its component values are MS-SSIM within the per-value bound, All: is area-weighted; the config key reaches
    the CSV's SSIM column"""
    from rtvqa_amd import frames, synth
    from rtvqa_amd import video_processing as vp
    h, w, n = 322, 386, 4
    r, d, planes = _frames("yuv420p10le", h, w, 10, "noise20", seed=6, n=n)
    pr, pd = str(tmp_path / "ref.y4m"), str(tmp_path / "enc.y4m")
    frames.write_y4m(pr, r, h, w, pixfmt="yuv420p10le")
    frames.write_y4m(pd, d, h, w, pixfmt="yuv420p10le")
    pl, sl = str(tmp_path / "psnr.log"), str(tmp_path / "ssim.log")
    assert vp.run_ffmpeg_metrics(pr, pd, pl, sl, None, ssim_mode="msssim", batch_size=3) is None
    lines = open(sl).read().splitlines()
    assert len(lines) == n
    sizes = [p[:2] for p in planes]
    areas = np.array([pw * ph for pw, ph in sizes], np.float64)
    pat = re.compile(r"^n:(\d+) Y:(\d\.\d{6}) U:(\d\.\d{6}) V:(\d\.\d{6}) All:(\d\.\d{6}) \((\d+\.\d{6}|inf)\)$")
    all_ref = re.compile(r"All:(\d+\.\d+)")                      # the reference's extract_metrics_from_logs regex for SSIM
    first_all = None
    for i, line in enumerate(lines):
        sse_w, cs_w, ssim_w, ms_w = M.frame_msssim(r[i], d[i], planes, 10)
        want = vp.ssim_stats_line(i + 1, ms_w, sizes, "yuv").rstrip("\n")
        m, mw = pat.match(line), pat.match(want)
        assert m and mw, (line, want)
        assert m.group(1) == mw.group(1) == str(i + 1)
        bounds = [M.value_bound(cs_w[p], ssim_w[p], BAR) for p in range(3)]
        assert None not in bounds
        for p in range(3):
            assert abs(float(m.group(2 + p)) - float(mw.group(2 + p))) <= bounds[p] + 1e-6, (i, p, line, want)   # (+ the text's 6 digits)
        all_bound = float((np.array(bounds) * areas).sum() / areas.sum()) + 1e-6
        assert abs(float(m.group(5)) - float(mw.group(5))) <= all_bound, (line, want)
        assert abs(float(all_ref.search(line).group(1)) - float((ms_w * areas).sum() / areas.sum())) <= all_bound
        if i == 0:
            first_all = float((ms_w * areas).sum() / areas.sum()), all_bound
    assert open(pl).read().splitlines()[0] == vp.psnr_stats_line(1, M.frame_msssim(r[0], d[0], planes, 10)[0], sizes, "yuv", peak=1023).rstrip("\n")
    cfg = {"crf": 23, "resize_width": 64, "resize_height": 64, "frame_interval": 1, "batch_size": 2, "ssim_mode": "msssim"}
    row = vp.process_video_and_extract_metrics(pr, pd, cfg, csv_file=str(tmp_path / "row.csv"), column_order="fixed",
                                               encoded_bgr=synth.s_natural(n, h, w, seed=12))
    assert abs(row["SSIM"] - first_all[0]) <= first_all[1], (row["SSIM"], first_all)


def test_profile_shows_one_pyramid_and_five_scales_per_plane_group():
    import rtvqa_amd
    from rtvqa_amd import _native as N
    r, d, planes = _frames("yuv420p", 322, 386, 8, "noise3", seed=9, n=3)
    with rtvqa_amd.Engine(0) as eng:
        eng.lib.vqa_kernel_name.restype = C.c_char_p
        assert eng.lib.vqa_kernel_name(N.K_MS_PYRAMID) == b"k_ms_pyramid"
        eng.set_overlap(False)
        eng.profile(True)
        eng.quality(r, d, planes, N.SSIM_MS)
        prof = eng.profile_read(reset=True)
        assert prof["k_ms_pyramid"][1] == 2 and prof["k_ssim_gauss"][1] == 10, prof       # luma; the two chroma planes together
        assert prof["k_ms_pyramid"][0] > 0 and prof["k_ssim_gauss"][0] > 0
        rb, db, pb = _frames("bgr24", 177, 263, 8, "noise3", seed=9, n=2)
        eng.quality(rb, db, pb, N.SSIM_MS)
        prof = eng.profile_read(reset=True)
        assert prof["k_ms_pyramid"][1] == 1 and prof["k_ssim_gauss"][1] == 5, prof        # B, G, R are one group
        eng.quality(r, d, planes, N.SSIM_GAUSS)
        prof = eng.profile_read(reset=True)
        assert "k_ms_pyramid" not in prof and prof["k_ssim_gauss"][1] == 2, prof
