"""GPU: PSNR's SSE and both SSIM definitions on 9..16-bit samples and 4:2:0 / 4:2:2 / 4:4:4 / mono planes, through the C
ABI and the reference-shaped entry point, against the float64 / integer reference of tests/hbd_reference.py."""
import csv
import importlib.util
import json
import os

import numpy as np
import pytest

import hbd_reference as ref

pytestmark = pytest.mark.gpu

RTOL = 1e-4  # north_star's bar for SSIM floats (the existing suite's)
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("gauss", "ffmpeg")


def _mode(name):
    from rtvqa_amd import _native as N
    return N.SSIM_GAUSS if name == "gauss" else N.SSIM_FFMPEG


def _pair(n, h, w, chroma, depth, seed=0, noise=3):
    """n frame pairs of natural-looking content at `depth` bits, planes back to back (yuv_planes' layout); dist = ref plus a
    few grey levels of noise, clipped to [0, 2^depth - 1].  -> (ref, dist, planes) with [n, samples] uint16 / uint8 frames"""
    from rtvqa_amd import synth
    from rtvqa_amd.engine import yuv_planes
    planes = yuv_planes(h, w, chroma, depth)
    mx = (1 << depth) - 1
    rng = np.random.default_rng(seed)
    parts_r, parts_d = [], []
    for k, (pw, ph, *_rest) in enumerate(planes):
        g = synth.s_natural(n, max(ph, 16), max(pw, 16), seed=seed * 7 + k)[:, :ph, :pw, k % 3].astype(np.int64)
        x = (g << (depth - 8)) + rng.integers(0, 1 << (depth - 8), g.shape) if depth > 8 else g
        d = np.clip(x + rng.integers(-noise, noise + 1, x.shape) * (1 << max(depth - 8, 0)), 0, mx)
        parts_r.append(x.reshape(n, -1))
        parts_d.append(d.reshape(n, -1))
    dt = np.uint16 if depth > 8 else np.uint8
    return np.concatenate(parts_r, 1).astype(dt), np.concatenate(parts_d, 1).astype(dt), planes


def _check(res, r, d, planes, mode, depth):
    for i in range(r.shape[0]):
        sse, ssim = ref.frame_quality(r[i], d[i], planes, mode, depth)
        for p in range(len(planes)):
            assert int(res[i, p]["sse"]) == sse[p], (i, p, int(res[i, p]["sse"]), sse[p])
            got = float(res[i, p]["ssim"])
            assert abs(got - ssim[p]) <= RTOL * abs(ssim[p]), (i, p, got, ssim[p])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("chroma", ["420", "422", "444", "mono"])
@pytest.mark.parametrize("depth", [10, 12, 16])
@pytest.mark.parametrize("h,w", [(67, 259), (135, 241)])
def test_high_depth_planes_match_the_reference(engine, mode, chroma, depth, h, w):
    r, d, planes = _pair(2, h, w, chroma, depth, seed=depth + h)
    res = engine.quality(r, d, planes, _mode(mode))
    _check(res, r, d, planes, mode, depth)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("depth", [10, 16])
def test_1080p_420(engine, mode, depth):
    r, d, planes = _pair(1, 1080, 1920, "420", depth, seed=5, noise=6)
    _check(engine.quality(r, d, planes, _mode(mode)), r, d, planes, mode, depth)


@pytest.mark.parametrize("mode", MODES)
def test_tiny_planes_are_refused_as_at_8_bits(engine, mode):
    from rtvqa_amd import _native as N
    from rtvqa_amd.engine import yuv_planes
    outcomes = []
    for depth in (8, 10):
        r, d, planes = _pair(1, 2, 2, "420", depth)
        try:
            engine.quality(r, d, planes, _mode(mode))
            outcomes.append("ok")
        except N.VqaError as e:
            outcomes.append(e.status)
    assert outcomes[0] == outcomes[1] == N.VQA_ERR_UNSUPPORTED
    assert yuv_planes(2, 2, "420", 10)[1][:2] == (1, 1)


@pytest.mark.parametrize("mode", MODES)
def test_known_answers(engine, mode):
    from rtvqa_amd.engine import yuv_planes
    h, w = 67, 259
    r, _d, planes = _pair(3, h, w, "420", 10, seed=1)
    res = engine.quality(r, r, planes, _mode(mode))
    assert (res["sse"] == 0).all()
    if mode == "ffmpeg":
        assert (res["ssim"] == 1.0).all()   # numerator == denominator: the same integers through the same double operations
    else:
        assert np.allclose(res["ssim"], 1.0, rtol=0, atol=1e-6)
    r = np.minimum(r, 1022).astype(np.uint16)
    res = engine.quality(r, r + 1, planes, _mode(mode))
    assert [list(map(int, row)) for row in res["sse"]] == [[pw * ph for pw, ph, *_ in planes]] * 3
    # 10-bit frames that are 8-bit frames << 2: every squared difference times 16
    r8, d8, planes8 = _pair(3, h, w, "420", 8, seed=2)
    res8 = engine.quality(r8, d8, planes8, _mode(mode))
    res10 = engine.quality(r8.astype(np.uint16) << 2, d8.astype(np.uint16) << 2, yuv_planes(h, w, "420", 10), _mode(mode))
    assert (res10["sse"] == 16 * res8["sse"]).all()


def test_batches_and_residences_give_the_same_bits(engine):
    from rtvqa_amd import video_processing as vp
    h, w = 67, 259
    r, d, planes = _pair(64, h, w, "420", 10, seed=3)
    for mode in MODES:
        whole = engine.quality(r, d, planes, _mode(mode))
        _check(whole[:2], r[:2], d[:2], planes, mode, 10)
        for bs in (1, 7):
            parts = np.concatenate([engine.quality(r[a:a + bs], d[a:a + bs], planes, _mode(mode)) for a in range(0, 64, bs)])
            assert parts.tobytes() == whole.tobytes(), (mode, bs)
        # device-resident and pinned inputs
        dr, dd = engine.upload(r), engine.upload(d)
        assert dr.itemsize == 2
        assert engine.quality(dr, dd, planes, _mode(mode)).tobytes() == whole.tobytes()
        pr, pd = engine.alloc_pinned(r.shape, np.uint16), engine.alloc_pinned(d.shape, np.uint16)
        pr[:], pd[:] = r, d
        assert engine.is_pinned(pr)
        assert engine.quality(pr, pd, planes, _mode(mode)).tobytes() == whole.tobytes()
        # the one-pass stream (pinned ring for pageable arrays, the copy lane, two lanes) at batch sizes 1, 7, 64
        for src_r, src_d in ((r, d), (pr, pd), (dr, dd)):
            for bs in (1, 7, 64):
                sse, ssim, _sizes = vp.frame_quality(src_r, src_d, "yuv420p10le", mode, h, w, batch_size=bs)
                assert sse.tobytes() == np.ascontiguousarray(whole["sse"]).tobytes(), (mode, bs)
                assert ssim.tobytes() == np.ascontiguousarray(whole["ssim"]).tobytes(), (mode, bs)
        engine.free_pinned(pr)
        engine.free_pinned(pd)


def test_dtype_must_match_the_depth(engine):
    from rtvqa_amd.engine import yuv420p_planes, yuv_planes
    r, d, planes = _pair(1, 32, 48, "420", 10)
    with pytest.raises(ValueError):
        engine.quality(r, d, yuv420p_planes(32, 48))
    with pytest.raises(ValueError):
        engine.quality(engine.upload(r[:, :32 * 48 * 3 // 2].astype(np.uint8)), engine.upload(d[:, :32 * 48 * 3 // 2].astype(np.uint8)),
                       yuv_planes(32, 48, "420", 10))


def test_bad_depths_are_invalid_arguments_and_the_context_survives(engine):
    from rtvqa_amd import _native as N
    from rtvqa_amd.engine import plane_descs, yuv420p_planes, yuv_planes
    h, w = 32, 48
    r, d, planes = _pair(2, h, w, "420", 10)
    fb = r.shape[1] * 2

    def submit(pl):
        descs = plane_descs(pl)
        st = engine.lib.vqa_quality_submit(engine.ctx, r.ctypes.data, d.ctypes.data, N.VQA_MEM_HOST, 2, fb, fb, descs, len(pl),
                                           N.SSIM_FFMPEG)
        if st == N.VQA_OK:
            engine._pending_q = (2, len(pl), (r, d))
            engine.quality_wait()
        return st
    mixed = planes[:1] + [p[:5] for p in planes[1:]]                       # 10-bit luma, 8-bit chroma
    assert submit(mixed) == N.VQA_ERR_INVALID
    for bad in (7, 17, -1, 1):
        assert submit([p[:5] + (bad,) for p in planes]) == N.VQA_ERR_INVALID, bad
    odd = [(p[0], p[1], p[2], p[3] + 1, p[4], p[5]) for p in planes]       # an odd 16-bit row stride
    assert submit(odd) == N.VQA_ERR_INVALID
    odd_off = [planes[0], (planes[1][0], planes[1][1], planes[1][2] + 1) + planes[1][3:], planes[2]]
    assert submit(odd_off) == N.VQA_ERR_INVALID
    assert submit(planes) == N.VQA_OK
    _check(engine.quality(r, d, planes, N.SSIM_FFMPEG), r, d, planes, "ffmpeg", 10)
    assert yuv420p_planes(h, w) == [p[:5] for p in yuv_planes(h, w)]


def test_8bit_records_are_bit_identical_to_the_committed_golden(engine):
    """the 8-bit kernels did not change: test_quality_bgr_and_yuv420p's inputs give the records the GPU gave before 9..16-bit
    samples were added (tests/golden/quality8_records.json, scripts/gen_quality8_golden.py)"""
    spec = importlib.util.spec_from_file_location("gen_quality8_golden", os.path.join(REPO, "scripts", "gen_quality8_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(os.path.join(REPO, "tests", "golden", "quality8_records.json")) as f:
        want = json.load(f)
    got = gen.records(engine)
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k]["sse"] == want[k]["sse"], k
        assert got[k]["ssim"] == want[k]["ssim"], k


@pytest.mark.parametrize("ssim_mode", MODES)
def test_entry_point_on_a_10bit_y4m_pair(tmp_path, ssim_mode):
    """process_video_and_extract_metrics on a 10-bit 4:2:0 .y4m pair with the encoded stream's BGR frames: a CSV row whose
    PSNR / SSIM are FFmpeg's (peak 1023, components weighted by plane area) of the first frame pair"""
    from rtvqa_amd import frames, synth
    from rtvqa_amd import video_processing as vp
    h, w, n = 67, 259, 5
    r, d, planes = _pair(n, h, w, "420", 10, seed=11, noise=5)
    pr, pd = str(tmp_path / "ref.y4m"), str(tmp_path / "enc.y4m")
    frames.write_y4m(pr, r, h, w, pixfmt="yuv420p10le")
    frames.write_y4m(pd, d, h, w, pixfmt="yuv420p10le")
    enc = synth.s_natural(n, h, w, seed=12)
    cfg = {"crf": 23, "resize_width": 64, "resize_height": 64, "frame_interval": 1, "batch_size": 2, "ssim_mode": ssim_mode}
    out = str(tmp_path / "row.csv")
    m = vp.process_video_and_extract_metrics(pr, pd, cfg, csv_file=out, column_order="fixed", encoded_bgr=enc)
    rows = list(csv.reader(open(out)))
    assert len(rows) == 2 and "PSNR" in rows[0] and "SSIM" in rows[0]
    sse, ssim = ref.frame_quality(r[0], d[0], planes, ssim_mode, 10)
    areas = np.array([pw * ph for pw, ph, *_ in planes], np.float64)
    mse_avg = float(((np.array(sse) / areas) * (areas / areas.sum())).sum())
    assert abs(m["PSNR"] - 10 * np.log10(1023.0 ** 2 / mse_avg)) <= 6e-3, (m["PSNR"], mse_avg)
    want_all = float((np.array(ssim) * areas).sum() / areas.sum())
    assert abs(m["SSIM"] - want_all) <= (2e-6 if ssim_mode == "ffmpeg" else RTOL * want_all + 1e-6), (m["SSIM"], want_all)
    assert float(rows[1][rows[0].index("PSNR")]) == m["PSNR"]
    # run_ffmpeg_metrics alone: the stats files of every frame, y/u/v components at peak 1023
    pl, sl = str(tmp_path / "psnr.log"), str(tmp_path / "ssim.log")
    assert vp.run_ffmpeg_metrics(pr, pd, pl, sl, None, ssim_mode=ssim_mode, batch_size=3) is None
    lines = open(pl).read().splitlines()
    assert len(lines) == n and lines[0].startswith("n:1 mse_avg:") and " psnr_y:" in lines[0] and " psnr_v:" in lines[0]
    assert lines[0] == vp.psnr_stats_line(1, sse, [p[:2] for p in planes], "yuv", peak=1023).rstrip("\n")
    assert len(open(sl).read().splitlines()) == n
