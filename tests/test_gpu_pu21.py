"""GPU: PU21-PSNR / PU21-SSIM (vqa_pu21_submit / vqa_pu21_wait) against the restatements of tests/pu21_reference.py (written from
the definition in include/vqa.h).

The parity matrix runs ONCE in a child process on the LAB library, which alone can read the two q_Y maps back; the child stores
every case's records and maps and the tests below check them:
  maps      |q_gpu - q_restatement| <= 1 at every sample (the device's double chain is within a few ulp of NumPy's, orders below
            the quantum of 2^-16; one such ulp may flip one rint)
  words     from the GPU's OWN maps: the two sse_y half-words equal the integer sums EXACTLY, and |ssim_q - sum u| <= windows, one
            unit a window (fp64 evaluation error of about 1e-10 against a quantum of 6e-8)
  doubles   the record is the host formula of its own words; mse_y, mse_rgb and pu_ssim against the UNQUANTISED restatement within
            the bars of test_pu21_host.py, unchanged (mse: 2^-15 sqrt(mse) + 2^-32, derived; pu_ssim: pu21_reference.SSIM_BAR)
Everything else - batch invariance from every memory and view, the state machine, the entry points - runs in this process on the
shipped library, which the child's records of three cases tie to the lab one byte for byte."""
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

import pu21_cases as PC
import pu21_reference as R

pytestmark = pytest.mark.gpu

FIELDS = ("sse_y_lo", "sse_y_hi", "sse_rgb_lo", "sse_rgb_hi", "ssim_q", "windows", "mse_y", "mse_rgb", "pu_psnr", "pu_psnr_rgb",
          "pu_ssim")
WORST = {"map": 0, "u": 0.0, "mse": 0.0, "ssim": 0.0, "tag_map": "", "tag_u": "", "tag_mse": "", "tag_ssim": ""}


def _child(out_path):
    import rtvqa_amd
    got = {}
    with rtvqa_amd.Engine(0) as eng:
        assert eng.lib.vqa_build_flavour() == 3
        for k, case in enumerate(PC.matrix()):
            g, d, lay, c, tn, t, full = case
            r, x, planes = PC.case_clip(case)
            rec, maps = eng.pu21(r, x, planes, transfer=tn, full_range=full, maps=True)
            assert maps.shape == (PC.N_FRAMES, 2, g[0], g[1]) and maps.dtype == np.uint32
            got["rec%d" % k] = np.frombuffer(rec.tobytes(), np.uint8)
            got["map%d" % k] = maps
    np.savez(out_path, **got)
    print("PU21-LAB-OK", len(got))


@pytest.fixture(scope="module")
def lab(tmp_path_factory):
    from rtvqa_amd import _native as N
    from rtvqa_amd.engine import PU21_DTYPE
    out = str(tmp_path_factory.mktemp("pu21lab") / "lab.npz")
    env = dict(os.environ, VQA_LIB_PATH=N.LAB_LIB_PATH)
    env.pop("VQA_PU21_SUBSLICE", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True, timeout=300, cwd=REPO)
    assert r.returncode == 0 and "PU21-LAB-OK" in r.stdout, (r.stdout[-300:], r.stderr[-2000:])
    with np.load(out) as z:
        return {k: (np.frombuffer(z[k].tobytes(), PU21_DTYPE) if k.startswith("rec") else z[k]) for k in z.files}


@pytest.mark.parametrize("k", range(len(PC.matrix())), ids=PC.matrix_ids())
def test_parity_on_every_shape_content_and_transfer(lab, k):
    case = PC.matrix()[k]
    (h, w), content = case[0], case[3]
    tag = PC.case_id(case)
    rec, maps = lab["rec%d" % k], lab["map%d" % k]
    assert rec.shape == (PC.N_FRAMES,) and rec.dtype.names == FIELDS
    for i, (flt, qrec, qa, qb) in enumerate(PC.reference(case)):
        ga, gb = maps[i, 0].astype(np.int64), maps[i, 1].astype(np.int64)
        gap_map = int(max(np.abs(ga - qa).max(), np.abs(gb - qb).max()))
        got = {f: rec[i][f].item() for f in FIELDS}
        # from the GPU's own maps
        lo, hi = R.sse_words(ga, gb)
        want_u = R.ssim_word(ga, gb)
        gap_u = abs(got["ssim_q"] - want_u) / got["windows"]
        own = R.finalize((got["sse_y_lo"], got["sse_y_hi"], got["sse_rgb_lo"], got["sse_rgb_hi"], got["ssim_q"]), h, w)
        bars = {key: 2.0 ** -15 * np.sqrt(flt[key]) + 2.0 ** -32 for key in ("mse_y", "mse_rgb")}
        gaps = {key: abs(got[key] - flt[key]) for key in ("mse_y", "mse_rgb", "pu_ssim")}
        print("%s frame %d: maps within %d, words %s the quantised restatement's, |ssim_q - sum u| / windows %.3f, mse_y gap %.3e (bar "
              "%.3e), mse_rgb gap %.3e (bar %.3e), pu_ssim %.9f gap %.3e (bar %.1e)"
              % (tag, i, gap_map, "=" if all(got[f] == qrec[f] for f in FIELDS[:5]) else "!=", gap_u, gaps["mse_y"], bars["mse_y"],
                 gaps["mse_rgb"], bars["mse_rgb"], got["pu_ssim"], gaps["pu_ssim"], R.SSIM_BAR))
        for name, val, where in (("map", gap_map, tag), ("u", gap_u, tag), ("ssim", gaps["pu_ssim"], tag),
                                 ("mse", max(gaps[key] / bars[key] for key in bars), tag)):
            if val > WORST[name]:
                WORST[name] = val
                WORST["tag_" + name] = "%s frame %d" % (where, i)
        assert gap_map <= 1, (tag, i)
        assert (got["sse_y_lo"], got["sse_y_hi"]) == (lo, hi), (tag, i)
        assert abs(got["ssim_q"] - want_u) <= got["windows"], (tag, i, got["ssim_q"], want_u)
        assert got["windows"] == (h - 10) * (w - 10)
        for f in ("mse_y", "mse_rgb", "pu_ssim"):                              # the record is the host formula of its own words
            assert got[f] == own[f], (tag, i, f)
        for f in ("pu_psnr", "pu_psnr_rgb"):
            assert got[f] == own[f] or abs(got[f] - own[f]) <= 1e-12 * abs(own[f]), (tag, i, f)
        for key in ("mse_y", "mse_rgb"):
            assert gaps[key] <= bars[key], (tag, i, key, got[key], flt[key])
        assert gaps["pu_ssim"] <= R.SSIM_BAR, (tag, i, got["pu_ssim"], flt["pu_ssim"])
        if content == "equal":                                                    # identical frames: the exact values
            assert got["sse_y_lo"] == got["sse_y_hi"] == got["sse_rgb_lo"] == got["sse_rgb_hi"] == 0
            assert got["ssim_q"] == got["windows"] << 24 and got["pu_ssim"] == 1.0
            assert got["pu_psnr"] == float("inf") == got["pu_psnr_rgb"] and got["mse_y"] == 0.0 == got["mse_rgb"]
            assert (ga == gb).all()
        if content == "extremes":
            assert got["sse_y_hi"] > 0 and got["sse_rgb_hi"] > 0 and np.isfinite(got["pu_psnr"])   # terms past 2^32: the high words at work


def test_the_worst_gaps_of_the_parity_matrix():
    """runs after the parity tests of this module (pytest keeps the file's order): the figures DESIGN.md 4s quotes"""
    print("parity matrix: largest map difference %d (%s); largest |ssim_q - sum u| per window %.3f (%s); largest mse gap %.3f of its "
          "bar (%s); largest pu_ssim gap %.3e (%s; bar %.1e)" % (WORST["map"], WORST["tag_map"], WORST["u"], WORST["tag_u"],
                                                                 WORST["mse"], WORST["tag_mse"], WORST["ssim"], WORST["tag_ssim"],
                                                                 R.SSIM_BAR))


def test_the_shipped_library_gives_the_lab_librarys_records(engine, lab):
    assert engine.lib.vqa_build_flavour() == 0
    for k in PC.SHIPPED:
        case = PC.matrix()[k]
        r, x, planes = PC.case_clip(case)
        got = engine.pu21(r, x, planes, transfer=case[4], full_range=case[6])
        assert got.tobytes() == lab["rec%d" % k].tobytes(), PC.case_id(case)
    with pytest.raises(RuntimeError, match="lab library only"):
        engine.pu21_maps()


def test_batches_positions_memory_kinds_and_views_give_the_same_words(engine):
    """frames of n = 5 against each frame alone, word for word: from host, pinned and device memory, through the frame stride,
    the one-load-per-row path against the same samples through a view that cannot take it (a shifted start; w % 4 != 0; packed
    bgr24), and windows of resident frames against the same samples as frames of their own"""
    from rtvqa_amd.engine import DeviceFrames
    (h, w), depth, layout = PC.VECTOR
    n = 5
    r, d, planes = PC.clip("natural", layout, h, w, depth, n, seed=3)
    whole = engine.pu21(r, d, planes)
    assert engine.pu21(r, d, planes).tobytes() == whole.tobytes()            # run to run
    for i in range(n):
        assert engine.pu21(r[i:i + 1], d[i:i + 1], planes).tobytes() == whole[i:i + 1].tobytes(), i
    got = engine.pu21(r[[3, 0, 4]], d[[3, 0, 4]], planes)
    assert got.tobytes() == whole[[3, 0, 4]].tobytes()
    dr, dd = engine.upload(r), engine.upload(d)
    assert engine.pu21(dr, dd, planes).tobytes() == whole.tobytes()
    assert engine.pu21(dr.slice(1, 2), dd.slice(1, 2), planes).tobytes() == whole[1:2].tobytes()
    pr, pd = engine.alloc_pinned(r.shape, np.uint16), engine.alloc_pinned(d.shape, np.uint16)
    pr[...], pd[...] = r, d
    assert engine.pu21(pr, pd, planes).tobytes() == whole.tobytes()
    engine.free_pinned(pr)
    engine.free_pinned(pd)
    odd = [DeviceFrames(x.ptr + x.frame_stride, 2, x.h, x.w, frame_stride=2 * x.frame_stride, row_stride=x.row_stride, owner=x,
                        channels=x.channels, itemsize=x.itemsize) for x in (dr, dd)]
    assert engine.pu21(odd[0], odd[1], planes).tobytes() == whole[1:4:2].tobytes()
    # one sample of padding in front of every frame: the same samples go sample by sample - the same words
    pad = [np.concatenate([np.zeros((n, 1), np.uint16), x], axis=1) for x in (r, d)]
    shifted = [(p[0], p[1], p[2] + 2) + tuple(p[3:]) for p in planes]
    assert engine.pu21(pad[0], pad[1], shifted).tobytes() == whole.tobytes()
    # windows of resident 64 x 36 frames read as 4:4:4: (5, 3) with 33 columns is ragged (w % 4 != 0), (4, 8) with 40 is aligned
    import itp_cases as IC
    m = 2
    a3, b3, _ = PC.clip("natural", "yuv444p10le", h, w, depth, m, seed=4)
    a3, b3 = a3.reshape(m, 3 * h, w), b3.reshape(m, 3 * h, w)
    da, db = engine.upload(a3), engine.upload(b3)
    for win in IC.ROIS:
        y0, x0, hh, ww = win
        roi = [(ww, hh, k * h * w * 2, w * 2, 2, depth) for k in range(3)]
        ca, own = IC.window_cut(a3, win, m)
        cb, _ = IC.window_cut(b3, win, m)
        alone = engine.pu21(ca, cb, own)
        assert engine.pu21(da.roi(y0, y0 + hh, x0, x0 + ww), db.roi(y0, y0 + hh, x0, x0 + ww), roi).tobytes() == alone.tobytes()
        flat = [(ww, hh, (k * h * w + y0 * w + x0) * 2, w * 2, 2, depth) for k in range(3)]
        assert engine.pu21(a3.reshape(m, -1), b3.reshape(m, -1), flat).tobytes() == alone.tobytes()
    # packed bgr24 (pixel step 3: sample by sample): batch of 5 against each frame alone
    rb, db_, pb = PC.clip("natural", "bgr24", 18, 24, 8, n, seed=5)
    wb = engine.pu21(rb, db_, pb)
    for i in range(n):
        assert engine.pu21(rb[i:i + 1], db_[i:i + 1], pb).tobytes() == wb[i:i + 1].tobytes(), i
    assert engine.pu21(rb, db_, pb, full_range=True).tobytes() == wb.tobytes()    # the range does not reach B, G, R
    assert engine.pu21(r, d, planes, transfer="hlg").tobytes() != whole.tobytes()
    assert engine.pu21(r, d, planes, full_range=True).tobytes() != whole.tobytes()


def test_in_flight_next_to_itp_and_ciede(engine):
    (h, w), depth, layout = PC.VECTOR
    r, d, planes = PC.clip("natural", layout, h, w, depth, 3, seed=6)
    want = {"pu21": engine.pu21(r, d, planes, transfer="hlg"), "itp": engine.itp(r, d, planes), "ciede": engine.ciede(r, d, planes)}
    dr, dd = engine.upload(r), engine.upload(d)
    for src in ((dr, dd), (r, d)):                                        # resident frames; host frames share one staging
        for order in (("pu21", "itp", "ciede"), ("ciede", "pu21", "itp"), ("itp", "ciede", "pu21")):
            engine.ciede_submit(src[0], src[1], planes)
            engine.pu21_submit(src[0], src[1], planes, transfer="hlg")
            engine.itp_submit(src[0], src[1], planes)
            for kind in order:
                assert getattr(engine, kind + "_wait")().tobytes() == want[kind].tobytes(), (order, kind)


def _submit(engine, f, d, planes, n=None, model=0, transfer=0, full_range=0):
    from rtvqa_amd import _native as N
    from rtvqa_amd.engine import plane_descs
    fb = f.reshape(f.shape[0], -1).shape[1] * f.dtype.itemsize
    return engine.lib.vqa_pu21_submit(engine.ctx, f.ctypes.data, d.ctypes.data, N.VQA_MEM_HOST, f.shape[0] if n is None else n,
                                      fb, fb, plane_descs(planes), len(planes), model, transfer, full_range)


def test_the_state_machine_and_the_refusals(engine):
    from rtvqa_amd import _native as N
    from rtvqa_amd.engine import plane_descs, yuv_planes
    f, d, planes = PC.clip("natural", "yuv420p", 32, 48, 8, 2, seed=8)
    want = engine.pu21(f, d, planes)
    iwant = engine.itp(f, d, planes)
    uout, iout = (N.VqaPu21Metrics * 2)(), (N.VqaItpMetrics * 2)()
    lib, ctx = engine.lib, engine.ctx

    def idle():
        return lib.vqa_pu21_wait(ctx, uout, 2) == N.VQA_ERR_STATE
    assert idle()                                                         # wait without submit
    assert _submit(engine, f, d, planes) == N.VQA_OK
    assert _submit(engine, f, d, planes) == N.VQA_ERR_STATE              # submit while pending
    assert lib.vqa_itp_wait(ctx, iout, 2) == N.VQA_ERR_STATE             # another kind's wait: the batch survives
    assert lib.vqa_trim(ctx) == N.VQA_ERR_STATE
    assert lib.vqa_pu21_wait(ctx, uout, 6) == N.VQA_ERR_STATE            # a wrong entry count: one entry per FRAME
    assert lib.vqa_pu21_wait(ctx, uout, 2) == N.VQA_OK
    assert bytes(uout) == want.tobytes()
    fb = f.shape[1]
    pd = plane_descs(planes)
    assert lib.vqa_itp_submit(ctx, f.ctypes.data, d.ctypes.data, N.VQA_MEM_HOST, 2, fb, fb, pd, 3, 0, 0, 0) == N.VQA_OK
    assert idle()                                                         # a wait with only another kind pending
    assert lib.vqa_itp_wait(ctx, iout, 2) == N.VQA_OK and bytes(iout) == iwant.tobytes()
    Y, U, V = planes
    z16 = np.zeros((2, 32 * 48 * 3), np.uint16)
    p10 = yuv_planes(32, 48, "420", 10)
    refused = [
        (f, planes[:2], {}, N.VQA_ERR_INVALID),                                             # two planes
        (f, planes[:1], {}, N.VQA_ERR_INVALID),                                             # one: one-plane layouts are an error
        (f, planes + [V], {}, N.VQA_ERR_INVALID),                                           # four
        (f, [Y, U, (V[0] - 1,) + V[1:]], {}, N.VQA_ERR_INVALID),                            # Cb and Cr geometries differ
        (f, [Y, (20, 16, U[2], 20, 1), (20, 16, V[2], 20, 1)], {}, N.VQA_ERR_INVALID),      # neither full nor ceil-half
        (f, planes, {"model": N.ITP_BGR}, N.VQA_ERR_INVALID),                               # B, G, R must share one geometry
        (f, planes, {"model": 2}, N.VQA_ERR_INVALID),
        (f, planes, {"transfer": 2}, N.VQA_ERR_INVALID),
        (f, planes, {"transfer": -1}, N.VQA_ERR_INVALID),
        (f, planes, {"full_range": 2}, N.VQA_ERR_INVALID),
        (z16, p10[:1] + [p[:5] for p in p10[1:]], {}, N.VQA_ERR_INVALID),                   # mixed depths
        (f, [(16, 15, 0, 16, 1), (8, 8, 240, 8, 1), (8, 8, 304, 8, 1)], {}, N.VQA_ERR_UNSUPPORTED),   # luma 15 rows x 16
        (f, [(15, 16, 0, 15, 1), (8, 8, 240, 8, 1), (8, 8, 304, 8, 1)], {}, N.VQA_ERR_UNSUPPORTED),
        (f, [(16385, 16384, 0, 16385, 1)] * 3, {}, N.VQA_ERR_UNSUPPORTED),                  # more than 2^28 pixels
    ]
    for k, (buf, pl, kw, status) in enumerate(refused):
        assert _submit(engine, buf, buf, pl, n=1, **kw) == status, k
        assert idle(), k
    assert lib.vqa_pu21_submit(ctx, f.ctypes.data, d.ctypes.data, N.VQA_MEM_HOST, 2, fb - 1, fb, pd, 3, 0, 0, 0) == N.VQA_ERR_INVALID
    assert lib.vqa_pu21_submit(ctx, f.ctypes.data, None, N.VQA_MEM_HOST, 2, fb, fb, pd, 3, 0, 0, 0) == N.VQA_ERR_INVALID
    assert idle()
    with pytest.raises(ValueError, match="transfer must be 'pq' or 'hlg'"):
        engine.pu21(f, d, planes, transfer="sdr")
    with pytest.raises(ValueError, match="full_range must be True or False"):
        engine.pu21(f, d, planes, full_range="full")
    assert idle()
    z = np.zeros((1, 16 * 16 * 3 // 2), np.uint8)                          # a 16 x 16 4:2:0 frame is measured
    assert _submit(engine, z, z, yuv_planes(16, 16, "420", 8)) == N.VQA_OK and lib.vqa_pu21_wait(ctx, uout, 1) == N.VQA_OK
    assert engine.pu21(f, d, planes).tobytes() == want.tobytes()
    engine.trim()
    assert engine.pu21(f, d, planes).tobytes() == want.tobytes()
    assert engine.itp(f, d, planes).tobytes() == iwant.tobytes()


def test_one_pass_entry_points(engine, tmp_path):
    """Engine.pu21, frame_pu21, a Quality(pu21=True) pass and the pu_* values of run_ffmpeg_metrics' log agree; the psnr / ssim
    files and every other key are those of a run without pu21, byte for byte; the row gains the three columns after DELTA_ITP_MAX"""
    from rtvqa_amd import stream, synth
    from rtvqa_amd import video_processing as vp
    (h, w), depth, layout = PC.VECTOR
    n = 5
    r, d, planes = PC.clip("natural", layout, h, w, depth, n, seed=9)
    d[2] = r[2]                                                  # one identical frame
    whole = engine.pu21(r, d, planes)
    assert whole["pu_ssim"][2] == 1.0 and whole["pu_psnr"][2] == np.inf and (whole["pu_ssim"][[0, 1, 3, 4]] < 1.0).all()
    out = vp.frame_pu21(r, d, layout, h, w, batch_size=2)
    for arr, key in zip(out, ("pu_psnr", "pu_psnr_rgb", "pu_ssim", "mse_y", "mse_rgb")):
        assert arr.tobytes() == np.ascontiguousarray(whole[key]).tobytes(), key
    q, _ = stream.run(d, r, quality=stream.Quality(planes, itp=True, pu21=True), batch_size=2)
    assert q[-1].tobytes() == whole.tobytes() and q[-2].dtype.names[-1] == "de_max"       # the last element, after dE_ITP's
    q, _ = stream.run(d, r, quality=stream.Quality(planes, pu21="only", pu21_transfer="hlg", pu21_full_range=True), batch_size=3)
    assert q[0] is None and q[-1].tobytes() == engine.pu21(r, d, planes, transfer="hlg", full_range=True).tobytes()
    kw = dict(layout=layout, height=h, width=w)
    logs = {k: [str(tmp_path / ("%s_%s.log" % (k, t))) for t in ("psnr", "ssim", "vmaf")] for k in ("plain", "it", "both", "only", "off")}
    vp.run_ffmpeg_metrics(r, d, *logs["plain"], batch_size=2, **kw)
    vp.run_ffmpeg_metrics(r, d, *logs["off"], batch_size=2, pu21=False, **kw)
    vp.run_ffmpeg_metrics(r, d, *logs["it"], batch_size=2, delta_itp=True, **kw)
    vp.run_ffmpeg_metrics(r, d, *logs["both"], batch_size=2, delta_itp=True, pu21=True, **kw)
    vp.run_ffmpeg_metrics(r, d, *logs["only"], batch_size=3, pu21=True, **kw)
    for k in (0, 1):
        for kind in ("it", "both", "only", "off"):
            assert open(logs["plain"][k], "rb").read() == open(logs[kind][k], "rb").read(), (kind, k)
    it, both, only = (json.load(open(logs[k][2])) for k in ("it", "both", "only"))
    assert list(both["frames"][0]["metrics"]) == ["delta_itp", "delta_itp_max", "pu_psnr", "pu_psnr_rgb", "pu_ssim"]
    assert list(only["frames"][0]["metrics"]) == ["pu_psnr", "pu_psnr_rgb", "pu_ssim"] and "pu_" not in json.dumps(it)
    for i in range(n):
        for doc in (both, only):
            m = doc["frames"][i]["metrics"]
            assert m["pu_psnr"] == min(float(whole["pu_psnr"][i]), 100.0) and m["pu_ssim"] == float(whole["pu_ssim"][i])
        assert both["frames"][i]["metrics"]["delta_itp"] == it["frames"][i]["metrics"]["delta_itp"]
    assert both["frames"][2]["metrics"]["pu_psnr"] == 100.0
    bgr = synth.s_natural(n, h, w, seed=12)
    cfg = {"crf": 23, "resize_width": 32, "resize_height": 32, "frame_interval": 1, "batch_size": 2, "pixfmt": layout}

    def row(name, **more):
        return vp.process_video_and_extract_metrics(r, d, dict(cfg, **more), csv_file=str(tmp_path / (name + ".csv")),
                                                    column_order="fixed", encoded_bgr=bgr)

    def same(a, b):
        return a == b or (a != a and b != b)

    row0, row1 = row("row0", delta_itp=True), row("row1", delta_itp=True, pu21=True)
    k0 = list(row0)
    at = k0.index("DELTA_ITP_MAX") + 1
    assert list(row1) == k0[:at] + ["PU_PSNR", "PU_PSNR_RGB", "PU_SSIM"] + k0[at:]
    assert all(same(row0[k], row1[k]) for k in k0)
    assert abs(row1["PU_SSIM"] - whole["pu_ssim"].mean()) <= 1e-12
    assert abs(row1["PU_PSNR"] - np.minimum(whole["pu_psnr"], 100.0).mean()) <= 1e-9 and row1["PU_PSNR"] <= 100.0
    row("row0b", delta_itp=True, pu21=False, pu21_transfer="hlg", pu21_range="full")
    assert open(str(tmp_path / "row0.csv"), "rb").read() == open(str(tmp_path / "row0b.csv"), "rb").read()
    assert b"PU_PSNR" not in open(str(tmp_path / "row0.csv"), "rb").read()
    assert b"DELTA_ITP_MAX,PU_PSNR,PU_PSNR_RGB,PU_SSIM" in open(str(tmp_path / "row1.csv"), "rb").read()


def test_profile_counts_one_launch_per_kernel_and_submit():
    import rtvqa_amd
    from rtvqa_amd import _native as N
    f, d, planes = PC.clip("natural", "yuv420p", 32, 48, 8, 3, seed=10)
    with rtvqa_amd.Engine(0) as eng:
        eng.profile(True)
        eng.pu21(f, d, planes)
        prof = eng.profile_read(reset=True)
        assert prof["k_pu21_encode"][1] == 1 and prof["k_pu21_ssim"][1] == 1 and "k_itp" not in prof, prof
        eng.itp(f, d, planes)
        assert "k_pu21_encode" not in eng.profile_read(reset=True)
        ms, cnt = C.c_double(0), C.c_int64(0)
        for bad in (N.K_VERGE, N.K_RIM):                                   # ids 52 and 55 are unknown
            assert eng.lib.vqa_profile_read(eng.ctx, bad, C.byref(ms), C.byref(cnt), 0) == N.VQA_ERR_INVALID


if __name__ == "__main__":
    _child(sys.argv[1])
