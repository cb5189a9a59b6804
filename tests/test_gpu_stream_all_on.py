"""GPU: one pass with every switch of stream.Quality on - the configuration "all true" in config.json gives.

stream._run_locked then issues nineteen submits per chunk on one lane (SSE / SSIM, the seventeen plane-batch kinds of
stream.PLANE_KINDS and, fused, the complexity batch), collects nineteen results and builds a positional tuple whose layout depends on
the switches; video_processing._write_feature_log reads that tuple by kind name (stream.records_by_kind).  Every other file turns
on three switches at most.

Expected values: the whole clip (seven frames and a distorted copy; yuv420p at 66 x 98, yuv420p10le at 70 x 74) through the
direct engine calls, one kind at a time, n = 7 from host frames, on the session engine - CAMBI, the artefact measures and
BRISQUE on the distorted frames, motion, SI/TI and VCA on the reference frames, stream.motion_records over motion.  Those calls
are what tests/test_gpu_all_kinds.py and the per-metric files tie to the CPU references; nothing here has a tolerance: every
element of the tuple equals the expected records field by field as bytes, and the JSON values are compared with ==.

The tuple's layout is restated here from the Quality docstring (_want_tuple), not taken from the code."""
import json
import os

import numpy as np
import pytest

import motion_cases as K

pytestmark = pytest.mark.gpu

N_FRAMES = 7
GEOMETRIES = {"yuv420p": (66, 98, 8), "yuv420p10le": (70, 74, 10)}
# the switches in the order their elements take in the tuple (vca_blocks shapes VCA's element)
SWITCHES = ("vif", "adm", "motion", "siti", "psnr_hvs", "ciede", "gmsd", "cambi", "xpsnr", "haarpsi", "vca", "vca_blocks", "artifacts",
            "brisque", "mdsi", "itp", "pu21", "fsim")
ALL_ON = {k: True for k in SWITCHES}
ELEMENTS = 2 + 17                               # sse, ssim and one element per switch but vca_blocks
AFTER_MOTION = ("siti", "psnr_hvs", "ciede", "gmsd", "cambi", "xpsnr", "haarpsi", "vca", "artifacts", "brisque", "mdsi",
                "itp", "pu21", "fsim")
ONE_STREAM = {"cambi": "dist", "artifacts": "dist", "brisque": "dist", "vca": "ref", "motion": "ref", "siti": "ref"}


def _clip(layout):
    """-> (ref, dist [7, samples], planes): the suite's natural clip and a copy with a few levels of noise on every sample"""
    h, w, depth = GEOMETRIES[layout]
    r, planes = K.clip(layout, h, w, depth, "natural", seed=h + w, n=N_FRAMES)
    rng = np.random.default_rng(h + w + 1)
    u, peak = 1 << (depth - 8), (1 << depth) - 1
    d = np.clip(r.astype(np.int64) + rng.integers(-4, 5, r.shape) * u + (rng.integers(0, u, r.shape) if depth > 8 else 0), 0, peak)
    return r, d.astype(r.dtype), planes


def _expected(eng, r, d, planes):
    """every kind alone over the whole clip, through the direct engine calls"""
    from rtvqa_amd import _native as N
    from rtvqa_amd import stream
    q = eng.quality(r, d, planes, N.SSIM_GAUSS)
    rec, maps = eng.vca(r, planes, blocks=True)
    return {"sse": q["sse"], "ssim": q["ssim"], "vif": eng.vif(r, d, planes), "adm": eng.adm(r, d, planes),
            "motion": stream.motion_records(eng.motion(r, planes)), "siti": eng.siti(r, planes),
            "psnr_hvs": eng.psnr_hvs(r, d, planes), "ciede": eng.ciede(r, d, planes), "gmsd": eng.gmsd(r, d, planes),
            "cambi": eng.cambi(d, planes), "xpsnr": eng.xpsnr(r, d, planes), "haarpsi": eng.haarpsi(r, d, planes),
            "vca": rec, "vca_maps": maps, "artifacts": eng.artifacts(d, planes), "brisque": eng.brisque(d, planes),
            "mdsi": eng.mdsi(r, d, planes), "itp": eng.itp(r, d, planes), "pu21": eng.pu21(r, d, planes),
            "fsim": eng.fsim(r, d, planes)}


@pytest.fixture(scope="module")
def clips(engine):
    """layout -> (ref, dist, planes, expected), computed once"""
    out = {}
    for layout in GEOMETRIES:
        r, d, planes = _clip(layout)
        out[layout] = (r, d, planes, _expected(engine, r, d, planes))
    return out


def _want_tuple(exp, **kw):
    """the tuple stream.run documents for Quality(planes, **kw), filled from the expected records"""
    only = any(v == "only" for v in kw.values())
    t = [None, None] if only else [exp["sse"], exp["ssim"]]
    vif, adm, motion = (bool(kw.get(k)) for k in ("vif", "adm", "motion"))
    if vif or adm or motion:
        t.append(exp["vif"] if vif else None)
    if adm or motion:
        t.append(exp["adm"] if adm else None)
    if motion:
        t.append(exp["motion"])
    for k in AFTER_MOTION:
        if kw.get(k):
            t.append((exp["vca"], exp["vca_maps"]) if k == "vca" and kw.get("vca_blocks") else exp[k])
    return t


def _same(got, want, what):
    """one element of the tuple: None for None, the promised dtype and shape, every field the same bytes"""
    if want is None:
        assert got is None, what
        return
    assert isinstance(got, np.ndarray) and got.dtype == want.dtype and got.shape == want.shape, (what, getattr(got, "dtype", None), getattr(got, "shape", None))
    for f in (want.dtype.names or (None,)):
        a, b = (got, want) if f is None else (got[f], want[f])
        assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), (what, f)


def _same_tuple(q, want, what):
    assert isinstance(q, tuple) and len(q) == len(want), (what, len(q), len(want))
    for at, (g, w) in enumerate(zip(q, want)):
        if isinstance(w, tuple):                 # VCA with its block maps: (records, one dict(qh, s) per plane)
            assert isinstance(g, tuple) and len(g) == 2 and len(g[1]) == len(w[1]), (what, at)
            _same(g[0], w[0], (what, at, "vca records"))
            for p, (gm, wm) in enumerate(zip(g[1], w[1])):
                assert sorted(gm) == ["qh", "s"], (what, at, p)
                for key in ("qh", "s"):
                    _same(gm[key], wm[key], (what, at, "vca map", p, key))
        else:
            _same(g, w, (what, at))


def _promised(q, planes, n):
    """the dtype and shape the Quality docstring promises for every position of the all-on tuple"""
    from rtvqa_amd import engine as E
    from rtvqa_amd import stream
    p = len(planes)
    assert len(q) == ELEMENTS
    assert q[0].dtype == np.uint64 and q[1].dtype == np.float64 and q[0].shape == q[1].shape == (n, p)
    per_plane = (E.VIF_DTYPE, E.ADM_DTYPE, stream.MOTION_PASS_DTYPE, E.SITI_DTYPE, E.PSNR_HVS_DTYPE, None, E.GMSD_DTYPE, E.CAMBI_DTYPE,
                 E.XPSNR_DTYPE, E.HAARPSI_DTYPE, None, E.ARTIFACTS_DTYPE, E.BRISQUE_DTYPE, None, None, None, None)
    for at, dt in enumerate(per_plane, start=2):
        if dt is not None:
            assert q[at].dtype == dt and q[at].shape == (n, p), at
    assert q[7].dtype == E.CIEDE_DTYPE and q[7].shape == (n,)                    # one per frame
    for at, dt in ((15, E.MDSI_DTYPE), (16, E.ITP_DTYPE), (17, E.PU21_DTYPE), (18, E.FSIM_DTYPE)):
        assert q[at].dtype == dt and q[at].shape == (n,), at
    rec, maps = q[12]
    assert rec.dtype == E.VCA_DTYPE and rec.shape == (n, p) and len(maps) == p
    for pl, m in zip(planes, maps):
        gx, gy = E.vca_grid(pl[0], pl[1])
        assert m["qh"].shape == m["s"].shape == (n, gy, gx) and m["qh"].dtype == m["s"].dtype == np.uint64


def _sources(r, d, where):
    """-> (ref, dist, what to free afterwards)"""
    if where == "host":
        return r, d, ()
    from rtvqa_amd import stream
    eng = stream.get_engine()
    dr, dd = eng.upload(r), eng.upload(d)
    return dr, dd, (dr, dd)


def _free(bufs):
    for b in bufs:
        b._owner.free()


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("batch", [3, 100])
@pytest.mark.parametrize("layout", list(GEOMETRIES))
def test_every_switch_on(clips, layout, batch, where):
    """batch_size 3: chunks of 3 + 3 + 1, the prev0 halo of motion, SI/TI, XPSNR and VCA crosses two seams; 100: one chunk"""
    from rtvqa_amd import stream
    r, d, planes, exp = clips[layout]
    rs, ds, bufs = _sources(r, d, where)
    try:
        q, series = stream.run(ds, rs, quality=stream.Quality(planes, **ALL_ON), batch_size=batch)
    finally:
        _free(bufs)
    assert series is None
    _promised(q, planes, N_FRAMES)
    _same_tuple(q, _want_tuple(exp, **ALL_ON), (layout, batch, where))


@pytest.mark.parametrize("lanes", [1, 3])
@pytest.mark.parametrize("layout", list(GEOMETRIES))
def test_every_switch_on_with_any_number_of_lanes(clips, monkeypatch, layout, lanes):
    """stream.MAX_LANES engines alternate the chunks (default 2): one lane, and three with a chunk each"""
    from rtvqa_amd import stream
    r, d, planes, exp = clips[layout]
    monkeypatch.setattr(stream, "MAX_LANES", lanes)
    for where in ("host", "device"):
        rs, ds, bufs = _sources(r, d, where)
        try:
            q, _ = stream.run(ds, rs, quality=stream.Quality(planes, **ALL_ON), batch_size=3)
        finally:
            _free(bufs)
        _same_tuple(q, _want_tuple(exp, **ALL_ON), (layout, lanes, where))


@pytest.mark.parametrize("drop", SWITCHES)
def test_one_switch_less(clips, drop):
    """the all-on request without one switch: the tuple loses exactly that element (vif and adm leave None while a later one of
    the three is on; vca_blocks leaves VCA's records without the maps) and every other element keeps its bytes"""
    from rtvqa_amd import stream
    r, d, planes, exp = clips["yuv420p"]
    kw = dict(ALL_ON, **{drop: False})
    q, _ = stream.run(d, r, quality=stream.Quality(planes, **kw), batch_size=3)
    want = _want_tuple(exp, **kw)
    assert len(want) == ELEMENTS - (0 if drop in ("vif", "adm", "vca_blocks") else 1)
    if drop in ("vif", "adm"):
        assert want[2 + ("vif", "adm").index(drop)] is None
    _same_tuple(q, want, ("without", drop))


@pytest.mark.parametrize("layout", list(GEOMETRIES))
@pytest.mark.parametrize("kind", list(ONE_STREAM))
def test_a_one_stream_kind_alone_beside_a_two_stream_switch(clips, layout, kind):
    """kind="only" with gmsd=True: no SSE / SSIM, but GMSD needs the pair, so the pass reads both streams; CAMBI, the artefact
    measures and BRISQUE then measure the distorted stream and VCA, motion and SI/TI the reference - reference and distorted
    frames differ on every sample, so the other stream's records are other records"""
    from rtvqa_amd import stream
    r, d, planes, exp = clips[layout]
    kw = {kind: "only", "gmsd": True}
    want = _want_tuple(exp, **kw)
    assert want[0] is None and want[1] is None and len(want) == (6 if kind == "motion" else 4)
    for where in ("host", "device"):
        rs, ds, bufs = _sources(r, d, where)
        try:
            q, _ = stream.run(ds, rs, quality=stream.Quality(planes, **kw), batch_size=3)
        finally:
            _free(bufs)
        _same_tuple(q, want, (layout, kind, where))
    # (not vacuous: the kind's records of the other stream are not these)
    eng = stream.get_engine()
    mine, other = (d, r) if ONE_STREAM[kind] == "dist" else (r, d)
    assert getattr(eng, kind)(other, planes).tobytes() != getattr(eng, kind)(mine, planes).tobytes()


@pytest.mark.parametrize("layout", list(GEOMETRIES))
def test_the_fused_pass_with_every_switch_on(clips, layout):
    """a Complexity((64, 64), 3) half beside the all-on quality half, as process_video_and_extract_metrics runs it: BGR frames for
    the complexity kernels, the planar pair for the quality kernels, three chunks"""
    from rtvqa_amd import stream, synth
    from test_gpu_stream import _same_series
    r, d, planes, exp = clips[layout]
    h, w, _depth = GEOMETRIES[layout]
    bgr = synth.s_natural(N_FRAMES, h, w, seed=12)
    cx = stream.Complexity((64, 64), 3)
    _none, alone = stream.run(bgr, complexity=cx, batch_size=1)
    assert len(alone["dct"]) == 1 and alone["range"] == (0, 1)
    q, series = stream.run(bgr, r, quality=stream.Quality(planes, **ALL_ON), complexity=cx, batch_size=1, qdist=d)
    _promised(q, planes, N_FRAMES)
    _same_tuple(q, _want_tuple(exp, **ALL_ON), (layout, "fused"))
    _same_series(series, alone)


# ---- the log and the row ----------------------------------------------------------------------------------------------------
FLAGS = ("vif", "adm", "motion", "siti", "psnr_hvs", "ciede", "gmsd", "cambi", "xpsnr", "haarpsi", "vca", "artifacts", "brisque", "mdsi",
         "delta_itp", "pu21", "fsim")
BASE_COLUMNS = ["Bitrate (kbps)", "Resolution (px)", "Frame Rate (fps)", "CRF", "PSNR", "SSIM"]


@pytest.mark.parametrize("layout", list(GEOMETRIES))
def test_run_ffmpeg_metrics_with_every_flag(clips, tmp_path, layout):
    """a .y4m pair of the clip, every flag true and a VMAF model file: frames[i].metrics holds, key by key, the values of the log
    a run with that one flag wrote (vmaf: the run with the model alone), in the order of the single-flag logs one after the
    other; extract_metrics_from_logs' row has the union of their columns with their values; the psnr and ssim stats files are
    byte for byte those of a run without any flag"""
    import test_gpu_motion as TMO
    import vmaf_reference as VR
    from rtvqa_amd import frames
    from rtvqa_amd import video_processing as vp
    r, d, _planes, exp = clips[layout]
    h, w, _depth = GEOMETRIES[layout]
    pr, pd = str(tmp_path / "ref.y4m"), str(tmp_path / "enc.y4m")
    frames.write_y4m(pr, r, h, w, pixfmt=layout)
    frames.write_y4m(pd, d, h, w, pixfmt=layout)
    logs = {k: [str(tmp_path / ("%s_%s.log" % (k, t))) for t in ("psnr", "ssim", "vmaf")] for k in ("plain", "model", "all") + FLAGS}
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["plain"], batch_size=3) is None
    assert not os.path.exists(logs["plain"][2])
    for flag in FLAGS:
        assert vp.run_ffmpeg_metrics(pr, pd, *logs[flag], batch_size=3, **{flag: True}) is None
    docs = {k: json.load(open(logs[k][2])) for k in FLAGS}
    one = {k: [fr["metrics"] for fr in docs[k]["frames"]] for k in FLAGS}
    feats = [[{**one["vif"][i], **one["adm"][i], **one["motion"][i]}[k] for k in VR.FEATURES_V061] for i in range(N_FRAMES)]
    model = TMO._model_file(str(tmp_path / "model.json"), "json", feats)
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["model"], model, batch_size=3) is None
    assert vp.run_ffmpeg_metrics(pr, pd, *logs["all"], model, batch_size=3, **{flag: True for flag in FLAGS}) is None
    doc, mdoc = json.load(open(logs["all"][2])), json.load(open(logs["model"][2]))
    # the stats files
    for k in (0, 1):
        plain = open(logs["plain"][k], "rb").read()
        assert len(plain.splitlines()) == N_FRAMES
        for run in ("model", "all") + FLAGS:
            assert open(logs[run][k], "rb").read() == plain, (run, k)
    # the keys and their order
    names = [k for flag in FLAGS for k in one[flag][0]]
    assert len(names) == len(set(names)) == 4 + 5 + 2 + 2 + 2 + 1 + 1 + 1 + 1 + 1 + 3 + 3 + 36 + 1 + 2 + 3 + 2
    assert len(doc["frames"]) == N_FRAMES
    assert list(doc["pooled_metrics"]) == names + ["vmaf"]
    for i in range(N_FRAMES):
        m = doc["frames"][i]["metrics"]
        assert doc["frames"][i]["frameNum"] == i and list(m) == names + ["vmaf"], i
        for flag in FLAGS:
            assert docs[flag]["frames"][i]["frameNum"] == i
            for k, v in one[flag][i].items():
                assert m[k] == v, (i, flag, k, m[k], v)
        assert m["vmaf"] == mdoc["frames"][i]["metrics"]["vmaf"], i
    for flag in FLAGS:
        for k, pooled in docs[flag]["pooled_metrics"].items():
            assert doc["pooled_metrics"][k] == pooled, (flag, k)
    assert doc["pooled_metrics"]["vmaf"] == mdoc["pooled_metrics"]["vmaf"]
    # the logs say what the engine says of these frames (one value per kind: the rest is the per-metric files')
    for i in range(N_FRAMES):
        m = doc["frames"][i]["metrics"]
        assert m["gmsd"] == float(exp["gmsd"][i, 0]["gmsd"]) and m["mdsi"] == float(exp["mdsi"][i]["mdsi"])
        assert m["cambi"] == float(exp["cambi"][i, 0]["cambi"]) and m["vca_e"] == float(exp["vca"][i, 0]["e"])
        assert m["motion"] == float(exp["motion"][i, 0]["motion"]) and m["si"] == float(exp["siti"][i, 0]["si"])
        assert m["brisque_07"] == float(exp["brisque"][i, 0]["features"][7]) and m["noise"] == float(exp["artifacts"][i, 0]["noise"])
        assert m["delta_itp"] == float(exp["itp"][i]["de_mean"]) and m["delta_itp_max"] == float(exp["itp"][i]["de_max"])
        assert m["pu_ssim"] == float(exp["pu21"][i]["pu_ssim"]) and m["pu_psnr"] == min(float(exp["pu21"][i]["pu_psnr"]), vp.PU21_PSNR_CAP)
        assert m["fsim"] == float(exp["fsim"][i]["fsim"]) and m["fsimc"] == float(exp["fsim"][i]["fsimc"])
    # the row
    args = ("x", 23, 1000, "%dx%d" % (w, h), 30.0)
    row = vp.extract_metrics_from_logs(*logs["all"], *args)
    rows = {k: vp.extract_metrics_from_logs(*logs[k], *args) for k in ("plain", "model") + FLAGS}
    assert list(rows["plain"]) == BASE_COLUMNS
    extra = [k for flag in FLAGS for k in list(rows[flag])[len(BASE_COLUMNS):]]
    assert len(extra) == len(set(extra)) and len(extra) >= len(FLAGS)
    assert list(row) == BASE_COLUMNS + ["VMAF"] + extra
    for flag in FLAGS:
        for k, v in rows[flag].items():
            assert row[k] == v, (flag, k)
    assert row["VMAF"] == rows["model"]["VMAF"]
