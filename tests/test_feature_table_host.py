"""The feature table (rtvqa_amd.features.FEATURES) and what reads it, on the host (no GPU).

(1) Byte identity: tests/golden/feature_logs.json holds what write_vif_log wrote and extract_metrics_from_logs read back for
    seeded records of every kind BEFORE the table replaced the per-kind chains (oracle/gen_feature_logs.py, run once by the
    commit before); the same calls must give the same text, byte for byte, and the same row, in order and value.
(2) The table is consistent with stream.PLANE_KINDS, stream.Quality and the entry points' signatures.  write_vif_log keeps its
    signature, so VIF's records arrive under `scale` and a kind's parameters (ciede_weights ...) are no arguments of it: the
    flags are checked against both signatures, the parameters' keywords against run_ffmpeg_metrics'.
(3) config -> switches, against a dict written out here, and the messages of the boolean keys.
(4) flags -> Quality: run_ffmpeg_metrics with every flag and parameter set, stream.run replaced by a recorder.
(5) The order of the frame_* calls' argument errors, before a stream is opened.
"""
import inspect
import json
import os

import numpy as np
import pytest

import brisque_cases as BC
from oracle import gen_feature_logs as G
from rtvqa_amd import _native as N
from rtvqa_amd import features, stream
from rtvqa_amd import video_processing as vp
from rtvqa_amd.engine import yuv420p_planes

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOOD = {"crf": 23, "vmaf_model_path": None, "resize_width": 64, "resize_height": 64, "frame_interval": 10}
with open(os.path.join(REPO, "tests", "golden", "feature_logs.json")) as _f:
    GOLDEN = json.load(_f)
SWITCH_KEYS = ("vif", "adm", "motion_feature", "siti", "psnr_hvs", "ciede", "gmsd", "cambi", "xpsnr", "haarpsi", "vca", "artifacts",
               "brisque", "mdsi", "delta_itp", "pu21", "fsim", "sigstats")
VMAF_MODEL = ("svm_type nu_svr\nkernel_type rbf\ngamma 0.05\nnr_class 2\ntotal_sv 2\nrho -1.5\nSV\n"
              "0.5 1:0.1 2:0.2 3:0.3 4:0.4 5:0.5 6:0.6\n-0.25 1:0.6 3:0.2\n")


# ---- (1) byte identity against the code the table replaced -------------------------------------------------------------------
CASES = G.cases()


def test_the_fixture_covers_every_kind():
    assert len(json.dumps(GOLDEN)) < 100 * 1024
    flags = ["scale" if f.kind == "vif" else f.flag for f in vp.FEATURES]
    assert sorted(GOLDEN) == sorted(CASES) == sorted(["all", "vmaf"] + flags)
    assert sorted(CASES["all"]) == sorted(flags)
    rec = CASES["all"]
    assert (rec["sigstats"]["count"] > 0).all()
    for name, field, frame in G.INFINITE:
        assert np.isinf(rec[name][field][frame]) and np.isfinite(np.delete(rec[name][field], frame)).all()


@pytest.mark.parametrize("case", sorted(GOLDEN))
def test_the_log_and_the_row_are_what_they_were(case, tmp_path):
    text, row = G.render(CASES[case], str(tmp_path))
    assert text == GOLDEN[case]["log"], case
    assert row == GOLDEN[case]["row"], case                     # (a list of [column, value]: the order and the values)
    assert [type(v) for _, v in row] == [type(v) for _, v in GOLDEN[case]["row"]]


def test_where_vmaf_stands():
    doc = json.loads(GOLDEN["vmaf"]["log"])
    assert list(doc["pooled_metrics"])[-1] == "vmaf" and list(doc["frames"][0]["metrics"])[-1] == "vmaf"
    cols = [c for c, _ in GOLDEN["vmaf"]["row"]]
    assert cols[cols.index("SSIM") + 1] == "VMAF"


# ---- (2) the table -----------------------------------------------------------------------------------------------------------
def test_the_table_is_consistent():
    F = vp.FEATURES
    assert F is features.FEATURES
    assert [f.kind for f in F] == [k.name for k in stream.PLANE_KINDS]
    assert [f.flag for f in F] == [{"itp": "delta_itp"}.get(k.name, k.name) for k in stream.PLANE_KINDS]
    assert [f.config_key for f in F] == list(SWITCH_KEYS)
    run_args = inspect.signature(vp.run_ffmpeg_metrics).parameters
    log_args = inspect.signature(vp.write_vif_log).parameters
    quality_args = inspect.signature(stream.Quality.__init__).parameters
    for f in F:
        assert f.flag in run_args and run_args[f.flag].default is False, f.flag
        assert ("scale" if f.kind == "vif" else f.flag) in log_args, f.flag
        assert f.kind in quality_args
        declared = dict(stream.PLANE_KINDS[[k.name for k in stream.PLANE_KINDS].index(f.kind)].params)
        assert [p.quality for p in f.params if p.quality] == list(declared), f.kind   # every parameter Quality has for the kind
        for p in f.params:
            assert p.flag in run_args, p.flag
            assert p.quality is None or p.quality in quality_args, p.quality
            if p.quality is not None:    # the entry point's default is Quality's
                assert run_args[p.flag].default == quality_args[p.quality].default, p.flag
    keys = [key for f in F for key, _, _ in f.log]
    cols = [c for f in F for c, _, _ in f.row] + [c for c, _ in features.SIGNAL_COLUMNS] + list(features.CROP_COLUMNS)
    assert len(set(keys)) == len(keys) and "vmaf" not in keys
    assert len(set(cols)) == len(cols) and "VMAF" not in cols
    assert all(key in keys for f in F for _, key, _ in f.row)
    assert {stat for f in F for _, _, stat in f.row} == {"mean", "max", "min"}
    by_stat = {c: stat for f in F for c, _, stat in f.row if stat != "mean"}
    assert by_stat == {"SI": "max", "TI": "max", "DELTA_ITP_MAX": "max", "Y_HIGH": "max", "Y_LOW": "min"}
    capped = {key: cap for f in F for key, _, cap in f.log if cap is not None}
    assert capped == {"psnr_hvs": vp.PSNR_HVS_DB_CAP, "psnr_hvsm": vp.PSNR_HVS_DB_CAP, "ciede2000": vp.PSNR_HVS_DB_CAP,
                      "xpsnr": vp.PSNR_HVS_DB_CAP, "pu_psnr": vp.PU21_PSNR_CAP, "pu_psnr_rgb": vp.PU21_PSNR_CAP}
    # the golden log of every kind at once has exactly the table's keys (BRISQUE's score needs its model), in its order
    assert list(json.loads(GOLDEN["all"]["log"])["pooled_metrics"]) == [k for k in keys if k != "brisque"]


def test_the_callers_keywords_stay_checked(tmp_path):
    log = str(tmp_path / "v.json")
    with pytest.raises(TypeError):
        vp.write_vif_log(log, itp=None)                          # the kind's name is not the flag
    with pytest.raises(TypeError):
        vp.write_vif_log(log, None, None, None)                  # motion and what follows it are keyword-only
    with pytest.raises(TypeError):
        vp._write_feature_log(log, (None, None), True, False)    # no positional switches any more
    vp._write_feature_log(log, (np.zeros((0, 1), np.uint64), np.zeros((0, 1))), {})
    assert json.load(open(log)) == {"frames": [], "pooled_metrics": {}}


# ---- (3) config -> switches --------------------------------------------------------------------------------------------------
def test_config_to_switches():
    config = dict(GOOD, vif=True, adm=True, motion_feature=True, motion="farneback", siti=True, psnr_hvs=True, ciede=True,
                  ciede_weights=[0.65, 1, 4], gmsd=True, cambi=True, xpsnr=True, haarpsi=True, vca=True, artifacts=True, brisque=True,
                  brisque_model_path="b.model", brisque_range_path="b.range", mdsi=True, delta_itp=True, delta_itp_transfer="hlg",
                  delta_itp_range="full", pu21=True, pu21_transfer="hlg", pu21_range="full", fsim=True, sigstats=True,
                  sigstats_black=40, sigstats_crop=12, vmaf_model_path="v.json")
    assert vp._config_switches(config) == {
        "vif": True, "adm": True, "motion": True, "siti": True, "psnr_hvs": True, "ciede": True, "ciede_weights": (0.65, 1, 4),
        "gmsd": True, "cambi": True, "xpsnr": True, "haarpsi": True, "vca": True, "artifacts": True, "brisque": True,
        "brisque_model_path": "b.model", "brisque_range_path": "b.range", "mdsi": True, "itp": True, "itp_transfer": "hlg",
        "itp_full_range": True, "pu21": True, "pu21_transfer": "hlg", "pu21_full_range": True, "fsim": True, "sigstats": True,
        "sigstats_black": 40, "sigstats_crop": 12, "vmaf_model_path": "v.json"}
    off = {k.name: False for k in stream.PLANE_KINDS}
    assert vp._config_switches(dict(GOOD)) == dict(off, vmaf_model_path=None)
    # the config's "motion" is the complexity half's motion mode, "motion_feature" the kind's switch
    assert vp._config_switches(dict(GOOD, motion="sad")) == dict(off, vmaf_model_path=None)
    assert vp._config_switches(dict(GOOD, motion_feature=True)) == dict(off, motion=True, vmaf_model_path=None)
    # the model files turn their kinds on; the ranges go through ITP_RANGES
    assert vp._config_switches(dict(GOOD, brisque_model_path="b.model")) == dict(off, brisque=True, brisque_model_path="b.model",
                                                                               vmaf_model_path=None)
    assert vp._config_switches(dict(GOOD, brisque=False, brisque_model_path=None)) == dict(off, brisque_model_path=None,
                                                                                         vmaf_model_path=None)
    assert vp._config_switches(dict(GOOD, vmaf_model_path="v.json", adm=False)) == dict(off, vif=True, adm=True, motion=True,
                                                                                      vmaf_model_path="v.json")
    assert vp._config_switches(dict(GOOD, delta_itp_range="limited", pu21_range="full")) == dict(
        off, itp_full_range=False, pu21_full_range=True, vmaf_model_path=None)
    # what the switches say beyond the paths is exactly what Quality takes
    sw = vp._config_switches(config)
    q = stream.Quality(yuv420p_planes(64, 64), **{k: v for k, v in sw.items() if k not in features.MODEL_PATHS})
    assert q.itp is True and q.itp_full_range is True and q.ciede_weights == (0.65, 1.0, 4.0)


@pytest.mark.parametrize("key", SWITCH_KEYS)
def test_a_boolean_key_that_is_no_boolean(key, tmp_path, monkeypatch):
    def no_device(*a, **kw):
        raise AssertionError("the pass started")
    monkeypatch.setattr(stream, "run", no_device)
    monkeypatch.setattr(stream, "get_engine", no_device)
    fr = np.zeros((2, 32, 32, 3), np.uint8)
    for bad in (1, 0, "true", None, "only"):
        with pytest.raises(ValueError) as e:
            vp.validate_config(dict(GOOD, **{key: bad}))
        assert str(e.value) == "%s must be true or false." % key
        with pytest.raises(ValueError) as e:
            vp.process_video_and_extract_metrics(fr, fr, dict(GOOD, **{key: bad}), csv_file=str(tmp_path / "row.csv"))
        assert str(e.value) == "%s must be true or false." % key
    assert not os.path.exists(str(tmp_path / "row.csv"))
    vp.validate_config(dict(GOOD, **{key: True}))
    vp.validate_config(dict(GOOD, **{key: False}))


def test_the_parameters_messages():
    """one bad key at a time: the messages of the kinds' parameters, as they were"""
    for key, bad, want in (
            ("ciede_weights", [1, 1], "ciede_weights must be three positive numbers [kL, kC, kH]."),
            ("ciede_weights", [1, 1, True], "ciede_weights must be three positive numbers [kL, kC, kH]."),
            ("brisque_model_path", "/nowhere/m.model", "brisque_model_path must be null or the path of a readable file."),
            ("brisque_range_path", "/nowhere/m.range", "brisque_range_path must be null or the path of a readable file."),
            ("brisque_range_path", __file__, "brisque_range_path needs a brisque_model_path."),
            ("delta_itp_transfer", "sdr", 'delta_itp_transfer must be "pq" or "hlg".'),
            ("delta_itp_range", True, 'delta_itp_range must be "limited" or "full".'),
            ("pu21_transfer", None, 'pu21_transfer must be "pq" or "hlg".'),
            ("pu21_range", "tv", 'pu21_range must be "limited" or "full".'),
            ("sigstats_black", -1, "sigstats_black must be null or an integer from 0 to 65535."),
            ("sigstats_crop", 1.5, "sigstats_crop must be null or an integer from 0 to 65535.")):
        with pytest.raises(ValueError) as e:
            vp.validate_config(dict(GOOD, **{key: bad}))
        assert str(e.value) == want, key


# ---- (4) flags -> Quality ----------------------------------------------------------------------------------------------------
def test_flags_to_quality(tmp_path, monkeypatch):
    h = w = 64
    planes = yuv420p_planes(h, w)
    n, p = 2, len(planes)
    seen = []

    def recorder(frames, ref, quality=None, **kw):
        """-> records of zeros in the layout stream.run states: sse, ssim, then vif / adm / motion up to the last of them that
        is on (None where one is off) and one element per later kind that is on, in the table's order"""
        seen.append((frames, ref, quality, kw))
        on = {k.name: getattr(quality, k.name) for k in stream.PLANE_KINDS}
        head = 3 if on["motion"] else 2 if on["adm"] else 1 if on["vif"] else 0
        out = [np.zeros((n, p), np.uint64), np.zeros((n, p), np.float64)]
        for k in list(stream.PLANE_KINDS[:head]) + [k for k in stream.PLANE_KINDS[3:] if on[k.name]]:
            dtype = stream.MOTION_PASS_DTYPE if k.name == "motion" else k.dtype
            out.append(np.zeros((n,) if k.per_frame else (n, p), dtype) if on[k.name] else None)
            if k.name == "sigstats":
                out[-1]["count"] = 1
        return tuple(out), None

    monkeypatch.setattr(stream, "run", recorder)
    rng = np.random.default_rng(3)
    paths = {k: tmp_path / k for k in ("v.model", "b.model", "b.range")}
    paths["v.model"].write_text(VMAF_MODEL)
    paths["b.model"].write_text(BC.model_text(rng))
    paths["b.range"].write_text(BC.range_text(rng.uniform(-2, 0, 36), rng.uniform(1, 3, 36)))
    logs = [str(tmp_path / k) for k in ("psnr.log", "ssim.log", "vmaf.json")]
    ref, dist = np.zeros((n, h * w * 3 // 2), np.uint8), np.ones((n, h * w * 3 // 2), np.uint8)
    assert vp.run_ffmpeg_metrics(
        ref, dist, *logs, vmaf_model_path=str(paths["v.model"]), layout="yuv420p", ssim_mode="ffmpeg", height=h, width=w,
        batch_size=5, device=None, vif=True, adm=True, motion=True, siti=True, psnr_hvs=True, ciede=True, ciede_weights=(0.65, 1, 4),
        gmsd=True, cambi=True, xpsnr=True, haarpsi=True, vca=True, artifacts=True, brisque=True,
        brisque_model_path=str(paths["b.model"]), brisque_range_path=str(paths["b.range"]), mdsi=True, delta_itp=True,
        delta_itp_transfer="hlg", delta_itp_full_range=True, pu21=True, pu21_transfer="hlg", pu21_full_range=True, fsim=True,
        sigstats=True, sigstats_black=40, sigstats_crop=12) is None
    assert len(seen) == 1
    frames, reference, quality, kw = seen[0]
    assert frames is dist and reference is ref                       # the distorted stream first, as stream.run takes them
    assert sorted(kw) == ["batch_size", "device", "on_quality"] and kw["batch_size"] == 5 and kw["device"] is None
    got = {k: v for k, v in vars(quality).items() if k != "planes"}
    assert got == {
        "ssim_mode": N.SSIM_FFMPEG, "scales": False, "ssim": True, "dist_planes": None, "scale": None, "vif": True, "adm": True,
        "motion": True, "siti": True, "psnr_hvs": True, "ciede": True, "ciede_weights": (0.65, 1.0, 4.0), "gmsd": True, "cambi": True,
        "xpsnr": True, "haarpsi": True, "vca": True, "vca_blocks": False, "artifacts": True, "brisque": True, "mdsi": True, "itp": True,
        "itp_transfer": "hlg", "itp_full_range": True, "pu21": True, "pu21_transfer": "hlg", "pu21_full_range": True, "fsim": True,
        "sigstats": True, "sigstats_black": 40, "sigstats_crop": 12}
    assert list(quality.planes) == list(planes)
    doc = json.load(open(logs[2]))
    keys = list(json.loads(GOLDEN["all"]["log"])["pooled_metrics"])   # the order the code before the table wrote
    at = keys.index("brisque_35") + 1
    want = keys[:at] + ["brisque"] + keys[at:] + ["vmaf"]
    assert list(doc) == ["frames", "pooled_metrics", "signal"] and len(doc["frames"]) == n
    assert list(doc["pooled_metrics"]) == want and all(list(f["metrics"]) == want for f in doc["frames"])
    # nothing asked for: the same one pass, every kind off, and no feature log
    os.remove(logs[2])
    vp.run_ffmpeg_metrics(ref, dist, *logs, layout="yuv420p", height=h, width=w)
    quality = seen[1][2]
    assert not any(getattr(quality, k.name) for k in stream.PLANE_KINDS) and quality.ssim_mode == N.SSIM_GAUSS
    assert (quality.ciede_weights, quality.itp_transfer, quality.pu21_full_range, quality.sigstats_black) == (
        tuple(float(x) for x in N.CIEDE_WEIGHTS_CIE), "pq", False, None)
    assert not os.path.exists(logs[2])
    # a model file alone turns its kinds on
    vp.run_ffmpeg_metrics(ref, dist, *logs, layout="yuv420p", height=h, width=w, vmaf_model_path=str(paths["v.model"]))
    on = [k.name for k in stream.PLANE_KINDS if getattr(seen[2][2], k.name)]
    assert on == ["vif", "adm", "motion"] and list(json.load(open(logs[2]))["pooled_metrics"])[-1] == "vmaf"
    vp.run_ffmpeg_metrics(ref, dist, *logs, layout="yuv420p", height=h, width=w, brisque_model_path=str(paths["b.model"]))
    assert [k.name for k in stream.PLANE_KINDS if getattr(seen[3][2], k.name)] == ["brisque"]
    assert list(json.load(open(logs[2]))["pooled_metrics"]) == keys[keys.index("brisque_00"):at] + ["brisque"]


# ---- (5) the frame_* calls' argument errors ----------------------------------------------------------------------------------
def test_which_error_of_a_frame_call_comes_first(monkeypatch):
    def no_device(*a, **kw):
        raise AssertionError("the pass started")
    monkeypatch.setattr(stream, "run", no_device)
    g, y = np.zeros((2, 16, 16), np.uint8), np.zeros((2, 384), np.uint8)
    fl = np.zeros((2, 384), np.float32)
    with pytest.raises(ValueError) as e:
        vp.frame_ciede(fl[:, :256].reshape(2, 16, 16), g, "gray", 16, 16)      # the layout before the frames' type
    assert str(e.value) == "ciede needs three planes"
    with pytest.raises(ValueError) as e:
        vp.frame_delta_itp(fl, y, "yuv420p", 16, 16, transfer="sdr")            # the transfer before the frames' type
    assert str(e.value) == "delta_itp_transfer must be 'pq' or 'hlg'"
    with pytest.raises(ValueError) as e:
        vp.frame_pu21(g, g, "gray", 16, 16, transfer="sdr")                     # the layout before the transfer
    assert str(e.value) == "pu21 needs three planes"
    with pytest.raises(ValueError) as e:
        vp.frame_pu21(y, y[:, :383], "yuv420p", 16, 16, full_range=1)           # the range before the shapes
    assert str(e.value) == "pu21_full_range must be True or False"
    for call in (vp.frame_vif, vp.frame_psnr_hvs, vp.frame_ciede, vp.frame_delta_itp, vp.frame_fsim):
        with pytest.raises(ValueError) as e:
            call(fl, y[:, :383], "yuv420p", 16, 16)                              # the frames' type before the shapes
        assert str(e.value) == "frames must be uint8 (got float32)"
        with pytest.raises(ValueError) as e:
            call(y, y[:1], "yuv420p", 16, 16)
        assert str(e.value) == "ref and dist must have the same shape"
    for call in (vp.frame_motion, vp.frame_cambi, vp.frame_sigstats):
        with pytest.raises(ValueError) as e:
            call(fl, "yuv420p", 16, 16)
        assert str(e.value) == "frames must be uint8 (got float32)"
    with pytest.raises(ValueError) as e:
        vp.frame_sigstats(y, "yuv420p", 16, 16, black_level=-1)                 # Quality's own check, under Quality's name
    assert str(e.value) == "sigstats_black must be None or an integer from 0 to 65535"
