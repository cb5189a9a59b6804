"""The VMAF predictor on the host (no GPU): vmaf_model.load_model / predict against hand-computed answers and against the
plain-loop float64 restatement of tests/vmaf_reference.py, on models the tests write in both accepted formats; the inputs that
are refused; the "vmaf" key of the JSON log, the VMAF column of the row and the validation of vmaf_model_path."""
import json
import math

import numpy as np
import pytest

import vmaf_reference as R
from rtvqa_amd import stream, tails, vmaf_model
from rtvqa_amd import video_processing as vp

GOOD = {"crf": 23, "vmaf_model_path": None, "resize_width": 64, "resize_height": 64, "frame_interval": 10}
# magnitudes of vmaf_v0.6.1: slopes / intercepts (index 0: the score), clip, gamma, |coef| <= 4
SLOPES = [0.012020766332648465, 2.8098077502505414, 0.06264407466686016, 1.2227634563978586, 1.5360318811084146,
          1.7620864995501058, 2.08656468286432]
INTERCEPTS = [-0.3092981927591963, -1.7993968597186747, -0.003017198086831897, -0.1728125095425364, -0.5294309090081222,
              -0.7577185792093722, -1.083428597549764]
CLIP = (0.0, 100.0)
GAMMA = 0.04


def _random_model(seed=7, n_sv=211, k=6):
    rng = np.random.default_rng(seed)
    sv = rng.random((n_sv, k))
    sv[rng.random((n_sv, k)) < 0.15] = 0.0          # zeros: the sparse text leaves them out
    sv[3] = 0.0                                     # a support vector with no index at all
    coef = rng.uniform(-4.0, 4.0, n_sv)
    coef[:20] = 4.0 * np.sign(coef[:20])            # bounded ones sit at +-C
    return sv, coef


def _features(n, seed=8):
    """per frame: adm2, motion2, vif_scale0..3 in their natural ranges"""
    rng = np.random.default_rng(seed)
    f = np.stack([rng.uniform(0.6, 1.0, n), rng.uniform(0.0, 20.0, n)] + [rng.uniform(0.3 + 0.15 * s, 1.0, n) for s in range(4)], axis=1)
    f[0, 1] = 0.0
    return f


def _rho_for(sv, coef, feats, target=0.3):
    """the rho that puts the median frame at y = target (a score of about 50)"""
    ys = [R.predict_one(list(f), [1.0] + SLOPES[1:], [0.0] + INTERCEPTS[1:], None, GAMMA, 0.0, coef, sv) for f in feats]
    return float(np.median(ys) - target)


def test_one_support_vector_by_hand(tmp_path):
    """x' = sv gives the kernel value 1: y = coef - rho; one unit away along one axis gives coef exp(-gamma) - rho"""
    sv, coef, rho, gamma = [[0.5, 0.25, 0.0, 1.0, 0.75, 0.125]], [2.5], 0.75, 0.5
    p = tmp_path / "one.model"
    p.write_text(R.libsvm_text(gamma, rho, coef, sv))
    m = vmaf_model.load_model(str(p))
    assert m.features == R.FEATURES_V061 and m.score_clip is None and m.sv.shape == (1, 6) and m.sv[0].tolist() == sv[0]
    assert vmaf_model.predict(m, [sv[0]]).tolist() == [2.5 - 0.75]
    f = list(sv[0])
    f[2] += 1.0
    assert abs(vmaf_model.predict(m, [f])[0] - (2.5 * math.exp(-0.5) - 0.75)) <= 1e-15
    # the JSON form: x' = slope f + intercept, score = (y - intercept_0) / slope_0
    slopes, intercepts = [0.5, 2.0, 1.0, 1.0, 4.0, 1.0, 1.0], [-1.0, 0.1, 0.0, 0.0, -1.0, 0.0, 0.0]
    q = tmp_path / "one.json"
    q.write_text(R.json_model(gamma, rho, coef, sv, slopes, intercepts))
    mj = vmaf_model.load_model(str(q))
    f = [(0.5 - 0.1) / 2.0, 0.25, 0.0, (1.0 + 1.0) / 4.0, 0.75, 0.125]        # lands exactly on the support vector
    assert abs(vmaf_model.predict(mj, [f])[0] - ((2.5 - 0.75) + 1.0) / 0.5) <= 1e-12
    assert vmaf_model.predict(mj, f).shape == (1,)


def test_a_random_model_in_both_formats_against_the_loops(tmp_path):
    sv, coef = _random_model()
    feats = _features(300)
    rho = _rho_for(sv, coef, feats)
    pj, pt = tmp_path / "m.json", tmp_path / "m.model"
    pj.write_text(R.json_model(GAMMA, rho, coef, sv, SLOPES, INTERCEPTS, CLIP))
    pt.write_text(R.libsvm_text(GAMMA, rho, coef, sv))
    assert len(pt.read_text().splitlines()[7 + 3].split()) == 1            # support vector 3 is all zeros: the coefficient alone
    mj, mt = vmaf_model.load_model(str(pj)), vmaf_model.load_model(str(pt))
    assert np.array_equal(mj.sv, sv) and np.array_equal(mt.sv, sv) and np.array_equal(mj.coef, coef)   # repr round-trips; sparse
    assert mj.features == R.FEATURES_V061 and mj.score_clip == CLIP and mt.score_clip is None
    got = vmaf_model.predict(mj, feats)
    want = np.array(R.predict(feats, SLOPES, INTERCEPTS, CLIP, GAMMA, rho, coef, sv))
    raw = np.array(R.predict(feats, SLOPES, INTERCEPTS, None, GAMMA, rho, coef, sv))
    inside = (raw > 0.0) & (raw < 100.0)
    print("scores inside [0, 100]:", int(inside.sum()), "of", len(raw), "worst gap %.3e" % np.abs(got - want).max())
    assert inside.sum() >= 20 and (raw < 0.0).any() and (raw > 100.0).any()
    assert got.dtype == np.float64 and np.abs(got - want)[inside].max() <= 1e-9
    # the clip is applied
    assert (got[raw <= 0.0] == 0.0).all() and (got[raw >= 100.0] == 100.0).all() and got.min() >= 0.0 and got.max() <= 100.0
    # the bare text model: no normalisation, no clip
    got_t = vmaf_model.predict(mt, feats)
    want_t = np.array(R.predict(feats, [1.0] * 7, [0.0] * 7, None, GAMMA, rho, coef, sv))
    assert np.abs(got_t - want_t).max() <= 1e-9
    # a frame's score does not depend on the other frames of the call
    for i in (0, 1, 77, 299):
        assert vmaf_model.predict(mj, feats[i:i + 1])[0] == got[i]
    assert vmaf_model.predict(mj, feats[:0]).shape == (0,)
    # epsilon_svr reads the same; score_transform is ignored, as libvmaf does by default
    pe = tmp_path / "e.json"
    pe.write_text(R.json_model(GAMMA, rho, coef, sv, SLOPES, INTERCEPTS, CLIP,
                               score_transform={"p0": 1.7, "p1": 1.04, "p2": -0.002, "out_gte_in": "true"},
                               feature_opts_dicts=[{}] * 6).replace("svm_type nu_svr", "svm_type epsilon_svr"))
    assert np.array_equal(vmaf_model.predict(vmaf_model.load_model(str(pe)), feats), got)
    # the features may come in another order and be others of the log's
    names = ("vif_scale3", "adm_scale1", "motion")
    pm = tmp_path / "other.json"
    pm.write_text(R.json_model(GAMMA, 0.1, coef[:5], sv[:5, :3], SLOPES[:4], INTERCEPTS[:4], None, features=names))
    mo = vmaf_model.load_model(str(pm))
    assert mo.features == names
    cols = {"motion": feats[:, 1], "adm_scale1": feats[:, 0], "vif_scale3": feats[:, 5], "adm2": feats[:, 0]}
    x = vmaf_model.feature_matrix(mo, cols)
    assert np.array_equal(x, np.stack([feats[:, 5], feats[:, 0], feats[:, 1]], axis=1))
    want_o = np.array(R.predict(x, SLOPES[:4], INTERCEPTS[:4], None, GAMMA, 0.1, coef[:5], sv[:5, :3]))
    assert np.abs(vmaf_model.predict(mo, x) - want_o).max() <= 1e-9
    with pytest.raises(ValueError, match="not measured: motion"):
        vmaf_model.feature_matrix(mo, {"adm_scale1": feats[:, 0], "vif_scale3": feats[:, 5]})
    with pytest.raises(ValueError, match="3 features"):
        vmaf_model.predict(mo, feats)


def _bad_json(tmp_path, name, **change):
    sv, coef = [[0.5] * 6, [0.25] * 6], [1.0, -1.0]
    doc = json.loads(R.json_model(0.04, 0.5, coef, sv, SLOPES, INTERCEPTS, CLIP))
    for k, v in change.items():
        if v is None:
            doc["model_dict"].pop(k)
        else:
            doc["model_dict"][k] = v
    p = tmp_path / name
    p.write_text(json.dumps(doc))
    return str(p)


def test_what_is_refused_names_what_was_met(tmp_path):
    text = R.libsvm_text(0.04, 0.5, [1.0, -1.0], [[0.5] * 6, [0.25] * 6])
    vmaf_model.load_model(_bad_json(tmp_path, "ok.json"))
    cases = [
        (_bad_json(tmp_path, "a.json", model=text.replace("kernel_type rbf", "kernel_type linear")), "kernel_type must be rbf .got 'linear'"),
        (_bad_json(tmp_path, "b.json", model=text.replace("svm_type nu_svr", "svm_type c_svc")), "svm_type must be nu_svr or epsilon_svr .got 'c_svc'"),
        (_bad_json(tmp_path, "c.json", feature_names=["VMAF_feature_adm2_score", "VMAF_feature_ansnr_score"] + ["VMAF_feature_vif_scale%d_score" % s for s in range(4)]),
         "unknown feature name 'VMAF_feature_ansnr_score'"),
        (_bad_json(tmp_path, "d.json", slopes=SLOPES[:6]), "slopes must have 1 . 6 entries .got 6"),
        (_bad_json(tmp_path, "e.json", intercepts=INTERCEPTS + [0.0]), "intercepts must have 1 . 6 entries .got 8"),
        (_bad_json(tmp_path, "f.json", model_type="RESIDUEBOOTSTRAP_LIBSVMNUSVR"), "model_type must be LIBSVMNUSVR .got 'RESIDUEBOOTSTRAP_LIBSVMNUSVR'"),
        (_bad_json(tmp_path, "g.json", norm_type="clip_0to1"), "norm_type must be linear_rescale .got 'clip_0to1'"),
        (_bad_json(tmp_path, "h.json", model=text.replace("total_sv 2", "total_sv 3")), "total_sv says 3 support vectors, 2 follow"),
        (_bad_json(tmp_path, "i.json", model=text.replace("6:0.5", "7:0.5")), "index 7, the model has 6 features"),
        (_bad_json(tmp_path, "j.json", model=text.replace("rho 0.5", "rho 0.5\nprobA 1.0")), "unsupported header line 'probA 1.0'"),
        (_bad_json(tmp_path, "k.json", model=text.replace("gamma 0.04\n", "")), "no 'gamma' line"),
        (_bad_json(tmp_path, "l.json", score_clip=[0.0]), "score_clip must be .lo, hi."),
        (_bad_json(tmp_path, "m.json", feature_opts_dicts=[{"adm_enhn_gain_limit": 1.0}] + [{}] * 5), "feature options are not supported"),
        (_bad_json(tmp_path, "n.json", model=None), "'model' must be libsvm's text model"),
        (_bad_json(tmp_path, "o.json", transform_something=1), "unsupported key 'transform_something'"),
        (_bad_json(tmp_path, "p.json", model=text.replace("SV\n", "")), "unsupported header line|no 'SV' line"),
    ]
    for path, msg in cases:
        with pytest.raises(ValueError, match=msg):
            vmaf_model.load_model(path)
    p = tmp_path / "q.json"
    p.write_text('{"model_dict": ')
    with pytest.raises(ValueError, match="not valid JSON"):
        vmaf_model.load_model(str(p))
    p = tmp_path / "r.json"
    p.write_text('{"other": 1}')
    with pytest.raises(ValueError, match="needs a 'model_dict' object"):
        vmaf_model.load_model(str(p))
    p = tmp_path / "s.model"
    p.write_text(text.replace("kernel_type rbf", "kernel_type polynomial\ndegree 3"))
    with pytest.raises(ValueError, match="unsupported header line 'degree 3'|kernel_type must be rbf"):
        vmaf_model.load_model(str(p))
    p.write_text(text.replace("1:0.5", "1:abc", 1))
    with pytest.raises(ValueError, match="cannot read support vector line"):
        vmaf_model.load_model(str(p))
    with pytest.raises(OSError):
        vmaf_model.load_model(str(tmp_path / "absent.json"))


def _log_inputs(n=5, seed=3):
    from rtvqa_amd.engine import ADM_DTYPE
    f = _features(n, seed)
    adm = np.zeros(n, ADM_DTYPE)
    adm["adm2"], adm["scale"] = f[:, 0], 0.9
    mot = np.zeros(n, stream.MOTION_PASS_DTYPE)
    mot["motion"] = np.append(0.0, f[1:, 1] + 1.0)
    mot["motion2"] = tails.motion2(mot["motion"])
    return f[:, 2:6], adm, mot


def test_the_vmaf_key_of_the_log_and_the_vmaf_column_of_the_row(tmp_path):
    sv, coef = _random_model()
    vif, adm, mot = _log_inputs()
    feats = np.column_stack([adm["adm2"], mot["motion2"], vif])
    rho = _rho_for(sv, coef, feats)
    pj = tmp_path / "m.json"
    pj.write_text(R.json_model(GAMMA, rho, coef, sv, SLOPES, INTERCEPTS, CLIP))
    model = vmaf_model.load_model(str(pj))
    plain, log = str(tmp_path / "plain.json"), str(tmp_path / "vmaf.json")
    vp.write_vif_log(plain, vif, adm, motion=mot)
    vp.write_vif_log(log, vif, adm, motion=mot, model=model)
    doc0, doc = json.load(open(plain)), json.load(open(log))
    assert "vmaf" not in json.dumps(doc0)
    names0 = list(doc0["frames"][0]["metrics"])
    assert list(doc["frames"][0]["metrics"]) == names0 + ["vmaf"] and list(doc["pooled_metrics"]) == names0 + ["vmaf"]
    want = np.array(R.predict(feats, SLOPES, INTERCEPTS, CLIP, GAMMA, rho, coef, sv))
    for i, fr in enumerate(doc["frames"]):
        m = fr["metrics"]
        assert {k: m[k] for k in names0} == doc0["frames"][i]["metrics"]
        logged = [m[k] for k in R.FEATURES_V061]
        assert m["vmaf"] == vmaf_model.predict(model, [logged])[0]        # bit for bit, from the frame's own logged features
        assert abs(m["vmaf"] - want[i]) <= 1e-9
    x = np.array([fr["metrics"]["vmaf"] for fr in doc["frames"]])
    p = doc["pooled_metrics"]["vmaf"]
    assert sorted(p) == ["harmonic_mean", "max", "mean", "min"]
    assert p["min"] == x.min() and p["max"] == x.max() and abs(p["mean"] - x.mean()) <= 1e-13
    assert abs(p["harmonic_mean"] - (len(x) / (1.0 / (x + 1.0)).sum() - 1.0)) <= 1e-13
    # a model that needs what was not measured
    with pytest.raises(ValueError, match="not measured: motion2"):
        vp.write_vif_log(str(tmp_path / "x.json"), vif, adm, model=model)
    pl, sl = tmp_path / "psnr.log", tmp_path / "ssim.log"
    pl.write_text("n:1 mse_avg:1.00 psnr_avg:48.13 \n")
    sl.write_text("n:1 Y:0.990000 All:0.990000 (20.000000)\n")
    row0 = vp.extract_metrics_from_logs(str(pl), str(sl), plain, "x", 23, 1000, "64x64", 30.0)
    row = vp.extract_metrics_from_logs(str(pl), str(sl), log, "x", 23, 1000, "64x64", 30.0)
    assert "VMAF" not in row0 and list(row0)[-2:] == ["MOTION2", "MOTION"]
    keys = list(row)
    assert keys[keys.index("SSIM") + 1] == "VMAF" and keys[-2:] == ["MOTION2", "MOTION"]
    assert [k for k in keys if k != "VMAF"] == list(row0) and {k: row[k] for k in row0} == row0
    assert row["VMAF"] == p["mean"]


def test_config_key_vmaf_model_path_names_a_readable_file(tmp_path):
    msg = "vmaf_model_path must be null or the path of a readable model file."
    vp.validate_config(dict(GOOD))
    p = tmp_path / "m.json"
    p.write_text("{}")
    vp.validate_config(dict(GOOD, vmaf_model_path=str(p)))               # (what the file holds is load_model's business)
    for bad in (str(tmp_path / "absent.json"), str(tmp_path), 1, True, ["x"], ""):
        with pytest.raises(ValueError) as e:
            vp.validate_config(dict(GOOD, vmaf_model_path=bad))
        assert str(e.value) == msg
    cfg = tmp_path / "config.json"
    cfg.write_text(json.dumps(dict(GOOD, vmaf_model_path=str(p), motion_feature=True)))
    assert vp.load_config(str(cfg))["vmaf_model_path"] == str(p)


def test_a_bad_model_stops_the_entry_points_before_any_pass(tmp_path):
    """the model is loaded before the streams are opened: a bad file raises its ValueError with no device in sight"""
    p = tmp_path / "bad.json"
    p.write_text(json.dumps({"model_dict": {"model_type": "LIBSVMNUSVR", "norm_type": "none"}}))
    z = np.zeros((2, 16, 16, 3), np.uint8)
    with pytest.raises(ValueError, match="norm_type must be linear_rescale"):
        vp.run_ffmpeg_metrics(z, z, str(tmp_path / "p.log"), str(tmp_path / "s.log"), str(tmp_path / "v.json"), str(p))
    assert not (tmp_path / "p.log").exists()
    with pytest.raises(ValueError, match="norm_type must be linear_rescale"):
        vp.process_video_and_extract_metrics(z, z, dict(GOOD, vmaf_model_path=str(p)), csv_file=str(tmp_path / "row.csv"))
    assert not (tmp_path / "row.csv").exists()
