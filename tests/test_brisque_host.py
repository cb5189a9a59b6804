"""CPU: the float64 restatement of BRISQUE's features (tests/brisque_reference.py) against SciPy, torch and closed forms; the
integer restatement (quantised u, exact-sign classing) against it within the derived bars; the admission rule; the model and
range files; the log and the row; the ABI.

The admission rule.  The issue states it per content: admitted when moving each ratio by its bar moves alpha by at most 2 grid
steps.  Measured here, the natural-like content does not pass it as a whole on 10 of the grid's 61 planes: one or two of their
ten fits miss it, nearly always the GGD of scale 1 on planes whose scale-1 field has at most 425 samples, where alpha sits at
4 .. 6 and the ratio curve is flat (spans of 3 .. 5 steps).  So admission is kept PER FIT - the same criterion, applied to each
alpha by itself - and the fits that miss it are named one by one in brisque_cases.NOT_ADMITTED: test_the_admission_rule holds
that set to be exactly those 11 of 610, none of them at scale 0."""
import ctypes as C
import json
import math

import numpy as np
import pytest

import brisque_cases as BC
import brisque_reference as R
from rtvqa_amd import _native as N
from rtvqa_amd import stream
from rtvqa_amd import video_processing as vp

GOOD = {"crf": 23, "resize_width": 64, "resize_height": 64, "frame_interval": 1}
FIELDS = BC.FIELDS
W0 = R.window()[3, 3]
M_BOUND = math.sqrt((1.0 - W0) / W0)


# ---- (a) the pieces of the float64 restatement ------------------------------------------------------------------------------
def test_the_window_and_the_moments_against_scipy():
    from scipy import ndimage
    assert abs(W0 - 0.11740) < 5e-6 and abs(M_BOUND - 2.742) < 5e-4 and abs(R.window().sum() - 1.0) < 1e-15
    assert R.M_MAX >= M_BOUND
    rng = np.random.default_rng(1)
    for shape, peak in (((16, 16), 255), ((23, 31), 1023), ((40, 17), 65535)):
        x = rng.integers(0, peak + 1, shape).astype(np.float64)
        mu, sxx = R.moments(x)
        want_mu = ndimage.correlate(x, R.window(), mode="constant", cval=0.0)
        want_sxx = ndimage.correlate(x * x, R.window(), mode="constant", cval=0.0)
        assert np.abs(mu - want_mu).max() <= 1e-12 * peak and np.abs(sxx - want_sxx).max() <= 1e-12 * peak * peak


def test_half_against_torch_on_the_interior_of_even_sizes():
    import torch
    rng = np.random.default_rng(2)
    for shape, peak in (((16, 16), 255), ((24, 40), 255), ((32, 20), 65535)):
        x = rng.integers(0, peak + 1, shape).astype(np.int64)
        t = torch.from_numpy(x.astype(np.float64))[None, None]
        want = torch.nn.functional.interpolate(t, scale_factor=0.5, mode="bicubic", antialias=True)[0, 0].numpy()
        got = R.half(x)
        assert got.shape == want.shape == (shape[0] // 2, shape[1] // 2)
        assert np.array_equal(got[2:-2, 2:-2], want[2:-2, 2:-2])           # torch renormalises the outer two of each edge
        assert not np.array_equal(got, want)


def test_half_borders_odd_sizes_and_flat_planes_by_hand():
    t = [-3, -9, 29, 111, 111, 29, -9, -3]
    row = np.arange(17, dtype=np.int64) ** 2 % 23                          # 17 wide: 9 outputs
    x = np.broadcast_to(row, (16, 17)).copy()
    got = R.half_int(x)
    assert got.shape == (8, 9)

    def at(i):                                                             # aux = [0 .. 16, 16 .. 0], index mod 34
        m = i % 34
        return int(row[m] if m < 17 else row[33 - m])

    want = [sum(t[k] * at(2 * o - 3 + k) for k in range(8)) for o in range(9)]
    assert at(-1) == row[0] and at(-3) == row[2] and at(17) == row[16] and at(20) == row[13]
    assert got[3].tolist() == [256 * v for v in want]                      # (a constant column: the column pass multiplies by 256)
    assert want[0] == -3 * row[2] - 9 * row[1] + 29 * row[0] + 111 * row[0] + 111 * row[1] + 29 * row[2] - 9 * row[3] - 3 * row[4]
    assert want[8] == -3 * row[13] - 9 * row[14] + 29 * row[15] + 111 * row[16] + 111 * row[16] + 29 * row[15] - 9 * row[14] - 3 * row[13]
    for shape in ((16, 16), (17, 25), (33, 16)):
        flat = R.half_int(np.full(shape, 200, np.int64))
        assert flat.shape == ((shape[0] + 1) // 2, (shape[1] + 1) // 2) and (flat == 200 * 65536).all()
    # it overshoots: below zero and above the peak, beyond 32 bits at 16 bits
    x = np.zeros((16, 16), np.int64)
    x[:, 8:] = 65535
    h = R.half_int(x)
    assert h.min() < 0 and h.max() > 65535 * 65536 and h.max() > 2 ** 32 and abs(h).max() <= 304 * 304 * 65535


def test_the_gamma_ratios_against_scipy():
    from scipy.special import gamma
    r, inv = R.tables()
    assert len(r) == 9801 and R.GAM[0] == 0.2 and R.GAM[-1] == 10.0 and R.GAM[1800] == 2.0
    for k in (0, 1, 300, 800, 1800, 5000, 9800):
        g = R.GAM[k]
        want = gamma(1.0 / g) * gamma(3.0 / g) / gamma(2.0 / g) ** 2
        assert abs(r[k] - want) <= 1e-11 * want and abs(inv[k] - 1.0 / want) <= 1e-11 / want
    assert abs(r[1800] - math.pi / 2.0) < 1e-12 and abs(r[800] - 2.0) < 1e-12   # the Gaussian and the Laplacian
    assert (np.diff(r) < 0).all() and (np.diff(inv) > 0).all()


@pytest.mark.parametrize("beta", [0.7, 1.0, 2.0, 3.5])
def test_the_ggd_fit_recovers_gennorm(beta):
    """4e5 seeded draws: the ratio's sampling error is about 3 / sqrt(n) = 0.5 %, which moves alpha by up to 1.5 % at beta 3.5
    where the curve is flattest: the bar is 2 %"""
    from scipy.stats import gennorm
    x = gennorm.rvs(beta, size=400000, random_state=np.random.default_rng(int(beta * 10)))
    alpha, _k = R.fit_ggd(float((x * x).mean()), float(np.abs(x).mean()))
    assert abs(alpha - beta) <= 0.02 * beta, (beta, alpha)


def test_the_aggd_fit_recovers_a_two_sided_gennorm():
    """left scale 1, right scale 2, shape 1.5: alpha, and l^2 / r^2 in the ratio of the squared scales"""
    from scipy.stats import gennorm
    rng = np.random.default_rng(5)
    x = np.abs(gennorm.rvs(1.5, size=400000, random_state=rng))
    right = rng.random(400000) < 2.0 / 3.0                                 # mass in proportion to the scale
    p = np.where(right, 2.0 * x, -x)
    n = p.size
    l, r, rn = R.aggd_rn(n, int((p < 0).sum()), int((p > 0).sum()), np.abs(p).sum() / n, (p[p < 0] ** 2).sum() / n,
                         (p[p > 0] ** 2).sum() / n)
    alpha, _k = R.fit_rn(rn)
    assert abs(alpha - 1.5) <= 0.03 and abs(r / l - 2.0) <= 0.02
    assert R.aggd_mean(l, r, alpha) > 0 and R.aggd_mean(r, l, alpha) == -R.aggd_mean(l, r, alpha)


@pytest.mark.parametrize("depth,v", [(8, 200), (16, 65535)])
def test_an_impulse_has_the_closed_form(depth, v):
    c = ((1 << depth) - 1) / 255.0
    x = np.zeros((21, 23), np.int64)
    x[10, 11] = v
    m = R.mscn(x, depth)
    win = R.window()
    for a in range(-3, 4):
        for b in range(-3, 4):
            w = win[3 - a, 3 - b]
            centre = 1.0 if (a, b) == (0, 0) else 0.0
            want = (centre - w) * v / (v * math.sqrt(w * (1.0 - w)) + c)
            assert abs(m[10 + a, 11 + b] - want) <= 1e-12, (a, b)
    assert (m[:6] == 0).all() and (m[:, :7] == 0).all()
    assert m.max() == m[10, 11] <= M_BOUND and (depth == 8 or m.max() > 0.98 * M_BOUND)   # (C over v s costs 1.2 % at the peak)


def test_the_bound_of_m_and_the_zero_plane():
    worst = 0.0
    for (h, w), depth, layout, n in BC.GRID:
        for kind in BC.KINDS:
            for row in BC.restated(layout, h, w, depth, kind, n):
                for e in row:
                    worst = max(worst, max(float(np.abs(d["m"]).max()) for d in e["moments"]))
                    assert not np.isnan(e["features"]).any()
                    if kind == "zeros":
                        assert e["flags"] == 0x3ff and (e["features"] == 0).all()
                        wf = R.word_features(R.words(e["x"], depth), *e["x"].shape)
                        assert wf[1] == 0x3ff and (wf[0] == 0).all()
                    else:
                        assert e["flags"] == 0
    assert 1.5 < worst <= M_BOUND


def test_single_flag_bits_and_the_features_of_a_degenerate_fit():
    """rows of 0 and 255 (BC.rows): period 2 sets the bit of scale 0's H fit alone, period 1 those of H, V, D1 and D2; and the host
    formulas on hand-made words, one denominator zero at a time"""
    for period, bits in ((2, 0b00010), (1, 0b11110)):
        p = BC.rows(40, 56, period)
        ft, flags, ks = R.float_features(p, 8)
        wf, wflags, wks = R.word_features(R.words(p, 8), 40, 56)
        assert flags & 0x1f == bits == wflags & 0x1f and flags == wflags, (period, flags, wflags)
        for o in range(4):
            gone = bits >> (1 + o) & 1
            for f in (ft, wf):
                assert (f[2 + 4 * o: 6 + 4 * o] == 0).all() if gone else f[2 + 4 * o] > 0
            assert (ks[1 + o] == -1) == bool(gone) == (wks[1 + o] == -1)
        assert ft[0] > 0 and wf[0] > 0 and not np.isnan(ft).any() and not np.isnan(wf).any()
    good = dict(sum_abs_u=3 << 20, sum_u2=5 << 34, n_neg=[40] * 4, n_pos=[60] * 4, sum_abs_p=[2 << 20] * 4,
                sq_neg_lo=[7 << 28] * 4, sq_neg_hi=[1] * 4, sq_pos_lo=[9 << 28] * 4, sq_pos_hi=[2] * 4)
    assert R.word_features([good, good], 10, 10)[1] == 0
    for o, (key, bit) in enumerate((("n_neg", 1), ("n_pos", 2), ("sq_pos", 3))):
        bad = {k: (list(v) if isinstance(v, list) else v) for k, v in good.items()}
        if key == "sq_pos":
            bad["sq_pos_lo"][o], bad["sq_pos_hi"][o] = 0, 0
        else:
            bad[key][o] = 0
        ft, flags, ks = R.word_features([good, bad], 10, 10)
        assert flags == 1 << (5 + bit) and ks[5 + bit] == -1 and (ft[18 + 2 + 4 * o: 18 + 6 + 4 * o] == 0).all()
        assert (ft[:18] != 0).all() and np.count_nonzero(ft[18:]) == 14 and not np.isnan(ft).any()
    none = dict(good, sum_abs_u=0, sum_u2=0)
    ft, flags, ks = R.word_features([none, good], 10, 10)
    assert flags == 1 and ft[0] == 0 and ft[1] == 0 and (ft[2:] != 0).all()


# ---- (b) the integer restatement against the float one ---------------------------------------------------------------------
def test_the_integer_restatement_is_within_the_bars_of_the_float_one():
    assert R.BAR_ABS_M < 8e-6 and R.BAR_M2 < 4.3e-5 and R.BAR_ABS_P < 5e-5 and R.BAR_P2 < 7.6e-4
    seen = 0
    for (h, w), depth, layout, n in BC.GRID:
        for kind in BC.KINDS:
            for i, row in enumerate(BC.restated(layout, h, w, depth, kind, n)):
                for j, e in enumerate(row):
                    ph, pw = e["x"].shape
                    ws = R.words(e["x"], depth)
                    BC.close_moments(R.word_moments(ws, ph, pw), e["moments"], (h, w, layout, kind, i, j))
                    ft, flags, ks = R.word_features(ws, ph, pw)
                    assert flags == e["flags"]
                    for f in range(10):
                        if e["spans"][f] is not None and e["spans"][f] <= 2:
                            assert abs(ks[f] - e["ks"][f]) <= e["spans"][f], (h, w, layout, kind, i, j, f)
                            seen += 1
    assert seen > 1000


def test_classing_before_rounding_is_what_keeps_the_classes():
    """rounding the product first moves samples between classes; classing the exact product does not"""
    x = BC.plane("natural", 66, 98, 8, 4)
    m = R.mscn(x, 8)
    u = R.quantise(m)
    for b_m, b_u in zip(R.shifted(m), R.shifted(u)):
        exact = np.sign(u * b_u)
        agree = exact == np.sign(m * b_m)
        near = np.minimum(np.abs(m), np.abs(b_m)) <= R.BAR_ABS_M
        assert (agree | near).all()


def test_the_admission_rule():
    """a fit is admitted when moving every moment by its bar moves its float64 alpha by at most 2 grid steps.  Of the
    natural-like content exactly the fits that BC.NOT_ADMITTED names are not admitted - none of them at scale 0 - and every
    other one, 1009 of 1020, is compared end to end on the GPU"""
    missed, fits = set(), 0
    for ((h, w), depth, layout, n), gid in zip(BC.GRID, BC.IDS):
        for i, row in enumerate(BC.restated(layout, h, w, depth, "natural", n)):
            for j, e in enumerate(row):
                fits += 10
                missed |= {(gid, i, j, f) for f, s in enumerate(e["spans"]) if s is None or s > 2}
        # the clamp case: uniform noise on a plane of 2000 samples or more saturates the scale-0 GGD at the grid's end
        for row in BC.restated(layout, h, w, depth, "noise", n):
            for e in row:
                if e["x"].size >= 2000:
                    assert e["features"][0] == 10.0 and e["ks"][0] == 9800, (h, w, layout, e["x"].shape, e["features"][0])
    assert missed == BC.NOT_ADMITTED and all(f >= 5 for _g, _i, _j, f in missed)
    assert fits == 610 and len(missed) == 11


# ---- (c) the model and the range file ----------------------------------------------------------------------------------------
def test_the_model_scores_what_libsvm_would(tmp_path):
    from rtvqa_amd import brisque_model as bm
    from rtvqa_amd import vmaf_model
    rng = np.random.default_rng(7)
    text = BC.model_text(rng)
    lo, hi = rng.uniform(-2, 0, 36), rng.uniform(1, 3, 36)
    hi[4] = lo[4]                                                          # max == min: the feature maps to lower
    mp, rp = tmp_path / "m.model", tmp_path / "m.range"
    mp.write_text(text)
    rp.write_text(BC.range_text(lo, hi))
    model = bm.load_model(str(mp), str(rp))
    assert model.features == bm.FEATURE_NAMES and model.features[0] == "brisque_00" and model.features[35] == "brisque_35"
    assert model.score_clip is None
    f = rng.uniform(-2, 3, (4, 36))
    span = np.where(hi == lo, 1.0, hi - lo)
    x = np.where(hi == lo, -1.0, -1.0 + 2.0 * (f - lo) / span)
    gamma, rho, coef, sv = vmaf_model.parse_libsvm(text, 36)
    want = np.array([sum(c * math.exp(-gamma * float(((xi - s) ** 2).sum())) for c, s in zip(coef, sv)) - rho for xi in x])
    got = bm.predict(model, f)
    assert got.shape == (4,) and np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    assert abs(bm.predict(model, f[0])[0] - want[0]) <= 1e-12
    plain = bm.load_model(str(mp))                                         # no range file: the features as they are
    assert (plain.slopes == 1).all() and (plain.intercepts == 0).all()
    assert not np.allclose(bm.predict(plain, f), got)


def test_malformed_model_and_range_files_are_value_errors(tmp_path):
    from rtvqa_amd import brisque_model as bm
    rng = np.random.default_rng(8)
    good = BC.range_text(np.zeros(36), np.ones(36))
    bm.parse_range(good)
    cases = {"y\n-1 1\n": "'x'", "": "'x'", "x\n": "lower upper", "x\n-1\n": "lower upper", "x\n1 -1\n": "lower < upper",
             "x\n-1 1\n1 0\n": "index min max", "x\n-1 1\n37 0 1\n": "index 37", "x\n-1 1\n0 0 1\n": "index 0",
             "x\n-1 1\n2 0 1\n2 0 1\n": "index 2 twice", "x\n-1 1\n3 2 1\n": "index 3", "x\n-1 1\n3 a 1\n": "'3 a 1'",
             "x\n-1 nan\n": "finite"}
    for text, what in cases.items():
        with pytest.raises(ValueError) as e:
            bm.parse_range(text)
        assert what in str(e.value), (text, str(e.value))
    mp = tmp_path / "m.model"
    text = BC.model_text(rng)
    for bad, what in ((text.replace("kernel_type rbf", "kernel_type linear"), "kernel_type"),
                      (text.replace("total_sv 5", "total_sv 6"), "total_sv"),
                      (text.replace("SV\n", ""), "unsupported header line"),
                      (text + "0.5 37:1.0\n", "total_sv")):
        mp.write_text(bad)
        with pytest.raises(ValueError) as e:
            bm.load_model(str(mp))
        assert what in str(e.value), str(e.value)
    mp.write_text(text.replace("total_sv 5", "total_sv 6") + "0.5 37:1.0\n")
    with pytest.raises(ValueError) as e:
        bm.load_model(str(mp))
    assert "index 37" in str(e.value)
    with pytest.raises(ValueError):
        vp._brisque_model(None, str(mp))                                   # a range file without a model


# ---- (d) the ABI -----------------------------------------------------------------------------------------------------------------
def test_the_abi():
    from rtvqa_amd.engine import BRISQUE_DTYPE
    assert BRISQUE_DTYPE.names == FIELDS and [f[0] for f in N.VqaBrisqueMetrics._fields_] == list(FIELDS)
    assert BRISQUE_DTYPE.itemsize == C.sizeof(N.VqaBrisqueMetrics) == 60 * 8 + 8 + 36 * 8
    offs = {k: BRISQUE_DTYPE.fields[k][1] for k in FIELDS}
    assert offs == {k: getattr(N.VqaBrisqueMetrics, k).offset for k in FIELDS}
    assert (offs["sum_abs_u"], offs["sum_u2"], offs["n_neg"], offs["sq_pos_hi"], offs["flags"], offs["reserved"],
            offs["features"]) == (0, 16, 32, 416, 480, 484, 488)
    assert BRISQUE_DTYPE["n_neg"].shape == (2, 4) and BRISQUE_DTYPE["features"].shape == (36,)
    assert N.BRISQUE_MIN_DIM == 16 and N.BRISQUE_Q == R.Q == 16 and N.BRISQUE_FEATURES == 36
    assert (N.K_BRISQUE_HALF, N.K_BRISQUE_MSCN, N.K_BRISQUE_SEAM, N.K_EDGE) == (44, 45, 46, 47)
    assert (N.K_CLOSE, N.K_STOP) == (41, 43) and N.K_IDS_WHOLE == N.K_IDS_FULL + (44, 45, 46)
    for sym in ("vqa_brisque_submit", "vqa_brisque_wait"):
        assert sym in N.SIGNATURES
    lib = N.load()
    assert lib.vqa_abi_version() == 8
    lib.vqa_kernel_name.restype = C.c_char_p
    assert [lib.vqa_kernel_name(k) for k in (44, 45, 46)] == [b"k_brisque_half", b"k_brisque_mscn", b"k_brisque_seam"]
    assert lib.vqa_kernel_name(42) == b"k_artifacts"
    for unknown in (41, 43, 47):
        assert lib.vqa_kernel_name(unknown) == b"?"


# ---- (e) config, log and row ---------------------------------------------------------------------------------------------------
def test_config_keys(tmp_path):
    vp.validate_config(dict(GOOD))
    vp.validate_config(dict(GOOD, brisque=True))
    vp.validate_config(dict(GOOD, brisque=False, artifacts=True, cambi=True))
    for bad in (1, 0, "true", None, "only"):
        with pytest.raises(ValueError) as e:
            vp.validate_config(dict(GOOD, brisque=bad))
        assert str(e.value) == "brisque must be true or false."
    mp, rp = tmp_path / "m.model", tmp_path / "m.range"
    mp.write_text(BC.model_text(np.random.default_rng(1)))
    rp.write_text(BC.range_text(np.zeros(36), np.ones(36)))
    vp.validate_config(dict(GOOD, brisque_model_path=str(mp), brisque_range_path=str(rp)))
    vp.validate_config(dict(GOOD, brisque_model_path=str(mp)))
    for key in ("brisque_model_path", "brisque_range_path"):
        with pytest.raises(ValueError) as e:
            vp.validate_config(dict(dict(GOOD, brisque_model_path=str(mp)), **{key: str(tmp_path / "none")}))
        assert key in str(e.value)
    with pytest.raises(ValueError) as e:
        vp.validate_config(dict(GOOD, brisque_range_path=str(rp)))
    assert "brisque_model_path" in str(e.value)


def _records(n):
    from rtvqa_amd.engine import BRISQUE_DTYPE
    rec = np.zeros(n, BRISQUE_DTYPE)
    rec["features"] = (np.arange(36)[None, :] * 0.25 + np.arange(n)[:, None] * 2.0)
    rec["features"][:, 3] *= -1.0                                          # (an AGGD mean may be negative)
    rec["sum_u2"], rec["flags"] = 99, 0                                    # (never logged)
    return rec


def test_the_json_log_and_what_the_row_takes_from_it(tmp_path):
    from rtvqa_amd import brisque_model as bm
    from rtvqa_amd.engine import ARTIFACTS_DTYPE
    art = np.zeros(3, ARTIFACTS_DTYPE)
    art["blockiness"], art["blur"], art["noise"] = [0.25, -0.5, 1.0], [0.125, 0.5, 0.75], [4.0, 2.5, 0.0]
    vif = np.array([[0.5, 0.9, 0.95, 0.99], [0.7, 0.8, 0.97, 1.01], [0.6, 0.85, 0.96, 1.0]])
    rec = _records(3)
    mine = ["brisque_%02d" % k for k in range(36)]
    old, log, only, scored = (str(tmp_path / k) for k in ("old.json", "vmaf.json", "brisque.json", "scored.json"))
    vp.write_vif_log(old, vif, artifacts=art)
    vp.write_vif_log(log, vif, artifacts=art, brisque=rec)
    doc0, doc = json.load(open(old)), json.load(open(log))
    assert "brisque" not in json.dumps(doc0)
    names0 = list(doc0["frames"][0]["metrics"])
    assert names0[-1] == "noise"
    assert list(doc["frames"][1]["metrics"]) == names0 + mine == list(doc["pooled_metrics"])
    for i in range(3):
        m = doc["frames"][i]["metrics"]
        assert {k: m[k] for k in names0} == doc0["frames"][i]["metrics"]
        assert [m[k] for k in mine] == rec["features"][i].tolist()
    assert {k: doc["pooled_metrics"][k] for k in names0} == doc0["pooled_metrics"]
    p = doc["pooled_metrics"]["brisque_01"]
    assert sorted(p) == ["harmonic_mean", "max", "mean", "min"] and (p["min"], p["max"], p["mean"]) == (0.25, 4.25, 2.25)
    # with a model: "brisque" after brisque_35
    mp, rp = tmp_path / "m.model", tmp_path / "m.range"
    mp.write_text(BC.model_text(np.random.default_rng(3)))
    rp.write_text(BC.range_text(np.full(36, -10.0), np.full(36, 20.0)))
    model = bm.load_model(str(mp), str(rp))
    vp.write_vif_log(scored, vif, artifacts=art, brisque=rec, brisque_model=model)
    sdoc = json.load(open(scored))
    assert list(sdoc["frames"][0]["metrics"]) == names0 + mine + ["brisque"] == list(sdoc["pooled_metrics"])
    want = bm.predict(model, rec["features"])
    assert [fr["metrics"]["brisque"] for fr in sdoc["frames"]] == want.tolist() and len(set(want.tolist())) == 3
    assert {k: sdoc["pooled_metrics"][k] for k in names0 + mine} == doc["pooled_metrics"]
    vp.write_vif_log(only, brisque=rec)
    assert list(json.load(open(only))["frames"][0]["metrics"]) == mine
    pl, sl = tmp_path / "psnr.log", tmp_path / "ssim.log"
    pl.write_text("n:1 mse_avg:1.00 psnr_avg:48.13 \n")
    sl.write_text("n:1 Y:0.990000 All:0.990000 (20.000000)\n")
    args = ("x", 23, 1000, "64x64", 30.0)
    m0 = vp.extract_metrics_from_logs(str(pl), str(sl), old, *args)
    m = vp.extract_metrics_from_logs(str(pl), str(sl), log, *args)
    ms = vp.extract_metrics_from_logs(str(pl), str(sl), scored, *args)
    assert list(m0)[-1] == "NOISE" and list(m) == list(m0) + ["BRISQUE_ALPHA", "BRISQUE_SIGMA2"]          # after NOISE
    assert list(ms) == list(m) + ["BRISQUE"] and {k: ms[k] for k in m} == m and {k: m[k] for k in m0} == m0
    assert m["BRISQUE_ALPHA"] == 2.0 and m["BRISQUE_SIGMA2"] == 2.25 and ms["BRISQUE"] == float(want.mean())
    base = ["Bitrate (kbps)", "Resolution (px)", "Frame Rate (fps)", "CRF", "PSNR", "SSIM"]
    assert list(vp.extract_metrics_from_logs(str(pl), str(sl), only, *args)) == base + ["BRISQUE_ALPHA", "BRISQUE_SIGMA2"]
    # logs without the key are what they were, byte for byte
    again = str(tmp_path / "again.json")
    vp.write_vif_log(again, vif, artifacts=art, brisque=None, brisque_model=None)
    assert open(again, "rb").read() == open(old, "rb").read()
    # the pass's tuple -> the log: the last element is the BRISQUE records [n, p], the artefact measures' the one before it
    from rtvqa_amd.engine import VIF_DTYPE
    v = np.zeros((3, 1), VIF_DTYPE)
    v["scale"][:, 0, :] = vif
    q = (None, None, v, art[:, None], rec[:, None])
    vp._write_feature_log(again, q, dict(vif=True, adm=False, artifacts=True, brisque=True))
    assert open(again, "rb").read() == open(log, "rb").read()
    vp._write_feature_log(again, q, dict(vif=True, adm=False, artifacts=True, brisque=True), brisque_model=model)
    assert open(again, "rb").read() == open(scored, "rb").read()
    vp._write_feature_log(again, q[:-1], dict(vif=True, adm=False, artifacts=True))
    assert open(again, "rb").read() == open(old, "rb").read()
    vp._write_feature_log(again, (None, None, rec[:, None]), dict(vif=False, adm=False, brisque=True))
    assert open(again, "rb").read() == open(only, "rb").read()


def test_a_vmaf_model_does_not_read_the_new_keys():
    from rtvqa_amd import vmaf_model

    class Model:
        features = ["vif_scale0", "adm2", "motion2"]

    x = vmaf_model.feature_matrix(Model, {"vif_scale0": [0.5, 0.7], "adm2": [0.9, 0.95], "motion2": [0.0, 1.0],
                                          "brisque_00": [2.0, 2.1], "brisque": [30.0, 40.0]})
    assert x.shape == (2, 3)


def test_the_stream_request():
    p = [(32, 32, 0, 32, 1), (32, 32, 1024, 32, 1), (32, 32, 2048, 32, 1)]
    every = dict(vif=True, adm=True, motion=True, siti=True, psnr_hvs=True, ciede=True, gmsd=True, cambi=True, xpsnr=True,
                 haarpsi=True, vca=True, artifacts=True)
    assert stream.Quality(p).brisque is False and stream.Quality(p, **every).brisque is False
    assert stream.Quality(p, brisque=True).brisque is True and stream.Quality(p, brisque="only").brisque == "only"
    assert stream.Quality(p, brisque=True).ssim is True and stream.Quality(p, brisque="only").ssim is False
    assert stream.Quality(p, brisque=True).artifacts is False
    for bad in (1, "yes", None):
        with pytest.raises(ValueError):
            stream.Quality(p, brisque=bad)
    with pytest.raises(ValueError):
        stream.Quality(p, N.SSIM_MS, scales=True, brisque="only")
    z = np.zeros((0, 3072), np.uint8)
    # an empty clip: without the request the tuples are what they were; with it ONE further last element, after the artefacts'
    for kw, length in ((dict(), 2), (dict(vif=True), 3), (dict(artifacts=True), 3), (dict(cambi=True, artifacts=True), 4),
                       (every, 14)):
        q0, _ = stream.run(z, z, quality=stream.Quality(p, **kw))
        q1, _ = stream.run(z, z, quality=stream.Quality(p, brisque=True, **kw))
        assert len(q0) == length and len(q1) == length + 1, kw
        assert q1[-1].shape == (0, 3) and q1[-1].dtype.names == FIELDS
        for a, b in zip(q0, q1):
            assert (a is None and b is None) or (a.dtype == b.dtype and a.shape == b.shape)
    q, _ = stream.run(z, z, quality=stream.Quality(p, brisque="only"))
    assert len(q) == 3 and q[0] is None and q[1] is None and q[2].shape == (0, 3)
