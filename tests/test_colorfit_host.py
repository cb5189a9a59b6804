"""Colour registration on the host side (no GPU): rtvqa_amd/colorfit.py - exact rational fits off the integer moments - run on
records made by the NumPy restatement of tests/colorfit_reference.py.

Figures quoted in the docstrings were measured here on the CPU in float64; the tests assert names, exact identities and the
rule's own threshold 10 log10(2), never those figures."""
import math
from fractions import Fraction

import numpy as np
import pytest

import colorfit_reference as CR

HALF = 10.0 * math.log10(2.0)


def _planes(h, w, layout="420"):
    cw, ch = ((w + 1) // 2, (h + 1) // 2) if layout == "420" else (w, h)
    if layout == "gray":
        return [(w, h, 0, w, 1)]
    return [(w, h, 0, w, 1), (cw, ch, w * h, cw, 1), (cw, ch, w * h + cw * ch, cw, 1)]


def _planes16(planes, depth):
    return [(p[0], p[1], 2 * p[2], 2 * p[3], 2, depth) for p in planes]


def _records(ref, dist, planes):
    return CR.records(ref, dist, planes)


def _apply(entry, clip, planes, peak=255):
    """a catalogue map d = b + M r on a planar clip, plane by plane at the plane's own size (the luma row reads the chroma
    replicated to its grid; the chroma rows of every catalogue map read no luma), as float64 before any rounding"""
    _name, M, b = entry
    M = np.array([[float(v) for v in row] for row in M])
    b = np.array([float(v) for v in b])
    bps = clip.dtype.itemsize
    w, h = planes[0][0], planes[0][1]
    out = np.zeros(clip.shape, np.float64)
    for f in range(len(clip)):
        g = [CR.grid(clip[f], p, h, w).astype(np.float64) for p in planes]
        for k, (pw, ph, off, _rs, _st, *_d) in enumerate(planes):
            assert k == 0 or len(planes) == 1 or M[k][0] == 0.0
            full = b[k] + sum(M[k][i] * g[i] for i in range(len(planes)))
            out[f, off // bps: off // bps + pw * ph] = full[::(h + ph - 1) // ph, ::(w + pw - 1) // pw][:ph, :pw].ravel()
    return out


def _finish(x, peak, dtype):
    return np.clip(np.rint(x), 0, peak).astype(dtype)


@pytest.fixture(scope="module")
def natural():
    from rtvqa_amd import frames, synth
    h, w = 72, 104
    bgr = synth.s_natural(3, h, w)
    return frames.bgr_to_yuv420p(bgr), frames.bgr_to_yuv420p(synth.distort(bgr)), _planes(h, w)


def test_a_two_by_two_example_by_hand():
    """r = 0, 1, 2, 3 and d = 1, 3, 5, 8: n = 4, sum_r = 6, sum_d = 17, rr = 14, rd = 37, dd = 99, sse = 39; var = 20, cov = 46"""
    from rtvqa_amd import colorfit as CF
    planes = [(2, 2, 0, 2, 1)]
    rec = CR.record(np.array([0, 1, 2, 3], np.uint8), np.array([1, 3, 5, 8], np.uint8), planes)
    assert (rec["count"], rec["sum_r"][0], rec["sum_d"][0], rec["rr"][0], rec["rd"][0], rec["dd"][0], rec["sse"][0]) == \
        (4, 6, 17, 14, 37, 99, 39)
    out = CF.analyse([rec], 8, "gray")
    assert out["sse_given"] == [39]
    assert out["gain"] == [Fraction(23, 10)] and out["offset"] == [Fraction(4, 5)] and out["sse_affine"] == [Fraction(3, 10)]
    assert out["matrix"] == [[Fraction(23, 10)]] and out["matrix_offset"] == [Fraction(4, 5)]      # one plane: the levels fit
    assert out["sse_matrix"] == [Fraction(3, 10)]
    assert out["psnr_gain"] == 10.0 * math.log10(130)   # 39 / (3 / 10)
    assert out["match"] == "none" and out["match_psnr_gain"] == 0.0
    assert CF.sse_of(CF.moments(rec), 0, Fraction(4, 5), [Fraction(23, 10)]) == Fraction(3, 10)
    tab = CR.tables(np.array([[0, 1, 2, 3]], np.uint8), np.array([[1, 3, 5, 8]], np.uint8), planes, 8)
    full = CF.analyse([rec], 8, "gray", tab.tolist())
    assert full["sse_lut"] == [0] and full["curve"][0][:4] == [1.0, 3.0, 5.0, 8.0] and math.isnan(full["curve"][0][4])
    assert full["tone_psnr_gain"] == [math.inf] and full["lut_psnr_gain"] == [math.inf]
    assert CF.db(0, 0) == 0.0 and CF.db(0, 5) == 0.0 and CF.db(5, 0) == math.inf and CF.db(20, 2) == 10.0


def test_the_quadratic_form_is_the_direct_sum():
    from rtvqa_amd import colorfit as CF
    h, w = 6, 8
    planes = _planes(h, w, "444")
    rng = np.random.default_rng(11)
    ref, dist = rng.integers(0, 256, (1, 3 * h * w)).astype(np.uint8), rng.integers(0, 256, (1, 3 * h * w)).astype(np.uint8)
    m = CF.moments(_records(ref, dist, planes)[0])
    M = [[Fraction(int(rng.integers(-40, 41)), 17) for _ in range(3)] for _ in range(3)]
    b = [Fraction(int(rng.integers(-300, 301)), 7) for _ in range(3)]
    r = [[int(v) for v in CR.grid(ref[0], p, h, w).ravel()] for p in planes]
    d = [[int(v) for v in CR.grid(dist[0], p, h, w).ravel()] for p in planes]
    for k in range(3):
        direct = sum((d[k][j] - (b[k] + sum(M[k][i] * r[i][j] for i in range(3)))) ** 2 for j in range(h * w))
        assert CF.sse_of(m, k, b[k], M[k]) == direct, k
        assert CF.sse_of(m, k, 0, [int(i == k) for i in range(3)]) == m["sse"][k]       # the identity map: the error as given


def _clips(natural):
    """(tag, ref, dist, planes, depth, model) over layouts, depths and kinds of damage"""
    ref, dist, planes = natural
    rng = np.random.default_rng(2)
    out = [("natural", ref, dist, planes, 8, "yuv")]
    h, w = 18, 22
    for layout, model in (("420", "yuv"), ("444", "yuv"), ("444", "bgr"), ("gray", "gray")):
        pl = _planes(h, w, layout)
        total = max(p[2] + p[0] * p[1] for p in pl)
        a = rng.integers(0, 256, (2, total)).astype(np.uint8)
        b = np.clip(0.8 * a + 20 + rng.normal(0, 3, a.shape), 0, 255).astype(np.uint8)
        out.append(("noise-" + layout + model, a, b, pl, 8, model))
        a10 = (a.astype(np.uint16) * 4 + rng.integers(0, 4, a.shape)).astype(np.uint16)
        b10 = np.clip(1.1 * a10 - 30 + rng.normal(0, 9, a.shape), 0, 1023).astype(np.uint16)
        out.append(("noise10-" + layout + model, a10, b10, _planes16(pl, 10), 10, model))
    return out


def test_the_fits_are_ordered_exactly(natural):
    """sse_matrix <= sse_affine <= sse_given per plane; sse_lut <= sse_affine wherever bins are codes (depth <= 10)"""
    from rtvqa_amd import colorfit as CF
    for tag, ref, dist, planes, depth, model in _clips(natural):
        out = CF.analyse(_records(ref, dist, planes), depth, model, CR.tables(ref, dist, planes, depth).tolist())
        for p in range(out["planes"]):
            assert 0 <= out["sse_matrix"][p] <= out["sse_affine"][p] <= out["sse_given"][p], (tag, p)
            assert 0 <= out["sse_lut"][p] <= out["sse_affine"][p], (tag, p)
            assert out["tone_psnr_gain"][p] >= 0.0 and out["lut_psnr_gain"][p] >= out["tone_psnr_gain"][p], (tag, p)
            m = CF.moments(_records(ref, dist, planes)[0])
            for f in _records(ref, dist, planes)[1:]:
                m = CF.add(m, CF.moments(f))
            # the reported fits leave what the quadratic form says they leave
            assert CF.sse_of(m, p, out["offset"][p], [out["gain"][p] if i == p else 0 for i in range(3)]) == out["sse_affine"][p]
            assert CF.sse_of(m, p, out["matrix_offset"][p], out["matrix"][p]) == out["sse_matrix"][p], (tag, p)
        assert out["psnr_gain"] >= 0.0 and out["count"] == len(ref) * planes[0][0] * planes[0][1]


def test_flat_planes_and_identical_streams_raise_nothing():
    from rtvqa_amd import colorfit as CF
    h, w = 16, 20
    planes = _planes(h, w)
    rng = np.random.default_rng(4)
    luma = rng.integers(16, 236, (2, h * w)).astype(np.uint8)
    flat_chroma = np.concatenate([luma, np.full((2, 2 * (h // 2) * (w // 2)), 128, np.uint8)], axis=1)
    flat_all = np.full_like(flat_chroma, 77)
    noise = rng.integers(0, 256, flat_chroma.shape).astype(np.uint8)
    for tag, clip in (("flat chroma", flat_chroma), ("flat everything", flat_all), ("identical", noise)):
        out = CF.analyse(_records(clip, clip, planes), 8, "yuv", CR.tables(clip, clip, planes, 8).tolist())
        assert out["match"] == "none" and out["per_frame"] == ["none", "none"] and out["frames_off"] == 0, tag
        assert out["psnr_gain"] == 0.0 and out["match_psnr_gain"] == 0.0, tag
        assert out["tone_psnr_gain"] == [0.0] * 3 and out["lut_psnr_gain"] == [0.0] * 3, tag
        assert out["sse_given"] == [0, 0, 0] and out["sse_matrix"] == [0, 0, 0] and out["sse_affine"] == [0, 0, 0], tag
        keys = CF.log_keys(out, 8)
        assert tuple(keys) == CF.COLORFIT_KEYS and keys["COLORFIT_MATCH"] == "none" and keys["COLORFIT_PSNR_GAIN"] == 0.0
    out = CF.analyse(_records(flat_all, flat_all, planes), 8, "yuv")
    assert out["gain"] == [1, 1, 1] and out["offset"] == [0, 0, 0] and out["matrix"] == [[0] * 3] * 3      # every plane dropped
    # flat chroma under a damaged luma: the chroma planes are dropped (coefficient 0 in all three fits), the luma is fitted
    hurt = flat_chroma.copy()
    hurt[:, :h * w] = np.clip(0.5 * luma + 40, 0, 255).astype(np.uint8)
    out = CF.analyse(_records(flat_chroma, hurt, planes), 8, "yuv")
    assert all(out["matrix"][k][i] == 0 for k in range(3) for i in (1, 2)) and out["matrix"][0][0] == out["gain"][0]
    assert out["sse_matrix"] == out["sse_affine"] and out["offset"][1:] == [0, 0] and out["gain"][1:] == [1, 1]
    # an exact linear dependence between reference planes (V = 2 U - 3 on 4:4:4): the third pivot is zero, nothing raises
    pl = _planes(h, w, "444")
    y, u = rng.integers(0, 256, (2, 1, h * w))
    u = u // 3 + 10
    ref = np.concatenate([y, u, 2 * u - 3], axis=1).astype(np.uint8)
    dist = np.clip(ref.astype(np.int64) + rng.integers(-2, 3, ref.shape), 0, 255).astype(np.uint8)
    out = CF.analyse(_records(ref, dist, pl), 8, "yuv")
    assert all(out["matrix"][k][2] == 0 for k in range(3)) and all(0 <= a <= b for a, b in zip(out["sse_matrix"], out["sse_affine"]))
    with pytest.raises(ValueError):
        CF.analyse([], 8, "yuv")
    with pytest.raises(ValueError):
        CF.analyse(_records(ref, dist, pl), 8, "rgb")


def test_the_catalogue_decimals_and_inverses():
    from rtvqa_amd import colorfit as CF
    a, b = CF.ypbpr_matrix("bt601", "bt709"), CF.ypbpr_matrix("bt709", "bt601")
    assert [[round(float(v), 4) + 0.0 for v in row] for row in a] == [[1, -0.1182, -0.2127], [0, 1.0186, 0.1146], [0, 0.0750, 1.0253]]
    assert [[round(float(v), 4) + 0.0 for v in row] for row in b] == [[1, 0.1016, 0.1961], [0, 0.9899, -0.1107], [0, -0.0725, 0.9834]]
    eye = [[Fraction(int(i == j)) for j in range(3)] for i in range(3)]

    def mul(p, q):
        return [[sum(p[i][j] * q[j][k] for j in range(len(q))) for k in range(len(q))] for i in range(len(p))]

    assert mul(a, b) == eye and mul(b, a) == eye
    for depth in (8, 10, 12, 16):
        cat = CF.catalogue(depth, "yuv")
        assert [c[0] for c in cat] == ["limited_to_full", "full_to_limited", "bt601_to_bt709", "bt709_to_bt601"]
        s, P = 1 << (depth - 8), (1 << depth) - 1
        for fwd, rev in ((cat[0], cat[1]), (cat[2], cat[3])):     # each is the other's inverse as an affine map
            assert mul(fwd[1], rev[1]) == eye
            assert [fwd[2][i] + sum(fwd[1][i][j] * rev[2][j] for j in range(3)) for i in range(3)] == [0, 0, 0]
        l2f = cat[0]
        assert l2f[2][0] + l2f[1][0][0] * 16 * s == 0 and l2f[2][0] + l2f[1][0][0] * 235 * s == P       # black and white
        assert l2f[2][1] + l2f[1][1][1] * 128 * s == 128 * s                                              # neutral chroma stays
        assert [c[0] for c in CF.catalogue(depth, "bgr")] == ["limited_to_full", "full_to_limited"]
        g = CF.catalogue(depth, "gray")
        assert len(g) == 2 and g[0][1] == [[Fraction(P, 219 * s)]] and g[1][2] == [16 * s]
        assert CF.catalogue(depth, "bgr")[0][1][2][2] == Fraction(P, 219 * s)                             # the luma constants on every plane
        m = cat[2]
        centre = [16 * s, 128 * s, 128 * s]
        assert [m[2][i] + sum(m[1][i][j] * centre[j] for j in range(3)) for i in range(3)] == centre      # about the centre


def _damaged(natural, depth, sigma, seed=5):
    """the clip with each mishap applied, rounded and clipped -> [(name, ref, dist, planes)], then the pairs that carry none"""
    from rtvqa_amd import colorfit as CF
    ref8, dist8, planes = natural
    rng = np.random.default_rng(seed)
    if depth == 8:
        ref, syn, pl, dt = ref8, dist8, planes, np.uint8
    else:   # ref * 4 plus two random low bits
        ref = (ref8.astype(np.uint16) * 4 + rng.integers(0, 4, ref8.shape)).astype(np.uint16)
        syn = np.clip(ref.astype(np.int64) + 4 * (dist8.astype(np.int64) - ref8), 0, 1023).astype(np.uint16)
        pl, dt = _planes16(planes, 10), np.uint16
    peak = (1 << depth) - 1
    out = []
    for entry in CF.catalogue(depth, "yuv"):
        out.append((entry[0], ref, _finish(_apply(entry, ref, pl) + (rng.normal(0, sigma, ref.shape) if sigma else 0), peak, dt), pl))
    out.append(("none", ref, ref.copy(), pl))
    out.append(("none", ref, _finish(ref + rng.normal(0, max(sigma, 1), ref.shape), peak, dt), pl))
    out.append(("none", ref, syn, pl))
    return out


@pytest.mark.parametrize("depth,sigma", [(8, 0), (8, 1), (10, 4)])
def test_the_catalogue_names_each_mishap_on_the_natural_clip(natural, depth, sigma):
    """Measured: clean 8-bit 22.9, 21.2, 16.8, 16.4 dB; with sigma 1 noise 11.9, 10.7, 6.5, 6.0 dB; at 10 bits with sigma 4
    12.6, 11.4, 6.6, 6.2 dB - against the rule's 3.01 dB.  The untouched pair, the noisy pair and synth.distort give "none"."""
    from rtvqa_amd import colorfit as CF
    for name, ref, dist, planes in _damaged(natural, depth, sigma):
        out = CF.analyse(_records(ref, dist, planes), depth, "yuv")
        print(depth, sigma, name, out["match"], round(out["match_psnr_gain"], 2), round(out["psnr_gain"], 2))
        assert out["match"] == name, (name, out["match"])
        assert out["frames_off"] == 0 and out["per_frame"] == [name] * 3
        if name != "none":
            assert out["match_psnr_gain"] > HALF and out["psnr_gain"] >= out["match_psnr_gain"]
            assert 2 * out["match_sse"] <= sum(out["sse_given"])
        else:
            assert out["match_psnr_gain"] == 0.0 and out["match_sse"] is None


def test_a_range_mix_up_costs_more_than_20_db(natural):
    """what the feature is for: the untouched clip against its limited-to-full copy, as PSNR of the luma plane"""
    from rtvqa_amd import colorfit as CF
    ref, _dist, planes = natural
    hurt = _finish(_apply(CF.catalogue(8, "yuv")[0], ref, planes), 255, np.uint8)
    out = CF.analyse(_records(ref, hurt, planes), 8, "yuv")
    assert out["match"] == "limited_to_full" and out["psnr_gain"] > 20.0
    assert abs(float(out["gain"][0]) - 255.0 / 219.0) < 0.02


def test_a_gamma_mismatch_shows_in_the_tone_gain(natural):
    """d_Y = rint(255 (r_Y / 255)^(1 / 1.2)): a per-code curve explains all of it, gain and offset do not.  Measured: given
    4 967 073, affine 20 308, gain 0.949, offset 21.3"""
    from rtvqa_amd import colorfit as CF
    ref, _dist, planes = natural
    n_y = planes[0][0] * planes[0][1]
    hurt = ref.copy()
    hurt[:, :n_y] = np.rint(255.0 * (ref[:, :n_y] / 255.0) ** (1.0 / 1.2)).astype(np.uint8)
    out = CF.analyse(_records(ref, hurt, planes), 8, "yuv", CR.tables(ref, hurt, planes, 8).tolist())
    print(out["sse_given"][0], float(out["sse_affine"][0]), float(out["gain"][0]), float(out["offset"][0]))
    assert out["sse_lut"][0] == 0 and out["sse_affine"][0] > 0 and out["tone_psnr_gain"][0] == math.inf
    assert out["tone_psnr_gain"][1:] == [0.0, 0.0] and out["match"] == "none"
    keys = CF.log_keys(out, 8)
    assert keys["COLORFIT_TONE_PSNR_GAIN"] == 100.0 and keys["COLORFIT_OFFSET_Y"] == float(out["offset"][0])
    # a pure levels error does NOT show there: gain and offset explain what the curve explains, up to the rounding
    lev = ref.copy()
    lev[:, :n_y] = np.rint(0.8 * ref[:, :n_y] + 20).astype(np.uint8)
    out = CF.analyse(_records(ref, lev, planes), 8, "yuv", CR.tables(ref, lev, planes, 8).tolist())
    assert out["sse_lut"][0] == 0 and out["lut_psnr_gain"][0] == math.inf
    assert float(out["sse_affine"][0]) / (3 * n_y) < 1.0 / 12.0 + 0.01           # the rounding's own variance, no more


def test_frames_off_counts_the_frames_that_differ(natural):
    from rtvqa_amd import colorfit as CF
    ref, _dist, planes = natural
    hurt = ref.copy()
    hurt[1] = _finish(_apply(CF.catalogue(8, "yuv")[0], ref[1:2], planes), 255, np.uint8)[0]
    out = CF.analyse(_records(ref, hurt, planes), 8, "yuv")
    assert out["per_frame"] == ["none", "limited_to_full", "none"]
    assert out["match"] == "none" and out["frames_off"] == 1
    ten = CF.log_keys(CF.analyse(_records(ref, hurt, planes), 8, "yuv"), 10)
    assert ten["COLORFIT_OFFSET_Y"] * 4 == CF.log_keys(out, 8)["COLORFIT_OFFSET_Y"] and ten["COLORFIT_FRAMES_OFF"] == 1


def test_the_config_key_and_the_requests():
    from rtvqa_amd import video_processing as vp
    base = {"crf": 23, "resize_width": 64, "resize_height": 64}
    vp.validate_config(dict(base, colorfit=True))
    vp.validate_config(dict(base, colorfit=False, scale="bicubic", dist_height=36, dist_width=52))
    with pytest.raises(ValueError, match="colorfit must be true or false"):
        vp.validate_config(dict(base, colorfit=1))
    with pytest.raises(ValueError, match="colorfit and scale"):
        vp.validate_config(dict(base, colorfit=True, scale="bicubic", dist_height=36, dist_width=52))
    assert vp.colorfit_model("bgr24") == "bgr" and vp.colorfit_model("gray") == "gray" and vp.colorfit_model("yuv420p10le") == "yuv"
