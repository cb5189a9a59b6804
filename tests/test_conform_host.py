"""CPU: conform.plan's geometry, time and colour maps (pure Python), the NumPy restatement of vqa_conform_submit
(tests/conform_reference.py) and what is refused before a GPU is asked."""
from fractions import Fraction

import numpy as np
import pytest

import conform_reference as R
from rtvqa_amd import colorfit as CF
from rtvqa_amd import conform as CO
from rtvqa_amd import video_processing as vp
from rtvqa_amd.engine import bgr_planes, check_conform_args, mono_planes, yuv_planes

LAYOUTS = {"420": lambda h, w: yuv_planes(h, w, "420"), "422": lambda h, w: yuv_planes(h, w, "422"),
           "444": lambda h, w: yuv_planes(h, w, "444"), "mono": mono_planes, "bgr24": bgr_planes}
SUB = {"420": (1, 1), "422": (0, 1), "444": (0, 0), "mono": (0, 0), "bgr24": (0, 0)}
MODEL = {"420": "yuv", "422": "yuv", "444": "yuv", "mono": "gray", "bgr24": "bgr"}
SHIFTS = [(dy, dx) for dy in range(-3, 4) for dx in range(-3, 4)]


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("size", ((33, 47), (100, 101), (32, 48), (35, 64)))
def test_geometry_for_every_shift(layout, size):
    h, w = size
    fn, (sy, sx) = LAYOUTS[layout], SUB[layout]
    full = fn(h, w)
    for dy, dx in SHIFTS:
        g = CO.geometry(fn, h, w, (dy, dx))
        oh, ow = g["out_h"], g["out_w"]
        # the luma window: h - |dy| by w - |dx| rounded DOWN to the subsampling, where the definition puts it
        assert oh == (h - abs(dy)) >> sy << sy and ow == (w - abs(dx)) >> sx << sx
        assert g["dist_origin"][0] == (max(0, -dy), max(0, -dx)) and g["ref_origin"][0] == (max(0, dy), max(0, dx))
        out = fn(oh, ow)
        for p, (src, dst) in enumerate(zip(full, out)):
            for side in ("ref_origin", "dist_origin"):   # both streams' windows: equal in size, inside their planes
                y0, x0 = g[side][p]
                assert 0 <= y0 and y0 + dst[1] <= src[1] and 0 <= x0 and x0 + dst[0] <= src[0], (p, side, dy, dx)
            if p:   # a chroma window is origin >> s and size >> s
                assert (dst[1], dst[0]) == (oh >> sy, ow >> sx)
                assert g["dist_origin"][p] == (max(0, -dy) >> sy, max(0, -dx) >> sx)
                assert g["ref_origin"][p] == (max(0, dy) >> sy, max(0, dx) >> sx)
        # half a chroma sample stays exactly where an odd shift meets a subsampled axis
        assert g["chroma_half"] == int((sy and dy % 2 == 1) or (sx and dx % 2 == 1))
        # the luma windows show the same picture: reference (y + dy, x + dx) under distorted (y, x)
        ry, rx = g["ref_origin"][0]
        qy, qx = g["dist_origin"][0]
        assert (ry - qy, rx - qx) == (dy, dx)


def test_a_shift_that_leaves_nothing_is_refused():
    with pytest.raises(ValueError):
        CO.geometry(mono_planes, 16, 16, (16, 0))
    with pytest.raises(ValueError):
        CO.geometry(LAYOUTS["420"], 16, 17, (0, -16))


def test_time_by_offset_and_by_path():
    for n_ref, n_dist, k in ((12, 12, 0), (12, 12, 2), (12, 12, -3), (10, 14, 1), (14, 10, -2), (5, 9, 4)):
        ref, dist = CO.timing(n_ref, n_dist, k)
        assert len(ref) == len(dist) and all(r - d == k for r, d in zip(ref, dist))
        assert ref == sorted(ref) and 0 <= ref[0] and ref[-1] < n_ref and 0 <= dist[0] and dist[-1] < n_dist
        # sync's trim, exactly
        from rtvqa_amd import sync as S
        assert (ref[0], dist[0], len(ref)) == (max(0, k), max(0, -k), S.overlap(k, n_dist, n_ref))
    # a path: a drop, a repeat, a partner that does not exist at either end
    ref, dist = CO.timing(6, 7, ref_index=[-1, 0, 1, 1, 3, 5, 6])
    assert dist == [1, 2, 3, 4, 5] and ref == [0, 1, 1, 3, 5]
    with pytest.raises(ValueError):
        CO.timing(4, 4, 4)                      # no pair
    with pytest.raises(ValueError):
        CO.timing(4, 4, ref_index=[0, 1, 2])    # a path for another clip
    plan = CO.plan(mono_planes, 32, 32, 8, "gray", offset=2, n_ref=12)
    assert plan["ref"]["index"] == list(range(2, 12)) and plan["dist"]["index"] == list(range(10))
    assert plan["summary"]["CONFORM_FRAMES"] == 10 and plan["summary"]["CONFORM_OFFSET"] == 2
    assert CO.plan(mono_planes, 32, 32, 8, "gray", n_ref=12)["summary"]["identity"]
    assert not CO.plan(mono_planes, 32, 32, 8, "gray", shift=(0, 1), n_ref=12)["summary"]["identity"]
    assert list(CO.log_keys(plan["summary"])) == list(CO.CONFORM_KEYS)


def _frames(layout, h, w, depth, n=3, seed=0):
    rng = np.random.default_rng(seed)
    fn = LAYOUTS[layout] if depth == 8 else (lambda h, w: yuv_planes(h, w, layout, depth))
    return [[rng.integers(0, 1 << depth, (p[1], p[0])).astype(np.uint16 if depth > 8 else np.uint8) for p in fn(h, w)]
            for _ in range(n)], fn


@pytest.mark.parametrize("layout,depth", (("420", 8), ("422", 10), ("444", 16), ("mono", 12), ("bgr24", 8)))
def test_the_restatement_with_identity_arguments_is_a_copy(layout, depth):
    frames, fn = _frames(layout, 33, 47, depth)
    sizes = [(p[1], p[0]) for p in fn(33, 47)]
    ident_lut = np.tile(np.arange(1 << depth), (len(sizes), 1))
    ident_m = np.array([[65536, 0, 0, 0], [0, 65536, 0, 0], [0, 0, 65536, 0]], np.int64)
    for kw in ({}, {"origin": [(0, 0)] * len(sizes)}, {"index": [0, 1, 2]}, {"lut": ident_lut},
               {"matrix": ident_m} if len(sizes) == 3 else {}):
        out = R.conform(frames, sizes, depth=depth, **kw)
        assert len(out) == 3
        for a, b in zip(frames, out):
            for x, y in zip(a, b):
                assert x.dtype == y.dtype and (x == y).all()


def test_the_restatement_by_hand():
    """4:2:0, 3 x 4 luma: cells of four, two, two and one luma samples; a matrix that passes Ybar to plane 1"""
    y = np.array([[10, 20, 30, 41], [50, 60, 70, 80], [91, 100, 110, 121]], np.uint8)
    u = np.array([[1, 2], [3, 4]], np.uint8)
    v = np.array([[5, 6], [7, 8]], np.uint8)
    m = np.array([[65536, 65536, 0, 0], [65536, 0, 0, 0], [0, 0, 2 * 65536, -3 * 65536]], np.int64)
    (t0, t1, t2), = R.conform([[y, u, v]], [(3, 4), (2, 2), (2, 2)], matrix=m)
    assert (t0 == y + np.array([[1, 1, 2, 2], [1, 1, 2, 2], [3, 3, 4, 4]])).all()           # chroma replicated
    assert (t1 == [[35, 55], [96, 116]]).all()     # (10+20+50+60+2)//4, (30+41+70+80+2)//4, (91+100+1)//2, (110+121+1)//2
    assert (t2 == [[7, 9], [11, 13]]).all()
    # the window, the gather and the table
    lut = np.tile(np.arange(256)[::-1], (3, 1))
    out = R.conform([[y, u, v], [y + 1, u, v]], [(2, 2), (1, 1), (1, 1)], origin=[(1, 2), (0, 1), (1, 0)], index=[1, 1, 0], lut=lut)
    assert len(out) == 3 and (out[0][0] == 255 - (y + 1)[1:3, 2:4]).all() and out[2][1][0, 0] == 255 - 2 and out[2][2][0, 0] == 255 - 7
    # clips at both ends
    big = np.array([[3 * 65536, 0, 0, 0], [0, -65536, 0, 0], [0, 0, 65536, 0]], np.int64)
    (c0, c1, _), = R.conform([[y, u, v]], [(3, 4), (2, 2), (2, 2)], matrix=big)
    assert c0.max() == 255 and (c1 == 0).all()


@pytest.mark.parametrize("depth", (8, 10, 12))
@pytest.mark.parametrize("model", CF.MODELS)
def test_range_mishap_and_its_correction_return_every_in_range_code(depth, model):
    """limited_to_full (rounded and clipped), then conform's full_to_limited correction: every code of the limited range comes
    back within one unit, on every plane"""
    s, peak = 1 << (depth - 8), (1 << depth) - 1
    cat = {n: (M, b) for n, M, b in CF.catalogue(depth, model)}
    M, b = cat["limited_to_full"]
    label, lut, matrix = CO.color_map(("match", "limited_to_full"), depth, model)
    assert label == "match:limited_to_full" and matrix is None and len(lut) == CF._planes_of(model)
    for p in range(len(lut)):
        chroma = model == "yuv" and p > 0
        lo, hi = 16 * s, (240 if chroma else 235) * s
        for c in range(lo, hi + 1):
            d = min(max(int((M[p][p] * c + b[p]) * 2 + 1) // 2, 0), peak)   # the mishap, rounded half up and clipped
            assert abs(lut[p][d] - c) <= 1, (p, c, d, lut[p][d])
    # and the other way round: full_to_limited, then the limited_to_full correction
    M, b = cat["full_to_limited"]
    _, lut, _ = CO.color_map(("match", "full_to_limited"), depth, model)
    worst = max(abs(lut[0][min(max(int((M[0][0] * c + b[0]) * 2 + 1) // 2, 0), peak)] - c) for c in range(peak + 1))
    assert worst <= 1


def test_the_matrix_mishaps_invert_and_other_models_have_none():
    label, lut, m = CO.color_map(("match", "bt601_to_bt709"), 8, "yuv")
    assert label == "match:bt601_to_bt709" and lut is None and len(m) == 3 and all(len(r) == 4 for r in m)
    cat = {n: (M, b) for n, M, b in CF.catalogue(8, "yuv")}
    want = CO.fixed_matrix(*cat["bt709_to_bt601"])
    assert m == want
    # forward then the correction: a mid-grey and a saturated code come back within a unit (rounding twice)
    M, b = cat["bt601_to_bt709"]
    for code in ((128, 128, 128), (81, 90, 240), (145, 54, 34), (41, 240, 110)):
        d = [int((sum(M[k][i] * code[i] for i in range(3)) + b[k]) * 2 + 1) // 2 for k in range(3)]
        back = [(sum(m[k][i] * d[i] for i in range(3)) + m[k][3] + 32768) >> 16 for k in range(3)]
        assert all(abs(x - y) <= 1 for x, y in zip(back, code)), (code, d, back)
    for model in ("bgr", "gray"):
        with pytest.raises(ValueError):
            CO.color_map(("match", "bt601_to_bt709"), 8, model)
    assert CO.color_map(("match", "none"), 8, "yuv") == ("none", None, None)
    assert CO.color_map(None, 10, "gray") == ("none", None, None)


def test_integer_matrix_rounding_against_fractions():
    vals = [Fraction(1, 3), Fraction(-1, 3), Fraction(1, 2 ** 17), Fraction(-1, 2 ** 17), Fraction(3, 2 ** 17), Fraction(-3, 2 ** 17),
            Fraction(219, 255), Fraction(-7, 9), 0, 1, -1, Fraction(5, 7) * 100]
    for v in vals:
        q = CO.fix16(v)
        # floor(v 2^16 + 1/2): the nearest integer, a tie going UP
        assert Fraction(q) - Fraction(1, 2) <= Fraction(v) * 65536 < Fraction(q) + Fraction(1, 2), v
    assert CO.fix16(Fraction(1, 2 ** 17)) == 1 and CO.fix16(Fraction(-1, 2 ** 17)) == 0
    rows = CO.fixed_matrix([[Fraction(1, 3), 0], [0, Fraction(219, 255)]], [Fraction(-1, 2), 16])
    assert rows == [[21845, 0, -32768], [0, 56284, 16 * 65536]]      # 21845.33 -> 21845, 56283.67 -> 56284
    assert CO.is_diagonal(rows) and not CO.is_diagonal([[1, 2, 0], [0, 1, 0]])
    # the bounds of vqa_conform_submit
    CO.fixed_matrix([[16]], [1 << 17])
    with pytest.raises(ValueError):
        CO.fixed_matrix([[Fraction(16) + Fraction(1, 65536)]], [0])
    with pytest.raises(ValueError):
        CO.fixed_matrix([[1]], [(1 << 17) + 1])
    # a diagonal map's table is the matrix's own arithmetic, sample by sample
    lut = CO.diagonal_lut([[56283, 0, 16 * 65536], [0, -65536, 300 * 65536]], 8)
    assert lut[0][0] == 16 and lut[0][255] == (56283 * 255 + 16 * 65536 + 32768) >> 16 and lut[1][0] == 255 and lut[1][255] == 45


def test_levels_and_matrix_fits_become_tables_or_a_matrix():
    label, lut, m = CO.color_map(("levels", [Fraction(255, 219)] * 3, [Fraction(-16 * 255, 219)] * 3), 8, "yuv")
    assert label == "levels" and m is None and lut[0][16] == 0 and lut[0][235] == 255 and lut[2][255] == 255 and lut[1][0] == 0
    M = [[Fraction(1), Fraction(1, 10), 0], [0, 1, 0], [0, 0, 1]]
    label, lut, m = CO.color_map(("matrix", M, [0, 1, -2]), 10, "yuv")
    assert label == "matrix" and lut is None and m[0][:3] == [65536, 6554, 0] and m[1][3] == 65536 and m[2][3] == -131072
    label, lut, m = CO.color_map(("matrix", [[2]], [3]), 8, "gray")     # one plane: always a table
    assert m is None and lut[0][:3] == [3, 5, 7] and lut[0][255] == 255
    with pytest.raises(ValueError):
        CO.color_map(("levels", [1], [0]), 8, "yuv")
    with pytest.raises(ValueError):
        CO.color_map(("gamma", 2.2), 8, "yuv")


def _tab(bins, filled):
    rows = [[0, 0, 0] for _ in range(bins)]
    for c, (count, total) in filled.items():
        rows[c] = [count, total, 0]
    return [rows]


def test_the_tone_table_fill_rule_by_hand():
    # filled bins: the mean rounded half up
    lut = CO.tone_lut(_tab(256, {10: (2, 41), 11: (4, 90), 12: (3, 100)}), 8)[0]
    assert lut[10] == 21 and lut[11] == 23 and lut[12] == 33          # 20.5 -> 21, 22.5 -> 23, 33.33 -> 33
    # a gap: integer linear interpolation, rounded half up
    lut = CO.tone_lut(_tab(256, {100: (1, 50), 104: (1, 60)}), 8)[0]
    assert lut[100:105] == [50, 53, 55, 58, 60]                          # 52.5 -> 53, 55, 57.5 -> 58
    lut = CO.tone_lut(_tab(256, {100: (1, 60), 103: (1, 50)}), 8)[0]
    assert lut[100:104] == [60, 57, 53, 50]                              # 56.67 -> 57, 53.33 -> 53
    # empty ends: slope one from the nearest filled bin, clipped to 0 .. peak
    lut = CO.tone_lut(_tab(256, {5: (1, 2), 250: (1, 253)}), 8)[0]
    assert lut[:6] == [0, 0, 0, 0, 1, 2] and lut[250:] == [253, 254, 255, 255, 255, 255]
    # a single filled bin: slope one everywhere around it
    lut = CO.tone_lut(_tab(1024, {512: (3, 1800)}), 10)[0]
    assert lut[512] == 600 and lut[0] == 88 and lut[511] == 599 and lut[935] == 1023 and lut[1023] == 1023
    # no filled bin: the identity
    assert CO.tone_lut(_tab(256, {}), 8)[0] == list(range(256))
    # through color_map, per plane
    label, lut, m = CO.color_map(("tone", _tab(256, {0: (1, 7)}) * 3), 8, "yuv")
    assert label == "tone" and m is None and len(lut) == 3 and lut[1][3] == 10


def test_refusals():
    with pytest.raises(ValueError):
        CO.tone_lut(_tab(4096, {}), 12)                                  # above 10 bits a bin holds several codes
    with pytest.raises(ValueError):
        CO.tone_lut(_tab(128, {}), 8)
    with pytest.raises(ValueError):
        CO.color_map(("tone", _tab(256, {})), 8, "yuv")                  # one plane's tables for a three-plane model
    with pytest.raises(ValueError):
        CO.plan(mono_planes, 32, 32, 8, "yuv")                           # the model's planes
    with pytest.raises(ValueError):
        CO.plan(mono_planes, 32, 32, 8, "gray", ref_index=[0, 1])        # a path without the counts
    with pytest.raises(ValueError):
        CO.plan(lambda h, w: [(w // 4, h, 0, w // 4, 1)], 32, 32, 8, "gray")   # neither the luma's size nor its half
    # the entry points' requests
    assert vp._conform_request(False, "match") is None
    assert vp._conform_request(True, "none", shift=4) == "none"
    assert vp._conform_request(True, "match", align=2, colorfit=True) == "match"
    for bad in (dict(conform=1), dict(conform=True, color="gamma"), dict(conform=True, color="none"),
                dict(conform=True, color="match", shift=4), dict(conform=True, color="none", shift=4, scale="bicubic")):
        with pytest.raises(ValueError):
            vp._conform_request(bad.pop("conform"), bad.pop("color", "match"), **bad)
    base = {"crf": 23, "resize_width": 64, "resize_height": 64}
    vp.validate_config(dict(base, conform=True, conform_color="levels", colorfit=True))
    vp.validate_config(dict(base, conform_color="tone"))
    for cfg in (dict(conform=True), dict(conform="yes", shift=2), dict(conform=True, shift=2), dict(conform_color="gamma"),
                dict(conform=True, conform_color="none", sync=True, scale="bicubic", dist_height=32, dist_width=32)):
        with pytest.raises(ValueError):
            vp.validate_config(dict(base, **cfg))
    # Engine.conform_submit's checks that need no GPU
    p64, p32 = mono_planes(64, 64), mono_planes(32, 32)
    o, ix, lut, m = check_conform_args(p64, p32, [(32, 32)], [1, 0, 1], np.arange(256)[None, ::-1], None)
    assert o.dtype == np.int32 and ix.dtype == np.int32 and lut.dtype == np.uint8 and lut[0, 0] == 255 and m is None
    p444 = yuv_planes(64, 64, "444", 10)
    _, _, lut, m = check_conform_args(p444, yuv_planes(32, 32, "444", 10), None, None, np.zeros((3, 1024), np.int64), np.eye(3, 4, dtype=int))
    assert lut.dtype == np.uint16 and m.dtype == np.int64
    for kw in (dict(origin=[(33, 0)]), dict(origin=[(0, -1)]), dict(origin=[(0, 0), (0, 0)]), dict(index=[]), dict(index=[0.5]),
               dict(lut=np.zeros((1, 255), np.uint8)), dict(lut=np.full((1, 256), 256)), dict(lut=np.zeros((1, 256))),
               dict(matrix=np.eye(3, 4, dtype=int))):
        with pytest.raises(ValueError):
            check_conform_args(p64, p32, **kw)
    with pytest.raises(ValueError):
        check_conform_args(p64, mono_planes(15, 32))
    with pytest.raises(ValueError):
        check_conform_args(p64, mono_planes(32, 32, 10))
    with pytest.raises(ValueError):
        check_conform_args(p444, p444, matrix=np.full((3, 4), 1 << 21))
    # the pass: a plan's out_planes are the pass's planes, and never under scale
    from rtvqa_amd import stream
    plan = CO.plan(LAYOUTS["420"], 48, 64, 8, "yuv", shift=(-1, 2))
    q = stream.Quality(plan["out_planes"], conform=plan)
    assert q.conform is plan and q.conform_args["dist"][0].tolist() == [[1, 0], [0, 0], [0, 0]]
    assert q.conform_args["ref"][0].tolist() == [[0, 2], [0, 1], [0, 1]] and plan["summary"]["CONFORM_CHROMA_HALF"] == 1
    with pytest.raises(ValueError):
        stream.Quality(plan["planes"], conform=plan)
    with pytest.raises(ValueError):
        stream.Quality(plan["out_planes"], conform=plan, dist_planes=LAYOUTS["420"](24, 32), scale="bicubic")
