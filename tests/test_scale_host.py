"""CPU: the resampler's definition.  tests/scale_reference.py against Pillow's pinned output (tests/golden/scale_pins.json,
scripts/gen_scale_pins.py), vqa_scale_tables against the restatement's tables, the consequences include/vqa.h states, the additive
ABI, and every ValueError of the Python layers - none of which needs a GPU."""
import base64
import ctypes as C
import json
import os
import re
import subprocess
import sys
import zlib

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (REPO, os.path.dirname(os.path.abspath(__file__))) if p not in sys.path]

import scale_reference as R
from rtvqa_amd import _native as N
from rtvqa_amd import engine as E
from rtvqa_amd import stream
from rtvqa_amd import video_processing as vp


@pytest.fixture(scope="module")
def pins():
    with open(os.path.join(REPO, "tests", "golden", "scale_pins.json")) as f:
        doc = json.load(f)
    out = []
    for i, c in enumerate(doc["cases"]):
        h, w = c["in"]
        oh, ow = c["out"]
        src = R.pin_input(doc["seed"], i, h, w, c["content"], c["depth"])
        want = np.frombuffer(zlib.decompress(base64.b64decode(c["data"])), "<u2" if c["depth"] > 8 else np.uint8).reshape(oh, ow)
        out.append((c, src, want))
    assert doc["tool"].startswith("Pillow ") and len(out) >= 60
    return out


def test_the_restatement_equals_pillow_in_mode_l_at_every_sample(pins):
    seen, clipped_lo, clipped_hi = set(), 0, 0
    for c, src, want in pins:
        if c["mode"] != "L":
            continue
        got = R.resample(src, want.shape[0], want.shape[1], 8, filter=c["filter"])
        assert got.dtype == np.uint8 and (got == want).all(), (c["filter"], c["in"], c["out"], c["content"])
        seen.add((c["filter"], tuple(c["in"]), tuple(c["out"])))
        if c["content"] == "binary" and c["filter"] != "bilinear":
            clipped_lo += int((want == 0).sum())
            clipped_hi += int((want == 255).sum())
    assert len(seen) == 30 and {s[0] for s in seen} == set(R.FILTERS)
    assert clipped_lo > 1000 and clipped_hi > 1000       # both clips act on the 0 / 255 content
    geos = {s[1:] for s in seen}
    assert any(i[0] == o[0] and i[1] != o[1] for i, o in geos) and any(i[1] == o[1] and i[0] != o[0] for i, o in geos)
    assert any(i[0] == 4 * o[0] for i, o in geos) and any(o[0] == 8 * i[0] for i, o in geos)


def test_the_i16_pins_lie_within_two_units(pins):
    """Pillow filters 16-bit data in double; the 2^-22 tables cost at most one unit a pass, two through both.  Seen on the
    four pinned cases: largest gap 1, 4 of 1052 samples unequal.  The inputs keep to the middle half of the
    range: where a pass leaves 0 .. 65535 Pillow saturates the high byte only (scripts/gen_scale_pins.py), which is no clip."""
    n, worst, unequal, total = 0, 0, 0, 0
    for c, src, want in pins:
        if c["mode"] != "I;16":
            continue
        assert c["depth"] == 16 and c["filter"] in ("bicubic", "lanczos") and src.dtype == np.uint16
        assert 0 < int(want.min()) and int(want.max()) < 65535
        got = R.resample(src, want.shape[0], want.shape[1], 16, filter=c["filter"])
        gap = np.abs(got.astype(np.int64) - want.astype(np.int64))
        worst, unequal, total, n = max(worst, int(gap.max())), unequal + int((gap > 0).sum()), total + gap.size, n + 1
    print("I;16: largest gap %d, %d of %d samples unequal" % (worst, unequal, total))
    assert n == 4 and worst <= 2


PAIRS = [(48, 72), (72, 48), (16, 128), (64, 16), (47, 94), (51, 153), (96, 64), (37, 59), (70, 23), (1080, 1920), (1920, 1080),
         (360, 1080), (1280, 1920), (33, 33), (4096, 1024)]


@pytest.mark.parametrize("filt", R.FILTERS)
def test_vqa_scale_tables_against_the_restatement(filt):
    for n_in, n_out in PAIRS:
        k, xmin, count = E.scale_tables(filt, n_in, n_out)
        rk, rxmin, rcount = R.tables(filt, n_in, n_out)
        assert k.shape == rk.shape == (n_out, R.ksize(filt, n_in, n_out)) and k.shape[1] <= 25
        assert (xmin == rxmin).all() and (count == rcount).all()
        gap = int(np.abs(k.astype(np.int64) - rk).max())
        assert gap <= (1 if filt == "lanczos" else 0), (filt, n_in, n_out, gap)   # (lanczos: libm's sin against Python's)
        # what the kernel's footprint rests on: neither end of a window ever moves back
        assert (np.diff(xmin) >= 0).all() and (np.diff(xmin + count) >= 0).all() and (count >= 1).all()
        assert (xmin >= 0).all() and (xmin + count <= n_in).all()
        rows = k.astype(np.int64).sum(axis=1)
        assert int(np.abs(rows - (1 << 22)).max()) <= k.shape[1] // 2 + 1
        if filt != "bilinear":
            assert 255 * int(np.abs(k.astype(np.int64)).sum(axis=1).max()) + (1 << 21) < (1 << 31)   # the uint8 sums fit 32 bits


def test_vqa_scale_tables_arguments():
    lib = N.load()
    ks = C.c_int(0)
    i32 = C.POINTER(C.c_int32)
    none = (None, None, None)
    assert lib.vqa_scale_tables(1, 64, 96, *none, C.byref(ks)) == N.VQA_OK and ks.value == 5
    assert lib.vqa_scale_tables(2, 64, 16, *none, C.byref(ks)) == N.VQA_OK and ks.value == 25
    assert lib.vqa_scale_tables(0, 64, 512, *none, C.byref(ks)) == N.VQA_OK and ks.value == 3
    assert lib.vqa_scale_tables(1, 64, 513, *none, C.byref(ks)) == N.VQA_ERR_UNSUPPORTED
    assert lib.vqa_scale_tables(1, 65, 16, *none, C.byref(ks)) == N.VQA_ERR_UNSUPPORTED
    for bad in (3, -1):
        assert lib.vqa_scale_tables(bad, 64, 96, *none, C.byref(ks)) == N.VQA_ERR_INVALID
    assert lib.vqa_scale_tables(1, 0, 96, *none, C.byref(ks)) == N.VQA_ERR_INVALID
    assert lib.vqa_scale_tables(1, 64, 96, *none, None) == N.VQA_ERR_INVALID
    one = np.zeros(96 * 5, np.int32)
    assert lib.vqa_scale_tables(1, 64, 96, one.ctypes.data_as(i32), None, None, C.byref(ks)) == N.VQA_ERR_INVALID
    k, xmin, count = E.scale_tables("bicubic", 40, 40)           # the formula's tables of an unchanged axis: the identity
    assert (xmin + np.argmax(k, axis=1) == np.arange(40)).all() and (k.max(axis=1) == 1 << 22).all() and (k.sum(axis=1) == 1 << 22).all()
    with pytest.raises(ValueError):
        E.scale_tables("nearest", 64, 96)
    with pytest.raises(N.VqaError):
        E.scale_tables("bicubic", 64, 1000)


@pytest.mark.parametrize("depth", (8, 9, 10, 12, 16))
def test_flat_planes_stay_flat(depth):
    peak = (1 << depth) - 1
    dt = np.uint16 if depth > 8 else np.uint8
    for filt in R.FILTERS:
        for (h, w), (oh, ow) in (((27, 48), (41, 72)), ((64, 96), (16, 24)), ((16, 16), (128, 128)), ((45, 37), (30, 59))):
            tx, ty = E.scale_tables(filt, w, ow), E.scale_tables(filt, h, oh)
            for level in (0, peak // 2, peak):
                got = R.resample(np.full((h, w), level, dt), oh, ow, depth, tx, ty)
                assert got.shape == (oh, ow) and (got == level).all(), (depth, filt, level)


def test_the_output_never_exceeds_the_peak():
    rng = np.random.default_rng(3)
    src = rng.integers(0, 65536, (27, 48)).astype(np.uint16)
    for depth in (9, 10, 15):
        assert int(R.resample(src, 41, 72, depth, filter="bicubic").max()) == (1 << depth) - 1
        assert int(R.resample(src, 27, 72, depth, filter="lanczos").max()) == (1 << depth) - 1
        assert int(R.resample(src, 27, 48, depth).max()) == (1 << depth) - 1     # both axes copied: still clipped


def test_the_additive_abi():
    assert N.VQA_ABI_VERSION == 8
    assert (N.K_SCALE, N.K_MARGIN, N.K_FRINGE) == (66, 67, 65)
    assert N.K_IDS_PRESENT == N.K_IDS_COMPLETE + (66,) and 65 not in N.K_IDS_PRESENT and 67 not in N.K_IDS_PRESENT
    assert (N.SCALE_BILINEAR, N.SCALE_BICUBIC, N.SCALE_LANCZOS) == (0, 1, 2)
    assert N.SCALE_FILTERS == {"bilinear": 0, "bicubic": 1, "lanczos": 2}
    txt = open(os.path.join(REPO, "include", "vqa.h")).read()
    for name, val in (("VQA_K_SCALE", 66), ("VQA_K_MARGIN", 67), ("VQA_K_FRINGE", 65), ("VQA_SCALE_BILINEAR", 0),
                      ("VQA_SCALE_BICUBIC", 1), ("VQA_SCALE_LANCZOS", 2)):
        assert re.search(r"%s\s*=\s*%d\b" % (name, val), txt), name
    assert re.search(r"#define VQA_ABI_VERSION\s+8", txt)
    part = txt[txt.index("---- The resampler"):]
    part = part[:part.index("VQA_API int vqa_scale_tables")]
    for word in ("ksize = 2 ceil(support) + 1", "(x + 0.5) scale", "2^22", ">> 22", "a = -0.5", "sinc(x) sinc(x / 3)", "[-3, 3)",
                 "centre-sited", "1/4 <= out / in <= 8", "at least 16 x 16", "2^28", "VQA_ERR_STATE", "32768", "no wait is needed",
                 "flat plane stays flat", "never exceeds 2^d - 1", "Not built", "a = -0.6", "left-sited", "overlaps"):
        assert word in part, word
    lib = N.load()
    lib.vqa_kernel_name.restype = C.c_char_p
    assert lib.vqa_kernel_name(66) == b"k_scale" and lib.vqa_kernel_name(65) == b"?" and lib.vqa_kernel_name(67) == b"?"
    assert lib.vqa_kernel_name(64) == b"k_sigstats_scan"
    assert lib.vqa_scale_submit(None, None, 0, 0, 0, None, None, 0, None, 0, 1) == N.VQA_ERR_INVALID
    assert lib.vqa_scale_wait(None) == N.VQA_ERR_INVALID
    for path in (N.LIB_PATH, N.LAB_LIB_PATH):
        assert all(hasattr(C.CDLL(path), f) for f in ("vqa_scale_submit", "vqa_scale_wait", "vqa_scale_tables"))


def test_the_header_to_the_c_compiler(tmp_path):
    src = ('#include <stdio.h>\n#include "vqa.h"\n'
           'int (*submit)(vqa_ctx *, const uint8_t *, int, int, int64_t, const vqa_plane_desc *, uint8_t *, int64_t, '
           'const vqa_plane_desc *, int, int) = vqa_scale_submit;\n'
           'int (*wait_)(vqa_ctx *) = vqa_scale_wait;\n'
           'int main(void){int ks = 0; int rc = vqa_scale_tables(VQA_SCALE_LANCZOS, 64, 16, 0, 0, 0, &ks);\n'
           'printf("%d %d %d %d %d %d %d %d\\n", VQA_K_SCALE, VQA_K_MARGIN, VQA_K_FRINGE, VQA_SCALE_BILINEAR, VQA_SCALE_BICUBIC, '
           'VQA_SCALE_LANCZOS, rc, ks); return submit == 0 || wait_ == 0;}\n')
    (tmp_path / "s.c").write_text(src)
    lib_dir = os.path.dirname(N.LIB_PATH)
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), "-o", str(tmp_path / "s"), str(tmp_path / "s.c"),
                           "-L", lib_dir, "-l:" + os.path.basename(N.LIB_PATH), "-Wl,-rpath," + lib_dir,
                           "-Wl,--allow-shlib-undefined"])
    assert [int(v) for v in subprocess.check_output([str(tmp_path / "s")]).decode().split()] == [66, 67, 65, 0, 1, 2, 0, 25]


# ---- the Python layers: every refusal comes before anything is uploaded (no engine is created here) -----------------------------
def test_check_scale_planes_and_the_filter_names():
    y = E.yuv_planes
    E.check_scale_planes(y(360, 640), y(1080, 1920))
    E.check_scale_planes(y(64, 64, "mono"), y(16, 512, "mono"))           # exactly 1/4 and exactly 8
    for a, b in ((y(64, 64, "mono"), y(15, 64, "mono")),                  # a side below 16
                 (y(30, 64), y(60, 128)),                                 # ... of a chroma plane
                 (y(64, 64, "mono"), y(64, 513, "mono")),                 # beyond 8
                 (y(65, 64, "mono"), y(16, 64, "mono")),                  # below 1/4
                 (y(64, 64), y(64, 64, "mono")),                          # another plane count
                 (y(64, 64, "444", 10), y(96, 96, "444", 8))):            # another depth
        with pytest.raises(ValueError):
            E.check_scale_planes(a, b)
    with pytest.raises(ValueError):
        E.check_scale_planes(y(64, 64, "444") + y(64, 64, "444")[:2], y(64, 64, "444") + y(64, 64, "444")[:2])
    assert [E.scale_filter(f) for f in ("bilinear", "bicubic", "lanczos", 2)] == [0, 1, 2, 2]
    for bad in ("nearest", 3, None, True):
        with pytest.raises(ValueError):
            E.scale_filter(bad)
    assert E.planes_span(y(33, 47)) == 33 * 47 + 2 * 17 * 24 and E.planes_span(E.bgr_planes(4, 5)) == 60


def test_quality_refuses_half_a_request_and_what_the_kernel_would():
    y = E.yuv_planes
    q = stream.Quality(y(64, 96), dist_planes=y(32, 48), scale="lanczos", gmsd=True)
    assert q.scale == "lanczos" and q.dist_planes == y(32, 48)
    assert stream.Quality(y(64, 96)).scale is None and stream.Quality(y(64, 96)).dist_planes is None
    for kw in (dict(dist_planes=y(32, 48)), dict(scale="bicubic"), dict(dist_planes=y(32, 48), scale="nearest"),
               dict(dist_planes=y(32, 48, "mono"), scale="bicubic"), dict(dist_planes=y(32, 48, "420", 10), scale="bicubic"),
               dict(dist_planes=y(16, 24), scale="bicubic"), dict(dist_planes=y(300, 400), scale="bicubic")):
        with pytest.raises(ValueError):
            stream.Quality(y(64, 96), **kw)


def test_a_pass_refuses_before_it_uploads():
    y = E.yuv_planes
    bgr = np.zeros((4, 32, 48, 3), np.uint8)
    ref = np.zeros((4, 64, 96, 3), np.uint8)
    q = stream.Quality(E.bgr_planes(64, 96), dist_planes=E.bgr_planes(32, 48), scale="bicubic")
    with pytest.raises(ValueError, match="one BGR stream serves both halves"):          # the combined one-stream form
        stream.run(bgr, ref, quality=q, complexity=stream.Complexity((64, 64), 1))
    with pytest.raises(ValueError):
        vp.run_ffmpeg_metrics(ref, bgr, "p", "s", "v", dist_height=32, dist_width=48)    # a size without a filter
    with pytest.raises(ValueError):
        vp.run_ffmpeg_metrics(ref, bgr, "p", "s", "v", scale="nearest")
    with pytest.raises(ValueError):
        vp.run_ffmpeg_metrics(ref, bgr, "p", "s", "v", scale="bicubic", dist_height=32)
    r420 = np.zeros((2, E.planes_span(y(64, 96))), np.uint8)
    d420 = np.zeros((2, E.planes_span(y(32, 48))), np.uint8)
    with pytest.raises(ValueError, match="dist_height and dist_width"):                 # planar arrays carry no size
        vp.run_ffmpeg_metrics(r420, d420, "p", "s", "v", layout="yuv420p", height=64, width=96, scale="bicubic")
    with pytest.raises(ValueError, match="ratios"):
        vp.run_ffmpeg_metrics(np.zeros((2, 512, 512, 3), np.uint8), np.zeros((2, 16, 16, 3), np.uint8), "p", "s", "v", scale="bicubic")
    assert not any(os.path.exists(p) for p in ("p", "s", "v")) or [os.remove(p) for p in ("p", "s", "v") if os.path.exists(p)]
    for cfg in ({"scale": "nearest"}, {"dist_height": 32, "dist_width": 48}, {"scale": "bicubic", "dist_width": 48},
                {"scale": "bicubic", "dist_height": 0, "dist_width": 48}, {"scale": True}):
        with pytest.raises(ValueError):
            vp._check_mode_keys(cfg)
    vp._check_mode_keys({"scale": "lanczos", "dist_height": 360, "dist_width": 640})
    vp._check_mode_keys({"scale": "lanczos"})          # (.y4m pairs bring their sizes)
    with pytest.raises(ValueError, match="one BGR stream"):
        vp.process_video_and_extract_metrics(ref, bgr, {"scale": "bicubic", "frame_interval": 1}, csv_file="unused.csv")
    assert not os.path.exists("unused.csv")
    with pytest.raises(ValueError):
        vp.frame_scale(np.zeros((1, 64, 64, 3), np.uint8), "bgr24", None, None, 15, 64)
    with pytest.raises(ValueError):
        vp.frame_scale(np.zeros((1, 64, 64, 3), np.uint8), "bgr24", None, None, 32, 32, filter="area")


def test_sizes_that_merely_differ_stay_the_error_they_were():
    ref = np.zeros((2, 64, 96, 3), np.uint8)
    with pytest.raises(ValueError, match="same shape"):
        vp.frame_quality(ref, np.zeros((2, 32, 48, 3), np.uint8))


def test_the_log_gains_the_two_keys_last(tmp_path):
    from rtvqa_amd.engine import GMSD_DTYPE
    rec = np.zeros(3, GMSD_DTYPE)
    old, new = str(tmp_path / "old.json"), str(tmp_path / "new.json")
    vp.write_vif_log(old, gmsd=rec)
    vp.write_vif_log(new, gmsd=rec, extra={"DIST_RES": "48x32", "SCALE": "bicubic"})
    a, b = json.load(open(old)), json.load(open(new))
    assert list(b)[-2:] == ["DIST_RES", "SCALE"] and b["DIST_RES"] == "48x32" and b["SCALE"] == "bicubic"
    assert {k: v for k, v in b.items() if k not in ("DIST_RES", "SCALE")} == a
    vp.write_vif_log(new, gmsd=rec, extra=None)
    assert open(new).read() == open(old).read()
