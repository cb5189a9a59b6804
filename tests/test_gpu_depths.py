"""GPU: every kind of plane batch at the sample depths no other file submits - 9, 11, 12, 13, 14 and 15 bits.

check_planes (csrc/vqa_capi.hip) and the Python layer accept every depth from 8 to 16; the other files run 8, 10 and 16, and two
of them 12.  The depth-dependent arithmetic differs in every kernel (tests/depth_cases.py lists it), so each new depth is a new
input.

  parity    one tests/test_gpu_all_kinds.py::Job per kind and depth - 4:2:0 at 70 x 74 (chroma 35 x 37: odd, two geometry groups),
            MS-SSIM on gray 177 x 263 - submitted alone from host memory and passed through that file's _anchor: the kind's own
            checker against the kind's own CPU reference at the kind's own bar.  PU21, which _anchor does not know, goes through
            depth_cases.pu21_check - the whole check of tests/test_gpu_pu21.py, maps, words and doubles, on the lab library's
            run in one child process, which the shipped library's records equal byte for byte - both transfers at 9 and 14 bits.
            No tolerance is introduced here.
  ends      a second clip per depth of range-end contents, through the same checker.  For the kinds whose device output is
            integer words compared for equality (CAMBI, the artefact measures, XPSNR, VCA, SI/TI, GMSD, HaarPSI, PSNR-HVS): the
            kind's own generator's (depth_cases.RANGE_ENDS; CAMBI also a ramp that ends AT the peak, where to10 rounds up to 1024
            and clamps).  For the kinds held to a float bar (Gaussian SSIM, MS-SSIM, VIF, ADM, CIEDE2000, MDSI, BRISQUE, dE_ITP,
            PU21): flat fields at the maximum and at 0, 0 against the maximum, and the own generators' range ends
            (depth_cases.FLOAT_ENDS), each admitted on the CPU by tests/test_depths_host.py with the kind's existing figure.
  shifted   for the kinds include/vqa.h defines on the 8-bit scale through an exact power of two (depth_cases.SHIFT says which, and
            why not the others): the 8-bit clip shifted left by depth - 8 and submitted at that depth gives the 8-bit clip's
            figures within twice the kind's bar (both sides are GPU runs) - a check that rests on no restatement.  SI/TI's integer
            words scale exactly and are compared exactly; CAMBI's record is the same bytes.
The last test prints the worst gap per kind and depth (DESIGN.md section 3 has the table)."""
import contextlib
import io
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path[:0] = [REPO, os.path.dirname(os.path.abspath(__file__))]

import depth_cases as DC
import test_gpu_all_kinds as TAK

pytestmark = pytest.mark.gpu

TABLE = {}
# kinds whose checker compares integer words for equality (BRISQUE: the moments from the record's words, every admitted alpha
# within its span): no gap to print.  Every other checker prints its figure, and a checker that stops doing so fails _note
WORDS = {"cambi": "words equal", "xpsnr": "words and block maps equal", "artifacts": "words equal",
         "brisque": "moments from the words, alpha within its admitted span"}
MARKER = {"vif": " worst ", "adm": " worst "}    # tests/test_gpu_vif.py, test_gpu_adm.py: '<tag> worst <figure>'; the others 'worst gap:'


def _note(label, kind, depth, text):
    """keeps what a checker printed about its worst gap"""
    if kind in WORDS:
        TABLE[label, depth] = WORDS[kind]
        return
    marker = MARKER.get(kind, "worst gap:")
    lines = [ln for ln in text.splitlines() if marker in ln]
    assert lines, (kind, depth, "the checker printed no line with %r: the table would have no figure" % marker)
    TABLE[label, depth] = lines[-1].split(marker, 1)[-1].strip()


def _run_and_anchor(engine, oracle, j, label):
    TAK._submit(engine, j)
    _bytes, raw = TAK._wait(engine, j)
    out = io.StringIO()
    try:
        with contextlib.redirect_stdout(out):
            TAK._anchor(j, raw, oracle)
    finally:
        print(out.getvalue()[-4000:])
    _note(label, j.kind, j.depth, out.getvalue())


@pytest.mark.parametrize("depth", DC.DEPTHS)
@pytest.mark.parametrize("kind", [k for k in DC.KINDS if k != "pu21"])
def test_parity_at_every_new_depth(engine, oracle, kind, depth):
    j = DC.job(kind, depth)
    assert j.depth == depth and j.host[0].dtype == np.uint16 and int(j.host[0].max()) <= (1 << depth) - 1
    _run_and_anchor(engine, oracle, j, kind)


@pytest.mark.parametrize("depth", DC.DEPTHS)
@pytest.mark.parametrize("kind", list(DC.RANGE_ENDS))
def test_the_range_ends_at_every_new_depth(engine, oracle, kind, depth):
    """the kinds whose device output is integer words: the range-end contents of the kind's own generator, word for word through
    the kind's own checker"""
    _run_and_anchor(engine, oracle, DC.range_end_job(kind, depth), kind + ", range ends")


@pytest.mark.parametrize("depth", DC.DEPTHS)
@pytest.mark.parametrize("kind", [k for k in DC.FLOAT_ENDS if k != "pu21"])
def test_the_range_ends_of_the_float_bar_kinds_at_every_new_depth(engine, oracle, kind, depth):
    """the kinds held to a float bar: flat fields at the maximum and at 0, 0 against the maximum, the kind's own range-end
    contents - one frame each (depth_cases.FLOAT_ENDS), every one admitted on the CPU by tests/test_depths_host.py - through the
    kind's own checker at the kind's own bar"""
    j = DC.float_end_job(kind, depth)
    assert j.n == len(DC.float_ends(kind, depth)) and j.host[0].dtype == np.uint16
    _run_and_anchor(engine, oracle, j, kind + ", range ends")


# ---- PU21: tests/test_gpu_pu21.py's whole check, whose q_Y maps only the lab library gives, in ONE child process -----------------
def _pu21_runs():
    return [(depth, content, transfer) for depth in DC.DEPTHS for content, transfer in DC.pu21_cases(depth)]


def _child(out_path):
    import rtvqa_amd
    got = {}
    with rtvqa_amd.Engine(0) as eng:
        assert eng.lib.vqa_build_flavour() == 3
        for depth, content, transfer in _pu21_runs():
            r, d, planes = DC.pu21_clip(content, depth)
            rec, maps = eng.pu21(r, d, planes, transfer=transfer, maps=True)
            got["rec-%d-%s-%s" % (depth, content, transfer)] = np.frombuffer(rec.tobytes(), np.uint8)
            got["map-%d-%s-%s" % (depth, content, transfer)] = maps
    np.savez(out_path, **got)
    print("PU21-DEPTHS-LAB-OK", len(got))


@pytest.fixture(scope="module")
def lab(tmp_path_factory):
    from rtvqa_amd import _native as N
    from rtvqa_amd.engine import PU21_DTYPE
    out = str(tmp_path_factory.mktemp("pu21depths") / "lab.npz")
    env = dict(os.environ, VQA_LIB_PATH=N.LAB_LIB_PATH)
    env.pop("VQA_PU21_SUBSLICE", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True, timeout=300, cwd=REPO)
    assert r.returncode == 0 and "PU21-DEPTHS-LAB-OK" in r.stdout, (r.stdout[-300:], r.stderr[-2000:])
    with np.load(out) as z:
        return {k: (np.frombuffer(z[k].tobytes(), PU21_DTYPE) if k.startswith("rec") else z[k]) for k in z.files}


@pytest.mark.parametrize("depth", DC.DEPTHS)
def test_pu21_parity_at_every_new_depth(engine, lab, depth):
    """natural content under PQ (HLG too at 9 and 14 bits) and black against peak white: the maps, the words and the doubles of
    the lab library's run (depth_cases.pu21_check), and the shipped library gives the lab library's records byte for byte"""
    worst = {}
    for content, transfer in DC.pu21_cases(depth):
        r, d, planes = DC.pu21_clip(content, depth)
        assert r.dtype == np.uint16 and int(max(r.max(), d.max())) <= (1 << depth) - 1 and planes[0][5] == depth
        key = "%d-%s-%s" % (depth, content, transfer)
        rec, maps = lab["rec-" + key], lab["map-" + key]
        assert maps.shape == (r.shape[0], 2) + DC.GEOMETRY and maps.dtype == np.uint32
        assert engine.pu21(r, d, planes, transfer=transfer).tobytes() == rec.tobytes(), key
        worst[content, transfer] = DC.pu21_check(rec, r, d, planes, depth, transfer, "depths: pu21 %s" % key, maps=maps)
        if content == "extremes":                # terms past 2^32: the high words at work
            assert rec[0]["sse_y_hi"] > 0 and rec[0]["sse_rgb_hi"] > 0 and np.isfinite(rec[0]["pu_psnr"])
    for content, label in (("natural", "pu21"), ("extremes", "pu21, range ends")):
        TABLE[label, depth] = "; ".join("%s: maps within %d, ssim_q %.3f of a unit a window, mse gap %.3f of its bar, pu_ssim gap %.2e"
                                        % (t, v["map"], v["u"], v["mse"], v["ssim"]) for (c, t), v in worst.items() if c == content)


def _gap(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


@pytest.mark.parametrize("depth", DC.DEPTHS)
@pytest.mark.parametrize("kind", DC.SHIFT_KINDS)
def test_the_shifted_8_bit_clip_gives_the_8_bit_figures(engine, kind, depth):
    import siti_reference as S
    import motion_cases as K
    import test_gpu_adm as TA
    import test_gpu_motion as TM
    import test_gpu_vif as TV
    low, high = DC.shifted_jobs(kind, depth)
    s = depth - 8
    TAK._submit(engine, low)
    a = TAK._wait(engine, low)[1]
    TAK._submit(engine, high)
    b = TAK._wait(engine, high)[1]
    if kind == "vif":
        gaps = {"scale": _gap(a["scale"], b["scale"]), "vif": _gap(a["vif"], b["vif"])}
        bars = {"scale": 2 * TV.BAR, "vif": 2 * TV.BAR}
    elif kind == "adm":
        gaps = {"scale": _gap(a["scale"], b["scale"]), "adm2": _gap(a["adm2"], b["adm2"])}
        bars = {"scale": 2 * TA.BAR, "adm2": 2 * TA.BAR}
    elif kind == "motion":
        gaps = {"motion": _gap(a["motion"], b["motion"]), "sad": _gap(a["sad"], b["sad"])}
        bars = {"motion": 2 * TM.BAR, "sad": 2 * TM.BAR}
    elif kind == "siti":
        # the header's integers scale exactly; ti is then the same double (every step scales by a power of two), si to the quantum
        assert np.array_equal(b["grad_sq"], a["grad_sq"] << np.uint64(2 * s)) and np.array_equal(b["diff_sq"], a["diff_sq"] << np.uint64(2 * s))
        assert np.array_equal(b["diff_sum"], a["diff_sum"] * (1 << s)) and np.array_equal(b["ti"], a["ti"])
        gaps, bars = {"si": 0.0}, {"si": 0.0}
        r8 = np.concatenate([low.host[2][None], low.host[0]])
        for jx, p in enumerate(low.planes):
            series = K.plane_series(r8, p)
            for i in range(low.n):
                _e, m, var = S.si_exact(series[i + 1])
                bar = S.quantum_bar(m, var) + S.quantum_bar(m * (1 << s), var * (1 << (2 * s)), depth)
                gap = abs(float(a[i, jx]["si"]) - float(b[i, jx]["si"]))
                assert gap <= bar, (kind, depth, i, jx, gap, bar)
                if gap >= gaps["si"]:
                    gaps["si"], bars["si"] = gap, bar
    elif kind == "cambi":                        # the same 10-bit image at every depth: the same record
        assert a.tobytes() == b.tobytes() and a["cambi"].max() > 0.0, (kind, depth)
        gaps, bars = {"bytes": 0.0}, {"bytes": 0.0}
    elif kind == "ciede":                        # ciede_cases.GPU_BAR is relative, on de_mean
        import ciede_cases as CDC
        rel = float((np.abs(a["de_mean"] - b["de_mean"]) / a["de_mean"]).max())
        gaps, bars = {"de_mean (relative)": rel}, {"de_mean (relative)": 2 * CDC.GPU_BAR}
    elif kind == "vca":
        ra, rb = a[0], b[0]
        assert np.array_equal(ra["nbx"], rb["nbx"]) and np.array_equal(ra["nby"], rb["nby"])
        gaps = {key: _gap(ra[key], rb[key]) for key in ("e", "h", "l")}
        bars = {key: 2e-4 * max(1.0, float(np.abs(ra[key]).max())) for key in ("e", "h", "l")}      # twice 1e-4 max(1, |value|): vqa.h
    else:
        raise KeyError(kind)
    print("depths, shifted 8-bit clip: %s %d bits" % (kind, depth), {k: "%.3e (bar %.3e)" % (gaps[k], bars[k]) for k in gaps})
    for key in gaps:
        assert gaps[key] <= bars[key], (kind, depth, key, gaps[key], bars[key])
    TABLE[kind + ", shifted", depth] = ", ".join("%s %.2e" % (k, gaps[k]) for k in gaps)


def test_the_worst_gap_per_kind_and_depth():
    """runs after the tests above (pytest keeps the file's order): the figures DESIGN.md section 3 quotes"""
    for (kind, depth), line in sorted(TABLE.items()):
        print("depths, worst gap: %-18s %2d bits  %s" % (kind, depth, line))


if __name__ == "__main__":
    _child(sys.argv[1])
