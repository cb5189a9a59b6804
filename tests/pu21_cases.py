"""The shapes and contents of the PU21 tests, shared by tests/test_pu21_host.py (the restatements against each other) and
tests/test_gpu_pu21.py (the GPU against them), so that both see the same bytes.  Integer-only and seeded.  Small shapes only; each
reaches one code path of k_pu21_encode (k_itp's loads) or of k_pu21_ssim (16 x 16 windows a tile)."""
import numpy as np

import itp_cases as IC
import pu21_reference as R

# (h, w), depth, layout:
#   16 x 16 4:4:4 at 8 bits          the minimum: 6 x 6 windows, one tile, one load per row
#   17 wide, 19 high 4:2:0 at 10     odd sizes, sample by sample, partial patches in both directions
#   33 wide, 35 high 4:2:0 at 12     odd 4:2:0; 23 x 25 windows: two tiles each way, the second ones ragged
#   27 x 27 4:2:2 at 12              ONE window past the tile in each direction (16 + 1 + 10)
#   20 wide, 16 high 4:4:4 at 16     the full code range of uint16
#   24 wide, 18 high packed bgr24    pixel step 3: sample by sample
#   64 wide, 36 high 4:2:0 at 10     one load per row; 54 x 26 windows: 4 x 2 tiles
GRID = [((16, 16), 8, "yuv444p"), ((19, 17), 10, "yuv420p10le"), ((35, 33), 12, "yuv420p12le"), ((27, 27), 12, "yuv422p12le"),
        ((16, 20), 16, "yuv444p16le"), ((18, 24), 8, "bgr24"), ((36, 64), 10, "yuv420p10le")]
VECTOR = ((36, 64), 10, "yuv420p10le")     # the clip the views and the batch tests use
RANGES_ON = ((19, 17), 10, "yuv420p10le")  # the one YUV case that also runs in full range
CONTENTS = ("natural", "noise", "flat_lo", "flat_hi", "extremes", "equal", "darkstep")
TRANSFERS = (("pq", R.PQ), ("hlg", R.HLG))
N_FRAMES = 2
SHIPPED = (0, 5, 12)                        # indices into matrix(): the cases the shipped library repeats

model_of, planes_of = IC.model_of, IC.planes_of


def clip(content, layout, h, w, depth, n, seed=0, full_range=False):
    """n frame pairs of one content -> (ref, dist, planes).
      natural   a smooth ramp with texture over most of the code range, and its copy with +-3 codes added
      noise     two unrelated clips, uniform over every code (out-of-gamut triples: the clamp)          [itp_cases]
      flat_lo   every pixel black as the range reads it, against black + 2 luma codes (bgr24: all three channels)
      flat_hi   every pixel peak white as the range reads it, against white - 2 codes
      extremes  every sample 0 against every sample 2^depth - 1: black against peak white                [itp_cases]
      equal     a noise clip against itself                                                             [itp_cases]
      darkstep  a flat field 4 codes above black against the next code: one code value on a dark flat field"""
    if content in ("noise", "extremes", "equal"):
        return IC.clip(content, layout, h, w, depth, n, seed, full_range)
    rng = np.random.default_rng([seed, h, w, depth, 100 + CONTENTS.index(content)])
    s, peak = 1 << (depth - 8), (1 << depth) - 1
    sizes = IC._sizes(layout, h, w)
    yuv = layout != "bgr24"
    if yuv and not full_range:
        black, white, neutral = 16 * s, 235 * s, 128 * s
    else:
        black, white, neutral = 0, peak, (1 << (depth - 1)) if yuv else 0
    if content == "natural":
        a = []
        for k, (pw, ph) in enumerate(sizes):
            yy, xx = np.mgrid[0:ph, 0:pw]
            ramp = (xx / max(pw - 1, 1)) * 0.7 + (yy / max(ph - 1, 1)) * 0.2 + 0.05
            if yuv and k > 0:
                ramp = 0.5 + 0.15 * np.sin(xx / 3.0 + k) * np.cos(yy / 4.0)
            base = np.rint(ramp * peak)[None] + rng.integers(-6 * s, 6 * s + 1, (n, ph, pw))
            a.append(np.clip(base, 0, peak).astype(np.int64))
        b = [np.clip(p + rng.integers(-3, 4, p.shape), 0, peak) for p in a]
    else:
        lo = {"flat_lo": black, "flat_hi": white, "darkstep": black + 4}[content]
        step = {"flat_lo": 2, "flat_hi": -2, "darkstep": 1}[content]
        a = [np.full((n, ph, pw), lo if (k == 0 or not yuv) else neutral, np.int64) for k, (pw, ph) in enumerate(sizes)]
        b = [p + (step if (k == 0 or not yuv) else 0) for k, p in enumerate(a)]
    return IC._pack(layout, a, n, h, w, depth), IC._pack(layout, b, n, h, w, depth), planes_of(layout, h, w, depth)


def matrix():
    """every (geometry, depth, layout, content, transfer name, transfer, full_range) of the parity matrix: both transfers
    everywhere, both ranges on one YUV case"""
    out = []
    for (g, d, lay) in GRID:
        for full in ((False, True) if (g, d, lay) == RANGES_ON else (False,)):
            for (tn, t) in TRANSFERS:
                for c in CONTENTS:
                    out.append((g, d, lay, c, tn, t, full))
    return out


def case_id(case):
    g, d, lay, c, tn, t, full = case
    return "%dx%d-%s-%s-%s-%s" % (g[1], g[0], lay, c, tn, "full" if full else "limited")


def matrix_ids():
    return [case_id(c) for c in matrix()]


def case_clip(case):
    g, d, lay, c, tn, t, full = case
    return clip(c, lay, g[0], g[1], d, N_FRAMES, full_range=full)


_REF = {}


def reference(case):
    """the restatements of every frame of a case -> list of (unquantised record, quantised record, q_Y ref, q_Y dist); computed
    once per case and shared"""
    key = case_id(case)
    if key not in _REF:
        g, d, lay, c, tn, t, full = case
        r, x, planes = case_clip(case)
        fr, fd = R.split_planes(r, planes), R.split_planes(x, planes)
        m = model_of(lay)
        _REF[key] = [(R.record(a, b, d, m, t, full),) + R.record_q(a, b, d, m, t, full) for a, b in zip(fr, fd)]
    return _REF[key]
