"""The shapes and contents of the dE_ITP tests, shared by tests/test_itp_host.py (the restatement's own properties, and what
float32 would cost) and tests/test_gpu_itp.py (the GPU against the float64 restatement), so that both see the same bytes.
Integer-only and seeded.  Small shapes only; each reaches one code path of k_itp."""
import numpy as np

import itp_reference as R

# (h, w), depth, layout:
#   16 x 16 4:4:4 at 8 bits          the minimum: 32 patches, one workgroup, one load per row
#   17 wide, 19 high 4:2:0 at 10     odd sizes, 9 x 10 chroma, sample by sample, partial patches in both directions
#   64 wide, 36 high 4:2:0 at 10     one load per row, 288 patches: five workgroups, the last one partly idle
#   36 wide, 20 high 4:2:2 at 12     halved width only
#   20 wide, 16 high 4:4:4 at 16     the full code range of uint16
#   24 wide, 18 high packed bgr24    pixel step 3: sample by sample
GRID = [((16, 16), 8, "yuv444p"), ((19, 17), 10, "yuv420p10le"), ((36, 64), 10, "yuv420p10le"), ((20, 36), 12, "yuv422p12le"),
        ((16, 20), 16, "yuv444p16le"), ((18, 24), 8, "bgr24")]
IDS = ["%dx%d-%s" % (g[0][1], g[0][0], g[2]) for g in GRID]
VECTOR = ((36, 64), 10, "yuv420p10le")     # the clip the windows, the strided view and the batch tests use
RANGES_ON = ((19, 17), 10, "yuv420p10le")  # the one YUV case that also runs in full range
CONTENTS = ("noise", "noise3", "equal", "graystep", "extremes", "dark")
TRANSFERS = (("pq", R.PQ), ("hlg", R.HLG))
COUNTS = (1, 3)
ROIS = [(5, 3, 21, 33), (4, 8, 24, 40)]      # (y0, x0, h, w) of the 64 x 36 clip as 4:4:4: an unaligned window; an aligned one


def model_of(layout):
    return R.BGR if layout == "bgr24" else R.YUV2020


def planes_of(layout, h, w, depth):
    from rtvqa_amd.engine import bgr_planes, yuv_planes
    from rtvqa_amd.frames import PIXFMTS
    return bgr_planes(h, w) if layout == "bgr24" else yuv_planes(h, w, PIXFMTS[layout][0], depth)


def _sizes(layout, h, w):
    from rtvqa_amd.frames import PIXFMTS, plane_sizes
    return [(w, h)] * 3 if layout == "bgr24" else plane_sizes(h, w, PIXFMTS[layout][0])


def _pack(layout, planes3, n, h, w, depth):
    """three arrays [n, ph, pw] -> frames: [n, h, w, 3] uint8 for bgr24, [n, samples] planar otherwise"""
    dt = np.uint16 if depth > 8 else np.uint8
    if layout == "bgr24":
        return np.ascontiguousarray(np.stack(planes3, axis=-1).astype(dt))
    return np.ascontiguousarray(np.concatenate([p.reshape(n, -1) for p in planes3], axis=1).astype(dt))


def clip(content, layout, h, w, depth, n, seed=0, full_range=False):
    """n frame pairs of one content -> (ref, dist, planes).
      noise     two unrelated clips, uniform over every code 0 .. 2^depth - 1 (out-of-gamut triples: the clamp)
      noise3    uniform noise and its copy with +-3 codes added, clipped to the code range
      equal     a noise clip against itself
      graystep  neutral chroma, luma flat at a mid code against the next code (bgr24: B = G = R likewise): under PQ the pair is
                720 / (219 s) apart per pixel in limited range (720 / 876 at 10 bits), 720 / P in full range and for bgr24
      extremes  every sample 0 against every sample 2^depth - 1
      dark      within 8 codes of black (black as the range reads it), with +-3 codes: where E'^(1/m2) - c1 cancels"""
    rng = np.random.default_rng([seed, h, w, depth, CONTENTS.index(content)])
    s, peak = 1 << (depth - 8), (1 << depth) - 1
    sizes = _sizes(layout, h, w)
    yuv = layout != "bgr24"
    if yuv and not full_range:
        black, neutral, mid = 16 * s, 128 * s, (502 * s) >> 2   # (10 bits: Y = 502 against 503, chroma 512)
    else:
        black, neutral, mid = 0, (1 << (depth - 1)) if yuv else 0, peak // 2
    if content in ("noise", "noise3", "equal"):
        a = [rng.integers(0, peak + 1, (n, ph, pw)) for (pw, ph) in sizes]
        if content == "noise":
            b = [rng.integers(0, peak + 1, (n, ph, pw)) for (pw, ph) in sizes]
        elif content == "noise3":
            b = [np.clip(p + rng.integers(-3, 4, p.shape), 0, peak) for p in a]
        else:
            b = [p.copy() for p in a]
    elif content == "graystep":
        if yuv:
            a = [np.full((n, ph, pw), mid if k == 0 else neutral) for k, (pw, ph) in enumerate(sizes)]
            b = [p + (1 if k == 0 else 0) for k, p in enumerate(a)]
        else:
            a = [np.full((n, ph, pw), mid) for (pw, ph) in sizes]
            b = [p + 1 for p in a]
    elif content == "extremes":
        a = [np.zeros((n, ph, pw), np.int64) for (pw, ph) in sizes]
        b = [np.full((n, ph, pw), peak) for (pw, ph) in sizes]
    elif content == "dark":
        a, b = [], []
        for k, (pw, ph) in enumerate(sizes):
            lo, hi = (black, black + 8) if (k == 0 or not yuv) else (neutral - 8, neutral + 8)
            p = rng.integers(lo, hi + 1, (n, ph, pw))
            a.append(p)
            b.append(np.clip(p + rng.integers(-3, 4, p.shape), max(lo, 0), hi))
    else:
        raise ValueError(content)
    return _pack(layout, a, n, h, w, depth), _pack(layout, b, n, h, w, depth), planes_of(layout, h, w, depth)


def graystep_answer(layout, depth, full_range):
    """dE_ITP of every pixel of the graystep pair under PQ: dI = the step of E', dT = dCp = 0"""
    if layout == "bgr24" or full_range:
        return 720.0 / ((1 << depth) - 1)
    return 720.0 / (219 << (depth - 8))


def matrix():
    """every (geometry, depth, layout, content, transfer name, transfer, full_range) of the GPU parity matrix: both transfers
    everywhere, both ranges on one YUV case"""
    out = []
    for (g, d, lay) in GRID:
        for full in ((False, True) if (g, d, lay) == RANGES_ON else (False,)):
            for (tn, t) in TRANSFERS:
                for c in CONTENTS:
                    out.append((g, d, lay, c, tn, t, full))
    return out


def matrix_ids():
    return ["%dx%d-%s-%s-%s-%s" % (g[1], g[0], lay, c, tn, "full" if full else "limited") for (g, d, lay, c, tn, t, full) in matrix()]


_REF = {}


def reference(frames_ref, frames_dist, planes, depth, model, transfer, full_range, key=None):
    """the float64 restatement of every frame of a clip -> list of itp_reference.record dicts; computed once per key and shared"""
    if key is not None and key in _REF:
        return _REF[key]
    fr, fd = R.split_planes(frames_ref, planes), R.split_planes(frames_dist, planes)
    out = [R.record(a, b, depth, model, transfer, full_range) for a, b in zip(fr, fd)]
    if key is not None:
        _REF[key] = out
    return out


def window_cut(x, window, n):
    """the window's samples of a [n, 3 * H, W] clip as frames of their own -> ([n, samples], planes)"""
    H, W = VECTOR[0]
    y0, x0, hh, ww = window
    cut = np.ascontiguousarray(x.reshape(n, 3, H, W)[:, :, y0:y0 + hh, x0:x0 + ww]).reshape(n, -1)
    bps = x.dtype.itemsize
    return cut, [(ww, hh, k * hh * ww * bps, ww * bps, bps, VECTOR[1]) for k in range(3)]
