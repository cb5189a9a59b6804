"""The shapes, layouts and contents of the FSIM parity matrix, shared by tests/test_fsim_host.py (the restatement's own
properties, the dense DFT against np.fft, the integer pooling against the float pooling) and tests/test_gpu_fsim.py (the GPU
against the restatement), so that both see the same samples.  mdsi_cases' pair / pack / engine_planes, and one content more.

Shapes (h, w), the smallest at which the kernels can still go wrong:
  16 x 16    one MFMA tile, even N
  33 x 67    odd N, 67 prime, K not a multiple of 4, tile tails
  67 x 130   past the 64 x 32 tile of the box stage in both directions
  20 x 300   a long K loop against a short one; more than one column strip of a workgroup of the DFT kernel
  385 x 391  f = 2
  897 x 900  f = 4, grid 225 x 225"""
import functools

import numpy as np

import mdsi_cases as MC

SMALL = ((16, 16), (33, 67), (67, 130))
WIDE = (20, 300)
LARGE = ((385, 391), (897, 900))
FACTORS = {(16, 16): 1, (33, 67): 1, (67, 130): 1, (20, 300): 1, (385, 391): 2, (897, 900): 4}
LAYOUTS = MC.LAYOUTS
CONTENTS = ("natural", "noise", "texture_flat", "half", "identical", "ends", "flat_zero", "flat_peak")
STRUCTURELESS = ("ends", "flat_zero", "flat_peak")      # P = 0: flag bit 0, both scores 1.0
MODEL = MC.MODEL
BAR_LIMIT = 1e-4       # no case's derived bar (fsim_reference.derived_bar) may exceed the project's bar
engine_planes, pack, plane_sizes, dtype_of = MC.engine_planes, MC.pack, MC.plane_sizes, MC.dtype_of


@functools.lru_cache(maxsize=None)
def pair(name, layout, h, w, depth=8, seed=0):
    """-> (ref, dist): two tuples of int64 planes of `depth` bits.  Cached: treat the arrays as read-only.  "half": the left half
    of every plane flat in both images, the right half textured, with +-12 levels (8-bit scale) of noise on the copy's right half -
    more than half of the smallest scale's responses are the filters' tails, so the median and T are small."""
    if name != "half":
        return MC.pair(name, layout, h, w, depth, seed)
    rng = np.random.default_rng(100000 * LAYOUTS.index(layout) + 1000 * h + w + 7 * depth + seed + 5)
    peak, mid = (1 << depth) - 1, 128 << (depth - 8)
    r, d = [], []
    for k, (ph, pw) in enumerate(plane_sizes(layout, h, w)):
        p = MC._texture(ph, pw, peak, float(k)).copy()
        p[:, :pw // 2] = mid
        q = np.clip(p + np.rint(rng.integers(-12, 13, p.shape) * (peak / 255.0)).astype(np.int64), 0, peak)
        q[:, :pw // 2] = mid
        for a in (p, q):
            a.setflags(write=False)
        r.append(p)
        d.append(q)
    return tuple(r), tuple(d)


def matrix():
    """(content, layout, shape, depth): every content in every layout on the small shapes at 8 bits; every content in yuv420p on
    20 x 300; every content at 10 and 16 bits in yuv420p and bgr24 on 33 x 67; natural and noise in yuv420p and bgr24 at f = 2, 4"""
    out = [(c, l, s, 8) for c in CONTENTS for l in LAYOUTS for s in SMALL]
    out += [(c, "yuv420p", WIDE, 8) for c in CONTENTS]
    out += [(c, l, (33, 67), dp) for c in CONTENTS for l in ("yuv420p", "bgr24") for dp in (10, 16)]
    out += [(c, l, s, 8) for c in ("natural", "noise") for l in ("yuv420p", "bgr24") for s in LARGE]
    return out


MATRIX_CASES = 8 * 5 * 3 + 8 + 8 * 2 * 2 + 2 * 2 * 2       # 168


def case_id(case):
    c, l, s, dp = case
    return "%s-%s-%dx%d-%d" % (c, l, s[0], s[1], dp)


@functools.lru_cache(maxsize=None)
def expected(case):
    """the unquantised float64 restatement of a case, computed once -> dict(fsim, fsimc, pc_r, pc_d, bar)"""
    import fsim_reference as R
    c, l, (h, w), dp = case
    r, d = pair(c, l, h, w, dp)
    fs, fc, pr, pd, _, _ = R.fsim_float(list(r), list(d), MODEL[l], dp)
    return dict(fsim=fs, fsimc=fc, pc_r=pr, pc_d=pd, bar=R.derived_bar(pr, pd))


SLICE_LAYOUTS = (("yuv420p", 33, 67, 8), ("bgr24", 16, 16, 10))
SLICE_FRAMES = 7


def slice_pool(layout, h, w, depth):
    """seven distinct frame pairs: natural, noise, half and texture_flat under changing seeds -> (ref frames, dist frames)"""
    names = ("natural", "noise", "texture_flat", "half", "natural", "noise", "half")
    pairs = [pair(nm, layout, h, w, depth, seed=11 + k) for k, nm in enumerate(names)]
    return [p[0] for p in pairs], [p[1] for p in pairs]
