"""Hostile content: the plane pairs and BGR frames on which kernels go wrong while natural texture and uniform noise pass - flat
fields at either end of the range (fp32 cancellation of a variance against C2), anti-correlated pairs (negative totals through the
fixed-point sums), faint texture around VIF's s1 = 2, equal SADs (the tie-break by the smaller d^2), Sobel magnitudes on and
beside Canny's thresholds, 0 against the maximum (the accumulators' ends).  Integer-only and seeded, like synth.py.  One module,
so that tests/test_hostile_host.py (is the reference alone stable on a content?) and tests/test_gpu_hostile.py (the parity
matrix) see the same bytes.  u = 2^(depth-8) is one 8-bit level, L = 2^depth - 1."""
import numpy as np

# ---- plane pairs --------------------------------------------------------------------------------------------------------
PAIRS = ("bright_flat", "dark_flat", "checker_inv", "checker2_noisy", "step_shift", "faint1.4", "faint2.83")
ENDS = "full_vs_zero"          # vf_ssim, SSE, the motion feature and SI/TI only: a plane without variance says nothing elsewhere
DEPTHS = (8, 10, 16)
# ADM takes the noisy checkerboard with 3-px cells: db2's low-pass has a zero at Nyquist, so one level down a 2-px checkerboard
# leaves h and v bands that are rounding noise alone and the angle test of the decoupling compares noise with noise - in float32
# the reference flips samples on almost every seed (1.5e-4 .. 1.6e-2 at 163x201).  A period of 6 never lands on Nyquist.
PAIRS_OF = {"ssim": PAIRS, "vif": PAIRS, "adm": tuple("checker3_noisy" if n == "checker2_noisy" else n for n in PAIRS)}
# what tests/test_hostile_host.py finds unstable in the reference's own float32 run: (content, depth) left out of a metric's
# matrix by name ("hostile content", has the deviations)
EXCLUDED = {
    "ssim": (),
    "vif": (("step_shift", 16),),
    "adm": (("bright_flat", 8), ("dark_flat", 8)),
}
MAX_EXCLUDED = 2               # of the seven pair contents (the two faint amplitudes are one), per metric and depth
SHAPES = {"ssim": [(67, 259)], "vif": [(47, 35), (163, 201)], "adm": [(47, 35), (163, 201)]}


def content_of(name):
    return "faint" if name.startswith("faint") else name


def pair(name, h, w, depth, seed=0):
    """-> (ref, dist) int64 [h, w] planes of `depth` bits"""
    u, L = 1 << (depth - 8), (1 << depth) - 1
    rng = np.random.default_rng(1000 * depth + seed)
    y, x = np.mgrid[0:h, 0:w]
    low = rng.integers(0, u, (h, w)) if depth > 8 else 0             # the low bits carry content too
    one = rng.integers(-1, 2, (h, w)) * u                             # a distortion of one level
    if name == "bright_flat":
        r = L - ((x + y) % 4) * u - low
        return r, np.clip(r + one, 0, L)
    if name == "dark_flat":
        r = ((x + y) % 4) * u + low
        return r, np.clip(r + one, 0, L)
    if name == "checker_inv":
        r = ((x + y) & 1) * L
        return r, L - r
    if name in ("checker2_noisy", "checker3_noisy"):
        c = int(name[7])                                              # the cell size
        r = (((x // c) + (y // c)) & 1) * L
        return r, np.clip(r + rng.integers(-40, 41, (h, w)) * u, 0, L)
    if name == "step_shift":
        return np.where(x < w // 2, 0, L), np.where(x < w // 2 + 1, 0, L)
    if name.startswith("faint"):
        a = float(name[5:])
        r = 128 * u + np.rint(a * u * np.sin(x / 2.0) * np.cos(y / 3.0)).astype(np.int64)
        return r, r + one
    if name == ENDS:
        return np.full((h, w), L, np.int64), np.zeros((h, w), np.int64)
    raise KeyError(name)


def natural_pair(h, w, depth, seed=0):
    """the suite's ordinary content: synth.s_natural plus a few levels of noise"""
    from rtvqa_amd import synth
    u, L = 1 << (depth - 8), (1 << depth) - 1
    rng = np.random.default_rng(seed)
    r = synth.s_natural(1, max(h, 32), max(w, 32), seed=seed)[0, :h, :w, seed % 3].astype(np.int64) * u
    if depth > 8:
        r = r + rng.integers(0, u, r.shape)
    return r, np.clip(r + rng.integers(-3, 4, r.shape) * u, 0, L)


def frames(names, h, w, depth, chroma="mono", seed=0):
    """one frame pair per name, every plane of the layout filled with that content at the plane's own size
    -> (ref, dist [n, samples] uint8 / uint16, planes)"""
    from rtvqa_amd.engine import yuv_planes
    names = [names] if isinstance(names, str) else list(names)
    planes = yuv_planes(h, w, chroma, depth)
    dt = np.uint16 if depth > 8 else np.uint8
    out = [[], []]
    for name in names:
        parts = [natural_pair(p[1], p[0], depth, seed + k) if name == "natural" else pair(name, p[1], p[0], depth, seed + k)
                 for k, p in enumerate(planes)]
        for o, j in zip(out, (0, 1)):
            o.append(np.concatenate([np.asarray(pt[j]).reshape(-1) for pt in parts]))
    return np.stack(out[0]).astype(dt), np.stack(out[1]).astype(dt), planes


def clip(name, h, w, depth, chroma="mono", seed=0):
    """the pair as two consecutive frames of one stream (the motion feature, SI / TI): -> (frames [2, samples], planes)"""
    r, d, planes = frames(name, h, w, depth, chroma, seed)
    return np.concatenate([r, d]), planes


def plane_of(frame, p):
    """plane tuple p of one flat frame as int64 [h, w]"""
    pw, ph, off, rs, step = p[:5]
    isz = frame.dtype.itemsize
    return np.lib.stride_tricks.as_strided(frame[off // isz:], shape=(ph, pw), strides=(rs, step)).astype(np.int64)


# one 4:2:0 case per metric: the chroma planes carry the content at their own (halved, odd) size
YUV420 = {"ssim": ("dark_flat", 10, 67, 259), "vif": ("faint2.83", 8, 47, 35), "adm": ("checker3_noisy", 16, 47, 35)}


def cases(metric):
    """every (name, depth, h, w, chroma) of a metric's GPU matrix"""
    out = [(n, d, h, w, "mono") for h, w in SHAPES[metric] for n, d in matrix(metric)]
    return out + [YUV420[metric] + ("420",)]


def case_planes(metric):
    """every (tag, ref plane, dist plane, depth) the GPU matrix of a metric compares"""
    for n, depth, h, w, chroma in cases(metric):
        r, d, planes = frames(n, h, w, depth, chroma)
        for k, p in enumerate(planes):
            yield "%s %d bits %dx%d %s plane %d" % (n, depth, h, w, chroma, k), plane_of(r[0], p), plane_of(d[0], p), depth


def matrix(metric):
    """every (name, depth) of a metric's GPU matrix: the pair contents less the exclusions"""
    return [(n, d) for d in DEPTHS for n in PAIRS_OF[metric] if (content_of(n), d) not in EXCLUDED[metric]]


# ---- BGR frames, 8 bits (B = G = R: the gray plane is the plane) ---------------------------------------------------------
SAD_TIES = ("stripes3_v", "stripes3_h", "flat_step")
CANNY = ("canny_steps", "diag45", "lines1", "checker2")
DEGENERATE = ("zeros", "full", "checker8", "vstep", "ramp")
COMPLEXITY = SAD_TIES + ("zero_full",) + CANNY + DEGENERATE
STEP_HEIGHTS = (24, 25, 26, 49, 50, 51)        # Sobel L1 = 4 d on a straight step: 96, 100, 104, 196, 200, 204
BGR_SHAPES = [(48, 80), (37, 53)]


def _staircase(n, heights, budget):
    """a step every 8 samples, heights cycling, upwards while the level stays within the budget, else downwards"""
    v, cur = np.zeros(n, np.int64), 0
    for k, at in enumerate(range(8, n - 7, 8)):
        d = heights[k % len(heights)]
        cur = cur + d if cur + d <= budget else cur - d
        assert 0 <= cur <= budget
        v[at:] = cur
    return v


def gray_pair(name, h, w):
    """-> (prev, curr) uint8 [h, w] gray planes"""
    y, x = np.mgrid[0:h, 0:w]
    pat = np.array([40, 120, 200])
    if name == "stripes3_v":       # curr[x] = prev[x + dx] for dx = 2, -1, 5, -4 and any dy: SAD 0 at all of them
        return pat[x % 3].astype(np.uint8), pat[(x + 2) % 3].astype(np.uint8)
    if name == "stripes3_h":
        return pat[y % 3].astype(np.uint8), pat[(y + 2) % 3].astype(np.uint8)
    if name == "flat_step":
        return np.full((h, w), 100, np.uint8), np.full((h, w), 140, np.uint8)
    if name == "zero_full":
        return np.zeros((h, w), np.uint8), np.full((h, w), 255, np.uint8)
    if name == "checker2":         # against its inverse
        c = ((((x >> 1) + (y >> 1)) & 1) * 255).astype(np.uint8)
        return 255 - c, c
    if name == "canny_steps":      # steps along x (vertical edges) plus steps along y (horizontal edges), 175 + 80 = 255
        c = _staircase(w, STEP_HEIGHTS, 175)[None, :] + _staircase(h, STEP_HEIGHTS[::-1], 80)[:, None]
    elif name == "diag45":         # |gx| = |gy| along the edge: the boundary between the NMS sectors
        c = np.where(x + y < (h + w) // 2, 255, 0)
    elif name == "lines1":
        c = np.where((y % 7 == 3) | (x % 9 == 4), 255, 0)
    elif name in DEGENERATE:       # static
        from rtvqa_amd import synth
        c = synth.s_degenerate(h, w)[name][..., 0]
        return c.copy(), c.copy()
    else:
        raise KeyError(name)
    c = c.astype(np.uint8)
    return np.roll(c, (1, 2), (0, 1)), c       # the frame before: the same content moved by (1, 2)


def bgr(g):
    return np.repeat(np.asarray(g, np.uint8)[..., None], 3, axis=-1)


def bgr_sequence(h, w, names=COMPLEXITY):
    """every content's (prev, curr) back to back as one stream: -> uint8 [2 len(names), h, w, 3]; frame 2 k + 1 follows its own
    prev, frame 2 k follows the previous content's curr (a hostile pair of another kind)"""
    out = []
    for n in names:
        out.extend(bgr(g) for g in gray_pair(n, h, w))
    return np.stack(out)
