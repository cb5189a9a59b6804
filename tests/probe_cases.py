"""Localised probes at the tile seams of Gaussian SSIM, vf_ssim, MS-SSIM and VIF: the planes, the probe centres, the patch and the
contents.  Integer-only and seeded, like hostile_cases.py.  One module, so that tests/test_probe_host.py (is the reference alone
stable on a probe, does the matrix have teeth?) and tests/test_gpu_probes.py (the parity matrix) see the same bytes.

A case is one batch: frame 0 is (ref, ref), frame k is (ref, dist_k), dist_k = ref with the patch of probe k - 1 applied.  The sums
behind every result are integers (2^-27 fixed point) or doubles of exact integers, so the windows the patch does not touch give
frame k bit for bit what they give frame 0, and  D(k) = N (value(frame 0) - value(frame k))  is the sum over the touched windows
alone (tests/probe_reference.py has the float64 / float32 side).  u = 2^(depth-8) is one 8-bit level."""
import functools

import numpy as np

# ---- the planes ------------------------------------------------------------------------------------------------------------------
# 140 x 264 (h x w), the smallest plane that crosses every seam of the three kernel families at once:
#   k_ssim_gauss_p2   254 map columns in blocks of 246: two column blocks, the seam at map column 246; ssim_max_strips(140) = 2
#                     and ceil(130 / 2) = 65 rounds up to a strip of 72 = 3 * 24 rows: the seam at map row 72
#   vf_ssim           66 block columns = 65 sample columns: two waves of 64 lanes that overlap by one, sample column 63 (block
#                     columns 63 | 64, pixel column 252 | 256) is the last of wave 0; 35 block rows = 34 sample rows: two strips of
#                     FS_ROWS = 32, the seam at sample row 32 (pixel row 128)
#   VIF               level s has 64 x 16 tiles (k_vif_stats) and decimation tiles of 32: seams at plane column 64 * 2^s and row
#                     16 * 2^s; row 128 is a seam of all four levels and column 256 of levels 0, 1 and 2 (level 3 is 17 x 33: its
#                     row 16 begins a second tile row, its 33 columns are one tile wide and column 32 is the decimation's seam)
PLANE = (140, 264)
# probe centres, in pixels; map row / column m of Gaussian SSIM is the window over pixels m .. m + 10, centred at m + 5
ROWS = (
    0,      # the top edge: the corner patch (with column 0 / 263) and clipped patches, VIF's reflecting border
    5,      # the centre of map row 0: the first whole patch
    66,     # the patch ends at pixel 68: the last Gaussian windows it touches are map rows 58 .. 68, all of strip 0
    72,     # patch 70 .. 74: touches map rows 60 .. 74, both sides of the strip seam at map row 72
    77,     # the centre of map row 72, the first row of strip 1 (and of its 8-row LDS round trip and ring slot 0)
    83,     # patch 81 .. 85: touches map rows 71 .. 85 - the last row of strip 0 by its outermost tap alone
    128,    # patch 126 .. 130 straddles pixel row 128: vf_ssim's strip seam (sample rows 31 | 32) and a VIF tile seam of every level
    134,    # the centre of map row 129, the last one; below vf_ssim's seam
    139,    # the bottom edge
)
COLS = (
    0,      # the left edge
    5,      # the centre of map column 0
    127,    # patch 125 .. 129: straddles pixel column 128 - an 8-lane column group boundary (128 = 16 * 8) and a VIF tile
    128,    #   seam of levels 0 and 1; 128 puts the patch's centre on the other side of it
    240,    # patch 238 .. 242: touches map columns 228 .. 242, all of column block 0
    246,    # patch 244 .. 248: touches map columns 234 .. 248, both sides of the block seam at map column 246
    251,    # the centre of map column 246, the first of block 1; patch 249 .. 253 covers vf_ssim's block column 63 (252 .. 255)
    256,    # patch 254 .. 258 straddles pixel column 256: vf_ssim's wave overlap (block columns 63 | 64), VIF's seam of levels 0 .. 2
    258,    # the centre of map column 253, the last one
    263,    # the right edge
)

# 352 x 528 for MS-SSIM: level 0 has 518 map columns = three column blocks (seams at map columns 246 and 492) and
# ssim_max_strips(352) = 5 strips of 72 rows (seams at map rows 72, 144, 216, 288); level 1 (176 x 264) has 254 map columns = two
# blocks (seam at its map column 246) and two strips of 96 rows (seam at its map row 96); levels 2, 3, 4 are 88 x 132, 44 x 66 and
# 22 x 33: one block and one strip each, their only seams are the plane's edges.  Every level is even until the last, so the
# pyramid never pads.
MS_PLANE = (352, 528)
# The rule of ROWS / COLS scaled to each level's own seams: a probe of tier t is stated in the coordinates of level t and its patch
# is the 5 x 5 (corner: 8 x 8) block of level t, 5 * 2^t pixels wide.  It is judged on levels 0 .. t: one level further its patch is
# less than 5 samples wide and what is left of it at an edge is float32 noise (measured: D_64 down to 1e-8 at level 2 for a
# 5-pixel patch).  (rows, columns) per tier, as for ROWS / COLS: the edges, the centre of the first and of the last map row /
# column, and for a seam at map row / column m the probes m (the patch straddles it) and m + 5 (the centre of its first window).
MS_TIERS = {
    0: ((0, 5, 72, 77, 216, 221, 346, 351),       # map rows 72 and 216: strip 0 | 1 and the inner strips 2 | 3; map row 341 is the last
        (0, 5, 246, 251, 492, 497, 522, 527)),    # map columns 246 and 492: block 1 has a neighbour on either side; 517 is the last
    1: ((0, 5, 96, 101, 170, 175),                # level 1, 176 x 264: its strip seam at map row 96; map row 165 is the last
        (0, 5, 246, 251, 258, 263)),              # its block seam at map column 246; map column 253 is the last
    4: ((0, 5, 11, 16, 21),                       # level 4, 22 x 33, 12 x 23 windows: edges, first / last map centre, the middle
        (0, 5, 16, 27, 32)),
}

PATCH, CORNER = 5, 8   # a 5 x 5 block centred on the probe; at the four corners an 8 x 8 block anchored at the corner (a 5 x 5 one
                       # is 3 x 3 after clipping and carries so little Gaussian weight that D is ~1e-3 and float32 noise)
# VIF takes 13 x 13: a 5 x 5 patch is 0.4 of a level-3 sample, D_64 of level 3 is ~1e-2 against a level total of 1900 and 21 of the
# 360 (probe, level) items are further than the cap allows from their own float32 run (up to 7e-2); with 13 x 13 - more than one
# level-3 sample either way - three are, all in the bottom row, whose patch lies below level 3's last row (17 * 8 = 136).  The patch
# still straddles every seam the probes were placed for.
PATCH_OF = {"vif": 13}
STEP = 64              # 8-bit levels added below mid-range, subtracted elsewhere: never clips

CONTENTS = ("noise", "smooth")
DEPTHS = {"gauss": (8, 10, 16), "ffmpeg": (8, 10), "ms": (8, 10), "vif": (8, 10)}
VIF_LEVELS, MS_LEVELS = 4, 5


def probes(kind="gauss"):
    """every probe of a kind's plane, in a fixed order: probe k - 1 is frame k of the batch.  (row, column) in pixels; MS-SSIM:
    (row, column, tier) in the coordinates of level `tier`"""
    if kind == "ms":
        return [(r, c, t) for t, (rows, cols) in MS_TIERS.items() for r in rows for c in cols]
    return [(r, c) for r in ROWS for c in COLS]


def tier(probe):
    return probe[2] if len(probe) > 2 else 0


def levels_of(kind, probe):
    """the levels a probe is judged on"""
    return range(VIF_LEVELS) if kind == "vif" else range(tier(probe) + 1) if kind == "ms" else range(1)


def plane_of(kind):
    return MS_PLANE if kind == "ms" else PLANE


def patch_size(kind):
    return PATCH_OF.get(kind, PATCH)


def patch_box(probe, shape, size=PATCH):
    """-> (y0, y1, x0, x1), the rows y0 .. y1 - 1 and columns x0 .. x1 - 1 (in pixels) the patch of a probe covers"""
    (r, c), t = probe[:2], tier(probe)
    h, w = shape[0] >> t, shape[1] >> t
    if r in (0, h - 1) and c in (0, w - 1):
        box = (0 if r == 0 else h - CORNER, CORNER if r == 0 else h, 0 if c == 0 else w - CORNER, CORNER if c == 0 else w)
    else:
        k = size // 2
        box = (max(r - k, 0), min(r + k + 1, h), max(c - k, 0), min(c + k + 1, w))
    return tuple(v << t for v in box)


def patch_samples(probe, shape, size=PATCH):
    y0, y1, x0, x1 = patch_box(probe, shape, size)
    return (y1 - y0) * (x1 - x0)


def apply_patch(a, probe, depth, size=PATCH):
    """a copy of int64 plane a with the probe's patch: + 64 u where the sample is below mid-range, - 64 u elsewhere"""
    y0, y1, x0, x1 = patch_box(probe, a.shape, size)
    d = a.copy()
    blk = d[y0:y1, x0:x1]
    d[y0:y1, x0:x1] = np.where(blk < (1 << (depth - 1)), blk + (STEP << (depth - 8)), blk - (STEP << (depth - 8)))
    return d


def sse_of(probe, shape, depth, size=PATCH):
    """the exact SSE of (ref, dist_k): every patch sample differs by 64 u"""
    return patch_samples(probe, shape, size) * (STEP << (depth - 8)) ** 2


def dist_plane(kind, name, depth, probe):
    """the probed plane of frame (ref, dist_k)"""
    return apply_patch(ref_plane(kind, name, depth), probe, depth, patch_size(kind))


def content(name, h, w, depth, seed=0):
    """-> the int64 [h, w] reference plane of `depth` bits"""
    u, L = 1 << (depth - 8), (1 << depth) - 1
    rng = np.random.default_rng(7000 + 100 * depth + seed)
    low = rng.integers(0, u, (h, w)) if depth > 8 else 0                  # the low bits carry noise too (hostile_cases.pair)
    if name == "noise":
        return rng.integers(0, 256, (h, w)) * u + low
    if name == "smooth":     # low variance: the fp32 cancellation of the variance terms against C2 is in play
        y, x = np.mgrid[0:h, 0:w]
        g = 128 + np.rint(60 * np.sin(x / 9.0) * np.cos(y / 7.0)).astype(np.int64) + rng.integers(-6, 7, (h, w))
        return np.clip(g * u + low, 0, L)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def ref_plane(kind, name, depth):
    """the probed plane's reference samples (shared, read-only)"""
    h, w = plane_of(kind)
    a = content(name, h, w, depth)
    a.setflags(write=False)
    return a


def filler(h, w, depth, seed):
    """what the planes around the probed one hold (B and R of bgr24, Y and V of 4:2:0): noise of their own"""
    return content("noise", h, w, depth, seed=seed)


# ---- layouts ---------------------------------------------------------------------------------------------------------------------
# name -> (planes of the frame, index of the probed plane, frame samples).  The probed plane always holds ref_plane(): its D does not
# depend on the layout, only the kernel path does.  vf_ssim's launch (csrc/k_quality.hip, launch_quality_ffmpeg) picks its kernel
# from the descriptor alone, with base pointers and frame strides multiples of 8 here (the engine's allocations; frames of
# 36960 samples and more, padded to a multiple of 8 below):
#   gray        8 bits, offset 0, step 1, row stride 264: offset & 3 == 0 and step 1      -> k_ssim_ffmpeg_fast<1>
#   bgr24       three planes of step 3 at offsets 0, 1, 2, row stride 792 (a multiple of 4) -> k_ssim_ffmpeg_fast<3>
#   gray-off1   the plane one byte into the frame: offset & 3 != 0                          -> k_ssim_ffmpeg (the byte kernel)
#   gray        10 bits, offset 0, step 2, row stride 528 (a multiple of 8)                  -> k_ssim_ffmpeg16<true>
#   gray-off2   10 bits, the plane one sample (2 bytes) into the frame: offset & 7 == 2    -> k_ssim_ffmpeg16<false>
# tests/layout_cases.ffmpeg_kernels restates that choice; tests/test_probe_host.py asserts each of the five is reached.
FFMPEG_PATHS = {("gray", 8): "fast<1>", ("bgr24", 8): "fast<3>", ("gray-off1", 8): "ffmpeg", ("gray", 10): "ffmpeg16<true>",
                ("gray-off2", 10): "ffmpeg16<false>"}
GAUSS_CASES = [("gray", 8), ("gray", 10), ("gray", 16), ("bgr24", 8), ("yuv420-u", 10)]
FFMPEG_CASES = list(FFMPEG_PATHS)


def layout(name, h, w, depth):
    """-> (planes, probed plane index, frame size in samples) of layout `name` around an h x w probed plane"""
    bps = 2 if depth > 8 else 1
    tail = (depth,) if depth > 8 else ()
    if name == "gray":
        return [(w, h, 0, w * bps, bps) + tail], 0, h * w
    if name in ("gray-off1", "gray-off2"):     # one sample in front of the plane, seven behind: the frame stride stays a multiple of 8
        return [(w, h, bps, w * bps, bps) + tail], 0, h * w + 8
    if name == "bgr24":                        # the patch in G: B and R ride in the same launch
        return [(w, h, c, 3 * w, 3) for c in range(3)], 1, 3 * h * w
    if name == "yuv420-u":                     # the patch in U: the luma plane is 2 h x 2 w
        from rtvqa_amd.engine import yuv_planes
        return yuv_planes(2 * h, 2 * w, "420", depth), 1, 6 * h * w
    raise KeyError(name)


def _view(frame, p):
    w, h, off, rs, step = p[:5]
    isz = frame.dtype.itemsize
    return np.lib.stride_tricks.as_strided(frame[off // isz:], shape=(h, w), strides=(rs, step))


def batch(kind, name, depth, lay="gray"):
    """one case: -> (ref, dist [1 + probes, samples] uint8 / uint16, planes, probed plane index); every ref frame is the same"""
    h, w = plane_of(kind)
    planes, probed, size = layout(lay, h, w, depth)
    a = ref_plane(kind, name, depth)
    pr = probes(kind)
    frame = np.zeros(size, np.uint16 if depth > 8 else np.uint8)
    for i, p in enumerate(planes):
        _view(frame, p)[...] = a if i == probed else filler(p[1], p[0], depth, seed=i + 1)
    ref = np.repeat(frame[None], 1 + len(pr), axis=0)
    dist = ref.copy()
    for k, probe in enumerate(pr):
        _view(dist[k + 1], planes[probed])[...] = apply_patch(a, probe, depth, patch_size(kind))
    return ref, dist, planes, probed


# ---- exclusions ------------------------------------------------------------------------------------------------------------------
# (kind, level, probe) left out of every group of that kind and level by name: items whose D_64 nearly cancels, so that the
# reference's own float32 run is further than the cap allows from its float64 run (tests/test_probe_host.py measures each and holds
# the share below MAX_EXCLUDED_SHARE; DESIGN.md section 3, "probe parity", has the figures)
CAP = 1e-3                     # no group's bar may exceed it
FLOOR = 1e-5                   # nor fall below this
MARGIN = 4.0                   # bar = MARGIN * the reference's own float32-to-float64 ratio
# A group whose margin is wider, with the arithmetic it comes from.  (kind, level, content, depth) -> margin.
#   ms-cs, level 0, noise, 10 bits.  cs = A / B, A = 2 s_xy + C2, B = s_xx + s_yy + C2.  Centred uniform noise has E x^2 = 5461, so
#   each second moment lies in [4096, 8192), where a float32 ulp is 2^-11 = 4.9e-4.  A moment is 22 multiply-adds (11 taps down, 11
#   across) that each round the partial sum by up to half an ulp: a random walk of sqrt(22 / 12) = 1.35 ulp = 6.6e-4 rms.  A carries
#   twice the error of s_xy and B those of s_xx and s_yy: sqrt(4 + 1 + 1) * 6.6e-4 / B = 1.5e-7 per window with B = 10981.  (Frame 0
#   has A = B from the same operations on the same numbers; its windows are 1 to the quotient's last bit.)  The probe the GPU is
#   furthest on, (5, 527), is cut by the right edge and touches W = 8 x 3 windows: sigma_D = 1.5e-7 sqrt(24) = 7.2e-7 against
#   D_64 = 4.23e-2, 1.7e-5 relative.  The group's r = 1.02e-5 is one NumPy draw of that noise at 0.6 sigma - the same level and
#   content at 8 bits drew 1.17e-5, Gaussian SSIM on the small plane 1.3 .. 2.4e-5 - so 4 r = 4.1e-5 is 2.4 sigma, and the largest of
#   the 64 tier-0 probes is expected near there whatever the order of evaluation (the GPU: 4.21e-5, 2.5 sigma).  Margin 7 puts the
#   bar at 7.2e-5 = 4.2 sigma of that probe, below the bars of its neighbours in the table (8.3e-5, 9.4e-5) and 14 times under the cap.
MARGIN_OF = {("ms-cs", 0, "noise", 10): 7.0}
MAX_EXCLUDED_SHARE = 1.0 / 16  # of the (probe, level) items of a kind
_BELOW_LEVEL3 = ("the patch lies in pixel rows 132 .. 139 and level 3's last row holds rows 128 .. 135: D_64 is 3e-2 .. 2e-1 against a "
                 "level total of 1900 and the float32 run is %s away, against 8.6e-5 for the worst probe kept")
EXCLUDED = {
    "gauss": {},
    "ffmpeg": {},
    "ms": {},
    "vif": {(3, (139, 5)): _BELOW_LEVEL3 % "1.8e-4", (3, (139, 256)): _BELOW_LEVEL3 % "1.4e-4", (3, (139, 263)): _BELOW_LEVEL3 % "2.5e-4"},
}

# the probes beside each seam, by row or column: a level of a kind must keep at least one probe of each (tests/test_probe_host.py)
SEAMS = {
    "gauss": {"strip seam, map row 72": ("row", (66, 72, 77, 83)), "block seam, map column 246": ("col", (240, 246, 251)),
              "lane group, column 128": ("col", (127, 128)), "top": ("row", (0, 5)), "bottom": ("row", (134, 139)),
              "left": ("col", (0, 5)), "right": ("col", (258, 263))},
    "ffmpeg": {"strip seam, sample row 32": ("row", (128, 134)), "wave overlap, sample column 63": ("col", (251, 256, 258)),
               "top": ("row", (0, 5)), "bottom": ("row", (134, 139)), "left": ("col", (0, 5)), "right": ("col", (258, 263))},
    "vif": {"tile row 128": ("row", (128, 134)), "tile column 128": ("col", (127, 128)), "tile column 256": ("col", (251, 256, 258)),
            "top": ("row", (0, 5)), "bottom": ("row", (134, 139)), "left": ("col", (0, 5)), "right": ("col", (258, 263))},
}


def excluded(kind, level, probe):
    return (level, tuple(probe)) in EXCLUDED[kind]
