"""Localised probes at the tile seams of Gaussian SSIM, vf_ssim, MS-SSIM, VIF, ADM and motion: the planes, the probe centres, the
patch and the contents.  Integer-only and seeded, like hostile_cases.py.  One module, so that tests/test_probe_host.py (is the reference alone
stable on a probe, does the matrix have teeth?) and tests/test_gpu_probes.py (the parity matrix) see the same bytes.

A case is one batch: frame 0 is (ref, ref), frame k is (ref, dist_k), dist_k = ref with the patch of probe k - 1 applied.  The sums
behind every result are integers (2^-27 fixed point) or doubles of exact integers, so the windows the patch does not touch give
frame k bit for bit what they give frame 0, and  D(k) = N (value(frame 0) - value(frame k))  is the sum over the touched windows
alone (tests/probe_reference.py has the float64 / float32 side).  u = 2^(depth-8) is one 8-bit level.

ADM ("adm": plane A, "adm-b": the same kind on plane B) sums float32 cubes per thread and doubles from there on, in a fixed order per
tile: a tile the patch does not reach gives frame k the partial it gives frame 0, and D = num[s](frame 0) - num[s](frame k) moves
with the touched tiles alone.  A motion case has no distorted stream: it is the sequence base, p_1, base, p_2, .., base, and D is
the pair's sad itself - the outputs the blur of the patch does not reach contribute exactly 0."""
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

# ---- ADM -------------------------------------------------------------------------------------------------------------------------
# k_adm_scale: a workgroup owns TW x TH = 32 x 16 band samples and computes a halo of one around them (EW x EH = 34 x 18) from
# IW x IH = 70 x 38 input samples; scale s + 1 reads the a band of scale s; adm_region_of crops what is pooled to
# rows [top, bh - top), columns [left, bw - left) with left = int(0.1 bw - 0.5), top = int(0.1 bh - 0.5).
# Plane A, 320 x 640: the smallest round size at which the POOLED REGION of every scale has samples on both sides of a tile seam
# either way.
#   scale   band        tiles    region (top, bottom, left, right)     tile seams at band rows | columns     in pixels (x 2^(s+1))
#   0       160 x 320   10 x 10  (15, 145, 31, 289)                    16, 32, .. 144 | 32, 64, .. 288       rows 32 k, columns 64 k
#   1        80 x 160    5 x 5   ( 7,  73, 15, 145)                    16, .. 64      | 32, .. 128           rows 64 k, columns 128 k
#   2        40 x 80     3 x 3   ( 3,  37,  7,  73)                    16, 32         | 32, 64               rows 128 k, columns 256 k
#   3        20 x 40     2 x 2   ( 1,  19,  3,  37)                    16             | 32                   row 256, column 512
# Scale 3 pools band rows 16 .. 18 and columns 32 .. 36 of its second tiles (a 17 x 33 band would pool neither: its region ends at
# row 16 and column 30).  Pixel row 256 and pixel column 512 are seams of all four scales; 128 | 256 of scales 0 .. 2, 64 | 128 of
# scales 0 and 1, 32 | 64 of scale 0 alone.  Band sample i reads inputs 2 i - 1 .. 2 i + 2, so a 5 x 5 patch centred on pixel c
# reaches band samples (c - 4) / 2 .. (c + 3) / 2 of scale 0 - two or three on either side of a seam it straddles - and the mask
# carries it one sample further.
ADM_PLANE_A = (320, 640)
ADM_ROW, ADM_COL = 100, 200     # where the column / row probes sit: inside every region, on no seam, band row 50 / column 100
ADM_ROWS_A = (
    29, 32, 35,       # scale 0's seam of band rows 15 | 16: the patch above it (27 .. 31), astride it, below it (33 .. 37)
    61, 64, 67,       # band rows 31 | 32 of scale 0, 15 | 16 of scale 1
    125, 128, 131,    # seams of scales 0, 1, 2
    253, 256, 259,    # of all four scales; scale 3: band rows 15 | 16, the second tile row's rows 16 .. 18 are pooled
    80,               # band row 40 = row 8 of the tile at rows 32 .. 47 of scale 0: between the two samples a thread owns (r | r + 8)
    96,               # band row 24 of scale 1 = row 8 of its tile at rows 16 .. 31
    192,              # band row 24 of scale 2 = row 8 of its tile at rows 16 .. 31  (scale 3's row 8 is pixel row 128, above)
    30,               # band row 15, the first pooled row of scale 0: a top bound of 14 or 16 moves D
    288,              # band row 144, the last pooled row of scale 0
)
ADM_COLS_A = (
    61, 64, 67,       # scale 0's seam of band columns 31 | 32 (31 is also the first pooled column: the seam and the bound meet)
    125, 128, 131,    # band columns 63 | 64 of scale 0, 31 | 32 of scale 1
    253, 256, 259,    # seams of scales 0, 1, 2
    509, 512, 515,    # of all four scales; scale 3: band columns 31 | 32, columns 32 .. 36 are pooled
    62,               # band column 31, the first pooled column of scale 0
    576,              # band column 288, the last pooled one
)
ADM_BOTH_A = ((32, 64), (64, 128), (128, 256), (256, 512))      # astride a row seam and a column seam at once: four tiles meet
ADM_OUTSIDE = (5, 5)            # reaches band rows and columns 0 .. 4 of scale 0 and 0 .. 1 of scale 3: outside every region
# Plane B, 48 x 112: the pooled region reaches the band's edge, so the band-edge neighbour rule (-1 reads 1, n reads n - 1) and the
# DWT's mirrored index (k >= n reads 2 n - k - 1) are pooled, which plane A never does.
#   scale   band       tiles   region
#   0       24 x 56    2 x 2   (1, 23, 5, 51)       one column seam at band column 32 = pixel column 64, one row seam at band row 16
#   1       12 x 28    1 x 1   (0, 12, 2, 26)       the whole height: band rows -1 and 12 are read by the mask
#   2        6 x 14    1 x 1   (0,  6, 0, 14)       the whole band
#   3        3 x 7     1 x 1   (0,  3, 0,  7)       the whole band
ADM_PLANE_B = (48, 112)
ADM_PROBES_B = (
    (0, 0), (0, 111), (47, 0), (47, 111),       # the four corners (8 x 8): both border rules in both directions
    (0, 56), (47, 56), (24, 0), (24, 111),      # the middles of the four edges
    (24, 64),                                   # astride the only column seam (scale 0, band columns 31 | 32)
    (32, 30),                                   # astride the only row seam (scale 0, band rows 15 | 16)
    (24, 30),                                   # the interior
)
ADM_LEVELS = 4

# ---- motion ----------------------------------------------------------------------------------------------------------------------
# k_motion_sad on PLANE (140 x 264): a workgroup owns a 64 x 32 tile and loads it with an apron of R = 2 (68 x 36); 5 x 5 tiles,
# seams at columns 64, 128, 192, 256 and rows 32, 64, 96, 128 - the last tile column is 8 wide, the last tile row 12 high.  The
# borders reflect (index -i reads i, index n - 1 + i reads n - i).  A thread forms the four outputs 4 q .. 4 q + 3 of rows r and r + 16.
# The patch centred on c covers c - 2 .. c + 2 and its blur reaches c - 4 .. c + 4: centred two samples before a seam it ends on
# the seam's last own column and only its blur crosses (the far tile sees it through its apron alone); two samples after, the same
# from the other side.
MOTION_ROW, MOTION_COL = 50, 150      # where the column / row probes sit: on no seam
MOTION_COLS = (
    0, 263,             # the left and the right edge: the reflecting border
    62, 64, 66,         # the interior seam 63 | 64: through tile 0's right apron alone, astride, through tile 1's left apron alone
    254, 256, 258,      # the last seam 255 | 256; the blur of 258 reaches column 262, the tile behind it is 8 columns wide
    99, 100,            # 99 = 4 * 24 + 3 is the last output of a thread's quad, 100 the first of the next
)
MOTION_ROWS = (
    0, 139,             # the top and the bottom edge
    16,                 # rows 15 | 16: the two rows a thread owns (r and r + 16)
    62, 64, 66,         # the interior seam 63 | 64
    126, 128, 130,      # the last seam 127 | 128, the tile below it is 12 rows high
)
MOTION_BOTH = ((0, 0), (0, 263), (139, 0), (139, 263), (64, 64), (128, 256))    # the corners (8 x 8), and where four tiles meet
MOTION_QUANTUM = 2.0 ** -17     # the 2^-16 fixed point rounds every output sample's |d| by at most half a unit

PATCH, CORNER = 5, 8   # a 5 x 5 block centred on the probe; at the four corners an 8 x 8 block anchored at the corner (a 5 x 5 one
                       # is 3 x 3 after clipping and carries so little Gaussian weight that D is ~1e-3 and float32 noise)
# VIF takes 13 x 13: a 5 x 5 patch is 0.4 of a level-3 sample, D_64 of level 3 is ~1e-2 against a level total of 1900 and 21 of the
# 360 (probe, level) items are further than the cap allows from their own float32 run (up to 7e-2); with 13 x 13 - more than one
# level-3 sample either way - three are, all in the bottom row, whose patch lies below level 3's last row (17 * 8 = 136).  The patch
# still straddles every seam the probes were placed for.
PATCH_OF = {"vif": 13}
STEP = 64              # 8-bit levels added below mid-range, subtracted elsewhere: never clips

CONTENTS = ("noise", "smooth")
DEPTHS = {"gauss": (8, 10, 16), "ffmpeg": (8, 10), "ms": (8, 10), "vif": (8, 10), "adm": (8, 10), "adm-b": (8, 10), "motion": (8, 10, 16)}
VIF_LEVELS, MS_LEVELS = 4, 5


def probes(kind="gauss"):
    """every probe of a kind's plane, in a fixed order: probe k - 1 is frame k of the batch.  (row, column) in pixels; MS-SSIM:
    (row, column, tier) in the coordinates of level `tier`"""
    if kind == "ms":
        return [(r, c, t) for t, (rows, cols) in MS_TIERS.items() for r in rows for c in cols]
    if kind == "adm":       # not the full product: 38 frames of 320 x 640
        return ([(r, ADM_COL) for r in ADM_ROWS_A] + [(ADM_ROW, c) for c in ADM_COLS_A] + list(ADM_BOTH_A) +
                [(ADM_ROW, ADM_COL), ADM_OUTSIDE])
    if kind == "adm-b":
        return list(ADM_PROBES_B)
    if kind == "motion":
        return [(r, MOTION_COL) for r in MOTION_ROWS] + [(MOTION_ROW, c) for c in MOTION_COLS] + list(MOTION_BOTH)
    return [(r, c) for r in ROWS for c in COLS]


def tier(probe):
    return probe[2] if len(probe) > 2 else 0


def levels_of(kind, probe):
    """the levels a probe is judged on"""
    if kind in ("adm", "adm-b"):     # the scales on which the patch reaches a pooled sample: elsewhere D is exactly 0
        return [s for s, hit in enumerate(adm_reach(probe, plane_of(kind), patch_size(kind))) if hit]
    return range(VIF_LEVELS) if kind == "vif" else range(tier(probe) + 1) if kind == "ms" else range(1)


def plane_of(kind):
    return {"ms": MS_PLANE, "adm": ADM_PLANE_A, "adm-b": ADM_PLANE_B}.get(kind, PLANE)


def adm_dwt_index(i, n):
    """the inputs band sample i of a length-n pass reads: |2 i - 1|, 2 i, 2 i + 1, 2 i + 2, an index k >= n reads 2 n - k - 1"""
    return [(k if k < n else 2 * n - k - 1) for k in (abs(2 * i - 1), 2 * i, 2 * i + 1, 2 * i + 2)]


def adm_region(bh, bw):
    """adm_region_of (csrc/vqa_kernels.hpp): -> (top, bottom, left, right)"""
    left, top = int(bw * 0.1 - 0.5), int(bh * 0.1 - 0.5)
    return top, bh - top, left, bw - left


def _adm_axis_reach(lo, hi, n):
    """one axis: samples lo .. hi - 1 of a length-n signal differ -> per scale, whether a pooled band index reads one of them through
    the DWT (scale s + 1 reads the a band of scale s) or through the mask's neighbours (-1 reads 1, n reads n - 1)"""
    out, touched = [], set(range(lo, hi))
    for _ in range(ADM_LEVELS):
        bn = (n + 1) // 2
        touched = {i for i in range(bn) if touched.intersection(adm_dwt_index(i, n))}
        first = int(bn * 0.1 - 0.5)
        nb = lambda i: 1 if i < 0 else bn - 1 if i >= bn else i
        out.append(any(touched.intersection((nb(p - 1), p, nb(p + 1))) for p in range(first, bn - first)))
        n = bn
    return out


@functools.lru_cache(maxsize=None)
def adm_reach(probe, shape, size=PATCH):
    """-> per scale, whether the probe's patch reaches a pooled sample (both axes do)"""
    y0, y1, x0, x1 = patch_box(probe, shape, size)
    return tuple(a and b for a, b in zip(_adm_axis_reach(y0, y1, shape[0]), _adm_axis_reach(x0, x1, shape[1])))


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
ADM_CASES = [("gray", 8), ("gray", 10), ("bgr24", 8)]          # k_adm_scale<uint8_t>, <uint16_t>; three planes in one group (ch, a_out)
MOTION_CASES = [("gray", 8), ("gray", 10), ("gray", 16), ("bgr24", 8)]
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


def motion_batch(name, depth, lay="gray"):
    """one motion case: -> (frames [2 probes + 1, samples], planes, probed plane index): base, p_1, base, p_2, .., base - frame
    2 k - 1 against its predecessor is the pair (p_k, base), frame 2 k the same pair reversed"""
    h, w = plane_of("motion")
    planes, probed, size = layout(lay, h, w, depth)
    a = ref_plane("motion", name, depth)
    pr = probes("motion")
    frame = np.zeros(size, np.uint16 if depth > 8 else np.uint8)
    for i, p in enumerate(planes):
        _view(frame, p)[...] = a if i == probed else filler(p[1], p[0], depth, seed=i + 1)
    frames = np.repeat(frame[None], 2 * len(pr) + 1, axis=0)
    for k, probe in enumerate(pr):
        _view(frames[2 * k + 1], planes[probed])[...] = apply_patch(a, probe, depth, patch_size("motion"))
    return frames, planes, probed


def motion_touched(probe):
    """the output samples the blur of a probe's patch reaches: the box grown by the radius 2, inside the plane (81 for a whole
    5 x 5 patch)"""
    h, w = plane_of("motion")
    y0, y1, x0, x1 = patch_box(probe, (h, w), patch_size("motion"))
    return (min(y1 + 2, h) - max(y0 - 2, 0)) * (min(x1 + 2, w) - max(x0 - 2, 0))


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
#   adm (plane B), scale 3, noise, 8 bits.  The band is 3 x 7 and all of it is pooled; the eight probes kept have D_64 from 2.3e-2
#   (the top edge, (0, 56)) to 2.16, a factor of 94, while the float32 noise on D is the same for all of them in ABSOLUTE terms:
#   probe_reference.adm_sigma.  A scale-3 detail coefficient has gone through 8 filter passes of 4 multiply-adds on values of
#   magnitude 64 .. 256 (ulp 2^-17 .. 2^-16); the reference's own float32 run is e = 1.2e-5 rms from its float64 run per
#   coefficient.  x = |rf r| - thr carries rf e = 5.5e-7, num = sum_b cbrt(sum x^3) moves by S_b^(-2/3) sum x^2 dx over the 4 .. 12
#   touched samples, and frame 0 and frame k round independently there: sigma_D = 2.7e-7 .. 7.9e-7 over the eight probes, 7.3e-7
#   for (0, 56).  The reference's own draws agree with it where r comes from: (24, 30) is 1.09e-6 off (sigma 7.9e-7), (32, 30)
#   9.0e-7 (sigma 7.7e-7) - and on (0, 56) it drew 2.4e-8, 0.03 sigma.  So r = 4.29e-6 is set by the probes with D = 0.25 and 0.71
#   and 4 r = 1.7e-5 is 3.9e-7 = 0.54 sigma on (0, 56): any other order of the same float32 operations is expected beyond it.
#   (The GPU: 3.6e-5, 8.3e-7 = 1.1 sigma.)  Margin 23 puts the bar at 9.9e-5 = 3.1 sigma of (0, 56) - the most that
#   tests/test_probe_host.py allows a derived margin, a tenth of the cap - and 13 .. 505 sigma of the other seven.
MARGIN_OF = {("ms-cs", 0, "noise", 10): 7.0, ("adm-b", 3, "noise", 8): 23.0}
MAX_EXCLUDED_SHARE = 1.0 / 16  # of the (probe, level) items of a kind
_BELOW_LEVEL3 = ("the patch lies in pixel rows 132 .. 139 and level 3's last row holds rows 128 .. 135: D_64 is 3e-2 .. 2e-1 against a "
                 "level total of 1900 and the float32 run is %s away, against 8.6e-5 for the worst probe kept")
_SMALL_D = ("plane B's %s: the band is 3 x 7 and what the patch leaves on this scale nearly cancels, D_64 is down to %s of num[s] "
            "and the float32 run is up to %s away, against %s for the worst item kept on that scale")
EXCLUDED = {
    "gauss": {},
    "ffmpeg": {},
    "ms": {},
    "vif": {(3, (139, 5)): _BELOW_LEVEL3 % "1.8e-4", (3, (139, 256)): _BELOW_LEVEL3 % "1.4e-4", (3, (139, 263)): _BELOW_LEVEL3 % "2.5e-4"},
    "adm": {},
    "adm-b": {(3, (24, 111)): _SMALL_D % ("right edge", "5.2e-6", "8.5e-4", "4.9e-6"),
              (3, (47, 56)): _SMALL_D % ("bottom edge", "1.8e-5", "8.5e-4", "4.9e-6"),
              (3, (47, 111)): _SMALL_D % ("bottom right corner", "7.2e-6", "3.6e-4", "4.9e-6")},
    "motion": {},
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
    # ADM and motion: (axis, the probes' rows or columns, the scales it is a seam of)
    "adm": {"tile rows, pixel row 32": ("row", (29, 32, 35), (0,)), "tile rows, pixel row 64": ("row", (61, 64, 67), (0, 1)),
            "tile rows, pixel row 128": ("row", (125, 128, 131), (0, 1, 2)), "tile rows, pixel row 256": ("row", (253, 256, 259), (0, 1, 2, 3)),
            "tile columns, pixel column 64": ("col", (61, 64, 67), (0,)), "tile columns, pixel column 128": ("col", (125, 128, 131), (0, 1)),
            "tile columns, pixel column 256": ("col", (253, 256, 259), (0, 1, 2)),
            "tile columns, pixel column 512": ("col", (509, 512, 515), (0, 1, 2, 3)),
            "rows r | r + 8, scale 0": ("row", (80,), (0,)), "rows r | r + 8, scale 1": ("row", (96,), (1,)),
            "rows r | r + 8, scale 2": ("row", (192,), (2,)), "rows r | r + 8, scale 3": ("row", (125, 128, 131), (3,)),
            "first pooled row": ("row", (30,), (0,)), "last pooled row": ("row", (288,), (0,)),
            "first pooled column": ("col", (62,), (0,)), "last pooled column": ("col", (576,), (0,))},
    "adm-b": {"top": ("row", (0,), (0, 1, 2, 3)), "bottom": ("row", (47,), (0, 1, 2, 3)), "left": ("col", (0,), (0, 1, 2, 3)),
              "right": ("col", (111,), (0, 1, 2, 3)), "tile columns, pixel column 64": ("col", (64,), (0,)),
              "tile rows, pixel row 32": ("row", (32,), (0,))},
    "motion": {"tile columns 63 | 64": ("col", (62, 64, 66), (0,)), "tile columns 255 | 256": ("col", (254, 256, 258), (0,)),
               "tile rows 63 | 64": ("row", (62, 64, 66), (0,)), "tile rows 127 | 128": ("row", (126, 128, 130), (0,)),
               "rows r | r + 16": ("row", (16,), (0,)), "quads 99 | 100": ("col", (99, 100), (0,)),
               "top": ("row", (0,), (0,)), "bottom": ("row", (139,), (0,)), "left": ("col", (0,), (0,)), "right": ("col", (263,), (0,))},
}


def excluded(kind, level, probe):
    return (level, tuple(probe)) in EXCLUDED[kind]
