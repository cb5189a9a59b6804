"""Content and shapes shared by the host and the GPU tests of XPSNR (vqa_xpsnr_submit).

Content stays inside the sample range (a ramp that saturates at the peak would make every block flat).  On the 8-bit scale, times
2^(depth - 8) above: the left half of every plane is a gentle ramp - a triangle wave of x + y with slope 1 between 64 and 160,
exactly linear between its turning points, so the high-pass f is 0 there -, the right half is 128 +- 40 of noise.  A frame's
predecessor is the frame shifted by one column plus +- 2 of noise; the distortion is +- 6 of noise.

Shapes (h, w), the smallest at which the kernels can still go wrong: 16 x 16 (one tile, B = 4, 16 blocks); 33 x 67, both odd,
past the 64-column tile seam; 67 x 130, past both seams of the 64 x 32 tile; 135 x 241 for 4:2:0 with odd chroma (B = 8, chroma
blocks of 4); above 2048 x 1152 samples the 2 x 2 path: 1154 x 2050 and 1155 x 2051 (B = 68, 34 on the activity grid, blocks cut
across tiles, an ignored odd row and column)."""
import numpy as np

MONO_SHAPES = ((16, 16), (33, 67), (67, 130))
YUV_SHAPE = (135, 241)
SMALL = (33, 67)
BIG_SHAPES = ((1154, 2050), (1155, 2051))
DEPTHS = (8, 10, 16)


def dtype_of(depth):
    return np.uint16 if depth > 8 else np.uint8


def base_plane(h, w, depth, seed):
    """one plane as int64: ramp | noise"""
    u = 1 << (depth - 8)
    y, x = np.mgrid[0:h, 0:w]
    t = (x + y) % 192
    ramp = (64 + np.where(t <= 96, t, 192 - t)) * u
    rng = np.random.default_rng(seed)
    noise = 128 * u + rng.integers(-40 * u, 40 * u + 1, (h, w))
    return np.where(x < w // 2, ramp, noise).astype(np.int64)


def predecessor(p, depth, seed):
    """the frame before p: p shifted by one column (the first column repeated) plus +- 2 of noise"""
    u, peak = 1 << (depth - 8), (1 << depth) - 1
    rng = np.random.default_rng(seed)
    s = np.concatenate([p[:, :1], p[:, :-1]], axis=1)
    return np.clip(s + rng.integers(-2 * u, 2 * u + 1, p.shape), 0, peak)


def distorted(p, depth, seed):
    u, peak = 1 << (depth - 8), (1 << depth) - 1
    rng = np.random.default_rng(seed)
    return np.clip(p + rng.integers(-6 * u, 6 * u + 1, p.shape), 0, peak)


def plane_sizes(h, w, chroma):
    """(height, width) of every plane of a layout: "mono" | "420" | "422" | "444" """
    if chroma == "mono":
        return [(h, w)]
    cw = (w + 1) // 2 if chroma in ("420", "422") else w
    ch = (h + 1) // 2 if chroma == "420" else h
    return [(h, w), (ch, cw), (ch, cw)]


def clip(n, h, w, chroma="mono", depth=8, seed=0):
    """-> (ref, dist, prev0): n frames as lists of int64 planes each, prev0 (a list of planes) the frame before frame 0.  The
    LAST frame is the clean content; every frame's predecessor is that frame shifted by one column plus +- 2 of noise, so the
    chain is built backwards from it"""
    sizes = plane_sizes(h, w, chroma)
    seq = [[base_plane(ph, pw, depth, seed * 1000 + j) for j, (ph, pw) in enumerate(sizes)]]
    for i in range(n):
        seq.insert(0, [predecessor(p, depth, seed * 1000 + 100 * (i + 1) + j) for j, p in enumerate(seq[0])])
    ref = seq[1:]
    dist = [[distorted(p, depth, seed * 1000 + 500 + 10 * i + j) for j, p in enumerate(fr)] for i, fr in enumerate(ref)]
    return ref, dist, seq[0]


def pack(frames, depth):
    """lists of planes -> the planar [n, samples] array of the layout (planes follow each other without padding)"""
    return np.stack([np.concatenate([p.reshape(-1) for p in fr]) for fr in frames]).astype(dtype_of(depth))


def matrix():
    """(chroma, (h, w), depth) of the small parity cases: every mono shape at 8 bits, 33 x 67 mono at 10 and 16, 4:2:0 at
    135 x 241 at 8 and 10, 4:2:2 and 4:4:4 at 33 x 67"""
    out = [("mono", s, 8) for s in MONO_SHAPES] + [("mono", SMALL, d) for d in DEPTHS if d != 8]
    out += [("420", YUV_SHAPE, 8), ("420", YUV_SHAPE, 10), ("422", SMALL, 8), ("444", SMALL, 8), ("444", SMALL, 16)]
    return out
