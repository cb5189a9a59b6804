"""The clips of the VCA tests (tests/test_vca_host.py, tests/test_gpu_vca*.py): the smallest shapes at which k_vca_blocks can go
wrong - one block, remainders on either side, a chroma plane of one row of blocks, an odd row stride, every depth - and the
content kinds: noise, a ramp, flat fields at both range ends, a flat field with sparse single-sample changes (where the DC leaks
into the AC terms unless it is taken off first) and a static clip."""
import numpy as np

CONTENT = ("noise", "ramp", "flat0", "flatpeak", "sparse", "static")
# (chroma, (h, w), depth)
SHAPES = (("mono", (32, 32), 8), ("mono", (33, 65), 8), ("mono", (63, 95), 8), ("420", (64, 96), 8), ("420", (70, 134), 8),
          ("444", (40, 72), 10), ("444", (40, 72), 12), ("444", (40, 72), 16), ("mono", (96, 160), 16))


def plane_sizes(h, w, chroma):
    if chroma == "mono":
        return [(h, w)]
    if chroma == "444":
        return [(h, w)] * 3
    assert chroma == "420"
    return [(h, w), ((h + 1) // 2, (w + 1) // 2), ((h + 1) // 2, (w + 1) // 2)]


def plane(kind, h, w, depth, rng, i=0):
    peak = (1 << depth) - 1
    if kind == "noise":
        return rng.integers(0, peak + 1, (h, w)).astype(np.int64)
    if kind == "ramp":
        y, x = np.mgrid[0:h, 0:w]
        return ((x * 3 + y * 5 + 7 * i) * (peak // 255 if depth > 8 else 1) % (peak + 1)).astype(np.int64)
    if kind == "flat0":
        return np.zeros((h, w), np.int64)
    if kind == "flatpeak":
        return np.full((h, w), peak, np.int64)
    if kind == "sparse":
        p = np.full((h, w), peak - 1 - i, np.int64)
        k = max(1, h * w // 700)
        p[rng.integers(0, h, k), rng.integers(0, w, k)] -= rng.integers(1, 4, k)
        return p
    raise ValueError(kind)


def clip(kind, n, h, w, chroma, depth, seed):
    """-> (frames, prev0): frames = n lists of planes (int64 [ph, pw]); prev0 = one more such list, the frame before frame 0"""
    rng = np.random.default_rng(seed)
    sizes = plane_sizes(h, w, chroma)
    if kind == "static":
        one = [plane("noise", ph, pw, depth, rng) for ph, pw in sizes]
        return [one] * n, one
    fr = [[plane(kind, ph, pw, depth, rng, i) for ph, pw in sizes] for i in range(n + 1)]
    return fr[1:], fr[0]


def pack(frames, depth):
    """lists of planes -> [n, samples] uint8 / uint16, the planes one after the other without padding"""
    dt = np.uint16 if depth > 8 else np.uint8
    return np.stack([np.concatenate([p.reshape(-1) for p in f]).astype(dt) for f in frames])


def pack_padded(frames, depth, pad):
    """as pack, with `pad` more samples at the end of every row -> ([n, samples], plane tuples for Engine calls)"""
    dt = np.uint16 if depth > 8 else np.uint8
    bps = np.dtype(dt).itemsize
    rows, planes, off = [], [], 0
    for p in frames[0]:
        ph, pw = p.shape
        tup = (pw, ph, off, (pw + pad) * bps, bps) + ((depth,) if depth > 8 else ())
        planes.append(tup)
        off += ph * (pw + pad) * bps
    for f in frames:
        rows.append(np.concatenate([np.pad(p, ((0, 0), (0, pad)), constant_values=3).reshape(-1) for p in f]).astype(dt))
    return np.stack(rows), planes
