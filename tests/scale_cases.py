"""The cases of tests/test_gpu_scale*.py: geometries against k_scale's 64 x 32 destination tile, layouts, content, and the
expected bytes - tests/scale_reference.resample fed the tables vqa_scale_tables built (so nothing depends on this machine's sin),
written into a canvas of pad bytes the way vqa_scale_submit writes the caller's destination."""
import functools

import numpy as np

import scale_reference as R

FILTERS = R.FILTERS
FILL = 0xA5   # what the destination holds before the resampler writes it
TILE_W, TILE_H = 64, 32

# (in h, in w, out h, out w, what it is there for); destination sizes are written w x h below, like the tile
GEOMETRIES = [
    (27, 48, 41, 72, "2/3 -> 1 (1.5x up); 72 x 41: one tile seam in each direction"),
    (41, 72, 27, 48, "1.5x down into one partial tile; the source spans a seam's worth of columns"),
    (22, 43, 33, 65, "non-integer odd ratio up; 65 x 33: ONE sample past both seams"),
    (35, 65, 70, 130, "2x up; 130 x 70: two seams in each direction, two samples past the second"),
    (18, 32, 54, 96, "3x up; 96 x 54: a half tile right, 22 rows below the seam"),
    (31, 57, 70, 130, "non-integer ratio 2.28 / 2.26 up with odd source sizes"),
    (81, 144, 54, 96, "1.5x down"),
    (132, 260, 33, 65, "4x down: the widest footprint (lanczos: 25 taps, chunks of 16 source rows)"),
    (16, 16, 128, 128, "8x up from the smallest plane: every window is cut at a border"),
    (54, 96, 54, 64, "the vertical axis unchanged (copied)"),
    (31, 40, 45, 40, "the horizontal axis unchanged (copied)"),
]


def planes_of(layout, h, w, depth=8):
    """layout "420" | "444" | "mono" (planar, tight) or "bgr24" (packed, 8 bits) -> plane tuples"""
    from rtvqa_amd.engine import bgr_planes, yuv_planes
    return bgr_planes(h, w) if layout == "bgr24" else yuv_planes(h, w, layout, depth)


def padded(planes, row_pad=0, lead=0, frame_pad=0):
    """the same planes with `row_pad` samples behind every row, `lead` bytes before the first plane and `frame_pad` bytes
    behind the last -> (planes, frame bytes)"""
    depth = (int(planes[0][5]) if len(planes[0]) > 5 else 0) or 8
    isz = 2 if depth > 8 else 1
    if int(planes[0][4]) != isz:   # packed: the planes interleave and share their rows
        rs = int(planes[0][3]) + row_pad * int(planes[0][4])
        out = [(int(p[0]), int(p[1]), lead + int(p[2]), rs, int(p[4])) + tuple(p[5:]) for p in planes]
        return out, lead + int(planes[0][1]) * rs + frame_pad
    out, off = [], lead
    for p in planes:
        w, h = int(p[0]), int(p[1])
        rs = (w + row_pad) * isz
        out.append((w, h, off, rs, isz) + tuple(p[5:]))
        off += h * rs
    return out, off + frame_pad


def frame_bytes(planes):
    from rtvqa_amd.engine import planes_span
    return planes_span(planes)


def _view(frame_u8, p, isz):
    """plane p of one frame (a uint8 vector) as a strided [h, w] view of its samples"""
    w, h, off, rs, step = (int(v) for v in p[:5])
    base = frame_u8[off:]
    if isz == 2:
        base = base[:len(base) // 2 * 2].view("<u2")
        return np.lib.stride_tricks.as_strided(base, (h, w), (rs, step), writeable=True)
    return np.lib.stride_tricks.as_strided(base, (h, w), (rs, step), writeable=True)


def content(n, planes, fb, depth, seed, above_peak=False):
    """n frames [n, fb] uint8 bytes holding `planes`: frame 0 noise, frame 1 0 / peak runs (overshoot clips at both ends),
    frame 2 flat at a level of its own per plane, later frames noise again.  above_peak: the noise of a 9..15-bit layout fills
    the whole uint16 range, and the runs are 0 / 65535."""
    isz = 2 if depth > 8 else 1
    peak = (1 << depth) - 1
    top = 65535 if (above_peak and isz == 2) else peak
    rng = np.random.default_rng(seed)
    out = np.full((n, fb), 0x3C, np.uint8)
    for i in range(n):
        for j, p in enumerate(planes):
            v = _view(out[i], p, isz)
            h, w = v.shape
            if i % 3 == 0:
                v[...] = rng.integers(0, top + 1, (h, w))
            elif i % 3 == 1:
                v[...] = rng.integers(0, 2, ((h + 2) // 3, (w + 2) // 3)).repeat(3, 0).repeat(3, 1)[:h, :w] * top
            else:
                v[...] = (0, peak, peak // 2 + 1, 1)[(i // 3 + j) % 4]
    return out


@functools.lru_cache(maxsize=None)
def c_tables(filter, n_in, n_out):
    """the tables the LIBRARY builds for one axis"""
    from rtvqa_amd.engine import scale_tables
    return scale_tables(filter, n_in, n_out)


def expected(frames_u8, planes, out_planes, out_fb, filter, depth, fill=FILL):
    """what the destination must hold, pad bytes included: [n, out_fb] uint8"""
    isz = 2 if depth > 8 else 1
    n = frames_u8.shape[0]
    out = np.full((n, out_fb), fill, np.uint8)
    for i in range(n):
        for p, q in zip(planes, out_planes):
            src = np.array(_view(np.array(frames_u8[i]), p, isz))
            h, w = src.shape
            oh, ow = int(q[1]), int(q[0])
            tx = c_tables(filter, w, ow) if ow != w else None
            ty = c_tables(filter, h, oh) if oh != h else None
            _view(out[i], q, isz)[...] = R.resample(src, oh, ow, depth, tx, ty)
    return out


def as_samples(frames_u8, depth):
    """the byte frames as the engine takes them: uint8, or uint16 above 8 bits"""
    return frames_u8 if depth <= 8 else np.ascontiguousarray(frames_u8).view("<u2")


def run(engine, frames_u8, planes, out_planes, out_fb, filter, depth, mem="host", fill=FILL):
    """the resampler into a destination prefilled with `fill` -> the whole destination as [n, out_fb] uint8"""
    from rtvqa_amd.engine import DeviceFrames
    n = frames_u8.shape[0]
    isz = 2 if depth > 8 else 1
    canvas = engine.upload(as_samples(np.full((n, out_fb), fill, np.uint8), depth))
    dst = DeviceFrames(canvas.ptr, n, 1, out_fb // isz, frame_stride=out_fb, owner=canvas, channels=1, itemsize=isz)
    src = as_samples(frames_u8, depth)
    keep = None
    if mem == "device":
        src = keep = engine.upload(src)
    elif mem == "pinned":
        keep = engine.alloc_pinned(src.shape, src.dtype)
        keep[...] = src
        src = keep
    try:
        res = engine.scale(src, planes, out_planes, filter, out=dst, frame_bytes=frames_u8.shape[1])
        got = engine.download(res, np.uint8)
    finally:
        if mem == "pinned":
            engine.free_pinned(keep)
        elif mem == "device":
            keep._owner.free()
        canvas._owner.free()
    return got
