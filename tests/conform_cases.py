"""The cases of tests/test_gpu_conform*.py: layouts, sizes against k_conform_copy's 16-byte granules and row bands, windows,
frame indices, tables and matrices; byte canvases built the way vqa_conform_submit writes the caller's destination, and the
expected bytes from tests/conform_reference.py."""
import numpy as np

import conform_reference as R
import scale_cases as SC

FILL = 0xA5   # what the destination holds before the kernel writes it
LAYOUTS = ("420", "422", "444", "mono", "bgr24")
DEPTHS = (8, 10, 12, 16)
# destination luma sizes (h, w): 16 x 16 is ONE 16-byte vector a row at 8 bits (and the smallest plane: 8 x 8 chroma, half a
# vector); 33 x 47 is odd on both axes, every row ends inside a vector; 64 x 80 is five whole vectors a row and, at 8 bits,
# chroma rows of 40 that end inside the third; 18 x 130 is two samples over eight vectors, few rows.  A workgroup's band is 64 KB
# of destination bytes: all of these are one band (test_more_rows_than_one_band covers the seam).
SIZES = ((16, 16), (33, 47), (64, 80), (18, 130))
# window corners (y0, x0) in the luma: x0 0 .. 5 are the byte phases 0 .. 5 (8 bits) and 0 .. 10 (16 bits) of the realign path,
# y0 0 .. 3
ORIGINS = ((0, 0), (1, 1), (2, 2), (3, 3), (0, 4), (1, 5))
INDICES = (None, (2, 1, 0), (2, 0, 0), (1, 1, 2, 0, 1))   # identity; reversed; a repeat and a drop; n_out != n_in


def layout_depths():
    return [(l, d) for l in LAYOUTS for d in DEPTHS if l != "bgr24" or d == 8]


def sub_of(layout):
    """the chroma shifts (sy, sx)"""
    return {"420": (1, 1), "422": (0, 1)}.get(layout, (0, 0))


def source_size(out_hw, origin, extra=(2, 3)):
    return out_hw[0] + origin[0] + extra[0], out_hw[1] + origin[1] + extra[1]


def plane_origins(layout, origin):
    """the luma corner -> one corner per plane, the chroma's shifted down as conform.plan does"""
    sy, sx = sub_of(layout)
    n = 1 if layout == "mono" else 3
    return [tuple(origin)] + [(origin[0] >> sy, origin[1] >> sx)] * (n - 1)


def step2_planes(h, w, depth, count=1):
    """`count` planes that interleave with a pixel step of `2` samples: one (the gather path) or two (an NV12-like pair)"""
    isz = 2 if depth > 8 else 1
    return [(w, h, c * isz, 2 * w * isz, 2 * isz) + ((depth,) if depth > 8 else ()) for c in range(count)]


def random_lut(n_planes, depth, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 1 << depth, (n_planes, 1 << depth)).astype(np.uint16 if depth > 8 else np.uint8)


def clipping_matrix(depth):
    """coefficients that drive every plane through both clips on noise, negative offsets among them (2^-16 fixed point)"""
    s = 1 << (depth - 8)
    m = np.array([[1.5, 0.375, -0.25, -40.0 * s], [-0.5, 1.25, 0.125, 30.0 * s], [0.25, -0.375, 2.0, -100.0 * s]])
    return np.floor(m * 65536 + 0.5).astype(np.int64)


def split(frames_u8, planes, depth):
    """byte frames [n, fb] -> a list of frames, each a list of [h_p, w_p] sample arrays (copies)"""
    isz = 2 if depth > 8 else 1
    return [[np.array(SC._view(np.array(f), p, isz)) for p in planes] for f in frames_u8]


def expected(frames_u8, planes, out_planes, out_fb, depth, origin=None, index=None, lut=None, matrix=None, fill=FILL):
    """what the destination must hold, pad bytes included: [n_out, out_fb] uint8"""
    isz = 2 if depth > 8 else 1
    sizes = [(int(q[1]), int(q[0])) for q in out_planes]
    res = R.conform(split(frames_u8, planes, depth), sizes, origin, index, lut, matrix, depth)
    out = np.full((len(res), out_fb), fill, np.uint8)
    for j, fr in enumerate(res):
        for q, a in zip(out_planes, fr):
            SC._view(out[j], q, isz)[...] = a
    return out


def run(engine, frames_u8, planes, out_planes, out_fb, depth, origin=None, index=None, lut=None, matrix=None, mem="host",
        fill=FILL, wait=True):
    """vqa_conform_submit into a destination prefilled with `fill` -> the whole destination as [n_out, out_fb] uint8 (wait=False:
    the DeviceFrames, the batch still pending)"""
    from rtvqa_amd.engine import DeviceFrames
    n_out = frames_u8.shape[0] if index is None else len(index)
    isz = 2 if depth > 8 else 1
    canvas = engine.upload(SC.as_samples(np.full((n_out, out_fb), fill, np.uint8), depth))
    dst = DeviceFrames(canvas.ptr, n_out, 1, out_fb // isz, frame_stride=out_fb, owner=canvas, channels=1, itemsize=isz)
    src = SC.as_samples(frames_u8, depth)
    keep = None
    if mem == "device":
        src = keep = engine.upload(src)
    elif mem == "pinned":
        keep = engine.alloc_pinned(src.shape, src.dtype)
        keep[...] = src
        src = keep
    try:
        res = engine.conform_submit(src, planes, out_planes, origin, index, lut, matrix, out=dst, frame_bytes=frames_u8.shape[1])
        if not wait:
            return res
        engine.conform_wait()
        got = engine.download(res, np.uint8)
    finally:
        if wait:
            if mem == "pinned":
                engine.free_pinned(keep)
            elif mem == "device":
                keep._owner.free()
            canvas._owner.free()
    return got


def check(engine, layout, depth, out_hw, origin=(0, 0), index=None, lut=None, matrix=None, seed=1, src_pad=(0, 0, 0),
          dst_pad=(0, 0, 0), mem="host", n=3, origins=None, extra=(2, 3)):
    """one case against the restatement, every byte of the destination; -> the bytes.  The source's luma is the window, its
    corner and `extra` rows and columns behind it."""
    sh, sw = source_size(out_hw, origin, extra)
    planes, fb = SC.padded(SC.planes_of(layout, sh, sw, depth), *src_pad)
    out_planes, ofb = SC.padded(SC.planes_of(layout, out_hw[0], out_hw[1], depth), *dst_pad)
    origins = plane_origins(layout, origin) if origins is None else origins
    frames = SC.content(n, planes, fb, depth, seed)
    want = expected(frames, planes, out_planes, ofb, depth, origins, index, lut, matrix)
    got = run(engine, frames, planes, out_planes, ofb, depth, origins, index, lut, matrix, mem)
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, (layout, depth, out_hw, origin, index, len(bad), bad[:4].tolist())
    return got
