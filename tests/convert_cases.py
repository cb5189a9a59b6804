"""The cases of the convert tests: plane lists with pads and steps of their own, content that holds 0 and the peak, the call into
the engine with a destination prefilled with a pattern, the expected bytes from convert_reference, and the thinned list of
(layouts, depths, options, size) cases that still holds every (relation per axis) x (filter, siting) x (Ts, Td) combination at an
odd and at an even size."""
import itertools

import numpy as np

import convert_reference as R

FILL = 0xA5
SIZES = ((16, 16), (17, 33), (18, 47), (34, 65), (50, 130))          # luma (h, w): around a 16-byte granule, odd and even
CHROMAS = ("420", "422", "444")
DEPTH_PAIRS = ((8, 10), (10, 8), (8, 16), (16, 8), (10, 12), (12, 10), (8, 8), (10, 10))
FILTERS = (("box", "center"), ("linear", "center"), ("linear", "left"))
RANGES = ("limited", "full")


def planes_of(h, w, chroma, depth, row_pad=0, lead=0, plane_pad=0, step=1):
    """planar frames of one chroma layout ("420" | "422" | "444" | "mono") -> (plane tuples, frame bytes); row_pad, lead and
    plane_pad in SAMPLES: behind every row, before the first plane, behind every plane; step: the pixel step in samples"""
    bps = 2 if depth > 8 else 1
    sizes = [(w, h)]
    if chroma != "mono":
        sizes += [((w + 1) >> 1 if chroma in ("420", "422") else w, (h + 1) >> 1 if chroma == "420" else h)] * 2
    planes, off = [], lead * bps
    for pw, ph in sizes:
        rs = (pw * step + row_pad) * bps
        planes.append((pw, ph, off, rs, step * bps, depth))
        off += ph * rs + plane_pad * bps
    return planes, off


def content(n, fb, depth, seed, above=False):
    """[n, fb] uint8: noise over the codes of the depth that holds 0 and the peak; above: over the whole sample type"""
    rng = np.random.default_rng(seed)
    if depth <= 8:
        out = rng.integers(0, 256, (n, fb), dtype=np.uint8)
        out[:, 8:12], out[:, 12:16] = 0, 255
        return out
    peak = (1 << depth) - 1
    v = rng.integers(0, 65536 if above else peak + 1, (n, (fb + 1) // 2), dtype=np.uint16)
    v[:, 4:6], v[:, 6:8] = 0, peak
    return np.ascontiguousarray(v.view(np.uint8)[:, :fb])


def as_samples(frames_u8, depth):
    return frames_u8 if depth <= 8 else np.ascontiguousarray(frames_u8).view("<u2")


def expected(frames_u8, planes, out_planes, ofb, chroma, siting, range, fill=FILL):
    """what the destination must hold, pad bytes included: [n, ofb] uint8"""
    out = np.full((frames_u8.shape[0], ofb), fill, np.uint8)
    return R.convert_frames(frames_u8, planes, out, out_planes, chroma, siting, range)


def run(engine, frames_u8, planes, out_planes, ofb, chroma, siting, range, mem="host", fill=FILL, wait=True):
    """vqa_convert_submit into a destination prefilled with `fill` -> the whole destination as [n, ofb] uint8 (wait=False: the
    DeviceFrames, the batch still pending)"""
    from rtvqa_amd.engine import DeviceFrames
    n, ds, dd = frames_u8.shape[0], int(planes[0][5]), int(out_planes[0][5])
    isz = 2 if dd > 8 else 1
    canvas = engine.upload(as_samples(np.full((n, ofb), fill, np.uint8), dd))
    dst = DeviceFrames(canvas.ptr, n, 1, ofb // isz, frame_stride=ofb, owner=canvas, channels=1, itemsize=isz)
    src = as_samples(frames_u8, ds)
    keep = None
    if mem == "device":
        src = keep = engine.upload(src)
    elif mem == "pinned":
        keep = engine.alloc_pinned(src.shape, src.dtype)
        keep[...] = src
        src = keep
    try:
        res = engine.convert_submit(src, planes, out_planes, chroma, siting, range, out=dst, frame_bytes=frames_u8.shape[1])
        if not wait:
            return res
        engine.convert_wait()
        got = engine.download(res, np.uint8)
    finally:
        if wait:
            if mem == "pinned":
                engine.free_pinned(keep)
            elif mem == "device":
                keep._owner.free()
            canvas._owner.free()
    return got


def check(engine, hw, cs, cd, ds, dd, chroma="linear", siting="center", range="limited", src_pad=(0, 0, 0), dst_pad=(0, 0, 0),
          src_step=1, dst_step=1, mem="host", n=2, seed=1, above=False):
    """one case against the restatement, every byte of the destination -> the bytes"""
    planes, fb = planes_of(hw[0], hw[1], cs, ds, *src_pad, step=src_step)
    out_planes, ofb = planes_of(hw[0], hw[1], cd, dd, *dst_pad, step=dst_step)
    fb += 6 * (2 if ds > 8 else 1) if any(src_pad) else 0          # a frame pad where there are pads at all
    ofb += 5 * (2 if dd > 8 else 1) if any(dst_pad) else 0
    frames = content(n, fb, ds, seed, above)
    want = expected(frames, planes, out_planes, ofb, chroma, siting, range)
    got = run(engine, frames, planes, out_planes, ofb, chroma, siting, range, mem)
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, (hw, cs, cd, ds, dd, chroma, siting, range, len(bad), bad[:4].tolist())
    return got


def relations(cs, cd):
    """(horizontal, vertical) relation of the chroma planes between two chroma layouts"""
    sub = {"420": (1, 1), "422": (1, 0), "444": (0, 0), "mono": (0, 0)}
    name = {0: "same", 1: "up", -1: "down"}
    return name[sub[cs][0] - sub[cd][0]], name[sub[cs][1] - sub[cd][1]]


def _thinned():
    """Every (layout pair, depth pair, filter and siting) - so every (relation per axis) x (filter, siting) x (Ts, Td) - at an
    even and at an odd size; the range, the further sizes and the pads walk along deterministically, so that every size, both
    ranges and every pad pattern meet every layout pair and every depth pair."""
    pads = (((0, 0, 0), (0, 0, 0)), ((3, 1, 5), (0, 0, 0)), ((0, 0, 0), (5, 3, 1)), ((2, 0, 0), (16, 0, 0)))
    even, odd = ((16, 16), (50, 130)), ((17, 33), (18, 47), (34, 65))
    cases, k = [], 0
    for cs, cd in list(itertools.product(CHROMAS, repeat=2)) + [("mono", "mono")]:
        for ds, dd in DEPTH_PAIRS:
            for chroma, siting in FILTERS:
                for j, group in enumerate((even, odd)):
                    cases.append((group[k % len(group)], cs, cd, ds, dd, chroma, siting, RANGES[(k + j) % 2], pads[(k + 2 * j) % 4]))
                k += 1
    return cases


CASES = _thinned()


def mixed_planes(hw, rx, ry, depth, side):
    """one plane on either side whose relation is (rx, ry): side "src" | "dst"; hw is the size of the larger extent per axis"""
    h, w = hw
    small = lambda n: (n + 1) >> 1
    sw, dw = {"same": (w, w), "up": (small(w), w), "down": (w, small(w))}[rx]
    sh, dh = {"same": (h, h), "up": (small(h), h), "down": (h, small(h))}[ry]
    pw, ph = (sw, sh) if side == "src" else (dw, dh)
    bps = 2 if depth > 8 else 1
    return [(pw, ph, 0, pw * bps, bps, depth)], pw * ph * bps


# (up, down) and (down, up): one plane each, every (filter, siting) x (Ts, Td) at an even and an odd size
MIXED = [(hw, rel, ds, dd, chroma, siting, RANGES[i % 2])
         for rel in (("up", "down"), ("down", "up")) for ds, dd in ((8, 8), (8, 10), (10, 8), (12, 10))
         for i, (chroma, siting) in enumerate(FILTERS) for hw in ((32, 64), (35, 47))]
