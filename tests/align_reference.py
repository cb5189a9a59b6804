"""The restatement of vqa_align_submit's definition (include/vqa.h) in NumPy: sse[j][c] = sum over the plane of (d_j - r_i)^2
with i = j + offset + (c - radius), formed DIRECTLY in int64, pair by pair - no Gram matrix, no shift, no energies, so it
shares no algebra with the kernel - and NONE where the reference frame does not exist."""
import numpy as np

NONE = (1 << 64) - 1


def plane_series(stream, plane, frame_bytes=None):
    """The samples of one plane tuple (width, height, offset, row_stride, pixel_step[, depth]) of every frame of a stream
    (an array whose first axis is the frame, or flat bytes with frame_bytes) -> int64 [n, h, w]"""
    w, h, off, rs, step = (int(v) for v in plane[:5])
    wide = len(plane) > 5 and int(plane[5]) > 8
    a = np.ascontiguousarray(stream)
    raw = a.reshape(-1).view(np.uint8)
    fs = int(frame_bytes) if frame_bytes else raw.size // a.shape[0]
    n = a.shape[0] if not frame_bytes else (raw.size - (off + (h - 1) * rs + (w - 1) * step + (2 if wide else 1))) // fs + 1
    out = np.empty((n, h, w), np.int64)
    for f in range(n):
        for y in range(h):
            at = f * fs + off + y * rs
            if wide:
                lo = raw[at:at + (w - 1) * step + 1:step].astype(np.int64)
                hi = raw[at + 1:at + (w - 1) * step + 2:step].astype(np.int64)
                out[f, y] = lo + 256 * hi
            else:
                out[f, y] = raw[at:at + (w - 1) * step + 1:step]
    return out


def pair_sse(d, r):
    """sum (d - r)^2 of two int64 planes, as a Python integer"""
    e = d.astype(np.int64) - r.astype(np.int64)
    return int((e * e).sum(dtype=np.int64))   # < 2^28 * 2^32 = 2^60: inside int64


def band(ref, dist, radius, offset=0):
    """ref [n_ref, h, w], dist [n_dist, h, w] (int64 planes) -> uint64 [n_dist, 2 radius + 1]"""
    n_ref, n_dist = ref.shape[0], dist.shape[0]
    out = np.full((n_dist, 2 * radius + 1), NONE, np.uint64)
    for j in range(n_dist):
        for c in range(2 * radius + 1):
            i = j + offset + c - radius
            if 0 <= i < n_ref:
                out[j, c] = pair_sse(dist[j], ref[i])
    return out
