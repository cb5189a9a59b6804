"""Frame ingest without OpenCV / FFmpeg.

The reference reads frames with cv2.VideoCapture (complexity_metrics.py:76-111) and lets the ffmpeg
binary decode both inputs of the quality filters (video_processing.py:284-291).  Neither exists in the
target image and decode is out of scope, so streams arrive already decoded:

  .npy          [N,H,W,3] uint8 packed BGR24 (complexity path; what cv2 would have produced)
  .y4m          YUV4MPEG2, planar 4:2:0 / 4:2:2 / 4:4:4 / mono at 8 bits (C420*, C422, C444, Cmono) or 10 / 12 / 16 bits
                (C420p10, C444p16, Cmono12 ... the tags FFmpeg's yuv4mpeg muxer writes; little-endian uint16 samples)
                (quality path: the planes FFmpeg's psnr/ssim see); open_y4m maps the file instead of reading it (a strided
                view: no host memory up front)
  .yuv / raw    headerless planar YUV / gray (config pixfmt, default yuv420p) with explicit width/height (mapped)
  .bgr / .bgr24 headerless packed BGR24 with explicit width/height (mapped)

Frames land in (optionally pinned) host buffers the engine can DMA from.
"""
import os

import numpy as np


# FFmpeg pix_fmt name -> (chroma layout, bit depth, the C tag FFmpeg's yuv4mpeg muxer writes for it).  Samples above 8 bits are
# little-endian uint16 (the "le" formats); planes follow each other Y, U, V (mono: Y only).
PIXFMTS = {
    "yuv420p": ("420", 8, "420jpeg"), "yuv422p": ("422", 8, "422"), "yuv444p": ("444", 8, "444"), "gray": ("mono", 8, "mono"),
    "yuv420p10le": ("420", 10, "420p10"), "yuv422p10le": ("422", 10, "422p10"), "yuv444p10le": ("444", 10, "444p10"),
    "yuv420p12le": ("420", 12, "420p12"), "yuv422p12le": ("422", 12, "422p12"), "yuv444p12le": ("444", 12, "444p12"),
    "yuv420p16le": ("420", 16, "420p16"), "yuv444p16le": ("444", 16, "444p16"),
    "gray10le": ("mono", 10, "mono10"), "gray12le": ("mono", 12, "mono12"), "gray16le": ("mono", 16, "mono16"),
}
_Y4M_TAGS = {tag: name for name, (_c, _d, tag) in PIXFMTS.items()}
_Y4M_TAGS.update({"420": "yuv420p", "420mpeg2": "yuv420p", "420paldv": "yuv420p"})   # the other 8-bit 4:2:0 siting tags


def plane_sizes(h, w, chroma):
    """-> [(width, height)] of the planes of one frame: Y, then U and V (none for mono)"""
    if chroma == "mono":
        return [(w, h)]
    cw = (w + 1) // 2 if chroma in ("420", "422") else w
    ch = (h + 1) // 2 if chroma == "420" else h
    return [(w, h), (cw, ch), (cw, ch)]


def frame_samples(h, w, pixfmt="yuv420p"):
    """samples per frame of a planar pix_fmt (PIXFMTS)"""
    return sum(pw * ph for pw, ph in plane_sizes(h, w, PIXFMTS[pixfmt][0]))


def sample_dtype(pixfmt):
    return np.dtype("<u2") if PIXFMTS[pixfmt][1] > 8 else np.dtype(np.uint8)


def frame_bytes_yuv420p(h, w):
    cw, ch = (w + 1) // 2, (h + 1) // 2
    return w * h + 2 * cw * ch


def _y4m_header_full(path):
    """-> (header length in bytes, height, width, fps, pix_fmt name)"""
    with open(path, "rb") as f:
        header = f.readline()
    if not header.startswith(b"YUV4MPEG2"):
        raise ValueError("not a YUV4MPEG2 stream: %s" % path)
    tok = header.decode("ascii", "replace").split()
    w = int(next(t[1:] for t in tok if t.startswith("W")))
    h = int(next(t[1:] for t in tok if t.startswith("H")))
    cs = next((t[1:] for t in tok if t.startswith("C")), "420jpeg")
    pixfmt = _Y4M_TAGS.get(cs)
    if pixfmt is None:
        raise ValueError("unsupported Y4M colour space C%s (supported: %s)" % (cs, ", ".join("C" + t for t in sorted(_Y4M_TAGS))))
    il = next((t[1:] for t in tok if t.startswith("I")), "p")
    if il not in ("p", "?"):
        raise ValueError("interlaced Y4M (I%s) is not supported: progressive frames only" % il)
    fr = next((t[1:] for t in tok if t.startswith("F")), "30:1")
    num, den = (int(x) for x in fr.split(":"))
    return len(header), h, w, (num / den if den else 0.0), pixfmt


def _y4m_header(path):
    """-> (header length in bytes, height, width, fps)"""
    return _y4m_header_full(path)[:4]


def y4m_pixfmt(path):
    """the FFmpeg pix_fmt name (PIXFMTS) of a .y4m file's C tag"""
    return _y4m_header_full(path)[4]


def open_y4m(path, max_frames=None):
    """-> (frames [N, samples_per_frame] in Y,U,V plane order - uint8, or little-endian uint16 above 8 bits (y4m_pixfmt tells
    the format) -, height, width, fps) WITHOUT reading the file: a strided view
    of a memory map (every frame sits a 6-byte FRAME line + bytes_per_frame after the previous one), so a clip of any length costs no
    host memory up front and the pass pages in what it gathers into the pinned ring (stream.py) - the reference hands the file
    to an ffmpeg subprocess that streams it the same way (video_processing.py:284-291).  Falls back to read_y4m (which parses
    frame by frame) when a frame header carries parameters, i.e. the frames are not equally spaced."""
    hl, h, w, fps, pixfmt = _y4m_header_full(path)
    dt = sample_dtype(pixfmt)
    ns = frame_samples(h, w, pixfmt)
    fb = ns * dt.itemsize
    size = os.path.getsize(path)
    n = (size - hl) // (fb + 6)
    if max_frames is not None:
        n = min(n, max_frames)
    if n <= 0:
        return np.zeros((0, ns), dt), h, w, fps
    mm = np.memmap(path, dtype=np.uint8, mode="r")
    marks = np.lib.stride_tricks.as_strided(mm[hl:], shape=(n, 6), strides=(fb + 6, 1), writeable=False)
    if not (marks == np.frombuffer(b"FRAME\n", np.uint8)).all():
        del marks, mm
        return read_y4m(path, max_frames)
    if dt.itemsize == 1:
        frames = np.lib.stride_tricks.as_strided(mm[hl + 6:], shape=(n, ns), strides=(fb + 6, 1), writeable=False)
    else:   # uint16 samples (not necessarily 2-byte aligned: the FRAME lines are 6 bytes), still a view of the map
        frames = np.ndarray((n, ns), dtype=dt, buffer=mm, offset=hl + 6, strides=(fb + 6, dt.itemsize))
        frames.flags.writeable = False
    return frames, h, w, fps


def read_y4m(path, max_frames=None, out=None):
    """-> (frames [N, samples_per_frame] in Y,U,V plane order (uint8, or uint16 above 8 bits), height, width, fps), read into
    memory frame by frame (frame headers with parameters are accepted); `out`: a (pinned) array to read into."""
    hl, h, w, fps, pixfmt = _y4m_header_full(path)
    dt = sample_dtype(pixfmt)
    ns = frame_samples(h, w, pixfmt)
    fb = ns * dt.itemsize
    with open(path, "rb") as f:
        f.seek(hl)
        frames = []
        while max_frames is None or len(frames) < max_frames:
            line = f.readline()
            if not line:
                break
            if not line.startswith(b"FRAME"):
                raise ValueError("corrupt Y4M frame header")
            buf = f.read(fb)
            if len(buf) < fb:
                break
            frames.append(np.frombuffer(buf, dt))
    arr = np.stack(frames) if frames else np.zeros((0, ns), dt)
    if out is not None:
        out[:arr.shape[0]] = arr
        arr = out[:arr.shape[0]]
    return arr, h, w, fps


def write_y4m(path, frames, h, w, fps=(30, 1), pixfmt="yuv420p"):
    """frames: [N, samples_per_frame] planar `pixfmt` (PIXFMTS: uint8, or uint16 above 8 bits, written little-endian)."""
    if pixfmt not in PIXFMTS:
        raise ValueError("unsupported pixfmt %r (supported: %s)" % (pixfmt, ", ".join(PIXFMTS)))
    dt = sample_dtype(pixfmt)
    frames = np.asarray(frames)
    if dt.itemsize > 1 and frames.dtype != np.uint16:
        raise ValueError("%s frames must be uint16 (got %s)" % (pixfmt, frames.dtype))
    frames = np.ascontiguousarray(frames, dt).reshape(-1, frame_samples(h, w, pixfmt))
    with open(path, "wb") as f:
        f.write(b"YUV4MPEG2 W%d H%d F%d:%d Ip A1:1 C%s\n" % (w, h, fps[0], fps[1], PIXFMTS[pixfmt][2].encode()))
        for fr in frames:
            f.write(b"FRAME\n")
            f.write(fr.tobytes())


def read_raw_yuv420p(path, h, w, max_frames=None, mmap=True):
    """headerless planar yuv420p -> [N, bytes_per_frame]; mapped, not read (mmap=False: loaded into memory)"""
    return read_raw_yuv(path, h, w, "yuv420p", max_frames, mmap)


def read_raw_yuv(path, h, w, pixfmt="yuv420p", max_frames=None, mmap=True):
    """headerless planar `pixfmt` (PIXFMTS) -> [N, samples_per_frame] uint8 / uint16; mapped, not read (mmap=False: loaded)"""
    dt = sample_dtype(pixfmt)
    ns = frame_samples(h, w, pixfmt)
    n = os.path.getsize(path) // (ns * dt.itemsize)
    if max_frames is not None:
        n = min(n, max_frames)
    if n <= 0:
        return np.zeros((0, ns), dt)
    if mmap:
        return np.memmap(path, dtype=dt, mode="r", shape=(n, ns))
    return np.fromfile(path, dt, count=n * ns).reshape(n, ns)


def open_raw_bgr24(path, h, w, max_frames=None):
    """headerless packed BGR24 (`ffmpeg -f rawvideo -pix_fmt bgr24`, what cv2.VideoCapture.read yields frame by frame,
    complexity_metrics.py:100) -> [N,H,W,3] uint8, mapped, not read"""
    fb = int(h) * int(w) * 3
    if fb <= 0:
        raise ValueError("raw BGR24 streams need height and width")
    n = os.path.getsize(path) // fb
    if max_frames is not None:
        n = min(n, max_frames)
    if n <= 0:
        return np.zeros((0, int(h), int(w), 3), np.uint8)
    return np.memmap(path, dtype=np.uint8, mode="r", shape=(n, int(h), int(w), 3))


def bgr_to_yuv420p(bgr):
    """Deterministic integer BT.601 limited-range conversion used to derive synthetic yuv420p streams
    from synthetic BGR ones (NOT a restatement of any decoder): Y = (66R+129G+25B+128>>8)+16, chroma
    from the 2x2 mean."""
    bgr = np.asarray(bgr, np.uint8)
    n, h, w, _ = bgr.shape
    b, g, r = (bgr[..., c].astype(np.int32) for c in range(3))
    y = ((66 * r + 129 * g + 25 * b + 128) >> 8) + 16
    def sub(p):
        ph, pw = (h + 1) // 2 * 2, (w + 1) // 2 * 2
        q = np.pad(p, ((0, 0), (0, ph - h), (0, pw - w)), mode="edge")
        return (q[:, 0::2, 0::2] + q[:, 0::2, 1::2] + q[:, 1::2, 0::2] + q[:, 1::2, 1::2] + 2) >> 2
    rb, gb, bb = sub(r), sub(g), sub(b)
    u = ((-38 * rb - 74 * gb + 112 * bb + 128) >> 8) + 128
    v = ((112 * rb - 94 * gb - 18 * bb + 128) >> 8) + 128
    out = np.empty((n, frame_bytes_yuv420p(h, w)), np.uint8)
    out[:, :h * w] = np.clip(y, 0, 255).reshape(n, -1)
    cs = u.shape[1] * u.shape[2]
    out[:, h * w:h * w + cs] = np.clip(u, 0, 255).reshape(n, -1)
    out[:, h * w + cs:] = np.clip(v, 0, 255).reshape(n, -1)
    return out
