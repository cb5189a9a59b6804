"""Frames, planes and rows that start beyond byte 2^31 and 2^32 of their stream: where the samples of every case lie in ONE device
arena.  Shared by tests/test_far_host.py (the geometry's own properties, on the CPU) and tests/test_gpu_far_addresses.py (every
kind gives the tight clip's bytes from there).  Pure integers, enumerated, nothing random.

include/vqa.h gives vqa_plane_desc 64-bit offsets and row strides and every submit 64-bit frame strides; a resident clip of a few
hundred 2160p frames puts frame i at i * frame_stride >= 2^32.  The kernels form these addresses in different ways (a 32-bit
scalar buffer offset in k_ssim_gauss, uniform_ptr(...)[u32] in k_sad, k_dct8 and k_canny, hand-written int64_t casts in the newer
ones), and one forgotten cast reads plausible samples from another place.

The arena is ARENA bytes, never initialised.  Its first and last GUARD = 2^31 + 2^20 bytes are described by no case: an address
that loses its upper 32 bits or takes a wrong sign out of a 32-bit term is still inside the arena, so a wrong kernel reads
uninitialised bytes of the test's own allocation and gives wrong numbers.  Every (clip, content, case) has a slot of its own,
SLOT bytes after its neighbour's, so the samples of two cases never share a byte and each is written once.

  F1   n = 3, ref_fs = 2^31 + 5 * 4096: frame 1 starts beyond 2^31 and frame 2 beyond 2^32; dist 2^20 after ref, with the same
       stride (F1a) or with 2^31 + 9 * 4096 (F1b); prev0 above ref's frame 2.  Every F1 frame is followed by one zero sample: the
       control moves the descriptors one sample on
  F2   n = 1, Y at offset 0, U at 2^31 + 2 * 4099, V at 2^32 + 2 * 8209 (U and V keep one stride and step); a single plane takes
       V's offset; prev0 and dist are views with the same descriptors 2^18 and 2^19 further on
  F3   n = 1, 34 rows of 50 (chroma 17 x 25), row_stride R = 2^27 + 3 * 4096 for every plane, U and V 2^16 and 2^17 after Y: rows
       16 .. 31 of Y start beyond 2^31, rows 32 and 33 beyond 2^32; a gray plane of 33 rows for VCA, whose blocks exclude 17-row
       chroma (32 R > 2^32); dist and prev0 2^18 and 2^19 further on
A packed BGR clip (the complexity batch) has no plane descriptors: it takes F1 (frame strides) and F3 (its row stride)."""
from collections import namedtuple

ARENA = 9 << 30
GUARD = (1 << 31) + (1 << 20)
SLOT = 1 << 22
MAX_SLOTS = 32                                   # 32 slots are 2^27 < R: the rows of one F3 slot never reach the next row of another

FS_A = (1 << 31) + 5 * 4096
FS_B = (1 << 31) + 9 * 4096
OFF_U = (1 << 31) + 2 * 4099
OFF_V = (1 << 32) + 2 * 8209
R = (1 << 27) + 3 * 4096
CASES = ("F1a", "F1b", "F2", "F3")

# name -> (layout "420" | "gray" | "bgr", height, width, depth)
CLIPS = {"yuv420p-66x98": ("420", 66, 98, 8), "yuv420p10-70x74": ("420", 70, 74, 10), "bgr-66x98": ("bgr", 66, 98, 8),
         "gray8-177x263": ("gray", 177, 263, 8)}
ROW_CLIPS = {"yuv420p-34x50": ("420", 34, 50, 8), "yuv420p10-34x50": ("420", 34, 50, 10), "bgr-34x50": ("bgr", 34, 50, 8),
             "gray8-33x50": ("gray", 33, 50, 8), "gray10-33x50": ("gray", 33, 50, 10)}
ANCHOR = {"complexity": "bgr-66x98", "ms": "gray8-177x263"}
ANCHOR_DEFAULT = "yuv420p-66x98"
N_FRAMES = 3

# MS-SSIM takes no plane under 161 x 161: vqa_quality_submit refuses the 34 x 50 clip of F3 for its SIZE, with the same status as
# for rows that span 2^31 bytes, so that clip does not pin the row rule for it.  One gray plane of MS_ROWS x MS_ROWS does: at the
# row stride MS_FAR its rows span 2^31 (refused), at MS_NEAR they do not (taken).  Nothing is written there - a refusal reads
# nothing, and the accepted submit's figures are of no interest - and both lie above every slot, inside the arena and outside
# its guards, as does an address whose row term was formed in 32 bits (tests/test_far_host.py).
MS_ROWS = 161
MS_FAR = (1 << 24) + 3 * 4096
MS_NEAR = (1 << 23) + 3 * 4096
MS_SPOT = GUARD + SLOT * MAX_SLOTS
MS_DIST = 4096                                   # dist's plane starts this far after ref's: its rows lie between ref's

Placed = namedtuple("Placed", "clip case n isz planes streams row_stride")      # streams: {"ref" | "dist" | "prev0": (spot, frame stride)}


def entry(name):
    return CLIPS[name] if name in CLIPS else ROW_CLIPS[name]


def isz_of(name):
    return 2 if entry(name)[3] > 8 else 1


def tight_planes(name):
    """the engine's plane tuples of the tight clip; a bgr clip: one pseudo-plane of 3 w bytes a row, for the embedding alone"""
    from rtvqa_amd.engine import yuv_planes
    layout, h, w, depth = entry(name)
    if layout == "bgr":
        return [(3 * w, h, 0, 3 * w, 1)]
    return [tuple(p) for p in yuv_planes(h, w, "mono" if layout == "gray" else "420", depth)]


def frame_bytes(name):
    isz = isz_of(name)
    return sum(p[0] * p[1] for p in tight_planes(name)) * isz


def contents_of(name):
    """the contents a clip is written with: CAMBI reads cambi_cases' dithered staircase (on noise its words are 0 wherever the
    samples lie), MDSI's anchor mdsi_cases' pairs"""
    layout = entry(name)[0]
    out = ["natural"]
    if layout == "420":
        out.append("cambi")
    if name == ANCHOR_DEFAULT:
        out.append("mdsi")
    return out


def cases_of(name):
    if name in ROW_CLIPS:
        return ("F3",)
    return ("F1a", "F1b") if entry(name)[0] == "bgr" else ("F1a", "F1b", "F2")


def slots():
    """every (clip, content, case) in a fixed order: the index is the slot"""
    return [(name, content, case) for name in list(CLIPS) + list(ROW_CLIPS) for content in contents_of(name) for case in cases_of(name)]


def place(name, content, case):
    """-> Placed: where the three streams of this case start (bytes from the arena's first byte), their frame strides and the
    descriptors they share"""
    base = GUARD + SLOT * slots().index((name, content, case))
    layout, h, w, depth = entry(name)
    isz, tight = isz_of(name), tight_planes(name)
    fb = frame_bytes(name)
    if case in ("F1a", "F1b"):
        dist_fs = FS_A if case == "F1a" else FS_B
        streams = {"ref": (base, FS_A), "dist": (base + (1 << 20), dist_fs), "prev0": (base + 2 * FS_A + (1 << 19), FS_A)}
        return Placed(name, case, N_FRAMES, isz, tight, streams, tight[0][3])
    # (n = 1: no frame stride is multiplied by anything; the complexity batch still wants one that holds the frame)
    fs = (OFF_V if case == "F2" else h * R) + (1 << 20)
    assert fs >= fb
    streams = {"ref": (base, fs), "prev0": (base + (1 << 18), fs), "dist": (base + (1 << 19), fs)}
    if case == "F2":
        assert layout != "bgr"
        offs = (0, OFF_U, OFF_V) if len(tight) == 3 else (OFF_V,)
        planes = [(p[0], p[1], o) + tuple(p[3:]) for p, o in zip(tight, offs)]
        return Placed(name, case, 1, isz, planes, streams, None)
    assert case == "F3"
    offs = (0, 1 << 16, 1 << 17)
    planes = [(p[0], p[1], o, R) + tuple(p[4:]) for p, o in zip(tight, offs)]
    return Placed(name, case, 1, isz, planes, streams, R)


def runs(pl):
    """the contiguous pieces a Placed case is written in -> [(arena offset, bytes, stream, frame, plane index or None, row or
    None)]: a whole plane where its rows follow each other, else one row; plane None: the zero sample behind an F1 frame"""
    out = []
    for key, (spot, fs) in pl.streams.items():
        for f in range(1 if key == "prev0" else pl.n):
            end = 0
            for pi, (w, h, off, rs, step, *_r) in enumerate(pl.planes):
                assert step == pl.isz
                if rs == w * step:
                    out.append((spot + f * fs + off, h * rs, key, f, pi, None))
                else:
                    out += [(spot + f * fs + off + y * rs, w * step, key, f, pi, y) for y in range(h)]
                end = max(end, off + (h - 1) * rs + w * step)
            if pl.case in ("F1a", "F1b"):
                out.append((spot + f * fs + end, pl.isz, key, f, None, None))
    return out


def described(pl, shift=0):
    """the first and last byte the descriptors of a Placed case address, per stream and frame -> [(first, last)] (from the
    descriptors alone, as a kernel forms them: pointer + frame * frame stride + offset + row * row stride + column * step)"""
    out = []
    for key, (spot, fs) in pl.streams.items():
        for f in range(1 if key == "prev0" else pl.n):
            for (w, h, off, rs, step, *_r) in pl.planes:
                first = spot + f * fs + off + shift
                out.append((first, first + (h - 1) * rs + (w - 1) * step + pl.isz - 1))
    return out


def crossings(pl):
    """the powers of two a case's address terms cross: -> {"frame" | "plane" | "row": sorted exponents e such that a term of that
    kind is >= 2^e, e in (31, 32)}"""
    got = {"frame": set(), "plane": set(), "row": set()}
    for e in (31, 32):
        for key, (_spot, fs) in pl.streams.items():
            if any(f * fs >= 1 << e for f in range(1 if key == "prev0" else pl.n)):
                got["frame"].add(e)
        for (_w, h, off, rs, *_r) in pl.planes:
            if off >= 1 << e:
                got["plane"].add(e)
            if (h - 1) * rs >= 1 << e:
                got["row"].add(e)
    return {k: sorted(v) for k, v in got.items()}


CLAIMS = {"F1a": {"frame": [31, 32], "plane": [], "row": []}, "F1b": {"frame": [31, 32], "plane": [], "row": []},
          "F2": {"frame": [], "plane": [31, 32], "row": []}, "F3": {"frame": [], "plane": [], "row": [31, 32]}}
