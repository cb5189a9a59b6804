"""One clip laid out in many ways: the embedding, the matrix of layouts and the launch predicates it has to reach.  Shared by
tests/test_layouts_host.py (the embedding's own properties, on the CPU) and tests/test_gpu_layouts.py (every kind gives the tight
clip's bytes from every layout).  Pure NumPy, enumerated, nothing random.

A tight clip is [n, samples] of uint8 / uint16 with the plane tuples the engine takes, (width, height, offset, row_stride,
pixel_step[, bit_depth]) in bytes.  A Spec moves its samples into a larger canvas; every figure of a Spec is in SAMPLES, so a
16-bit layout keeps offset, stride and step even, as the ABI demands:

  lead       samples before frame 0 (a device view starts at ptr + lead, a host submit carries it in the offsets)
  row_pad    samples added to each row, one figure for all plane groups or one per group
  gap        samples between two plane groups
  frame_pad  samples added to the frame stride
  groups     which planes share a pixel: None = as the tight clip has them (bgr24's three channels; every planar plane by itself);
             ((0,), (1, 2)) interleaves U and V as NV12 stores them
  step       the pixel step of every group, None = the planes of the group (1 planar, 3 for bgr24); a larger step leaves filler
             between the samples
  select     the descriptors handed out, a permutation or a subset of the planes over unchanged memory; None = all, in order

Every byte no sample owns is `fill`.  A canvas holds lead + n * frame_stride bytes."""
from collections import namedtuple

import numpy as np

Spec = namedtuple("Spec", "name lead row_pad gap frame_pad groups step select")


def spec(name, lead=0, row_pad=0, gap=0, frame_pad=0, groups=None, step=None, select=None):
    return Spec(name, lead, row_pad, gap, frame_pad, groups, step, select)


TIGHT = spec("tight")

# a case: the layout of the reference stream, of the distorted stream and of prev0 (None: the reference's), the memory kinds it runs
# from, and whether a device submit carries the lead in the offsets instead of the pointer.  dist and prev0 share the descriptors
# of ref, so their Specs differ from it in lead and frame_pad only; the host ABI has one frame stride and one descriptor list,
# so a case whose streams differ is device-only.
Case = namedtuple("Case", "name ref dist prev0 mems lead_in_offsets")
BOTH, DEVICE = ("host", "device"), ("device",)


def case(s, dist=None, prev0=None, mems=BOTH, lead_in_offsets=False, name=None):
    return Case(name or s.name, s, dist, prev0, mems, lead_in_offsets)


# ---- the embedding ---------------------------------------------------------------------------------------------------------------
def _view(buf, start, p, isz):
    """plane tuple p of the frame that starts at sample `start` of the flat array buf, in place: [h, w]"""
    w, h, off, rs, step = p[:5]
    return np.lib.stride_tricks.as_strided(buf[start + off // isz:], shape=(h, w), strides=(rs, step))


def natural_groups(planes, isz):
    """the planes that share a pixel in the tight clip: same size, stride and a step of several samples, offsets inside one pixel"""
    groups, done = [], set()
    for i, p in enumerate(planes):
        if i in done:
            continue
        g = [i]
        if p[4] > isz:
            g += [j for j in range(i + 1, len(planes)) if j not in done and tuple(planes[j][:2]) == tuple(p[:2]) and
                  tuple(planes[j][3:5]) == tuple(p[3:5]) and 0 < planes[j][2] - p[2] < p[4]]
        done.update(g)
        groups.append(tuple(g))
    return tuple(groups)


def applies(s, planes, isz):
    """whether Spec s can lay out a clip of these planes: its groups and its selection name planes the clip has, and the planes
    of a group share a size"""
    named = [i for g in (s.groups or ()) for i in g] + list(s.select or ())
    if any(i >= len(planes) for i in named):
        return False
    if s.groups and sorted(i for g in s.groups for i in g) != list(range(len(planes))):
        return False
    groups = s.groups or natural_groups(planes, isz)
    if s.step is not None and len(s.step) != len(groups):
        return False
    if not isinstance(s.row_pad, int) and len(s.row_pad) != len(groups):
        return False
    return all(tuple(planes[i][:2]) == tuple(planes[g[0]][:2]) for g in groups for i in g)


def embed(frames, planes, s, fill):
    """-> (canvas, new_planes, frame_bytes, lead_bytes): the tight clip's samples at the places Spec s gives them, `fill` elsewhere.
    new_planes are relative to a frame's first byte (the lead is not in them) and follow s.select."""
    frames = np.asarray(frames)
    isz, n = frames.dtype.itemsize, frames.shape[0]
    flat = frames.reshape(n, -1)
    groups = s.groups or natural_groups(planes, isz)
    new, cursor = [None] * len(planes), 0
    for gi, g in enumerate(groups):
        w, h = planes[g[0]][:2]
        step = s.step[gi] if s.step is not None else len(g)
        assert step >= len(g), s.name
        rs = w * step + (s.row_pad if isinstance(s.row_pad, int) else s.row_pad[gi])
        for slot, i in enumerate(g):
            new[i] = (w, h, (cursor + slot) * isz, rs * isz, step * isz) + tuple(planes[i][5:])
        cursor += h * rs + (s.gap if gi + 1 < len(groups) else 0)
    frame = cursor + s.frame_pad
    canvas = np.full(s.lead + n * frame, fill, frames.dtype)
    for f in range(n):
        for i, p in enumerate(planes):
            _view(canvas, s.lead + f * frame, new[i], isz)[...] = _view(flat[f], 0, p, isz)
    return canvas, selected(new, s), frame * isz, s.lead * isz


def selected(planes, s):
    """the descriptors Spec s hands out of a plane list (the tight clip's: what the layout has to be compared with)"""
    return [planes[i] for i in (s.select if s.select is not None else range(len(planes)))]


def extract(canvas, new_planes, n, frame_bytes, lead_bytes):
    """the inverse of embed: -> one [n, h, w] array per descriptor, copied out of the canvas"""
    isz = canvas.dtype.itemsize
    return [np.stack([_view(canvas, (lead_bytes + f * frame_bytes) // isz, p, isz).copy() for f in range(n)]) for p in new_planes]


def tight_planes_of(frames, planes):
    """extract() of a tight clip"""
    flat = np.asarray(frames).reshape(np.asarray(frames).shape[0], -1)
    return extract(flat.reshape(-1), planes, flat.shape[0], flat.shape[1] * flat.dtype.itemsize, 0)


def owned(new_planes, n, frame_bytes, lead_bytes, isz, size):
    """how many planes own each sample of a canvas of `size` samples (0: filler), from the descriptors alone; an address outside
    the canvas is an IndexError"""
    count = np.zeros(size, np.int32)
    for f in range(n):
        for (w, h, off, rs, step, *_rest) in new_planes:
            at = (lead_bytes + f * frame_bytes + off + rs * np.arange(h)[:, None] + step * np.arange(w)[None, :]).reshape(-1)
            assert (at % isz == 0).all()
            if at.min() < 0 or at.max() // isz >= size:
                raise IndexError("a descriptor addresses sample %d of %d" % (at.max() // isz, size))
            np.add.at(count, at // isz, 1)
    return count


def with_lead(planes, lead_bytes):
    """the descriptors of a submit whose base pointer is the canvas's first byte"""
    return [(p[0], p[1], p[2] + lead_bytes) + tuple(p[3:]) for p in planes]


def host_rows(canvas, n, frame_bytes, lead_bytes, fill):
    """the canvas as the [n, samples] host array a submit takes: rows of lead + frame stride (the canvas, then filler), so that a
    prev0 laid out the same way has a row's bytes and every staging copy ((n - 1) frame strides + the span) stays inside"""
    isz = canvas.dtype.itemsize
    out = np.full(n * (lead_bytes + frame_bytes) // isz, fill, canvas.dtype)
    out[:canvas.size] = canvas
    return out.reshape(n, -1)


# ---- the matrix ------------------------------------------------------------------------------------------------------------------
NV12 = ((0,), (1, 2))


def planar3_cases():
    """three planar planes (4:2:0, 4:4:4), 8 and 16 bits: figures in samples"""
    lead = [case(spec("lead%d" % k, lead=k)) for k in (1, 2, 3, 4, 8)]
    pads = [case(spec("pad%s" % "".join(map(str, p)), row_pad=p)) for p in
            ((1, 1, 1), (2, 2, 2), (3, 3, 3), (1, 0, 0), (0, 1, 1), (0, 1, 2), (3, 1, 1))]
    all_in = spec("lead3-pad123-gap1-fpad5", lead=3, row_pad=(1, 2, 3), gap=1, frame_pad=5)
    return [case(TIGHT)] + lead + pads + [
        case(spec("fpad1", frame_pad=1)), case(spec("fpad5", frame_pad=5)),
        case(spec("gap1", gap=1)), case(spec("gap1-fpad6", gap=1, frame_pad=6)),      # (two gaps and six: a frame stride of the tight one + 8)
        case(spec("nv12", groups=NV12, step=(1, 2))),
        case(spec("nv12-lead1-pad12", lead=1, row_pad=(1, 2), groups=NV12, step=(1, 2))),
        case(spec("order021", select=(0, 2, 1))),
        case(all_in),
        case(spec("lead2-in-offsets", lead=2, frame_pad=4), mems=DEVICE, lead_in_offsets=True),
    ] + stream_cases()


def stream_cases():
    """device only: the streams of one submit at different places"""
    return [
        case(spec("ref-lead1", lead=1), dist=TIGHT, prev0=TIGHT, mems=DEVICE),
        case(spec("dist-lead1"), dist=spec("", lead=1), mems=DEVICE),
        case(spec("ref-lead1-fpad1-dist-lead2-fpad5", lead=1, frame_pad=1), dist=spec("", lead=2, frame_pad=5), mems=DEVICE),
        case(spec("ref-fpad8-dist-fpad1", frame_pad=8), dist=spec("", frame_pad=1), mems=DEVICE),
        case(spec("prev0-lead3"), prev0=spec("", lead=3), mems=DEVICE),
        case(spec("lead4-prev0-lead1", lead=4), prev0=spec("", lead=1), mems=DEVICE),
    ]


def planar1_cases():
    """one plane (gray), 8 and 16 bits"""
    return [case(TIGHT)] + [case(spec("lead%d" % k, lead=k)) for k in (1, 2, 3, 4, 8)] + \
        [case(spec("pad%d" % k, row_pad=k)) for k in (1, 2, 3)] + [
        case(spec("fpad1", frame_pad=1)), case(spec("fpad5", frame_pad=5)),
        case(spec("step2", step=(2,))), case(spec("step4-lead1-pad1", lead=1, row_pad=1, step=(4,))),
        case(spec("lead3-pad2-fpad5", lead=3, row_pad=2, frame_pad=5)),
        case(spec("lead2-in-offsets", lead=2, frame_pad=4), mems=DEVICE, lead_in_offsets=True),
    ] + stream_cases()


def packed_cases():
    """bgr24, 8 bits: figures in bytes"""
    grid = [(1, 0), (2, 0), (3, 0), (0, 1), (0, 2), (0, 3), (1, 1), (2, 3), (3, 2), (1, 3)]
    return [case(TIGHT)] + [case(spec("lead%d-pad%d" % lp, lead=lp[0], row_pad=lp[1])) for lp in grid] + [
        case(spec("fpad1", frame_pad=1)), case(spec("fpad5", frame_pad=5)),
        case(spec("step4", step=(4,))), case(spec("step4-lead1-pad2", lead=1, row_pad=2, step=(4,))),
        case(spec("rgb", select=(2, 1, 0))), case(spec("rgb-lead1-pad1", lead=1, row_pad=1, select=(2, 1, 0))),
        case(spec("only-g", select=(1,))), case(spec("only-b-r-pad1", row_pad=1, select=(0, 2))),
        case(spec("lead2-in-offsets", lead=2, frame_pad=4), mems=DEVICE, lead_in_offsets=True),
    ] + stream_cases()


def complexity_cases():
    """packed_cases() as the complexity batch can take them: bgr24 itself (a step of 3, B, G, R in order), device frames only;
    the tight case of 48 x 64 is the one whose base, strides and width are all multiples of 16"""
    out = []
    for c in packed_cases():
        if c.ref.step is None and c.ref.select is None and not c.lead_in_offsets:
            out.append(c._replace(mems=DEVICE))
    return out


def cases_for(planes, isz):
    """the matrix of a clip with these tight planes"""
    if len(natural_groups(planes, isz)) < len(planes):
        return packed_cases()
    return planar3_cases() if len(planes) == 3 else planar1_cases()


def host_spec(s):
    """Spec s as a submit can take it whose offsets carry the lead: the ABI wants a frame stride of at least the span of the planes
    from the base pointer (csrc/vqa_capi.hip: ref_fs < B.span is VQA_ERR_INVALID), so the frame pad is at least the lead"""
    return s._replace(frame_pad=max(s.frame_pad, s.lead))


def resolve(c, frames, planes, fill, prev0=None, dist=None, mem="device"):
    """the canvases of one case: -> dict(planes=descriptors relative to a frame, ref / dist / prev0 = (canvas, frame_bytes,
    lead_bytes) or None).  mem "host": the layout as host_spec() has it"""
    out = {}
    if mem == "host":
        assert c.dist is None and c.prev0 is None
        c = c._replace(ref=host_spec(c.ref))
    for key, clip, s in (("ref", frames, c.ref), ("dist", dist, c.dist), ("prev0", prev0 if prev0 is None else prev0[None], c.prev0)):
        if clip is None:
            out[key] = None
            continue
        s = c.ref if s is None else c.ref._replace(lead=s.lead, frame_pad=s.frame_pad)
        canvas, new, fb, lb = embed(clip, planes, s, fill)
        out[key] = (canvas, fb, lb)
        if key == "ref":
            out["planes"] = new
        assert new == out["planes"]
    return out


# ---- what the launches read of a layout ------------------------------------------------------------------------------------------
# Each function restates one launch-time choice of a kernel from the numbers it is given (pointers, strides, offsets), with the
# source line it follows: a kernel change has this one place to update.  The tests use them to show that the matrix reaches
# both sides of every choice.
def groups_of(planes):
    """csrc/vqa_capi.hip, for_each_group: planes of one width, height, row stride and pixel step go out as one launch
    -> lists of plane indices"""
    out, done = [], set()
    for i, p in enumerate(planes):
        if i in done:
            continue
        g = [j for j in range(i, len(planes)) if j not in done and (planes[j][0], planes[j][1], planes[j][3], planes[j][4]) ==
             (p[0], p[1], p[3], p[4])]
        done.update(g)
        out.append(g)
    return out


def psnr_hvs_failing(ref, dist, ref_fs, dist_fs, planes, n, bps):
    """csrc/k_psnr_hvs.hip:241-244 -> per launch, the set of terms that keep it from the one-load-per-row kernel (empty: VEC)"""
    a, out = 8 * bps, []
    for g in groups_of(planes):
        bad = set()
        if ref % a:
            bad.add("ref")
        if dist % a:
            bad.add("dist")
        if planes[g[0]][3] % a:
            bad.add("row_stride")
        if n > 1 and (ref_fs % a or dist_fs % a):
            bad.add("frame_stride")
        if any(planes[i][2] % a for i in g):
            bad.add("offset")
        if planes[g[0]][4] != bps:
            bad.add("step")
        out.append(bad)
    return out


def ciede_failing(ref, dist, ref_fs, dist_fs, planes, n, bps):
    """csrc/k_ciede.hip:253-258 and csrc/k_itp.hip:282-287 (one launch over the three planes) -> (the set of failing terms, class
    0 fails, class 1 fails by its own terms): plane 0's addresses are multiples of 4 samples, those of planes 1 and 2 of 4
    samples, or of 2 where the chroma is halved"""
    y, u, v = planes
    a0, a1 = 4 * bps, (2 if u[0] != y[0] else 4) * bps
    bad = set()
    if ref % a0:
        bad.add("ref")
    if dist % a0:
        bad.add("dist")
    if n > 1 and (ref_fs % a0 or dist_fs % a0):
        bad.add("frame_stride")
    if y[3] % a0 or u[3] % a1:
        bad.add("row_stride")
    if y[2] % a0 or u[2] % a1 or v[2] % a1:
        bad.add("offset")
    if y[4] != bps or u[4] != bps:
        bad.add("step")
    if y[0] % 4:
        bad.add("w4")
    bits0 = ref | dist | y[3] | y[2] | ((ref_fs | dist_fs) if n > 1 else 0)
    return bad, bits0 % a0 != 0, (u[3] | u[2] | v[2]) % a1 != 0


def artifacts_paths(frames, fs, planes, n, isz):
    """csrc/k_artifacts.hip:71-74 and 190-195 -> the load paths its workgroups take, one per frame and plane: "planar4" (one
    aligned load of four samples), "packed4" (three dwords of four bgr24 pixels) or "single" (sample by sample)"""
    out = set()
    for g in groups_of(planes):
        rs, step = planes[g[0]][3], planes[g[0]][4]
        offs = [planes[i][2] for i in g]
        pixel0 = min(offs)
        packed = isz == 1 and len(g) == 3 and step == 3 and sorted(o - pixel0 for o in offs) == [0, 1, 2]
        for f in range(n):
            for o in offs:
                if step == isz and ((frames + f * fs + o) | rs) % (4 * isz) == 0:
                    out.add("planar4")
                elif packed and ((frames + f * fs + pixel0) | rs) % 4 == 0:
                    out.add("packed4")
                else:
                    out.add("single")
    return out


def ffmpeg_kernels(ref, dist, ref_fs, dist_fs, planes, depth):
    """csrc/k_quality.hip:1027-1066 -> the vf_ssim kernel every plane goes to"""
    out = []
    for g in groups_of(planes):
        p = planes[g[0]]
        if depth > 8:
            a8 = (ref | dist | ref_fs | dist_fs | p[3]) % 8 == 0
            out += ["ffmpeg16<true>" if a8 and planes[i][4] == 2 and planes[i][2] % 8 == 0 else "ffmpeg16<false>" for i in g]
            continue
        al = (ref | dist | ref_fs | dist_fs | p[3]) % 4 == 0
        if (al and len(g) == 3 and p[4] == 3 and p[2] % 4 == 0 and planes[g[1]][2] == p[2] + 1 and planes[g[2]][2] == p[2] + 2 and
                g[1] == g[0] + 1 and g[2] == g[0] + 2):
            out += ["fast<3>"] * 3
            continue
        out += ["fast<1>" if al and planes[i][4] == 1 and planes[i][2] % 4 == 0 else "ffmpeg" for i in g]
    return out


def engine_gray_pitch(w):
    """csrc/vqa_capi.hip:1075: the pitch of the gray planes the complexity batch builds for its own kernels"""
    return (w + 63) // 64 * 64


def gray_hist_vec(bgr, h, w, frame_stride, row_stride):
    """csrc/k_gray_hist.hip:209: sixteen pixels per load.  The gray plane it writes is the engine's own: a fresh allocation at a
    pitch of engine_gray_pitch(w) and a plane stride of h pitches, multiples of 16 whatever the caller's layout"""
    gp = engine_gray_pitch(w)
    return w % 16 == 0 and bgr % 16 == 0 and frame_stride % 16 == 0 and row_stride % 16 == 0 and gp % 16 == 0 and (h * gp) % 16 == 0


def canny_dword_rows(w):
    """csrc/k_canny.hip:84 reads a dword per four pixels of a row: it needs pitch % 4 == 0.  The plane is the engine's own (see
    gray_hist_vec), so no layout of the caller's frames reaches the other side: the test asserts this one"""
    return engine_gray_pitch(w) % 4 == 0


def farneback_dword_rows(h, w):
    """csrc/k_farneback.hip:320: pitch, plane stride and pointer & 3 - again of the engine's own gray planes"""
    gp = engine_gray_pitch(w)
    return gp % 4 == 0 and (h * gp) % 4 == 0


# ---- non-vacuity, from numbers alone ---------------------------------------------------------------------------------------------
def reached(shots):
    """shots: dicts(kind of clip "planar3" | "planar1" | "packed" | "bgr", bps, depth, n, planes, ref, dist, prev0 (addresses),
    ref_fs, dist_fs, h, w) of the device submits of a matrix -> what they reach of every predicate above, as a dict of sets"""
    out = {"hvs_vec": set(), "hvs_alone": set(), "ciede_vec": set(), "ciede_alone": set(), "ciede_class": set(),
           "artifacts": set(), "ffmpeg": set(), "gray_hist": set(), "canny": set(), "farneback": set()}
    for s in shots:
        bps, pl = s["bps"], s["planes"]
        if s["clip"] == "bgr":
            for ptr, fs in ((s["ref"], s["ref_fs"]), (s["prev0"], s["ref_fs"])):
                out["gray_hist"].add(gray_hist_vec(ptr, s["h"], s["w"], fs, pl[0][3]))
            out["canny"].add(canny_dword_rows(s["w"]))
            out["farneback"].add(farneback_dword_rows(s["h"], s["w"]))
            continue
        for bad in psnr_hvs_failing(s["ref"], s["dist"], s["ref_fs"], s["dist_fs"], pl, s["n"], bps):
            out["hvs_vec"].add((bps, not bad))
            if len(bad) == 1:
                out["hvs_alone"].add((bps, min(bad)))
        if len(pl) == 3 and pl[1][3:5] == pl[2][3:5]:
            bad, c0, c1 = ciede_failing(s["ref"], s["dist"], s["ref_fs"], s["dist_fs"], pl, s["n"], bps)
            out["ciede_vec"].add((bps, not bad))
            if len(bad) == 1:
                out["ciede_alone"].add((bps, min(bad)))
            if c0 != c1:
                out["ciede_class"].add((bps, "class0" if c0 else "class1"))
        out["artifacts"] |= {(bps, p) for p in artifacts_paths(s["dist"], s["dist_fs"], pl, s["n"], bps)}
        out["ffmpeg"] |= set(ffmpeg_kernels(s["ref"], s["dist"], s["ref_fs"], s["dist_fs"], pl, s["depth"]))
    return out


HVS_TERMS = ("ref", "dist", "row_stride", "frame_stride", "offset")
CIEDE_TERMS = HVS_TERMS + ("w4",)


def assert_reached(got):
    """the conditions on the matrix: both sides of every choice, and every named term failing on its own"""
    for bps in (1, 2):
        assert {(bps, True), (bps, False)} <= got["hvs_vec"], ("psnr_hvs VEC", bps, got["hvs_vec"])
        assert {(bps, t) for t in HVS_TERMS} <= got["hvs_alone"], ("psnr_hvs, a term alone", bps, got["hvs_alone"])
        assert {(bps, True), (bps, False)} <= got["ciede_vec"], ("ciede / itp vec", bps, got["ciede_vec"])
        assert {(bps, t) for t in CIEDE_TERMS} <= got["ciede_alone"], ("ciede / itp, a term alone", bps, got["ciede_alone"])
        assert {(bps, "class0"), (bps, "class1")} <= got["ciede_class"], ("ciede / itp, a class alone", bps, got["ciede_class"])
        assert {(bps, "planar4"), (bps, "single")} <= got["artifacts"], ("artifacts", bps, got["artifacts"])
    assert (1, "packed4") in got["artifacts"] and (2, "packed4") not in got["artifacts"], got["artifacts"]
    assert {"fast<1>", "fast<3>", "ffmpeg", "ffmpeg16<true>", "ffmpeg16<false>"} <= got["ffmpeg"], got["ffmpeg"]
    assert got["gray_hist"] == {True, False}, got["gray_hist"]
    assert got["canny"] == {True} and got["farneback"] == {True}      # (the engine's own planes: see canny_dword_rows)


# ---- the clips -------------------------------------------------------------------------------------------------------------------
# name -> (chroma | "bgr24" | "gray", width, height, depth).  The smallest that reach both sides of the width tests: 48 x 72 has
# whole patches of 4 and blocks of 8 in luma and chroma (24 x 36), 41 x 71 (chroma 21 x 36) every remainder; VCA wants 32 x 32
# of every plane, so its 4:2:0 clips are wider (chroma 32 x 36 and 33 x 36)
CLIPS = {
    "yuv420p-48x72": ("420", 48, 72, 8), "yuv420p-41x71": ("420", 41, 71, 8),
    "yuv420p10-48x72": ("420", 48, 72, 10), "yuv420p10-41x71": ("420", 41, 71, 10),
    "yuv444p-48x72": ("444", 48, 72, 8), "yuv444p-41x71": ("444", 41, 71, 8),
    "yuv444p10-48x72": ("444", 48, 72, 10), "yuv444p10-41x71": ("444", 41, 71, 10),
    "bgr24-40x56": ("bgr24", 40, 56, 8), "bgr24-37x53": ("bgr24", 37, 53, 8),
    "gray16-50x70": ("gray", 50, 70, 16),
}
VCA_CLIPS = {"yuv420p-64x72": ("420", 64, 72, 8), "yuv420p-65x71": ("420", 65, 71, 8),
             "yuv420p10-64x72": ("420", 64, 72, 10), "yuv420p10-65x71": ("420", 65, 71, 10)}
MS_CLIPS = {"gray8-170x161": ("gray", 170, 161, 8)}
BGR_CLIPS = {"bgr-48x64": ("bgr24", 48, 64, 8), "bgr-37x53": ("bgr24", 37, 53, 8)}      # the complexity batch's
ANCHOR = {"vca": "yuv420p-64x72", "ms": "gray8-170x161", "complexity": "bgr-48x64"}     # every other kind: the 8-bit 4:2:0 clip
ANCHOR_DEFAULT = "yuv420p-48x72"
FRAMES = 3


def clips_of(kind):
    """the clips a kind is run on"""
    if kind == "complexity":
        return dict(BGR_CLIPS)
    if kind == "ms":
        return dict(MS_CLIPS)
    if kind == "vca":
        return dict(VCA_CLIPS, **{k: v for k, v in CLIPS.items() if not k.startswith("yuv420p")})
    return dict(CLIPS)


def clip_planes(entry):
    from rtvqa_amd.engine import bgr_planes, yuv_planes
    chroma, w, h, depth = entry
    if chroma == "bgr24":
        return bgr_planes(h, w)
    return yuv_planes(h, w, "mono" if chroma == "gray" else chroma, depth)


def clip_cases(name, entry):
    planes = clip_planes(entry)
    isz = 2 if entry[3] > 8 else 1
    cases = complexity_cases() if name in BGR_CLIPS else cases_for(planes, isz)
    return [c for c in cases if applies(c.ref, planes, isz)]


def device_args(c, res, addr):
    """one case on device memory: addr = {"ref" | "dist" | "prev0": the address of that canvas's first byte} -> dict(planes,
    ref, dist, prev0 (addresses or None), ref_fs, dist_fs)"""
    out = {"planes": with_lead(res["planes"], res["ref"][2]) if c.lead_in_offsets else res["planes"]}
    for key in ("ref", "dist", "prev0"):
        out[key] = None if res[key] is None else addr[key] + (0 if c.lead_in_offsets else res[key][2])
    out["ref_fs"] = res["ref"][1]
    out["dist_fs"] = res["dist"][1] if res["dist"] is not None else res["ref"][1]
    return out


def shot_of(name, entry, args, n=FRAMES):
    """device_args -> the dict reached() reads (a stream the clip lacks counts as the reference's)"""
    chroma, w, h, depth = entry
    kind = "bgr" if name in BGR_CLIPS else "packed" if chroma == "bgr24" else "planar1" if chroma == "gray" else "planar3"
    ref = args["ref"]
    return dict(clip=kind, bps=2 if depth > 8 else 1, depth=depth, n=n, planes=args["planes"], ref=ref,
                dist=ref if args["dist"] is None else args["dist"], prev0=ref if args["prev0"] is None else args["prev0"],
                ref_fs=args["ref_fs"], dist_fs=args["dist_fs"], h=h, w=w)
