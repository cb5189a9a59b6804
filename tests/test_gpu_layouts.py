"""GPU: the same samples give the same bytes from any memory layout, for every kind of batch.

include/vqa.h promises that a plane's words do not depend on where its samples lie.  The other files reach offset, row stride,
pixel step and frame stride by the accident of their grids; several kernels choose their load path at launch from exactly these
numbers.  Here one small clip per sample type and geometry is laid out in the enumerated ways of tests/layout_cases.py - leads,
row pads (split over Y, U and V), gaps, frame pads, interleaved chroma, padded pixels, R, G, B order, single channels, streams
of one submit at different places - and submitted from pageable host memory (the lead in the offsets, frame_bytes) and from
device memory (views into ONE upload per clip), with filler bytes of 0x00 and of 0xFF.

Expected records: `base`, the same kind on the tight clip from host memory.  On the 8-bit 4:2:0 clip base passes once through the
kind's own checker, with the helpers and bars of tests/test_gpu_all_kinds.py::_anchor; no tolerance is introduced here.  Every
other comparison is of bytes, as tests/test_gpu_all_kinds.py::_wait returns them:
  1. every layout gives base;
  2. so do both fillers: nothing outside a plane enters a term;
  3. a control: the descriptors of one layout shifted by one sample do NOT give base;
  4. after the matrix the tight clip gives base again on the same context.
A kind is left out of a layout only where include/vqa.h has it refuse the descriptors (XPSNR and VCA off planar layouts, the
three-plane kinds on other plane counts or on U and V of different strides); the refusal is asserted instead.

test_the_matrix_reaches_both_sides_of_every_launch_time_choice evaluates the predicates of tests/layout_cases.py on the device
addresses the uploads actually got."""
import numpy as np
import pytest

import cambi_cases as CC
import hostile_cases as HK
import layout_cases as LC
import mdsi_cases as MC
import test_gpu_all_kinds as TAK

pytestmark = pytest.mark.gpu

KINDS = ("complexity", "gauss", "ffmpeg", "ms", "vif", "adm", "motion", "siti", "psnr_hvs", "ciede", "gmsd", "cambi", "xpsnr",
         "haarpsi", "vca", "artifacts", "brisque", "mdsi", "itp")
N = LC.FRAMES
THREE = ("ciede", "itp")                         # exactly three planes, taken together; MDSI: three or one
CONTROL = "lead2-in-offsets"                     # the case whose descriptors the control shifts: two samples of slack before frame 0


class Shot:
    """what tests/test_gpu_all_kinds.py::_submit, _wait and _anchor read of a job"""

    def __init__(self, kind, planes, host=None, dev=None, frame_bytes=None, model=None, **anchor):
        self.kind, self.planes, self.host, self.dev, self.frame_bytes, self.model = kind, planes, host, dev, frame_bytes, model
        self.__dict__.update(anchor)


def _content(name, entry, planes, content):
    """-> (ref, dist, prev0, lists): the tight clip, [N, samples] and [samples].  "natural": seeded noise on natural content, every
    plane of every frame seeded by itself.  "mdsi": mdsi_cases' contents (its checker admits no others), as TAK.Job has them.
    "cambi": cambi_cases' dithered staircase - on noise every word of CAMBI but k is 0 wherever the samples lie, and the control
    could not tell a shifted clip from the true one"""
    from rtvqa_amd import synth
    chroma, w, h, depth = entry
    seed = 1000 * (1 + sorted(list(LC.CLIPS) + list(LC.VCA_CLIPS) + list(LC.MS_CLIPS) + list(LC.BGR_CLIPS)).index(name))
    if name in LC.BGR_CLIPS:
        fr = synth.s_natural(N + 1, h, w, seed=seed)
        return np.ascontiguousarray(fr[1:]).reshape(N, -1), None, np.ascontiguousarray(fr[0]).reshape(-1), None
    dt = np.uint16 if depth > 8 else np.uint8
    if content == "mdsi":
        pairs = [MC.pair(TAK.MDSI_NAMES[i], "yuv420p", h, w, depth, seed=seed + i) for i in range(N)]
        lists = ([p[0] for p in pairs], [p[1] for p in pairs])
        return MC.pack(lists[0], "yuv420p", depth), MC.pack(lists[1], "yuv420p", depth), None, lists
    isz = dt().itemsize
    samples = max(p[2] + (p[1] - 1) * p[3] + (p[0] - 1) * p[4] + isz for p in planes) // isz
    out = np.zeros((2, N + 1, samples), dt)
    for i in range(N + 1):                       # (frame N is prev0)
        for j, p in enumerate(planes):
            if content == "cambi":
                pair = [CC.plane("dither", p[1], p[0], depth, seed + 10 * i + j + 5 * side) for side in (0, 1)]
            else:
                pair = HK.natural_pair(p[1], p[0], depth, seed + 10 * i + j)
            for side in (0, 1):
                LC._view(out[side, i], 0, p, isz)[...] = pair[side]
    return np.ascontiguousarray(out[0, :N]), np.ascontiguousarray(out[1, :N]), np.ascontiguousarray(out[0, N]), None


class Clip:
    """one tight clip, every case of its matrix embedded with both fillers, and all of it uploaded once"""

    def __init__(self, eng, name, entry, content="natural"):
        self.name, self.entry, self.bgr = name, entry, name in LC.BGR_CLIPS
        self.w, self.h, self.depth = entry[1], entry[2], entry[3]
        self.isz = 2 if self.depth > 8 else 1
        self.planes = [tuple(p) for p in LC.clip_planes(entry)]
        self.r, self.d, self.p0, self.lists = _content(name, entry, self.planes, content)
        self.cases = LC.clip_cases(name, entry)
        peak = (1 << (8 * self.isz)) - 1
        self.res, self.hres, parts, at = {}, {}, [], 0
        for ci, c in enumerate(self.cases):
            for fi, fill in enumerate((0, peak)):
                if "host" in c.mems:
                    self.hres[ci, fi] = LC.resolve(c, self.r, self.planes, fill, prev0=self.p0, dist=self.d, mem="host")
                res = LC.resolve(c, self.r, self.planes, fill, prev0=self.p0, dist=self.d)
                res["at"] = {}
                for key in ("ref", "dist", "prev0"):
                    if res[key] is not None:
                        res["at"][key] = at
                        parts.append((at, res[key][0]))
                        at += -(-res[key][0].nbytes // 256) * 256
                self.res[ci, fi] = res
        arena = np.zeros(at, np.uint8)
        for where, canvas in parts:
            arena[where:where + canvas.nbytes] = canvas.view(np.uint8)
        self.arena = eng.upload(arena[None, :])

    def free(self):
        self.arena._owner.free()

    def tight(self, select=None):
        return [self.planes[i] for i in (select if select is not None else range(len(self.planes)))]

    def host_of(self, a, n):
        """a tight stream as the engine's host argument"""
        if a is None:
            return None
        return a.reshape((n, self.h, self.w, 3) if n else (self.h, self.w, 3)) if self.bgr else a

    def base_shot(self, kind, select=None, model=None, **anchor):
        return Shot(kind, self.tight(select), host=(self.host_of(self.r, N), self.host_of(self.d, N), self.host_of(self.p0, 0)),
                    model=model, **anchor)

    def device_args(self, ci, fi):
        res = self.res[ci, fi]
        return LC.device_args(self.cases[ci], res, {k: self.arena.ptr + v for k, v in res["at"].items()})

    def shot(self, kind, ci, fi, mem, model=None, shift=0):
        """case ci with filler fi from `mem`; shift (bytes): the control's displacement of every descriptor"""
        if mem == "host":
            res = self.hres[ci, fi]
            peak = (1 << (8 * self.isz)) - 1
            canvas, fb, lb = res["ref"]
            rows = [None if res[k] is None else LC.host_rows(res[k][0], N if k != "prev0" else 1, fb, lb, (0, peak)[fi])
                    for k in ("ref", "dist", "prev0")]
            if rows[2] is not None:
                rows[2] = rows[2][0]
            return Shot(kind, LC.with_lead(res["planes"], lb + shift), host=tuple(rows), frame_bytes=fb, model=model)
        from rtvqa_amd.engine import DeviceFrames
        a = self.device_args(ci, fi)
        ch, rs = (3, a["planes"][0][3]) if self.bgr else (1, None)

        def view(ptr, n, fs):
            return None if ptr is None else DeviceFrames(ptr + (shift if self.bgr else 0), n, self.h, self.w, frame_stride=fs,
                                                         row_stride=rs, owner=self.arena._owner, channels=ch, itemsize=self.isz)
        planes = a["planes"] if self.bgr else LC.with_lead(a["planes"], shift)
        return Shot(kind, planes, dev=(view(a["ref"], N, a["ref_fs"]), view(a["dist"], N, a["dist_fs"]), view(a["prev0"], 1, a["ref_fs"])),
                    model=model)


@pytest.fixture(scope="module")
def clips(engine):
    """name, content -> Clip, built when first asked for and shared by the kinds"""
    made = {}

    def get(name, entry, content="natural"):
        if (name, content) not in made:
            made[name, content] = Clip(engine, name, entry, content)
        return made[name, content]
    yield get
    for c in made.values():
        c.free()


def _model(eng, kind, planes):
    """the colour model of the tight descriptors: a layout's pixel step must not change it"""
    return getattr(eng, kind + "_model")(planes) if kind in ("ciede", "mdsi", "itp") else None


def _refused(kind, planes, isz):
    """include/vqa.h: XPSNR and VCA take planar layouts; CIEDE2000 and dE_ITP three planes, MDSI three or one, whose second and
    third share stride and step"""
    if kind in ("xpsnr", "vca"):
        return any(p[4] != isz for p in planes)
    if kind in THREE + ("mdsi",):
        if len(planes) != 3:
            return kind in THREE or len(planes) != 1
        return tuple(planes[1][3:5]) != tuple(planes[2][3:5])
    return False


def _run(eng, shot, mem):
    TAK._submit(eng, shot, mem)
    return TAK._wait(eng, shot)


@pytest.mark.parametrize("kind", KINDS)
def test_every_layout_gives_the_bytes_of_the_tight_clip(engine, clips, oracle, kind):
    from rtvqa_amd import _native as NAT
    submits = 0
    for name, entry in LC.clips_of(kind).items():
        anchor = name == LC.ANCHOR.get(kind, LC.ANCHOR_DEFAULT)
        clip = clips(name, entry, "mdsi" if kind == "mdsi" and anchor else "cambi" if kind == "cambi" else "natural")
        base, refused = {}, set()

        def want(select):
            if select not in base:
                tight = clip.tight(select)
                base[select] = _run(engine, clip.base_shot(kind, select, _model(engine, kind, tight)), "host")
            return base[select][0]

        if _refused(kind, clip.planes, clip.isz):          # packed layouts for XPSNR and VCA, gray for the three-plane kinds
            with pytest.raises((ValueError, NAT.VqaError)):
                TAK._submit(engine, clip.base_shot(kind), "host")
            continue
        want(None)
        if anchor:                                         # base is what the kind's CPU reference says of these frames
            j = clip.base_shot(kind, None, index=0, n=N, h=clip.h, w=clip.w, depth=clip.depth, lists=clip.lists,
                               layout="gray" if entry[0] == "gray" else "yuv420p")
            TAK._anchor(j, base[None][1], oracle)
        for ci, c in enumerate(clip.cases):
            tight = clip.tight(c.ref.select)
            model = _model(engine, kind, tight)
            if _refused(kind, clip.res[ci, 0]["planes"], clip.isz):
                key = (c.ref.select, c.ref.groups, c.ref.step, c.ref.row_pad)
                if key not in refused:                     # each refused shape of descriptors once
                    refused.add(key)
                    with pytest.raises((ValueError, NAT.VqaError)):
                        TAK._submit(engine, clip.shot(kind, ci, 0, c.mems[0], model), c.mems[0])
                continue
            for fi in (0, 1):
                for mem in c.mems:
                    got = _run(engine, clip.shot(kind, ci, fi, mem, model), mem)[0]
                    submits += 1
                    assert got == want(c.ref.select), (kind, name, c.name, "filler %s" % ("0x00", "0xFF")[fi], mem)
        # the control: one sample earlier is inside the canvas (the lead is two) and is another clip
        ci = [c.name for c in clip.cases].index(CONTROL) if not clip.bgr else [c.name for c in clip.cases].index("lead2-pad0")
        assert clip.cases[ci].ref.lead >= 1 and clip.cases[ci].ref.select is None
        model = _model(engine, kind, clip.planes)
        assert _run(engine, clip.shot(kind, ci, 0, "device", model), "device")[0] == want(None)
        assert _run(engine, clip.shot(kind, ci, 0, "device", model, shift=-clip.isz), "device")[0] != want(None), (kind, name, "control")
        # and the context is as it was: the tight clip again
        assert _run(engine, clip.base_shot(kind, None, model), "host")[0] == want(None), (kind, name, "tight again")
    print("layouts:", kind, submits, "submits of the matrix")
    assert submits >= 50


def test_the_matrix_reaches_both_sides_of_every_launch_time_choice(engine, clips):
    """from the addresses the uploads got: the vector and the sample-by-sample side of k_psnr_hvs, k_ciede and k_itp with every
    named term failing on its own; planar4, packed4 and neither in k_artifacts; all five vf_ssim kernels; both sides of
    k_gray_hist's sixteen-pixel load (Canny and Farneback read the engine's own planes: one side, asserted as such)"""
    shots = []
    for name, entry in dict(LC.CLIPS, **LC.BGR_CLIPS).items():
        clip = clips(name, entry)
        assert clip.arena.ptr % 256 == 0
        for ci in range(len(clip.cases)):
            shots.append(LC.shot_of(name, entry, clip.device_args(ci, 0)))
    got = LC.reached(shots)
    print("layouts, reached:", {k: sorted(v, key=str) for k, v in got.items()})
    LC.assert_reached(got)
