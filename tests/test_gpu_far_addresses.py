"""GPU: frames, planes and rows that start beyond byte 2^31 and 2^32 of their stream give the bytes of the tight clip, for every kind.

include/vqa.h gives every submit 64-bit frame strides and every vqa_plane_desc a 64-bit offset and row stride, and a resident
clip of a few hundred 2160p frames uses them.  The other files stay within a few hundred kilobytes.  Here ONE device arena of
far_cases.ARENA bytes (uninitialised; freed at the end of the module) holds the samples of the cases of tests/far_cases.py - F1 far
frames (both streams with one stride, and with two), F2 far planes, F3 far rows - each written once with vqa_copy_h2d in pieces of
at most a few hundred KB, and every kind reads them in place through DeviceFrames views.  tests/test_far_host.py proves on the CPU
that every described byte is inside the arena and outside its guards, that no two pieces share a byte, and that an address whose
32-bit term wrapped is still a byte of the arena: a kernel with a forgotten cast gives wrong numbers, not a fault.

Expected records: `base`, the same kind on the tight clip from host memory (the frames of F1; frame 0 alone for F2 and F3).  On the
8-bit clip base passes once through the kind's own checker (tests/test_gpu_all_kinds.py::_anchor; PU21 through
depth_cases.pu21_check); no tolerance is introduced here.  Every other comparison is of bytes:
  1. F1a, F1b, F2 and F3 give base;
  2. the Gaussian modes refuse F3 with VQA_ERR_UNSUPPORTED (include/vqa.h: rows spanning 2^31 bytes) and leave the context usable;
  3. a control: the descriptors of F1a moved one sample on do NOT give base;
  4. after the cases the tight clip gives base again."""
import numpy as np
import pytest

import cambi_cases as CC
import depth_cases as DC
import far_cases as FC
import hostile_cases as HK
import layout_cases as LC
import mdsi_cases as MC
import test_gpu_all_kinds as TAK
import test_gpu_layouts as TL

pytestmark = pytest.mark.gpu

KINDS = TL.KINDS + ("pu21",)
GAUSSIAN = ("gauss", "ms")
N = FC.N_FRAMES


def _tight(name, content):
    """-> (ref, dist, prev0, lists): [N, samples], [N, samples], [samples] of the clip's sample type; a bgr clip: frames, None, prev0"""
    from rtvqa_amd import synth
    layout, h, w, depth = FC.entry(name)
    seed = 7000 + 100 * sorted(list(FC.CLIPS) + list(FC.ROW_CLIPS)).index(name)
    if layout == "bgr":
        fr = synth.s_natural(N + 1, h, w, seed=seed)
        return np.ascontiguousarray(fr[1:]).reshape(N, -1), None, np.ascontiguousarray(fr[0]).reshape(-1), None
    if content == "mdsi":
        pairs = [MC.pair(TAK.MDSI_NAMES[i], "yuv420p", h, w, depth, seed=seed + i) for i in range(N)]
        lists = ([p[0] for p in pairs], [p[1] for p in pairs])
        r, d = MC.pack(lists[0], "yuv420p", depth), MC.pack(lists[1], "yuv420p", depth)
        return r, d, np.ascontiguousarray(d[N - 1]), lists
    dt = np.uint16 if depth > 8 else np.uint8
    planes = FC.tight_planes(name)
    out = np.zeros((2, N + 1, FC.frame_bytes(name) // dt().itemsize), dt)
    for i in range(N + 1):                       # (frame N is prev0)
        for j, p in enumerate(planes):
            if content == "cambi":
                pair = [CC.plane("dither", p[1], p[0], depth, seed + 10 * i + j + 5 * side) for side in (0, 1)]
            else:
                pair = HK.natural_pair(p[1], p[0], depth, seed + 10 * i + j)
            for side in (0, 1):
                LC._view(out[side, i], 0, p, dt().itemsize)[...] = pair[side]
    return np.ascontiguousarray(out[0, :N]), np.ascontiguousarray(out[1, :N]), np.ascontiguousarray(out[0, N]), None


class Arena:
    """the one allocation, the tight clips and what has been written of them"""

    def __init__(self, eng):
        from rtvqa_amd.engine import DeviceBuffer
        self.eng, self.buf = eng, DeviceBuffer(eng, FC.ARENA)
        self.clips, self.placed, self.copies = {}, {}, 0

    def free(self):
        self.buf.free()

    def clip(self, name, content):
        if (name, content) not in self.clips:
            self.clips[name, content] = _tight(name, content)
        return self.clips[name, content]

    def place(self, name, content, case):
        """-> far_cases.Placed, its samples in the arena (written the first time it is asked for)"""
        from rtvqa_amd import _native as NAT
        key = (name, content, case)
        if key in self.placed:
            return self.placed[key]
        pl = FC.place(name, content, case)
        r, d, p0, _lists = self.clip(name, content)
        src = {"ref": r, "dist": d if d is not None else r, "prev0": p0[None]}
        tight, keep = FC.tight_planes(name), []
        for at, nbytes, stream, f, pi, row in FC.runs(pl):
            assert FC.GUARD <= at and at + nbytes <= FC.ARENA - FC.GUARD and nbytes <= 1 << 19
            if pi is None:
                piece = np.zeros(nbytes, np.uint8)
            else:
                plane = LC._view(src[stream][f], 0, tight[pi], pl.isz)
                piece = np.ascontiguousarray(plane if row is None else plane[row]).view(np.uint8).reshape(-1)
            assert piece.nbytes == nbytes
            keep.append(piece)
            NAT.check(self.eng.lib.vqa_copy_h2d(self.eng.ctx, self.buf.ptr + at, piece.ctypes.data, nbytes), "h2d", self.eng.ctx)
        self.eng.sync()
        self.copies += len(keep)
        self.placed[key] = pl
        return pl

    def shot(self, kind, name, content, case, model=None, shift=0):
        """the case as a device submit; shift (bytes): the control's displacement of every descriptor"""
        from rtvqa_amd.engine import DeviceFrames
        pl = self.place(name, content, case)
        layout, h, w, _depth = FC.entry(name)
        bgr = layout == "bgr"

        def view(key, n):
            spot, fs = pl.streams[key]
            return DeviceFrames(self.buf.ptr + spot + (shift if bgr else 0), n, h, w, frame_stride=fs, row_stride=pl.row_stride if bgr else None,
                                owner=self.buf, channels=3 if bgr else 1, itemsize=pl.isz)
        planes = None if bgr else LC.with_lead(pl.planes, shift)
        return TL.Shot(kind, planes, dev=(view("ref", pl.n), None if bgr else view("dist", pl.n), view("prev0", 1)), model=model)

    def base_shot(self, kind, name, content, n, model=None, **anchor):
        layout, h, w, _depth = FC.entry(name)
        r, d, p0, _lists = self.clip(name, content)
        if layout == "bgr":
            return TL.Shot(kind, None, host=(r[:n].reshape(n, h, w, 3), None, p0.reshape(h, w, 3)), model=model, **anchor)
        return TL.Shot(kind, FC.tight_planes(name), host=(r[:n], d[:n], p0), model=model, **anchor)


@pytest.fixture(scope="module")
def arena(engine):
    a = Arena(engine)
    yield a
    print("far addresses: %d pieces written into the arena" % a.copies)
    a.free()


def _run(eng, shot, mem):
    if shot.kind == "pu21":                      # (not in tests/test_gpu_all_kinds.py::_submit: a branch of its own)
        r, d, _p0 = shot.dev if mem == "device" else shot.host
        eng.pu21_submit(r, d, shot.planes)
        raw = eng.pu21_wait()
        return (raw.tobytes(),), raw
    TAK._submit(eng, shot, mem)
    return TAK._wait(eng, shot)


def _model(eng, kind, name):
    return TL._model(eng, kind, FC.tight_planes(name))


def _content(kind, name):
    return "mdsi" if kind == "mdsi" and name == FC.ANCHOR_DEFAULT else "cambi" if kind == "cambi" else "natural"


def _clips_of(kind):
    if kind == "complexity":
        return ["bgr-66x98"], ["bgr-34x50"]
    if kind == "ms":
        return ["gray8-177x263"], ["yuv420p-34x50"]
    if kind == "vca":                            # 32 x 32 blocks: no 17-row chroma
        return ["yuv420p-66x98", "yuv420p10-70x74"], ["gray8-33x50", "gray10-33x50"]
    return ["yuv420p-66x98", "yuv420p10-70x74"], ["yuv420p-34x50", "yuv420p10-34x50"]


def _anchor(kind, name, content, raw, clip, oracle):
    layout, h, w, depth = FC.entry(name)
    r, d, p0, lists = clip
    if kind == "pu21":
        DC.pu21_check(raw, r, d, FC.tight_planes(name), depth, "pq", "far addresses, base: pu21 %s" % name)
        return
    planes = FC.tight_planes(name) if layout != "bgr" else None
    host = (r.reshape(N, h, w, 3), None, p0.reshape(h, w, 3)) if layout == "bgr" else (r, d, p0)
    j = TL.Shot(kind, planes, host=host, index=0, n=N, h=h, w=w, depth=depth, lists=lists, layout="gray" if layout == "gray" else "yuv420p")
    TAK._anchor(j, raw, oracle)


def _the_row_rule_alone_refuses_ms(eng, arena):
    """one gray plane of far_cases.MS_ROWS rows, which MS-SSIM's size limit admits: refused at the row stride whose rows span 2^31
    bytes, taken at half that stride - so the refusal is the row rule's.  Nothing is written there (far_cases says why that is
    safe): the accepted submit's figures are waited for and dropped"""
    from rtvqa_amd import _native as NAT
    from rtvqa_amd.engine import DeviceFrames
    n = FC.MS_ROWS
    for rs, refused in ((FC.MS_FAR, True), (FC.MS_NEAR, False)):
        views = [DeviceFrames(arena.buf.ptr + FC.MS_SPOT + off, 1, n, n, frame_stride=n * rs, row_stride=None, owner=arena.buf, channels=1,
                              itemsize=1) for off in (0, FC.MS_DIST)]
        shot = TL.Shot("ms", [(n, n, 0, rs, 1)], dev=(views[0], views[1], None))
        if refused:
            with pytest.raises(NAT.VqaError) as err:
                _run(eng, shot, "device")
            assert err.value.status == NAT.VQA_ERR_UNSUPPORTED, rs
        else:
            res = _run(eng, shot, "device")[1][0]
            assert res.shape == (1, 1), rs


@pytest.mark.parametrize("kind", KINDS)
def test_far_frames_planes_and_rows_give_the_bytes_of_the_tight_clip(engine, arena, oracle, kind):
    from rtvqa_amd import _native as NAT
    main, rows = _clips_of(kind)
    ran, bases = [], {}
    for name in main:
        content = _content(kind, name)
        model = _model(engine, kind, name)
        base = {n: _run(engine, arena.base_shot(kind, name, content, n, model), "host") for n in (N, 1)}
        if name == FC.ANCHOR.get(kind, FC.ANCHOR_DEFAULT):
            _anchor(kind, name, content, base[N][1], arena.clip(name, content), oracle)
        for case in FC.cases_of(name):
            pl = arena.place(name, content, case)
            got = _run(engine, arena.shot(kind, name, content, case, model), "device")[0]
            assert got == base[pl.n][0], (kind, name, case)
            ran.append(case)
        # the control: one sample on is inside what was written (a zero sample follows every F1 frame) and is another clip
        isz = FC.isz_of(name)
        assert _run(engine, arena.shot(kind, name, content, "F1a", model, shift=isz), "device")[0] != base[N][0], (kind, name, "control")
        bases[name] = base[N][0]
    for name in rows:
        content = _content(kind, name)
        model = _model(engine, kind, name)
        if kind in GAUSSIAN:                     # vqa.h: the Gaussian modes address a plane's rows with 32 bits and say so
            with pytest.raises(NAT.VqaError) as err:
                _run(engine, arena.shot(kind, name, content, "F3", model), "device")
            assert err.value.status == NAT.VQA_ERR_UNSUPPORTED, (kind, name)
            ran.append("F3 refused")
            continue
        want = _run(engine, arena.base_shot(kind, name, content, 1, model), "host")[0]
        assert _run(engine, arena.shot(kind, name, content, "F3", model), "device")[0] == want, (kind, name, "F3")
        assert _run(engine, arena.base_shot(kind, name, content, 1, model), "host")[0] == want, (kind, name, "tight again")
        ran.append("F3")
    if kind == "ms":                             # (the 34 x 50 clip is below MS-SSIM's 161 x 161: refused for its size, rule or no rule)
        _the_row_rule_alone_refuses_ms(engine, arena)
        ran.append("F3 refused at 161 rows")
    for name in main:                            # and the context is as it was: the tight clip again
        content = _content(kind, name)
        model = _model(engine, kind, name)
        assert _run(engine, arena.base_shot(kind, name, content, N, model), "host")[0] == bases[name], (kind, name, "tight again")
    print("far addresses:", kind, ran)
    assert {"F1a", "F1b"} <= set(ran) and ("F3" in ran or "F3 refused" in ran) and ("F2" in ran or kind == "complexity")
