"""GPU: the same samples give the same bytes from any memory layout, for the signal statistics.  The enumerated matrix of
tests/layout_cases.py - leads, row pads, gaps, frame pads, interleaved chroma, padded packed pixels, R, G, B order, single channels,
the stream and prev0 at different places - as tests/test_gpu_layouts.py runs it for the other kinds: every case from pageable host
memory and from views into one upload, with filler bytes of 0x00 and of 0xFF, gives the records AND the profiles of the tight
clip; the tight clip's words are the restatement's; descriptors shifted by one sample do not give them.

k_sigstats_accum chooses between one 4- or 8-byte load and four sample loads from the pixel step and the address of every row
segment: the matrix holds both sides (tight planar rows whose segments are aligned, leads and pads that misalign them, steps of
2, 3 and 4)."""
import numpy as np
import pytest

import layout_cases as LC
import motion_cases as K
import sigstats_reference as R
import test_gpu_layouts as TL

pytestmark = pytest.mark.gpu

N = LC.FRAMES
CONTROL = "lead2-in-offsets"


def _run(eng, shot, mem):
    r, _d, p0 = shot.dev if mem == "device" else shot.host
    fb = {"frame_bytes": shot.frame_bytes} if mem == "host" and shot.frame_bytes else {}
    rec, sums = eng.sigstats(r, shot.planes, prev0=p0, profiles=True, **fb)
    return rec.tobytes(), tuple(s[k].tobytes() for s in sums for k in ("rows", "cols")), rec


@pytest.mark.parametrize("name", list(LC.CLIPS))
def test_every_layout_gives_the_bytes_of_the_tight_clip(engine, name):
    entry = LC.CLIPS[name]
    clip = TL.Clip(engine, name, entry)
    try:
        base = {}

        def want(select):
            if select not in base:
                base[select] = _run(engine, clip.base_shot("sigstats", select), "host")
            return base[select][:2]

        # the tight clip's words are the restatement's
        rec = (want(None), base[None][2])[1]
        for j, p in enumerate(clip.planes):
            series = K.plane_series(clip.r, p)
            ref = R.series(series, clip.depth, K.plane_series(clip.p0[None], p)[0])
            for i in range(N):
                assert not R.same_words(rec[i, j], ref[i]), (name, i, j, R.same_words(rec[i, j], ref[i]))
        submits = 0
        for ci, c in enumerate(clip.cases):
            for fi in (0, 1):
                for mem in c.mems:
                    got = _run(engine, clip.shot("sigstats", ci, fi, mem), mem)[:2]
                    submits += 1
                    assert got == want(c.ref.select), (name, c.name, "filler %s" % ("0x00", "0xFF")[fi], mem)
        # the control: one sample earlier is inside the canvas (the lead is two) and is another clip
        ci = [c.name for c in clip.cases].index(CONTROL)
        assert clip.cases[ci].ref.lead >= 1 and clip.cases[ci].ref.select is None
        assert _run(engine, clip.shot("sigstats", ci, 0, "device"), "device")[:2] == want(None)
        assert _run(engine, clip.shot("sigstats", ci, 0, "device", shift=-clip.isz), "device")[:2] != want(None), (name, "control")
        # and the context is as it was: the tight clip again
        assert _run(engine, clip.base_shot("sigstats"), "host")[:2] == want(None), (name, "tight again")
        print("layouts: sigstats", name, submits, "submits of the matrix")
        assert submits >= 40
    finally:
        clip.free()
