"""CPU: the embedding of tests/layout_cases.py is what tests/test_gpu_layouts.py takes it for - every sample where the descriptors
say, filler everywhere else, nothing outside the canvas - and the matrix reaches both sides of every launch-time choice it names
(evaluated on offsets and strides alone, every canvas at a 256-aligned address)."""
import numpy as np
import pytest

import layout_cases as LC

ALL_CLIPS = dict(LC.CLIPS, **LC.VCA_CLIPS, **LC.MS_CLIPS, **LC.BGR_CLIPS)
N = LC.FRAMES


def _clip(entry, seed):
    """a tight clip of distinct samples that avoid both fill values"""
    planes = LC.clip_planes(entry)
    depth = entry[3]
    dt = np.uint16 if depth > 8 else np.uint8
    samples = max(p[2] + (p[1] - 1) * p[3] + (p[0] - 1) * p[4] + dt().itemsize for p in planes) // dt().itemsize
    rng = np.random.default_rng(seed)
    return rng.integers(1, (1 << depth) - 1, (N, samples)).astype(dt), planes


def _specs(name, entry):
    """every Spec a clip's cases use, the streams' own included"""
    out = {}
    for c in LC.clip_cases(name, entry):
        for s in (c.ref, c.dist, c.prev0):
            if s is not None:
                s = c.ref._replace(lead=s.lead, frame_pad=s.frame_pad)
                out[s[1:]] = s
        if "host" in c.mems:
            out[LC.host_spec(c.ref)[1:]] = LC.host_spec(c.ref)
    return list(out.values())


@pytest.mark.parametrize("name", list(ALL_CLIPS))
def test_the_embedding_round_trips_and_the_fill_owns_the_rest(name):
    entry = ALL_CLIPS[name]
    x, planes = _clip(entry, 7)
    isz, peak = x.dtype.itemsize, (1 << (8 * x.dtype.itemsize)) - 1
    specs = _specs(name, entry)
    assert len(specs) >= 10
    for s in specs:
        want = LC.tight_planes_of(x, LC.selected(planes, s))
        canvases = []
        for fill in (0, peak):
            canvas, new, fb, lb = LC.embed(x, planes, s, fill)
            assert canvas.dtype == x.dtype and canvas.size * isz == lb + N * fb, s.name        # lead + n frame strides, no more
            got = LC.extract(canvas, new, N, fb, lb)
            assert all((g == w).all() for g, w in zip(got, want)) and len(got) == len(want), s.name
            # all planes of the layout (a selection leaves the others' samples where they are): none overlaps, all are inside
            every = LC.embed(x, planes, s._replace(select=None), fill)[1]
            count = LC.owned(every, N, fb, lb, isz, canvas.size)
            assert count.max() == 1 and count.sum() == N * sum(p[0] * p[1] for p in planes), s.name
            assert (canvas[count == 0] == fill).all() and (canvas[count == 1] != fill).all(), s.name
            if isz == 2:
                assert all(v % 2 == 0 for p in new for v in p[2:5]) and fb % 2 == 0 and lb % 2 == 0, s.name
            for p in new:                            # the ABI's own row rule (csrc/vqa_capi.hip, check_planes)
                assert p[3] >= p[0] * p[4] - (p[4] - isz) and fb >= max(q[2] + (q[1] - 1) * q[3] + (q[0] - 1) * q[4] + isz for q in new)
            canvases.append(canvas)
            if s != LC.host_spec(s):                 # only a device view can take it: the lead is in the pointer
                continue
            host = LC.host_rows(canvas, N, fb, lb, fill)
            span = max(q[2] + (q[1] - 1) * q[3] + (q[0] - 1) * q[4] + isz for q in LC.with_lead(new, lb))
            assert span <= fb, s.name                # the ABI's rule for a lead carried in the offsets
            assert host.shape[0] == N and (N - 1) * fb + span <= host.nbytes and span <= host[0].nbytes, s.name
            assert (host.reshape(-1)[:canvas.size] == canvas).all() and (host.reshape(-1)[canvas.size:] == fill).all()
        assert ((canvases[0] != canvases[1]) == (count == 0)).all(), s.name       # the two fills differ in the filler alone
    assert all(c.ref == LC.host_spec(c.ref) for c in LC.clip_cases(name, entry) if c.lead_in_offsets)
    tight = LC.embed(x, planes, LC.TIGHT, 0)
    assert (tight[0].reshape(N, -1) == x).all() and tight[1] == [tuple(p) for p in planes] and tight[3] == 0


def test_a_descriptor_outside_the_canvas_is_noticed():
    x, planes = _clip(LC.CLIPS["yuv420p-41x71"], 3)
    canvas, new, fb, lb = LC.embed(x, planes, LC.spec("lead1", lead=1), 0)
    with pytest.raises(IndexError):
        LC.owned(LC.with_lead(new, lb + 1), N, fb, 0, 1, canvas.size)
    LC.owned(LC.with_lead(new, lb - 1), N, fb, 0, 1, canvas.size)               # the shifted control stays inside


def test_every_clip_has_the_cases_the_matrix_names():
    for name, entry in ALL_CLIPS.items():
        cases = LC.clip_cases(name, entry)
        names = [c.name for c in cases]
        assert len(set(names)) == len(names) and names[0] == "tight", name
        leads = {c.ref.lead for c in cases}
        if name in LC.BGR_CLIPS or entry[0] == "bgr24":
            assert {0, 1, 2, 3} <= leads and {0, 1, 2, 3} <= {c.ref.row_pad for c in cases}, name
        else:
            assert {0, 1, 2, 3, 4, 8} <= leads, name
            pads = {p for c in cases for p in ((c.ref.row_pad,) if isinstance(c.ref.row_pad, int) else c.ref.row_pad)}
            assert {0, 1, 2, 3} <= pads, name
        assert {0, 1, 5} <= {c.ref.frame_pad for c in cases}, name
        assert any(c.dist is not None and (c.dist.lead, c.dist.frame_pad) != (c.ref.lead, c.ref.frame_pad) for c in cases), name
        assert any(c.prev0 is not None and c.prev0.lead != c.ref.lead for c in cases), name
        assert all(c.mems == LC.DEVICE for c in cases if c.dist is not None or c.prev0 is not None or c.lead_in_offsets), name
        if name in LC.BGR_CLIPS:
            assert all(c.mems == LC.DEVICE and c.ref.step is None and c.ref.select is None for c in cases), name
            continue
        if entry[0] == "bgr24":
            assert {(2, 1, 0), (1,), (0, 2)} <= {c.ref.select for c in cases} and any(c.ref.step == (4,) for c in cases), name
        elif entry[0] != "gray":
            assert any(c.ref.groups == LC.NV12 and c.ref.step == (1, 2) for c in cases), name
            assert any(c.ref.gap == 1 for c in cases) and any(c.ref.select == (0, 2, 1) for c in cases), name
            split = [c.ref.row_pad for c in cases if not isinstance(c.ref.row_pad, int) and len(c.ref.row_pad) == 3]
            assert any(p[1] != p[2] for p in split) and any(p[0] != p[1] for p in split), name      # U against V; Y against U / V


def test_the_matrix_reaches_both_sides_of_every_launch_time_choice():
    shots, base = [], 1 << 20
    for name, entry in dict(LC.CLIPS, **LC.BGR_CLIPS).items():
        x, planes = _clip(entry, 1)
        for c in LC.clip_cases(name, entry):
            res = LC.resolve(c, x, planes, 0, prev0=x[0], dist=x)
            shots.append(LC.shot_of(name, entry, LC.device_args(c, res, {"ref": base, "dist": base + 256, "prev0": base + 512})))
    LC.assert_reached(LC.reached(shots))
