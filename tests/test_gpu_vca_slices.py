"""GPU: the frame-slice seam of the VCA features.  vqa_vca_submit cuts a batch into slices of 32768 frames like every plane-batch
kind; what is its own is that the block map has one slot more than frames and a slice's first frame finds its predecessor - the
previous slice's LAST frame - in the slot the slice before filled.  One child process on the lab library creates an engine with
VQA_QSLICE unset and one with VQA_QSLICE=3 and runs the pool of tests/slice_cases.py (4:2:0 at 67 x 99, 8 and 10 bits: two
geometry groups per slice, a chroma plane of one block) at n = 3, 4 and 8 - one slice, one frame over, 3 + 3 + 2 -, with and
without prev0, from host and from device frames: the sliced engine's records and block words equal the unsliced engine's byte
for byte, and the unsliced records of every frame, the seam frames among them, are within the bar of the float64 restatement
with the right frame before them (l_sum equal to the quantised restatement's).  Then
32771 frames of 32 x 32 through the shipped library: every record equals the record one pool period before it, and the first
eight equal a short batch's."""
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path[:0] = [REPO, os.path.dirname(os.path.abspath(__file__))]

import motion_cases as K
import slice_cases as SC
import vca_reference as R

pytestmark = pytest.mark.gpu

PREV0_ENTRY = 6
BIG = ("mono", 32, 32, 8)


def _run(eng, r, planes, prev0):
    rec, maps = eng.vca(r, planes, prev0=prev0, blocks=True)
    return rec.tobytes() + b"".join(m[k].tobytes() for m in maps for k in ("qh", "s"))


def _child(out_path):
    import rtvqa_amd
    os.environ.pop("VQA_QSLICE", None)
    engines = {"plain": rtvqa_amd.Engine(0)}
    os.environ["VQA_QSLICE"] = "3"               # read once, in vqa_create
    engines["sliced"] = rtvqa_amd.Engine(0)
    os.environ.pop("VQA_QSLICE")
    assert engines["plain"].lib.vqa_build_flavour() == 3
    got = {}
    for li, lay in enumerate(SC.SMALL):
        r, _d, planes = SC.pool(*lay)
        for n in SC.SMALL_NS:
            br = SC.batch(r, n)
            for name, eng in engines.items():
                dr, dp = eng.upload(br), eng.upload(r[PREV0_ENTRY:PREV0_ENTRY + 1])
                for tag, hp, dev in (("p", r[PREV0_ENTRY:PREV0_ENTRY + 1], dp), ("n", None, None)):
                    got["%s|%d|%d|%s|host" % (name, li, n, tag)] = _run(eng, br, planes, hp)
                    got["%s|%d|%d|%s|device" % (name, li, n, tag)] = _run(eng, dr, planes, dev)
                for buf in (dr, dp):
                    buf._owner.free()
    for eng in engines.values():
        eng.close()
    np.savez(out_path, **{k: np.frombuffer(v, np.uint8) for k, v in got.items()})
    print("VCA-SLICES-OK", len(got))


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    from rtvqa_amd import _native as N
    out = str(tmp_path_factory.mktemp("tslices") / "small.npz")
    env = dict(os.environ, VQA_LIB_PATH=N.LAB_LIB_PATH)
    env.pop("VQA_QSLICE", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True, timeout=300, cwd=REPO)
    assert r.returncode == 0 and "VCA-SLICES-OK" in r.stdout, (r.stdout[-300:], r.stderr[-2000:])
    with np.load(out) as z:
        return {k: z[k].tobytes() for k in z.files}


def test_small_slices_give_the_bytes_of_one_slice(small):
    seen = 0
    for li in range(len(SC.SMALL)):
        for n in SC.SMALL_NS:
            for tag in ("p", "n"):
                plain = small["plain|%d|%d|%s|host" % (li, n, tag)]
                assert len(plain) > 0
                for mem in ("host", "device"):
                    assert small["sliced|%d|%d|%s|%s" % (li, n, tag, mem)] == plain, (li, n, tag, mem)
                    assert small["plain|%d|%d|%s|%s" % (li, n, tag, mem)] == plain, (li, n, tag, mem)
                    seen += 1
    assert seen == len(SC.SMALL) * 3 * 2 * 2


def test_the_seam_frames_have_the_frame_before_them(small):
    """the unsliced records against the restatement at n = 8: frames 3 and 6, the first of the second and the third slice of the
    sliced engine (whose bytes are the same), have frames 2 and 5 before them, and their gradient is not vacuous"""
    from rtvqa_amd.engine import VCA_DTYPE
    for li, lay in enumerate(SC.SMALL):
        r, _d, planes = SC.pool(*lay)
        depth, n, npl = lay[3], 8, len(planes)
        rec = np.frombuffer(small["plain|%d|%d|p|host" % (li, n)][:n * npl * VCA_DTYPE.itemsize], VCA_DTYPE).reshape(n, npl)
        bare = np.frombuffer(small["plain|%d|%d|n|host" % (li, n)][:n * npl * VCA_DTYPE.itemsize], VCA_DTYPE).reshape(n, npl)
        order = [PREV0_ENTRY] + [i % SC.PERIOD for i in range(n)]
        for j, p in enumerate(planes):
            series = K.plane_series(r, p)
            stack = np.stack([series[e] for e in order])
            want = R.features(stack[1:], depth, stack[0])
            wq = R.features(stack[1:], depth, stack[0], quantise=True)
            assert np.array_equal(rec[:, j]["l_sum"].astype(np.int64), wq["l_sum"]), (lay, j)
            for key in ("e", "h", "l"):
                assert (np.abs(rec[:, j][key] - want[key]) <= R.bar(want[key])).all(), (lay, j, key)
            assert int(bare[0, j]["h_sum"]) == 0 and bare[1:, j].tobytes() == rec[1:, j].tobytes()
        assert rec[3, 0]["h_sum"] > 0 and rec[6, 0]["h_sum"] > 0 and rec[3, 0]["h_sum"] != rec[6, 0]["h_sum"]


def test_a_batch_past_32768_frames_through_the_shipped_library(engine):
    """32771 frames of 32 x 32: slices of 32768 and 3.  Frame i is pool entry i % 7 with entry (i - 1) % 7 before it, so record
    i >= 8 equals record i - 7 - across the seam too, where the predecessor comes from the map slot the first slice filled - and
    the first eight equal a short batch's"""
    assert engine.lib.vqa_build_flavour() == 0
    r, _d, planes = SC.pool(*BIG)
    p0 = r[PREV0_ENTRY:PREV0_ENTRY + 1]
    short = engine.vca(SC.batch(r, 15), planes, prev0=p0)
    rec = engine.vca(SC.batch(r, SC.BIG_N), planes, prev0=p0)
    assert rec.shape == (SC.BIG_N, 1)
    assert rec[:15].tobytes() == short.tobytes()
    assert rec.tobytes() == rec[SC.temporal_map(SC.BIG_N)].tobytes()
    assert (rec["h_sum"][32766:32771, 0] > 0).all() and len(set(rec["h_sum"][1:8, 0].tolist())) > 3
    want = R.features(np.stack([K.plane_series(r, planes[0])[i % SC.PERIOD] for i in range(8)]), 8,
                      K.plane_series(r, planes[0])[PREV0_ENTRY])
    for key in ("e", "h", "l"):
        assert (np.abs(rec[:8, 0][key] - want[key]) <= R.bar(want[key])).all(), key


if __name__ == "__main__":
    _child(sys.argv[1])
