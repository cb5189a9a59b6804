"""GPU: the frame-slice seam of BRISQUE.  vqa_brisque_submit cuts a batch into slices of 32768 frames like every
plane-batch kind; a slice's records go behind those of the slice before.  One child process on the lab library creates an
engine with VQA_QSLICE unset and one with VQA_QSLICE=3 and runs the pool of tests/slice_cases.py (4:2:0 at 67 x 99, 8 and 10
bits: two geometry groups per slice) at n = 3, 4 and 8 - one slice, one frame over, 3 + 3 + 2 - from host and from device
frames: the sliced engine's records equal the unsliced engine's byte for byte, and the unsliced words state moments within the bars of the float64
restatement (tests/brisque_reference.py).
Then 32771 frames of 16 x 16 through the shipped library: every record equals the record of its pool entry, and the first eight
equal a short batch's.  Children are fresh processes; nothing replaces a running program."""
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path[:0] = [REPO, os.path.dirname(os.path.abspath(__file__))]

import brisque_cases as BC
import brisque_reference as R
import motion_cases as K
import slice_cases as SC

pytestmark = pytest.mark.gpu

BIG = ("mono", 16, 16, 8)


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
        _r, d, planes = SC.pool(*lay)
        for n in SC.SMALL_NS:
            bd = SC.batch(d, n)
            for name, eng in engines.items():
                dd = eng.upload(bd)
                got["%s|%d|%d|host" % (name, li, n)] = eng.brisque(bd, planes).tobytes()
                got["%s|%d|%d|device" % (name, li, n)] = eng.brisque(dd, planes).tobytes()
                dd._owner.free()
    for eng in engines.values():
        eng.close()
    np.savez(out_path, **{k: np.frombuffer(v, np.uint8) for k, v in got.items()})
    print("BRISQUE-SLICES-OK", len(got))


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    from rtvqa_amd import _native as N
    out = str(tmp_path_factory.mktemp("nslices") / "small.npz")
    env = dict(os.environ, VQA_LIB_PATH=N.LAB_LIB_PATH)
    env.pop("VQA_QSLICE", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True, timeout=300, cwd=REPO)
    assert r.returncode == 0 and "BRISQUE-SLICES-OK" in r.stdout, (r.stdout[-300:], r.stderr[-2000:])
    with np.load(out) as z:
        return {k: z[k].tobytes() for k in z.files}


def test_small_slices_give_the_bytes_of_one_slice(small):
    seen = 0
    for li in range(len(SC.SMALL)):
        for n in SC.SMALL_NS:
            plain = small["plain|%d|%d|host" % (li, n)]
            assert len(plain) > 0
            for mem in ("host", "device"):
                assert small["sliced|%d|%d|%s" % (li, n, mem)] == plain, (li, n, mem)
                assert small["plain|%d|%d|%s" % (li, n, mem)] == plain, (li, n, mem)
                seen += 1
    assert seen == len(SC.SMALL) * 3 * 2


def test_the_records_behind_the_seams_are_their_frames(small):
    """the unsliced words against the float64 restatement at n = 8: frames 3 and 6 open the second and the third slice of the sliced
    engine, whose bytes are the same"""
    from rtvqa_amd.engine import BRISQUE_DTYPE
    for li, lay in enumerate(SC.SMALL):
        _r, d, planes = SC.pool(*lay)
        n, npl = 8, len(planes)
        rec = np.frombuffer(small["plain|%d|%d|host" % (li, n)], BRISQUE_DTYPE).reshape(n, npl)
        for j, p in enumerate(planes):
            series = K.plane_series(d, p)
            for i in range(n):
                x = series[i % SC.PERIOD]
                got = R.word_moments(R.record_words(rec[i, j]), *x.shape)
                BC.close_moments(got, R.float_moments(x, lay[3]), (lay, i, j))
        assert rec[7].tobytes() == rec[0].tobytes() and len({rec[i].tobytes() for i in range(7)}) >= 6


def test_a_batch_past_32768_frames_through_the_shipped_library(engine):
    """32771 frames of 16 x 16: slices of 32768 and 3.  Frame i is pool entry i % 7, so record i equals record i % 7 - across the
    seam too - and the first eight equal a short batch's"""
    assert engine.lib.vqa_build_flavour() == 0
    _r, d, planes = SC.pool(*BIG)
    short = engine.brisque(SC.batch(d, 8), planes)
    rec = engine.brisque(SC.batch(d, SC.BIG_N), planes)
    assert rec.shape == (SC.BIG_N, 1)
    assert rec[:8].tobytes() == short.tobytes()
    assert rec.tobytes() == rec[SC.pair_map(SC.BIG_N)].tobytes()
    assert len({rec[i].tobytes() for i in range(7)}) >= 6
    series = K.plane_series(d, planes[0])
    for f in (32767, 32768, 32769, 32770):
        x = series[f % SC.PERIOD]
        BC.close_moments(R.word_moments(R.record_words(rec[f, 0]), *x.shape), R.float_moments(x, BIG[3]), f)


if __name__ == "__main__":
    _child(sys.argv[1])
