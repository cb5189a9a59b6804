"""GPU: the slice seams of the signal statistics.  vqa_sigstats_submit cuts a batch into slices of 32768 frames like every
plane-batch kind, and a slice into sub-slices of frames whose histograms stay within 256 MiB; a frame that opens a slice or a
sub-slice is measured against the last frame of the one before.  One child process on the lab library creates an engine with
VQA_QSLICE unset and one with VQA_QSLICE=3 and runs the reference stream of tests/slice_cases.py's pool (4:2:0 at 67 x 99, 8 and 10
bits) at n = 3, 4 and 8 from host and from device frames: the sliced engine's records and profiles equal the unsliced engine's
byte for byte - sad across the seam included - and the unsliced words equal the restatement's.  Then 32771 frames of 16 x 16
through the shipped library against the pool's periodicity, and 1100 frames of 16 x 16 gray16 - 1024 histograms of 65536 bins fill
the 256 MiB - against the same frames submitted in short batches.  Children are fresh processes; nothing replaces a running
program."""
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path[:0] = [REPO, os.path.dirname(os.path.abspath(__file__))]

import motion_cases as K
import sigstats_reference as R
import slice_cases as SC

pytestmark = pytest.mark.gpu

BIG = ("mono", 16, 16, 8)


def _bytes(res):
    rec, sums = res
    return rec.tobytes() + b"".join(s[k].tobytes() for s in sums for k in ("rows", "cols"))


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
                dr = eng.upload(br)
                got["%s|%d|%d|host" % (name, li, n)] = _bytes(eng.sigstats(br, planes, profiles=True))
                got["%s|%d|%d|device" % (name, li, n)] = _bytes(eng.sigstats(dr, planes, profiles=True))
                got["%s|%d|%d|prev0" % (name, li, n)] = _bytes(eng.sigstats(br, planes, prev0=r[6], profiles=True))
                dr._owner.free()
    for eng in engines.values():
        eng.close()
    np.savez(out_path, **{k: np.frombuffer(v, np.uint8) for k, v in got.items()})
    print("SIGSTATS-SLICES-OK", len(got))


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    from rtvqa_amd import _native as N
    out = str(tmp_path_factory.mktemp("zslices") / "small.npz")
    env = dict(os.environ, VQA_LIB_PATH=N.LAB_LIB_PATH)
    env.pop("VQA_QSLICE", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True, timeout=300, cwd=REPO)
    assert r.returncode == 0 and "SIGSTATS-SLICES-OK" in r.stdout, (r.stdout[-300:], r.stderr[-2000:])
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
            assert small["sliced|%d|%d|prev0" % (li, n)] == small["plain|%d|%d|prev0" % (li, n)] != plain, (li, n)
    assert seen == len(SC.SMALL) * 3 * 2


def test_the_records_behind_the_seams_are_their_frames(small):
    """the unsliced words against the restatement at n = 8: frames 3 and 6 open the second and the third slice of the sliced
    engine, whose bytes are the same - their sad and changed are against frames 2 and 5"""
    from rtvqa_amd.engine import SIGSTATS_DTYPE
    for li, lay in enumerate(SC.SMALL):
        r, _d, planes = SC.pool(*lay)
        n, npl, depth = 8, len(planes), lay[3]
        rec = np.frombuffer(small["plain|%d|%d|host" % (li, n)][:n * npl * SIGSTATS_DTYPE.itemsize], SIGSTATS_DTYPE).reshape(n, npl)
        for j, p in enumerate(planes):
            want = R.series(K.plane_series(SC.batch(r, n), p), depth)
            for i in range(n):
                assert not R.same_words(rec[i, j], want[i]), (lay, i, j, R.same_words(rec[i, j], want[i]))
        assert (rec[3]["sad"] > 0).all() and (rec[6]["sad"] > 0).all() and (rec[0]["sad"] == 0).all()


def test_a_batch_past_32768_frames_through_the_shipped_library(engine):
    """32771 frames of 16 x 16: slices of 32768 and 3.  Frame i is pool entry i % 7, so record i equals record
    temporal_map(i) - across the seam too, where the predecessor is the slice before's last frame - and the first eight equal a
    short batch's"""
    assert engine.lib.vqa_build_flavour() == 0
    r, _d, planes = SC.pool(*BIG)
    short = engine.sigstats(SC.batch(r, 8), planes)
    rec = engine.sigstats(SC.batch(r, SC.BIG_N), planes)
    assert rec.shape == (SC.BIG_N, 1)
    assert rec[:8].tobytes() == short.tobytes()
    assert rec.tobytes() == rec[SC.temporal_map(SC.BIG_N)].tobytes()
    assert len({rec[i].tobytes() for i in range(8)}) >= 7
    series = K.plane_series(r, planes[0])
    for f in (32767, 32768, 32769, 32770):
        want = R.record(series[f % SC.PERIOD], 8, series[(f - 1) % SC.PERIOD])
        assert not R.same_words(rec[f, 0], want), (f, R.same_words(rec[f, 0], want))


def test_a_uint16_batch_past_the_sub_slice_rule(engine):
    """1100 frames of 16 x 16 gray16: a histogram of 65536 32-bit bins is 256 KiB, so 1024 frames fill the 256 MiB and frames
    1024 .. 1099 go out as a second sub-slice.  Records equal those of the same frames submitted in short batches"""
    from rtvqa_amd.engine import mono_planes
    n, h, w = 1100, 16, 16
    rng = np.random.default_rng(16)
    f = rng.integers(0, 65536, (n, h * w)).astype(np.uint16)
    f[1024] = f[1023]                                      # the frame that opens the second sub-slice equals its predecessor
    planes = mono_planes(h, w, 16)
    whole = engine.sigstats(f, planes)
    assert whole.shape == (n, 1)
    parts = [engine.sigstats(f[a:a + 275], planes, prev0=f[a - 1] if a else None) for a in range(0, n, 275)]
    assert np.concatenate(parts).tobytes() == whole.tobytes()
    assert int(whole[1024, 0]["sad"]) == 0 and int(whole[1024, 0]["changed"]) == 0 and int(whole[1025, 0]["changed"]) > 200
    series = f.reshape(n, h, w).astype(np.int64)
    for i in (0, 1023, 1024, 1025, 1099):
        want = R.record(series[i], 16, series[i - 1] if i else None)
        assert not R.same_words(whole[i, 0], want), (i, R.same_words(whole[i, 0], want))


if __name__ == "__main__":
    _child(sys.argv[1])
