"""GPU: the frame-slice seam of dE_ITP.  vqa_itp_submit cuts a batch into slices of 32768 frames like every plane-batch kind; the
two words of frame a0 start at entry a0.  One child process on the lab library creates an engine with VQA_QSLICE unset and one
with VQA_QSLICE=3 and runs the 7 frames of slice_cases.pool (4:4:4 at 16 x 16, 10 bits) - 3 + 3 + 1 -, from host and from device
frames, under both transfers: the sliced engine's records equal the unsliced engine's byte for byte, and the unsliced record of
every frame is within the bar of the restatement's.  Then 32771 frames of 16 x 16 through the shipped library: every record
equals the record of its pool entry, and the first eight equal a short batch's."""
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path[:0] = [REPO, os.path.dirname(os.path.abspath(__file__))]

import itp_reference as R
import slice_cases as SC

pytestmark = pytest.mark.gpu

LAYOUT = SC.BIG_CIEDE          # ("444", 16, 16, 10): three planes, the smallest frame
TRANSFERS = ("pq", "hlg")


def _child(out_path):
    import rtvqa_amd
    os.environ.pop("VQA_QSLICE", None)
    engines = {"plain": rtvqa_amd.Engine(0)}
    os.environ["VQA_QSLICE"] = "3"               # read once, in vqa_create
    engines["sliced"] = rtvqa_amd.Engine(0)
    os.environ.pop("VQA_QSLICE")
    assert engines["plain"].lib.vqa_build_flavour() == 3
    got = {}
    r, d, planes = SC.pool(*LAYOUT)
    for name, eng in engines.items():
        dr, dd = eng.upload(r), eng.upload(d)
        for t in TRANSFERS:
            got["%s|%s|host" % (name, t)] = eng.itp(r, d, planes, transfer=t).tobytes()
            got["%s|%s|device" % (name, t)] = eng.itp(dr, dd, planes, transfer=t).tobytes()
        for buf in (dr, dd):
            buf._owner.free()
    for eng in engines.values():
        eng.close()
    np.savez(out_path, **{k: np.frombuffer(v, np.uint8) for k, v in got.items()})
    print("ITP-SLICES-OK", len(got))


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    from rtvqa_amd import _native as N
    out = str(tmp_path_factory.mktemp("islices") / "small.npz")
    env = dict(os.environ, VQA_LIB_PATH=N.LAB_LIB_PATH)
    env.pop("VQA_QSLICE", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True, timeout=300, cwd=REPO)
    assert r.returncode == 0 and "ITP-SLICES-OK" in r.stdout, (r.stdout[-300:], r.stderr[-2000:])
    with np.load(out) as z:
        return {k: z[k].tobytes() for k in z.files}


def test_three_slices_give_the_bytes_of_one_slice(small):
    for t in TRANSFERS:
        plain = small["plain|%s|host" % t]
        assert len(plain) == 40 * SC.PERIOD
        for mem in ("host", "device"):
            assert small["sliced|%s|%s" % (t, mem)] == plain, (t, mem)
            assert small["plain|%s|%s" % (t, mem)] == plain, (t, mem)
    assert small["plain|pq|host"] != small["plain|hlg|host"]


def test_every_frame_of_the_batch_is_its_own(small):
    """the unsliced records against the restatement: frame i is pool entry i, so a record written to another slice's slot would
    carry another entry's words"""
    from rtvqa_amd.engine import ITP_DTYPE
    r, d, planes = SC.pool(*LAYOUT)
    fr, fd = R.split_planes(r, planes), R.split_planes(d, planes)
    for t, tr in zip(TRANSFERS, (R.PQ, R.HLG)):
        rec = np.frombuffer(small["plain|%s|host" % t], ITP_DTYPE)
        assert rec.shape == (SC.PERIOD,)
        for i in range(SC.PERIOD):
            want = R.record(fr[i], fd[i], LAYOUT[3], R.YUV2020, tr)
            assert abs(float(rec[i]["de_mean"]) - want["de_mean"]) <= R.BAR, (t, i)
            assert abs(float(rec[i]["de_max"]) - want["de_max"]) <= R.BAR, (t, i)
        # (the inverted checkerboard and all-peak against all-zero hold the same pixel pairs up to their order: one record)
        assert len({rec[i].tobytes() for i in range(SC.PERIOD)}) == SC.PERIOD - 1


def test_a_batch_past_32768_frames_through_the_shipped_library(engine):
    """32771 frames of 16 x 16: slices of 32768 and 3.  Frame i is pool entry i % 7, so record i equals record i % 7 - across the
    seam too - and the first eight equal a short batch's"""
    assert engine.lib.vqa_build_flavour() == 0
    r, d, planes = SC.pool(*LAYOUT)
    short = engine.itp(SC.batch(r, 8), SC.batch(d, 8), planes)
    rec = engine.itp(SC.batch(r, SC.BIG_N), SC.batch(d, SC.BIG_N), planes)
    assert rec.shape == (SC.BIG_N,)
    assert rec[:8].tobytes() == short.tobytes()
    assert rec.tobytes() == rec[SC.pair_map(SC.BIG_N)].tobytes()
    assert len({rec[i].tobytes() for i in range(SC.PERIOD)}) == SC.PERIOD - 1


if __name__ == "__main__":
    _child(sys.argv[1])
