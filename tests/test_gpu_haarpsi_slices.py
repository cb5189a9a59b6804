"""GPU: the frame-slice seam of HaarPSI.  vqa_haarpsi_submit cuts a batch into slices of 32768 frames like every plane-batch
kind; the words of frame a0 start at entry a0 n_planes.  One child process on the lab library creates an engine with VQA_QSLICE
unset and one with VQA_QSLICE=3 and runs 7 frames of the pool of tests/slice_cases.py (4:2:0 at 67 x 99, 8 and 10 bits: two
geometry groups per slice) - 3 + 3 + 1 -, from host and from device frames: the sliced engine's records equal the unsliced
engine's word for word, and the unsliced den of every frame equals the restatement's."""
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path[:0] = [REPO, os.path.dirname(os.path.abspath(__file__))]

import haarpsi_reference as R
import motion_cases as K
import slice_cases as SC

pytestmark = pytest.mark.gpu

N_FRAMES = 7


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
        r, d, planes = SC.pool(*lay)
        br, bd = SC.batch(r, N_FRAMES), SC.batch(d, N_FRAMES)
        for name, eng in engines.items():
            dr, dd = eng.upload(br), eng.upload(bd)
            got["%s|%d|host" % (name, li)] = eng.haarpsi(br, bd, planes).tobytes()
            got["%s|%d|device" % (name, li)] = eng.haarpsi(dr, dd, planes).tobytes()
            for buf in (dr, dd):
                buf._owner.free()
    for eng in engines.values():
        eng.close()
    np.savez(out_path, **{k: np.frombuffer(v, np.uint8) for k, v in got.items()})
    print("HAARPSI-SLICES-OK", len(got))


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    from rtvqa_amd import _native as N
    out = str(tmp_path_factory.mktemp("wslices") / "small.npz")
    env = dict(os.environ, VQA_LIB_PATH=N.LAB_LIB_PATH)
    env.pop("VQA_QSLICE", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True, timeout=300, cwd=REPO)
    assert r.returncode == 0 and "HAARPSI-SLICES-OK" in r.stdout, (r.stdout[-300:], r.stderr[-2000:])
    with np.load(out) as z:
        return {k: z[k].tobytes() for k in z.files}


def test_three_slices_give_the_words_of_one_slice(small):
    for li in range(len(SC.SMALL)):
        plain = small["plain|%d|host" % li]
        assert len(plain) > 0
        for mem in ("host", "device"):
            assert small["sliced|%d|%s" % (li, mem)] == plain, (li, mem)
            assert small["plain|%d|%s" % (li, mem)] == plain, (li, mem)


def test_every_frame_of_the_batch_is_its_own(small):
    """the unsliced records against the restatement: frame i is pool entry i, so a record written to another slice's slot
    would carry another entry's den"""
    from rtvqa_amd.engine import HAARPSI_DTYPE
    for li, lay in enumerate(SC.SMALL):
        r, d, planes = SC.pool(*lay)
        rec = np.frombuffer(small["plain|%d|host" % li], HAARPSI_DTYPE).reshape(N_FRAMES, len(planes))
        dens = set()
        for j, p in enumerate(planes):
            rs, ds = K.plane_series(r, p), K.plane_series(d, p)
            for i in range(N_FRAMES):
                den, _lo, _hi = R.words(rs[i], ds[i], lay[3])
                assert int(rec[i, j]["den"]) == den, (lay, i, j)
                if j == 0:
                    dens.add(den)
        assert len(dens) == N_FRAMES


if __name__ == "__main__":
    _child(sys.argv[1])
