"""GPU: the frame-slice seam of MDSI.  vqa_mdsi_submit cuts a batch into slices of 32768 frames like every plane-batch kind; the
words of frame a0 start at entry a0 and every slice reuses the map of g from its start.  One child process on the lab library
creates an engine with VQA_QSLICE unset and one with VQA_QSLICE=3 and runs the 7 frames of mdsi_cases.slice_pool (4:2:0 at
33 x 67, 8 bits; packed BGR at 10 bits; every frame admitted by tests/test_mdsi_host.py) - 3 + 3 + 1 -, from host and from device
frames: the sliced engine's records equal the unsliced engine's byte for byte, and the unsliced words of every frame equal the
restatement's."""
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path[:0] = [REPO, os.path.dirname(os.path.abspath(__file__))]

import mdsi_cases as MC
import mdsi_reference as R

pytestmark = pytest.mark.gpu


def _batches(lay):
    layout, h, w, depth = lay
    rs, ds = MC.slice_pool(*lay)
    return MC.pack(rs, layout, depth), MC.pack(ds, layout, depth), MC.engine_planes(layout, h, w, depth)


def _child(out_path):
    import rtvqa_amd
    os.environ.pop("VQA_QSLICE", None)
    engines = {"plain": rtvqa_amd.Engine(0)}
    os.environ["VQA_QSLICE"] = "3"               # read once, in vqa_create
    engines["sliced"] = rtvqa_amd.Engine(0)
    os.environ.pop("VQA_QSLICE")
    assert engines["plain"].lib.vqa_build_flavour() == 3
    got = {}
    for li, lay in enumerate(MC.SLICE_LAYOUTS):
        br, bd, planes = _batches(lay)
        for name, eng in engines.items():
            dr, dd = eng.upload(br), eng.upload(bd)
            got["%s|%d|host" % (name, li)] = eng.mdsi(br, bd, planes).tobytes()
            got["%s|%d|device" % (name, li)] = eng.mdsi(dr, dd, planes).tobytes()
            for buf in (dr, dd):
                buf._owner.free()
    for eng in engines.values():
        eng.close()
    np.savez(out_path, **{k: np.frombuffer(v, np.uint8) for k, v in got.items()})
    print("MDSI-SLICES-OK", len(got))


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    from rtvqa_amd import _native as N
    out = str(tmp_path_factory.mktemp("dslices") / "small.npz")
    env = dict(os.environ, VQA_LIB_PATH=N.LAB_LIB_PATH)
    env.pop("VQA_QSLICE", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True, timeout=300, cwd=REPO)
    assert r.returncode == 0 and "MDSI-SLICES-OK" in r.stdout, (r.stdout[-300:], r.stderr[-2000:])
    with np.load(out) as z:
        return {k: z[k].tobytes() for k in z.files}


def test_three_slices_give_the_bytes_of_one_slice(small):
    for li in range(len(MC.SLICE_LAYOUTS)):
        plain = small["plain|%d|host" % li]
        assert len(plain) > 0
        for mem in ("host", "device"):
            assert small["sliced|%d|%s" % (li, mem)] == plain, (li, mem)
            assert small["plain|%d|%s" % (li, mem)] == plain, (li, mem)


def test_every_frame_of_the_batch_is_its_own(small):
    """the unsliced records against the restatement: frame i is pool entry i, so a record written to another slice's slot, or
    pooled over another slice's map, would carry another entry's words"""
    from rtvqa_amd.engine import MDSI_DTYPE
    for li, lay in enumerate(MC.SLICE_LAYOUTS):
        layout, h, w, depth = lay
        rs, ds = MC.slice_pool(*lay)
        rec = np.frombuffer(small["plain|%d|host" % li], MDSI_DTYPE)
        assert rec.shape == (MC.SLICE_FRAMES,)
        seen = set()
        for i in range(MC.SLICE_FRAMES):
            want = R.mdsi_quantised(rs[i], ds[i], MC.MODEL[layout], depth)
            assert (int(rec[i]["sum_pos"]), int(rec[i]["sum_neg"]), int(rec[i]["n_neg"]), int(rec[i]["sum_dev"])) == want, (lay, i)
            seen.add(want)
        assert len(seen) == MC.SLICE_FRAMES


if __name__ == "__main__":
    _child(sys.argv[1])
