"""GPU: the frame-slice seam of XPSNR.  vqa_xpsnr_submit cuts a batch into slices of 32768 frames like every plane-batch kind;
what is its own is that a slice's first frame takes the previous slice's LAST frame as its predecessor, and that the words of
frame a0 start at a0 frame_words.  One child process on the lab library creates an engine with VQA_QSLICE unset and one with
VQA_QSLICE=3 and runs the pool of tests/slice_cases.py (16 x 16 mono at 8 bits, 4:4:4 at 10) at n = 3, 4 and 8 - one slice, one
frame over, 3 + 3 + 2 -, with and without prev0, from host and from device frames: the sliced engine's records and block words
equal the unsliced engine's byte for byte, and the unsliced words of the seam frames equal the restatement's."""
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path[:0] = [REPO, os.path.dirname(os.path.abspath(__file__))]

import slice_cases as SC
import xpsnr_reference as R

pytestmark = pytest.mark.gpu

LAYOUTS = (("mono", 16, 16, 8), ("444", 16, 16, 10))
PREV0_ENTRY = 6


def _run(eng, r, d, planes, prev0):
    rec, blk = eng.xpsnr(r, d, planes, prev0=prev0, blocks=True)
    return rec.tobytes() + b"".join(blk[k].tobytes() for k in ("sa", "ta", "n", "sse"))


def _child(out_path):
    import rtvqa_amd
    os.environ.pop("VQA_QSLICE", None)
    engines = {"plain": rtvqa_amd.Engine(0)}
    os.environ["VQA_QSLICE"] = "3"               # read once, in vqa_create
    engines["sliced"] = rtvqa_amd.Engine(0)
    os.environ.pop("VQA_QSLICE")
    assert engines["plain"].lib.vqa_build_flavour() == 3
    got = {}
    for li, lay in enumerate(LAYOUTS):
        r, d, planes = SC.pool(*lay)
        for n in SC.SMALL_NS:
            br, bd = SC.batch(r, n), SC.batch(d, n)
            for name, eng in engines.items():
                dr, dd, dp = eng.upload(br), eng.upload(bd), eng.upload(r[PREV0_ENTRY:PREV0_ENTRY + 1])
                for tag, hp, dev in (("p", r[PREV0_ENTRY:PREV0_ENTRY + 1], dp), ("n", None, None)):
                    got["%s|%d|%d|%s|host" % (name, li, n, tag)] = _run(eng, br, bd, planes, hp)
                    got["%s|%d|%d|%s|device" % (name, li, n, tag)] = _run(eng, dr, dd, planes, dev)
                for buf in (dr, dd, dp):
                    buf._owner.free()
    for eng in engines.values():
        eng.close()
    np.savez(out_path, **{k: np.frombuffer(v, np.uint8) for k, v in got.items()})
    print("XPSNR-SLICES-OK", len(got))


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    from rtvqa_amd import _native as N
    out = str(tmp_path_factory.mktemp("xslices") / "small.npz")
    env = dict(os.environ, VQA_LIB_PATH=N.LAB_LIB_PATH)
    env.pop("VQA_QSLICE", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True, timeout=300, cwd=REPO)
    assert r.returncode == 0 and "XPSNR-SLICES-OK" in r.stdout, (r.stdout[-300:], r.stderr[-2000:])
    with np.load(out) as z:
        return {k: z[k].tobytes() for k in z.files}


def test_small_slices_give_the_bytes_of_one_slice(small):
    seen = 0
    for li in range(len(LAYOUTS)):
        for n in SC.SMALL_NS:
            for tag in ("p", "n"):
                plain = small["plain|%d|%d|%s|host" % (li, n, tag)]
                assert len(plain) > 0
                for mem in ("host", "device"):
                    assert small["sliced|%d|%d|%s|%s" % (li, n, tag, mem)] == plain, (li, n, tag, mem)
                    assert small["plain|%d|%d|%s|%s" % (li, n, tag, mem)] == plain, (li, n, tag, mem)
                    seen += 1
    assert seen == len(LAYOUTS) * 3 * 2 * 2


def test_the_seam_frames_have_the_frame_before_them(small):
    """the unsliced words against the restatement at n = 8: frames 3 and 6, the first of the second and the third slice of the
    sliced engine (whose bytes are the same), have frames 2 and 5 before them, and their temporal activity is not vacuous"""
    from rtvqa_amd.engine import XPSNR_DTYPE
    for li, lay in enumerate(LAYOUTS):
        r, d, planes = SC.pool(*lay)
        depth, n, npl = lay[3], 8, len(planes)
        raw = small["plain|%d|%d|p|host" % (li, n)]
        g = R.geometry(16, 16)
        nb = g["nbx"] * g["nby"]
        a = n * npl * XPSNR_DTYPE.itemsize
        words = np.frombuffer(raw[a:], np.uint64).astype(np.int64)
        sa, ta = words[:n * nb].reshape(n, nb), words[n * nb:2 * n * nb].reshape(n, nb)
        sse = words[3 * n * nb:].reshape(n, npl, nb)
        for i in range(n):
            def planes_of(arr, e):
                return [arr[e].reshape(npl, 16, 16)[p].astype(np.int64) for p in range(npl)]
            e = i % SC.PERIOD
            prev = planes_of(r, PREV0_ENTRY if i == 0 else (i - 1) % SC.PERIOD)[0]
            want = R.frame(planes_of(r, e), planes_of(d, e), prev, depth)
            assert (sa[i] == want["sa"].reshape(-1)).all() and (ta[i] == want["ta"].reshape(-1)).all(), (lay, i)
            assert (sse[i] == want["sse"].reshape(npl, -1)).all(), (lay, i)
        assert ta[3].sum() > 0 and ta[6].sum() > 0 and not (ta[3] == ta[6]).all()


if __name__ == "__main__":
    _child(sys.argv[1])
