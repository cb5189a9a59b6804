"""GPU: the slice and sub-slice seams of PU21.  vqa_pu21_submit cuts a batch into slices of 32768 frames like every plane-batch
kind, and each slice into sub-slices whose two q_Y maps fit 256 MiB; the five words of frame a start at entry a, and the maps of a
sub-slice are overwritten by the next.  One child process on the lab library creates an engine with no seam set and one with
VQA_QSLICE=3 and VQA_PU21_SUBSLICE=2 and runs the 7 frames of slice_cases.pool (4:4:4 at 16 x 16, 10 bits) - slices of 3 + 3 + 1,
sub-slices of 2 + 1, 2 + 1, 1 -, from host and from device frames, under both transfers: the cut engine's records AND maps equal
the uncut engine's byte for byte.  Then the entry point: run_ffmpeg_metrics(pu21=True) on a tiny y4m pair at C420p10 against
Engine.pu21 directly."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path[:0] = [REPO, os.path.dirname(os.path.abspath(__file__))]

import slice_cases as SC

pytestmark = pytest.mark.gpu

LAYOUT = SC.BIG_CIEDE          # ("444", 16, 16, 10): three planes, the smallest frame
TRANSFERS = ("pq", "hlg")


def _child(out_path):
    import rtvqa_amd
    for k in ("VQA_QSLICE", "VQA_PU21_SUBSLICE"):
        os.environ.pop(k, None)
    engines = {"plain": rtvqa_amd.Engine(0)}
    os.environ["VQA_QSLICE"], os.environ["VQA_PU21_SUBSLICE"] = "3", "2"   # read once, in vqa_create
    engines["cut"] = rtvqa_amd.Engine(0)
    for k in ("VQA_QSLICE", "VQA_PU21_SUBSLICE"):
        os.environ.pop(k)
    assert engines["plain"].lib.vqa_build_flavour() == 3
    got = {}
    r, d, planes = SC.pool(*LAYOUT)
    for name, eng in engines.items():
        dr, dd = eng.upload(r), eng.upload(d)
        eng.profile(True)
        for t in TRANSFERS:
            rec, maps = eng.pu21(r, d, planes, transfer=t, maps=True)
            got["%s|%s|host" % (name, t)] = np.frombuffer(rec.tobytes(), np.uint8)
            got["%s|%s|host|maps" % (name, t)] = maps
            rec, maps = eng.pu21(dr, dd, planes, transfer=t, maps=True)
            got["%s|%s|device" % (name, t)] = np.frombuffer(rec.tobytes(), np.uint8)
            got["%s|%s|device|maps" % (name, t)] = maps
        prof = eng.profile_read(reset=True)
        got["%s|launches" % name] = np.array([prof["k_pu21_encode"][1], prof["k_pu21_ssim"][1]], np.int64)
        for buf in (dr, dd):
            buf._owner.free()
    for eng in engines.values():
        eng.close()
    np.savez(out_path, **got)
    print("PU21-SLICES-OK", len(got))


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    from rtvqa_amd import _native as N
    out = str(tmp_path_factory.mktemp("uslices") / "small.npz")
    env = dict(os.environ, VQA_LIB_PATH=N.LAB_LIB_PATH)
    for k in ("VQA_QSLICE", "VQA_PU21_SUBSLICE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True, timeout=300, cwd=REPO)
    assert r.returncode == 0 and "PU21-SLICES-OK" in r.stdout, (r.stdout[-300:], r.stderr[-2000:])
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


def test_slices_and_sub_slices_give_the_bytes_of_one(small):
    for t in TRANSFERS:
        plain, pmaps = small["plain|%s|host" % t].tobytes(), small["plain|%s|host|maps" % t]
        assert len(plain) == 88 * SC.PERIOD and pmaps.shape == (SC.PERIOD, 2, 16, 16)
        for mem in ("host", "device"):
            for name in ("plain", "cut"):
                assert small["%s|%s|%s" % (name, t, mem)].tobytes() == plain, (name, t, mem)
                assert (small["%s|%s|%s|maps" % (name, t, mem)] == pmaps).all(), (name, t, mem)
    assert small["plain|pq|host"].tobytes() != small["plain|hlg|host"].tobytes()
    # one profile entry per kernel per sub-slice: 4 submits of 1 sub-slice; 4 submits of 2 + 2 + 1 = 5 sub-slices
    assert list(small["plain|launches"]) == [4, 4] and list(small["cut|launches"]) == [20, 20]


def test_every_frame_of_the_batch_is_its_own(small):
    """the uncut records and maps against the restatement: frame i is pool entry i, so words or a map written to another slot
    would carry another entry's"""
    import pu21_reference as R
    from rtvqa_amd.engine import PU21_DTYPE
    r, d, planes = SC.pool(*LAYOUT)
    fr, fd = R.split_planes(r, planes), R.split_planes(d, planes)
    for t, tr in zip(TRANSFERS, (R.PQ, R.HLG)):
        rec = np.frombuffer(small["plain|%s|host" % t].tobytes(), PU21_DTYPE)
        maps = small["plain|%s|host|maps" % t].astype(np.int64)
        for i in range(SC.PERIOD):
            want, qa, qb = R.record_q(fr[i], fd[i], LAYOUT[3], R.YUV2020, tr)
            assert np.abs(maps[i, 0] - qa).max() <= 1 and np.abs(maps[i, 1] - qb).max() <= 1, (t, i)
            assert (int(rec[i]["sse_y_lo"]), int(rec[i]["sse_y_hi"])) == R.sse_words(maps[i, 0], maps[i, 1]), (t, i)
            assert abs(int(rec[i]["ssim_q"]) - R.ssim_word(maps[i, 0], maps[i, 1])) <= 36, (t, i)


def test_the_entry_point_on_a_y4m_pair(engine, tmp_path):
    from rtvqa_amd import video_processing as vp
    from rtvqa_amd.engine import yuv_planes
    import pu21_cases as PC
    h, w, n = 36, 64, 3                                   # (the pass also measures PSNR and SSIM, whose planes have a minimum)
    r, d, planes = PC.clip("natural", "yuv420p10le", h, w, 10, n, seed=21)
    paths = []
    for name, frames in (("ref", r), ("enc", d)):
        p = str(tmp_path / (name + ".y4m"))
        with open(p, "wb") as f:
            f.write(b"YUV4MPEG2 W%d H%d F30:1 Ip A1:1 C420p10\n" % (w, h))
            for fr in frames:
                f.write(b"FRAME\n" + fr.astype("<u2").tobytes())
        paths.append(p)
    logs = [str(tmp_path / x) for x in ("p.log", "s.log", "v.json")]
    vp.run_ffmpeg_metrics(paths[0], paths[1], *logs, pu21=True)
    want = engine.pu21(r, d, yuv_planes(h, w, "420", 10))
    doc = json.load(open(logs[2]))
    assert len(doc["frames"]) == n
    for i in range(n):
        m = doc["frames"][i]["metrics"]
        assert m["pu_psnr"] == float(want["pu_psnr"][i]) and m["pu_psnr_rgb"] == float(want["pu_psnr_rgb"][i])
        assert m["pu_ssim"] == float(want["pu_ssim"][i])


if __name__ == "__main__":
    _child(sys.argv[1])
