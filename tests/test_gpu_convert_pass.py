"""GPU: convert through the reference-shaped entry points.  A small yuv422p10le reference against its yuv420p encode (4 frames,
64 x 48): what a converting run writes is compared byte for byte with a plain run over the reference and the clip that the
restatement (tests/convert_reference.py) converted - the stats files, and the feature log but for DIST_PIXFMT / CONVERT."""
import json

import numpy as np
import pytest

import convert_reference as R

pytestmark = pytest.mark.gpu

H, W, N_FRAMES = 48, 64, 4
REF, DIST = "yuv422p10le", "yuv420p"
KINDS = dict(gmsd=True, psnr_hvs=True, cambi=True)
OWN_KEYS = ("DIST_PIXFMT", "CONVERT")


def _planes(layout, h=H, w=W):
    from rtvqa_amd import video_processing as vp
    return vp.LAYOUTS[layout][0](h, w)


@pytest.fixture(scope="module")
def clip():
    """(the 10-bit 4:2:2 reference, its 8-bit 4:2:0 encode, the encode's BGR frames, the encode as a 32 x 24 rung)"""
    from rtvqa_amd import frames, synth
    bgr = synth.s_natural(N_FRAMES, H, W, seed=7)
    enc_bgr = synth.distort(bgr)
    src = frames.bgr_to_yuv420p(bgr)
    # the reference: the source's 4:2:0 frames taken up to 4:2:2 at ten bits, the two low bits filled with a pattern
    ref = R.convert_packed(src, _planes(DIST), _planes(REF), "linear", "center", "limited")
    ref = np.minimum(ref + (np.arange(ref.shape[1], dtype=np.uint16) % 4)[None], 1023).astype(np.uint16)
    dist = frames.bgr_to_yuv420p(enc_bgr)
    rung = frames.bgr_to_yuv420p(np.ascontiguousarray(enc_bgr[:, ::2, ::2]))
    return ref, dist, enc_bgr, rung


def _run(tmp_path, tag, ref, enc, **kw):
    from rtvqa_amd import video_processing as vp
    logs = [str(tmp_path / ("%s_%s.log" % (k, tag))) for k in ("psnr", "ssim", "vmaf")]
    assert vp.run_ffmpeg_metrics(ref, enc, *logs, layout=REF, height=H, width=W, batch_size=3, **kw) is None
    return logs


def _same(got, plain, keys):
    for x, y in zip(got[:2], plain[:2]):
        assert open(x, "rb").read() == open(y, "rb").read()         # the psnr and ssim stats lines, byte for byte
    doc = json.load(open(got[2]))
    for k, v in keys.items():
        assert doc[k] == v, k
    rest = {k: v for k, v in doc.items() if k not in keys}           # (DIST_PIXFMT / CONVERT; under scale DIST_RES / SCALE as well)
    assert open(plain[2]).read() == json.dumps(rest, indent=1) + "\n"
    return doc


@pytest.mark.parametrize("chroma,siting,rng", (("linear", "center", "limited"), ("box", "left", "full"), ("linear", "left", "limited")))
def test_a_mixed_pair_is_the_plain_run_over_the_restated_clip(engine, tmp_path, clip, chroma, siting, rng):
    ref, dist, _bgr, _rung = clip
    got = _run(tmp_path, "conv", ref, dist, dist_pixfmt=DIST, convert=chroma, convert_siting=siting, convert_range=rng, **KINDS)
    restated = R.convert_packed(dist, _planes(DIST), _planes(REF), chroma, siting, rng)
    plain = _run(tmp_path, "plain", ref, restated, **KINDS)
    doc = _same(got, plain, {"DIST_PIXFMT": DIST, "CONVERT": "%s/%s/%s" % (chroma, siting, rng)})
    assert list(doc)[-2:] == list(OWN_KEYS)
    assert float(np.mean([f["metrics"]["gmsd"] for f in doc["frames"]])) > 0


def test_y4m_files_bring_their_layouts_in_their_headers(engine, tmp_path, clip):
    from rtvqa_amd.frames import write_y4m
    ref, dist, _bgr, _rung = clip
    paths = [str(tmp_path / "ref.y4m"), str(tmp_path / "dist.y4m")]
    write_y4m(paths[0], ref, H, W, pixfmt=REF)
    write_y4m(paths[1], dist, H, W, pixfmt=DIST)
    from rtvqa_amd import video_processing as vp
    logs = [str(tmp_path / ("%s_y4m.log" % k)) for k in ("psnr", "ssim", "vmaf")]
    assert vp.run_ffmpeg_metrics(paths[0], paths[1], *logs, batch_size=3, convert="linear", **KINDS) is None
    plain = _run(tmp_path, "plain", ref, R.convert_packed(dist, _planes(DIST), _planes(REF)), **KINDS)
    _same(logs, plain, {"DIST_PIXFMT": DIST, "CONVERT": "linear/center/limited"})


def _row(tmp_path, tag, ref, enc, bgr, **keys):
    from rtvqa_amd import video_processing as vp
    cfg = dict({"crf": 23, "resize_width": 64, "resize_height": 64, "frame_interval": 1, "batch_size": 3, "pixfmt": REF,
                "height": H, "width": W}, **KINDS)
    cfg.update(keys)
    vp.validate_config(cfg)
    return vp.process_video_and_extract_metrics(ref, enc, cfg, csv_file=str(tmp_path / ("%s.csv" % tag)), column_order="fixed",
                                                encoded_bgr=bgr)


def test_the_config_keys_give_the_same_row(engine, tmp_path, clip):
    ref, dist, bgr, _rung = clip
    row = _row(tmp_path, "conv", ref, dist, bgr, dist_pixfmt=DIST, convert="linear", convert_siting="left", convert_range="full")
    restated = R.convert_packed(dist, _planes(DIST), _planes(REF), "linear", "left", "full")
    plain = _row(tmp_path, "plain", ref, restated, bgr)
    assert list(row)[-2:] == list(OWN_KEYS) and row["DIST_PIXFMT"] == DIST and row["CONVERT"] == "linear/left/full"
    assert list(row)[:-2] == list(plain)
    for k in plain:
        assert repr(row[k]) == repr(plain[k]), k
    assert open(tmp_path / "conv.csv").read().splitlines()[0].endswith("DIST_PIXFMT,CONVERT")


def test_an_eight_bit_rung_against_a_ten_bit_master(engine, tmp_path, clip):
    """convert first, to the reference's depth and chroma layout at the rung's size; scale follows on the same lane"""
    from rtvqa_amd import video_processing as vp
    ref, _dist, _bgr, rung = clip
    got = _run(tmp_path, "both", ref, rung, dist_pixfmt=DIST, convert="linear", scale="bicubic", dist_height=H // 2, dist_width=W // 2,
               **KINDS)
    mid = R.convert_packed(rung, _planes(DIST, H // 2, W // 2), _planes(REF, H // 2, W // 2))
    scaled = vp.frame_scale(mid, REF, H // 2, W // 2, H, W, "bicubic", engine=engine)
    plain = _run(tmp_path, "plain", ref, scaled, **KINDS)
    doc = _same(got, plain, {"DIST_RES": "%dx%d" % (W // 2, H // 2), "SCALE": "bicubic", "DIST_PIXFMT": DIST,
                             "CONVERT": "linear/center/limited"})
    assert list(doc)[-4:] == ["DIST_RES", "SCALE"] + list(OWN_KEYS)


def test_without_the_keys_a_run_is_what_it_was(engine, tmp_path, clip):
    """an equal-layout pair: the keywords at their defaults against the keywords simply absent"""
    ref, dist, bgr, _rung = clip
    ref8 = R.convert_packed(ref, _planes(REF), _planes(DIST))          # (any 8-bit 4:2:0 reference will do)
    from rtvqa_amd import video_processing as vp
    logs = {}
    for tag, kw in (("absent", {}), ("named", dict(dist_pixfmt=None, convert=None, convert_siting="center", convert_range="limited"))):
        logs[tag] = [str(tmp_path / ("%s_%s.log" % (k, tag))) for k in ("psnr", "ssim", "vmaf")]
        assert vp.run_ffmpeg_metrics(ref8, dist, *logs[tag], layout=DIST, height=H, width=W, batch_size=3, **KINDS, **kw) is None
    for x, y in zip(logs["absent"], logs["named"]):
        assert open(x, "rb").read() == open(y, "rb").read()
    assert not set(OWN_KEYS) & set(json.load(open(logs["absent"][2])))
    cfg = {"crf": 23, "resize_width": 64, "resize_height": 64, "frame_interval": 1, "batch_size": 3, "pixfmt": DIST, "height": H,
           "width": W, "gmsd": True}
    rows = [vp.process_video_and_extract_metrics(ref8, dist, dict(cfg, **kw), csv_file=str(tmp_path / ("eq%d.csv" % i)),
                                                 column_order="fixed", encoded_bgr=bgr)
            for i, kw in enumerate(({}, dict(dist_pixfmt=None, convert=None)))]
    assert list(rows[0]) == list(rows[1]) and all(repr(rows[0][k]) == repr(rows[1][k]) for k in rows[0])
    assert not set(OWN_KEYS) & set(rows[0])
