"""GPU: conform through the reference-shaped entry points - frame_conform, run_ffmpeg_metrics and
process_video_and_extract_metrics with and without the `conform` key.  A 4:2:0 clip of the project's synthetic content at
96 x 128; the distorted stream is made in NumPy: the reference delayed by two frames, shifted, put through full_to_limited (or a
gamma), plus noise of one unit.  What a conformed run writes is compared byte for byte with a plain run over the pair that the
restatement (tests/conform_reference.py) conformed by the same plan."""
import csv
import json
import logging
import os

import numpy as np
import pytest

import conform_cases as CC
import conform_reference as R

pytestmark = pytest.mark.gpu

H, W, N_FRAMES, DELAY = 96, 128, 12, 2
LAYOUT = {8: "yuv420p", 10: "yuv420p10le"}


def _planes(depth, h=H, w=W):
    from rtvqa_amd import video_processing as vp
    return vp.LAYOUTS[LAYOUT[depth]][0](h, w)


def _split(frames, depth, h=H, w=W):
    return CC.split(np.ascontiguousarray(frames).view(np.uint8).reshape(len(frames), -1), _planes(depth, h, w), depth)


def _join(frames, depth):
    """a list of frames (lists of plane arrays) -> the planar stream [n, samples] of the layout"""
    return np.stack([np.concatenate([a.reshape(-1) for a in fr]) for fr in frames]).astype(np.uint16 if depth > 8 else np.uint8)


def _moved(plane, dy, dx):
    """the plane that shows at (y, x) what `plane` shows at (y + dy, x + dx), its border repeated"""
    h, w = plane.shape
    return plane[np.clip(np.arange(h) + dy, 0, h - 1)][:, np.clip(np.arange(w) + dx, 0, w - 1)]


def _moved_chroma(plane, dy, dx):
    """a 4:2:0 chroma plane under the luma shift (dy, dx): half the shift, an odd one as the mean of the two whole chroma
    shifts around it (a picture moved by one luma line moves its chroma by half a chroma line), rounded"""
    parts = [_moved(plane, sy, sx).astype(np.float64) for sy in {dy // 2, -(-dy // 2)} for sx in {dx // 2, -(-dx // 2)}]
    return np.rint(sum(parts) / len(parts)).astype(plane.dtype)


def _full_to_limited(fr, depth):
    s, peak = 1 << (depth - 8), (1 << depth) - 1
    y = 16.0 * s + fr[0].astype(np.float64) * (219.0 * s / peak)
    c = [128.0 * s + (a.astype(np.float64) - 128.0 * s) * (224.0 * s / peak) for a in fr[1:]]
    return [np.clip(np.rint(a), 0, peak) for a in [y] + c]


def _gamma(fr, depth):
    peak = (1 << depth) - 1
    return [np.clip(np.rint(peak * (fr[0].astype(np.float64) / peak) ** 0.8), 0, peak)] + [a.astype(np.float64) for a in fr[1:]]


def _pair(depth, shift, colour, seed=3):
    """(ref, dist): dist[j] shows ref[j - DELAY] moved by `shift` in the luma and by half of it in the chroma (_moved_chroma)"""
    from rtvqa_amd import frames, synth
    src = frames.bgr_to_yuv420p(synth.s_natural(N_FRAMES + DELAY, H, W, seed=seed))
    if depth > 8:   # the same picture on ten bits, its two low bits filled
        src = src.astype(np.uint16) * 4 + (np.arange(src.shape[1], dtype=np.uint16) % 4)[None]
    rng = np.random.default_rng(seed)
    peak = (1 << depth) - 1
    dist = []
    for fr in _split(src[:N_FRAMES], depth):
        fr = [_moved(fr[0], *shift)] + [_moved_chroma(a, *shift) for a in fr[1:]]
        fr = colour(fr, depth)
        dist.append([np.clip(a + rng.integers(-1, 2, a.shape), 0, peak) for a in fr])
    return np.ascontiguousarray(src[DELAY:]), _join(dist, depth)


def _restated(ref, dist, depth, plan):
    """both streams conformed by the NumPy restatement with the plan's arguments -> planar streams of the conformed size"""
    sizes = [(int(q[1]), int(q[0])) for q in plan["out_planes"]]
    out = []
    for frames, side in ((ref, plan["ref"]), (dist, plan["dist"])):
        out.append(_join(R.conform(_split(frames, depth), sizes, side["origin"], side["index"], side["lut"], side["matrix"], depth),
                         depth))
    return out


def _run(tmp_path, tag, ref, enc, depth, h=H, w=W, **kw):
    from rtvqa_amd import video_processing as vp
    logs = [str(tmp_path / ("%s_%s.log" % (k, tag))) for k in ("psnr", "ssim", "vmaf")]
    assert vp.run_ffmpeg_metrics(ref, enc, *logs, layout=LAYOUT[depth], height=h, width=w, **kw) is None
    return logs


def _same_files(a, b, upto=2):
    for x, y in zip(a[:upto], b[:upto]):
        assert open(x, "rb").read() == open(y, "rb").read()


PRE_KEYS = ("ALIGN_", "SHIFT_", "COLORFIT_", "CONFORM_", "SYNC_")
KINDS = dict(gmsd=True, motion=True, cambi=True)   # a pair kind, a halo kind of the reference, a kind of the distorted stream


def _check_against_plain(tmp_path, tag, ref, dist, depth, plan, got, doc):
    cr, cd = _restated(ref, dist, depth, plan)
    oh, ow = plan["out_height"], plan["out_width"]
    assert doc["CONFORM_RES"] == "%dx%d" % (ow, oh) and doc["CONFORM_FRAMES"] == len(cr) == len(cd)
    plain = _run(tmp_path, tag + "_plain", cr, cd, depth, oh, ow, batch_size=4, **KINDS)
    _same_files(got, plain)                            # the psnr and ssim stats lines, byte for byte
    rest = {k: v for k, v in doc.items() if not k.startswith(PRE_KEYS)}
    assert open(plain[2]).read() == json.dumps(rest, indent=1) + "\n"     # and the feature log but for the pre-passes' keys


@pytest.mark.parametrize("depth,shift", ((8, (-1, 2)), (10, (-1, 2)), (8, (2, -2))))
def test_a_delayed_shifted_range_squeezed_stream_is_put_right(engine, tmp_path, caplog, depth, shift):
    from rtvqa_amd import conform as CO
    from rtvqa_amd import video_processing as vp
    ref, dist = _pair(depth, shift, _full_to_limited)
    with caplog.at_level(logging.WARNING):
        got = _run(tmp_path, "conf", ref, dist, depth, align=3, shift=4, colorfit=True, conform=True, batch_size=4, **KINDS)
    doc = json.load(open(got[2]))
    assert list(doc)[-7:] == list(CO.CONFORM_KEYS)
    odd = int(shift[0] % 2 or shift[1] % 2)
    want = {"CONFORM_OFFSET": -DELAY, "CONFORM_DY": shift[0], "CONFORM_DX": shift[1], "CONFORM_COLOR": "match:full_to_limited",
            "CONFORM_FRAMES": N_FRAMES - DELAY, "CONFORM_CHROMA_HALF": odd}
    assert {k: doc[k] for k in want} == want
    assert (doc["ALIGN_OFFSET"], doc["SHIFT_DY"], doc["SHIFT_DX"]) == (-DELAY, shift[0], shift[1])
    assert doc["COLORFIT_MATCH"] == "full_to_limited"            # measured on the pair registered in time and place
    assert bool([r for r in caplog.records if "half a chroma sample" in r.getMessage()]) == bool(odd)
    plan = vp._conform_plan(LAYOUT[depth], H, W, shift=shift, offset=-DELAY, n_ref=N_FRAMES, n_dist=N_FRAMES,
                            color=("match", "full_to_limited"))
    assert plan["summary"]["CONFORM_CHROMA_HALF"] == odd
    _check_against_plain(tmp_path, "conf", ref, dist, depth, plan, got, doc)
    # what it was worth: the luma of the conformed pair differs by the noise and two roundings alone
    psnr_y = lambda logs: float(open(logs[0]).readline().split("psnr_y:")[1].split()[0])
    assert psnr_y(got) > psnr_y(_run(tmp_path, "given", ref, dist, depth)) + 10.0


def test_every_prepass_on_through_both_entry_points(engine, tmp_path):
    """all six pre-passes at once: the one chain behind both entry points finds and writes the same, in the table's order"""
    from rtvqa_amd import synth
    from rtvqa_amd import video_processing as vp
    shift = (-1, 2)
    ref, dist = _pair(8, shift, _full_to_limited)
    on = dict(sync=True, sync_apply=True, light=True, align=3, shift=4, colorfit=True, conform=True)
    got = _run(tmp_path, "all", ref, dist, 8, batch_size=4, **on, **KINDS)
    doc = json.load(open(got[2]))
    cfg = {"crf": 23, "resize_width": 64, "resize_height": 64, "frame_interval": 1, "batch_size": 4, "pixfmt": "yuv420p",
           "height": H, "width": W}
    row = vp.process_video_and_extract_metrics(ref, dist, dict(cfg, **on), csv_file=str(tmp_path / "all.csv"), column_order="fixed",
                                               encoded_bgr=synth.s_natural(N_FRAMES, H, W, seed=3))
    keys = [k for p in vp.PREPASSES for k in p.keys]
    assert [p.name for p in vp.PREPASSES] == ["light", "sync", "colorfit", "align", "shift", "conform"]
    assert list(doc)[-len(keys):] == keys == list(row)[-len(keys):]                  # the table's order, log and row
    assert [(k, repr(doc[k])) for k in keys] == [(k, repr(row[k])) for k in keys]    # found alike by both entry points
    # sync's trim re-paired the streams, so align finds nothing left and conform applies no offset of its own
    want = {"SYNC_OFFSET": -DELAY, "SYNC_APPLIED": 1, "ALIGN_OFFSET": 0, "SHIFT_DY": shift[0], "SHIFT_DX": shift[1],
            "COLORFIT_MATCH": "full_to_limited", "CONFORM_OFFSET": 0, "CONFORM_DY": shift[0], "CONFORM_DX": shift[1],
            "CONFORM_COLOR": "match:full_to_limited", "CONFORM_FRAMES": N_FRAMES - DELAY, "CONFORM_CHROMA_HALF": 1}
    assert {k: doc[k] for k in want} == want
    assert 0.0 < doc["LIGHT_MAXFALL"] <= doc["LIGHT_MAXCLL"] <= 10000.0
    # the files are those of a plain run over the pair the restatement conformed: the same frames, named from the untrimmed streams
    plan = vp._conform_plan(LAYOUT[8], H, W, shift=shift, offset=-DELAY, n_ref=N_FRAMES, n_dist=N_FRAMES,
                            color=("match", "full_to_limited"))
    _check_against_plain(tmp_path, "all", ref, dist, 8, plan, got, {k: v for k, v in doc.items() if not k.startswith("LIGHT_")})
    # and the row's PSNR and SSIM are the first lines' of those files
    first = vp.extract_metrics_from_logs(got[0], got[1], "absent", "x", 23, 0, "%dx%d" % (W, H), 30.0)
    assert (row["PSNR"], row["SSIM"]) == (first["PSNR"], first["SSIM"])


def test_an_even_shift_leaves_the_chroma_exact(engine):
    from rtvqa_amd import video_processing as vp
    clean = lambda fr, depth: [a.astype(np.float64) for a in fr]
    ref, dist = _pair(8, (2, -2), clean)
    rng_free = _join([[_moved(fr[0], 2, -2)] + [_moved(a, 1, -1) for a in fr[1:]] for fr in _split(ref, 8)], 8)   # no delay, no noise
    cr, cd, summary = vp.frame_conform(ref, rng_free, LAYOUT[8], H, W, shift=(2, -2), engine=engine)
    assert summary["CONFORM_CHROMA_HALF"] == 0 and summary["CONFORM_RES"] == "126x94" and (cr == cd).all()
    odd = _join([[_moved(fr[0], -1, 2)] + [_moved(a, -1, 1) for a in fr[1:]] for fr in _split(ref, 8)], 8)
    cr, cd, summary = vp.frame_conform(ref, odd, LAYOUT[8], H, W, shift=(-1, 2), engine=engine)
    luma = (H - 2) * (W - 2)
    assert summary["CONFORM_CHROMA_HALF"] == 1 and summary["CONFORM_RES"] == "126x94" and (cr[:, :luma] == cd[:, :luma]).all()
    assert dist.shape == ref.shape


def test_frame_conform_equals_the_restatement_in_any_window(engine):
    from rtvqa_amd import video_processing as vp
    for depth in (8, 10):
        ref, dist = _pair(depth, (-1, 2), _full_to_limited)
        kw = dict(shift=(-1, 2), offset=-DELAY, color=("match", "full_to_limited"))
        plan = vp._conform_plan(LAYOUT[depth], H, W, n_ref=N_FRAMES, n_dist=N_FRAMES, **kw)
        want = _restated(ref, dist, depth, plan)
        for window, wrap in ((256, lambda a: a), (3, lambda a: a), (1, engine.upload)):
            cr, cd, summary = vp.frame_conform(wrap(ref), wrap(dist), LAYOUT[depth], H, W, engine=engine, window=window, **kw)
            assert (cr == want[0]).all() and (cd == want[1]).all() and cr.dtype == ref.dtype, (depth, window)
            assert summary["CONFORM_FRAMES"] == N_FRAMES - DELAY
    # a path: a repeat, a drop, a partner that does not exist
    ref, dist = _pair(8, (0, 0), _gamma)
    path = [-1, 0, 1, 1, 3, 4, 6, 7, 8, 9, 10, 12]
    plan = vp._conform_plan(LAYOUT[8], H, W, ref_index=path, n_ref=N_FRAMES, n_dist=N_FRAMES)
    want = _restated(ref, dist, 8, plan)
    cr, cd, summary = vp.frame_conform(ref, dist, LAYOUT[8], H, W, ref_index=path, engine=engine, window=4)
    assert summary["CONFORM_FRAMES"] == 10 and (cr == want[0]).all() and (cd == want[1]).all() and (cd == dist[1:11]).all()
    with pytest.raises(ValueError, match="window"):
        vp.frame_conform(ref, dist, LAYOUT[8], H, W, engine=engine, window=0)


@pytest.mark.parametrize("mode", ("levels", "tone", "matrix"))
def test_a_gamma_mismatch_corrected_by_a_fit(engine, tmp_path, mode):
    """no dB bar: what is applied is the fit of the registered pair with the roles swapped, and the files are those of the
    restatement's pair"""
    from rtvqa_amd import video_processing as vp
    shift = (2, -2)
    ref, dist = _pair(8, shift, _gamma)
    got = _run(tmp_path, mode, ref, dist, 8, align=3, shift=4, colorfit=True, conform=True, conform_color=mode, batch_size=4,
               **KINDS)
    doc = json.load(open(got[2]))
    assert doc["CONFORM_COLOR"] == mode and (doc["CONFORM_OFFSET"], doc["CONFORM_DY"], doc["CONFORM_DX"]) == (-DELAY,) + shift
    # the fit, from the restatement's pair registered in time and place: frame_colorfit(enc, ref)
    place = vp._conform_plan(LAYOUT[8], H, W, shift=shift, offset=-DELAY, n_ref=N_FRAMES, n_dist=N_FRAMES)
    cr, cd = _restated(ref, dist, 8, place)
    _rec, tab, res = vp.frame_colorfit(cd, cr, LAYOUT[8], place["out_height"], place["out_width"], engine=engine)
    color = {"levels": ("levels", res["gain"], res["offset"]), "matrix": ("matrix", res["matrix"], res["matrix_offset"]),
             "tone": ("tone", tab.tolist())}[mode]
    assert doc["COLORFIT_GAIN_Y"] == float(res["gain"][0])      # the COLORFIT_* keys describe the registered pair, roles swapped
    plan = vp._conform_plan(LAYOUT[8], H, W, shift=shift, offset=-DELAY, n_ref=N_FRAMES, n_dist=N_FRAMES, color=color)
    _check_against_plain(tmp_path, mode, ref, dist, 8, plan, got, doc)


def test_without_conform_every_file_is_what_it_was(engine, tmp_path):
    ref, dist = _pair(8, (-1, 2), _full_to_limited)
    for tag, keys in (("bare", {}), ("keys", dict(align=3, shift=4, colorfit=True, sync=True, **KINDS))):
        was = _run(tmp_path, tag + "_was", ref, dist, 8, **keys)
        off = _run(tmp_path, tag + "_off", ref, dist, 8, conform=False, conform_color="tone", **keys)
        _same_files(was, off, upto=3 if keys else 2)
        assert os.path.exists(was[2]) == bool(keys)
    # place alone: conform_color "none" needs no colorfit, and a "match" that finds nothing applies nothing
    a = _run(tmp_path, "none", ref, dist, 8, shift=4, conform=True, conform_color="none")
    doc = json.load(open(a[2]))
    assert (doc["CONFORM_OFFSET"], doc["CONFORM_COLOR"], doc["CONFORM_FRAMES"]) == (0, "none", N_FRAMES)
    b = _run(tmp_path, "nomatch", ref, ref.copy(), 8, shift=4, colorfit=True, conform=True)
    doc = json.load(open(b[2]))
    assert (doc["COLORFIT_MATCH"], doc["CONFORM_COLOR"], doc["CONFORM_DY"], doc["CONFORM_DX"]) == ("none", "none", 0, 0)
    assert doc["CONFORM_RES"] == "%dx%d" % (W, H)
    _same_files(b, _run(tmp_path, "self", ref, ref.copy(), 8))


def test_the_refusals_of_the_entry_point(tmp_path):
    ref = np.zeros((2, H * W * 3 // 2), np.uint8)
    for kw, said in ((dict(conform=True), "at least one"), (dict(conform=True, shift=2), "needs colorfit"),
                     (dict(conform=1, shift=2), "true or false"), (dict(conform=True, shift=2, conform_color="gamma"), "one of"),
                     (dict(conform=True, sync=True, conform_color="none", scale="bicubic", dist_height=H, dist_width=W), "scale")):
        with pytest.raises(ValueError, match=said):
            _run(tmp_path, "bad", ref, ref, 8, **kw)
    ten = np.zeros((2, H * W * 3 // 2), np.uint16)
    from rtvqa_amd import video_processing as vp
    logs = [str(tmp_path / ("%s_12.log" % k)) for k in ("psnr", "ssim", "vmaf")]
    with pytest.raises(ValueError, match="10 bits"):
        vp.run_ffmpeg_metrics(ten, ten, *logs, layout="yuv420p12le", height=H, width=W, colorfit=True, conform=True,
                              conform_color="tone")


def test_the_row_of_the_one_pass_entry_point(tmp_path):
    from rtvqa_amd import conform as CO
    from rtvqa_amd import shift as SH
    from rtvqa_amd import synth
    from rtvqa_amd import video_processing as vp
    ref, dist = _pair(8, (2, -2), _full_to_limited)
    cfg = {"crf": 23, "resize_width": 64, "resize_height": 64, "frame_interval": 1, "batch_size": 5, "pixfmt": "yuv420p",
           "height": H, "width": W}
    bgr = synth.s_natural(N_FRAMES, H, W, seed=3)
    plain = vp.process_video_and_extract_metrics(ref, dist, cfg, csv_file=str(tmp_path / "plain.csv"), column_order="fixed",
                                                 encoded_bgr=bgr)
    off = vp.process_video_and_extract_metrics(ref, dist, dict(cfg, conform=False), csv_file=str(tmp_path / "off.csv"),
                                               column_order="fixed", encoded_bgr=bgr)
    assert list(off) == list(plain) and all(repr(off[k]) == repr(plain[k]) for k in plain)
    assert open(str(tmp_path / "plain.csv"), "rb").read() == open(str(tmp_path / "off.csv"), "rb").read()
    row = vp.process_video_and_extract_metrics(ref, dist, dict(cfg, align=3, shift=4, colorfit=True, conform=True),
                                               csv_file=str(tmp_path / "conf.csv"), column_order="fixed", encoded_bgr=bgr)
    assert list(row)[-7:] == list(CO.CONFORM_KEYS) and list(row)[-12:-7] == list(SH.SHIFT_KEYS)
    assert (row["CONFORM_OFFSET"], row["CONFORM_DY"], row["CONFORM_DX"], row["CONFORM_COLOR"], row["CONFORM_RES"],
            row["CONFORM_FRAMES"], row["CONFORM_CHROMA_HALF"]) == (-DELAY, 2, -2, "match:full_to_limited", "126x94", 10, 0)
    assert row["PSNR"] > plain["PSNR"] + 10.0
    rows = list(csv.reader(open(str(tmp_path / "conf.csv"))))
    assert rows[0][-7:] == list(CO.CONFORM_KEYS) and rows[1][-4] == "match:full_to_limited"
    with pytest.raises(ValueError, match="quality half's own"):
        vp.process_video_and_extract_metrics(bgr, bgr, {"crf": 23, "resize_width": 64, "resize_height": 64, "shift": 2,
                                                        "conform": True, "conform_color": "none"},
                                             csv_file=str(tmp_path / "x.csv"))
