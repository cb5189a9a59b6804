"""Host-side mirror of the reference's quality-metric surface
(/root/reference/video_processing.py:145-177, :270-297), backed by the HIP engine.

run_ffmpeg_metrics keeps the reference's contract: it takes the reference and the
distorted stream plus the log paths, returns None and delivers its results as
FFmpeg-format stats files, so extract_metrics_from_logs' regular expressions
(:160, :166) parse them unchanged.  The streams are frame stacks (arrays / .npy)
instead of container files: decode is out of scope.  Without a model file
(vmaf_model_path None) there is no VMAF value and — as in the reference when the
log has none (:169-173) — the 'VMAF' key is simply missing; with one, the pass
also measures VIF, ADM and motion, vmaf_model.predict scores every frame and the
log carries pooled_metrics.vmaf, which extract_metrics_from_logs reads as the
reference does.
"""
import os
import re
import threading
from collections import namedtuple

import numpy as np

from . import _native as N
from . import stream
from .align import ALIGN_KEYS
from .colorfit import COLORFIT_KEYS
from .complexity_metrics import _open_frames
from .conform import CONFORM_KEYS
from .engine import DeviceFrames, bgr_planes, gray_planes, yuv420p_planes, yuv_planes
from .features import (FEATURES, ITP_RANGES, KINDS, MODEL_PATHS, PARAM_CHECKS, PSNR_HVS_DB_CAP, PU21_PSNR_CAP,  # noqa: F401
                       check_switch, switches)
from .frames import PIXFMTS, frame_samples
from .light import LIGHT_KEYS
from .shift import SHIFT_KEYS
from .sync import SYNC_KEYS

LAYOUTS = {
    # name: (plane builder, component letters as FFmpeg prints them)
    "bgr24": (bgr_planes, "bgr"),     # packed BGR24 frames [N,H,W,3]; FFmpeg labels RGB components r,g,b
    "gray": (gray_planes, "y"),       # [N,H,W]
    "yuv420p": (yuv420p_planes, "yuv"),  # [N, H*W*3/2] planar
}
# the other planar pix_fmts, by FFmpeg's names (frames.PIXFMTS): [N, samples per frame] planar, uint16 above 8 bits
for _name, (_chroma, _depth, _tag) in PIXFMTS.items():
    if _name not in LAYOUTS:
        LAYOUTS[_name] = ((lambda h, w, c=_chroma, d=_depth: yuv_planes(h, w, c, d)), "y" if _chroma == "mono" else "yuv")
_SSIM_MODES = {"gauss": N.SSIM_GAUSS, "ffmpeg": N.SSIM_FFMPEG, "msssim": N.SSIM_MS}


def layout_depth(layout):
    """bits per sample of a layout (8 for bgr24 / gray / yuv420p)"""
    return PIXFMTS[layout][1] if layout in PIXFMTS else 8


def _geometry(reference, layout, height, width):
    planar = layout not in ("bgr24", "gray")
    if isinstance(reference, DeviceFrames):
        if planar and reference.h == 1 and height and width:   # [N, samples] planar frames (Engine.upload of a 2-D array)
            return height, width
        return reference.h, reference.w
    if planar or reference.ndim == 2:   # planar [N, samples]: the geometry comes from the header / config
        return height, width
    return reference.shape[1], reference.shape[2]


def _host_stream(a, wide=False):
    """wide: a stream of the quality half, which may hold uint16 samples (9..16-bit planar frames)"""
    if isinstance(a, DeviceFrames):
        return a
    if type(a).__module__.startswith("torch") and hasattr(a, "is_cuda"):
        if wide and a.dtype.__str__() == "torch.uint16":
            a = DeviceFrames.from_torch(a if a.is_contiguous() else a.contiguous()) if a.is_cuda else a.numpy()
        else:
            from .complexity_metrics import _from_torch
            a = _from_torch(a)
        if isinstance(a, DeviceFrames):
            return a
    a = np.asarray(a)
    if a.dtype != np.uint8 and not (wide and a.dtype == np.uint16):  # a silent cast would turn float frames in 0..1 into all-zero planes
        raise ValueError("frames must be uint8 (got %s)" % a.dtype)
    return a


def _config_switches(config):
    """a validated config -> what it asks of the quality half (features.switches): stream.Quality's keywords for the kinds and
    their parameters, and the model files' paths.  Pure: no file and no device is touched."""
    return switches(config, config=True)


def _check_request(f, layout, values):
    """what can be said of a kind's request before a stream is opened, under the names the caller knows: the flag and
    run_ffmpeg_metrics' keywords, by which `values` goes"""
    if f.three_planes and len(LAYOUTS[layout][1]) != 3:
        raise ValueError("%s needs three planes" % f.flag)
    for p in f.params:
        if p.early:
            PARAM_CHECKS[p.quality](p.flag, values[p.flag])


def _only_pass(kind, streams, layout, height, width, engine, batch_size, device, **params):
    """One pass that measures `kind` alone (stream.Quality's "only") over streams = (reference, encoded) or the one stream the
    kind reads; params: the kind's parameters by run_ffmpeg_metrics' keywords, further Quality keywords as they are.
    -> (the pass's last element: the kind's records, planes)"""
    f = next(f for f in FEATURES if f.kind == kind)
    _check_request(f, layout, params)
    names = {p.flag: p.quality for p in f.params}   # the entry points' keyword -> Quality's
    quality = {names.get(k, k): v for k, v in params.items()}
    quality[kind] = "only"
    streams = [_host_stream(a, wide=True) for a in streams]
    if len(streams) == 2 and not isinstance(streams[0], DeviceFrames) and streams[0].shape != streams[1].shape:
        raise ValueError("ref and dist must have the same shape")
    h, w = _geometry(streams[0], layout, height, width)
    planes = LAYOUTS[layout][0](h, w)
    q, _ = stream.run(streams[-1], streams[0], quality=stream.Quality(planes, **quality), batch_size=batch_size, engine=engine,
                      device=device)
    return q[-1], planes


def _sizes(planes):
    return [(p[0], p[1]) for p in planes]


def frame_quality(reference, distorted, layout="bgr24", ssim_mode="gauss", height=None, width=None, engine=None,
                  batch_size=64, on_chunk=None, device=None, scales=False):
    """Per-frame SSE and SSIM per plane.  Returns (sse [n,p] uint64, ssim [n,p] float64, plane sizes).
    ssim_mode "msssim": the ssim values are multi-scale SSIM (five scales of the Gaussian window; every plane at least
    161 x 161, so a 4:2:0 frame at least 321 x 321); scales=True then appends {"cs": [n,p,5], "ssim": [n,p,5]}, the per-scale
    means the values are the product of.
    One pass (stream.run): chunks of up to batch_size frame pairs alternate between two engines; host streams travel
    from the caller's pinned memory or through the pinned ring.  on_chunk(first_frame, sse, ssim) sees every finished
    chunk in frame order while the next one is on the GPU."""
    reference, distorted = _host_stream(reference, wide=True), _host_stream(distorted, wide=True)
    if not isinstance(reference, DeviceFrames) and reference.shape != distorted.shape:
        raise ValueError("ref and dist must have the same shape")
    h, w = _geometry(reference, layout, height, width)
    planes = LAYOUTS[layout][0](h, w)
    q, _ = stream.run(distorted, reference, quality=stream.Quality(planes, _SSIM_MODES[ssim_mode], scales),
                      batch_size=batch_size, engine=engine, on_quality=on_chunk, device=device)
    sizes = [(p[0], p[1]) for p in planes]
    if scales:
        return q[0], q[1], sizes, {"cs": q[2], "ssim": q[3]}
    return q[0], q[1], sizes


def frame_vif(reference, distorted, layout="bgr24", height=None, width=None, engine=None, batch_size=64, device=None):
    """Per-frame VIF per plane on four scales (Engine.vif through the one-pass pipeline of frame_quality).
    Returns (scale [n,p,4] float64 - libvmaf's vif_scale0..3 -, vif [n,p] float64 - sum of the numerators over the sum of the
    denominators of the four scales -, plane sizes).  Every plane at least 16 x 16."""
    r, planes = _only_pass("vif", (reference, distorted), layout, height, width, engine, batch_size, device)
    return r["scale"], r["vif"], _sizes(planes)


def frame_adm(reference, distorted, layout="bgr24", height=None, width=None, engine=None, batch_size=64, device=None):
    """Per-frame ADM per plane on four scales (Engine.adm through the one-pass pipeline of frame_quality).
    Returns (scale [n,p,4] float64 - libvmaf's adm_scale0..3 -, adm2 [n,p] float64 - sum of the numerators over the sum of the
    denominators of the four scales -, plane sizes).  Every plane at least 16 x 16."""
    r, planes = _only_pass("adm", (reference, distorted), layout, height, width, engine, batch_size, device)
    return r["scale"], r["adm2"], _sizes(planes)


def frame_motion(reference, layout="bgr24", height=None, width=None, engine=None, batch_size=64, device=None):
    """Per-frame motion per plane of the REFERENCE stream (Engine.motion through the one-pass pipeline of frame_quality; the
    stream is uploaded once, there is no distorted stream).
    Returns (motion [n,p] float64 - libvmaf's `motion`: the mean absolute difference of the blurred frame and the blurred frame
    before it, 0 for frame 0 -, motion2 [n,p] float64 - min(motion[i], motion[i+1]), the last frame keeping its motion -, plane
    sizes).  Every plane at least 16 x 16."""
    r, planes = _only_pass("motion", (reference,), layout, height, width, engine, batch_size, device)
    return r["motion"], r["motion2"], _sizes(planes)


def frame_siti(reference, layout="bgr24", height=None, width=None, engine=None, batch_size=64, device=None):
    """Per-frame ITU-T P.910 spatial and temporal information per plane of the REFERENCE stream (Engine.siti through the
    one-pass pipeline of frame_quality; the stream is uploaded once, there is no distorted stream).
    Returns (si [n,p] float64 - the standard deviation of the Sobel magnitude over the plane's interior -, ti [n,p] float64 - the
    standard deviation of the difference to the frame before, 0 for frame 0 -, plane sizes), both on the 8-bit scale.  P.910's
    SI and TI of the clip are si.max(axis=0) and ti.max(axis=0).  Every plane at least 16 x 16."""
    r, planes = _only_pass("siti", (reference,), layout, height, width, engine, batch_size, device)
    return r["si"], r["ti"], _sizes(planes)


def frame_psnr_hvs(reference, encoded, layout="bgr24", height=None, width=None, engine=None, batch_size=64, device=None):
    """Per-frame PSNR-HVS and PSNR-HVS-M per plane (Engine.psnr_hvs through the one-pass pipeline of frame_quality; both
    streams are uploaded once).  The definition is include/vqa.h's: the published 8x8-block form, whole blocks only.
    Returns (psnr_hvs [n,p] float64 dB, psnr_hvsm [n,p] float64 dB - inf for identical planes: nothing is capped here -,
    s_hvs [n,p], s_hvsm [n,p] - the two CSF-weighted mean squared errors -, plane sizes).  Every plane at least 16 x 16."""
    r, planes = _only_pass("psnr_hvs", (reference, encoded), layout, height, width, engine, batch_size, device)
    return r["psnr_hvs"], r["psnr_hvsm"], r["s_hvs"], r["s_hvsm"], _sizes(planes)


def frame_ciede(reference, encoded, layout="bgr24", height=None, width=None, weights=N.CIEDE_WEIGHTS_CIE, engine=None,
                batch_size=64, device=None):
    """Per-frame CIEDE2000 (Engine.ciede through the one-pass pipeline of frame_quality; both streams are uploaded once): the
    three planes of a pixel taken together, by the definition in include/vqa.h - bgr24 as sRGB, the planar YUV layouts as BT.709
    limited range with replicated chroma.  weights: (kL, kC, kH); (1, 1, 1) is the CIE standard, N.CIEDE_WEIGHTS_LIBVMAF =
    (0.65, 1, 4) what libvmaf's ciede2000 feature is believed to use (unverified).
    Returns (ciede2000 [n] float64 = 45 - 20 log10(de_mean), inf for identical frames: nothing is capped here -, de_mean [n]).
    Luma at least 16 x 16; a one-plane layout is a ValueError."""
    r, _ = _only_pass("ciede", (reference, encoded), layout, height, width, engine, batch_size, device, ciede_weights=weights)
    return r["ciede2000"], r["de_mean"]


def frame_gmsd(reference, encoded, layout="bgr24", height=None, width=None, engine=None, batch_size=64, device=None):
    """Per-frame GMSD per plane (Engine.gmsd through the one-pass pipeline of frame_quality; both streams are uploaded once).
    The definition is include/vqa.h's: a 2x2 mean at step 2, Prewitt with a zero border, the similarity of the gradient
    magnitudes and its standard deviation (divisor N - 1) over the downsampled grid.
    Returns (gmsd [n,p] float64 - exactly 0 for identical planes -, gms_mean [n,p] float64 - the paper's GMSM, exactly 1 for
    identical planes -, plane sizes).  Every plane at least 16 x 16."""
    r, planes = _only_pass("gmsd", (reference, encoded), layout, height, width, engine, batch_size, device)
    return r["gmsd"], r["gms_mean"], _sizes(planes)


def frame_cambi(frames, layout="bgr24", height=None, width=None, engine=None, batch_size=64, device=None):
    """Per-frame CAMBI, the banding index, per plane of ONE stream (Engine.cambi through the one-pass pipeline of frame_quality;
    the stream is uploaded once, there is no second stream).  The definition is include/vqa.h's: 10 bits, a 2x2 anti-dither
    mean, a 7 x 7 flatness mask, five scales, the 65 x 65 contrast counts for steps of 1..4 levels, the top 30 % per scale
    and the scale weights 16, 8, 4, 2, 1 - integers up to the last division.
    Returns (cambi [n,p] float64 - exactly 0 for a plane without banding -, pool [n,p,5] float64, plane sizes).  Every plane
    at least 16 x 16."""
    r, planes = _only_pass("cambi", (frames,), layout, height, width, engine, batch_size, device)
    return r["cambi"], r["pool"], _sizes(planes)


def frame_xpsnr(reference, encoded, layout="yuv420p", height=None, width=None, engine=None, batch_size=64, device=None):
    """Per-frame XPSNR per plane (Engine.xpsnr through the one-pass pipeline of frame_quality; both streams are uploaded once,
    and every chunk after the first sees the reference frame before it).  The definition is include/vqa.h's: per block the
    squared error of every plane divided by the spatial and temporal activity of the REFERENCE's luma there (first-order
    temporal activity, no small-picture smoothing, plain 2 x 2 sums above HD - not FFmpeg's filter in these three).
    Returns (xpsnr [n,p] float64 in dB - inf for identical planes -, wsse [n,p] float64, plane sizes, block).  Planar layouts
    whose first plane is the luma (bgr24 is a ValueError); every plane at least 16 x 16."""
    from .engine import xpsnr_grid
    r, planes = _only_pass("xpsnr", (reference, encoded), layout, height, width, engine, batch_size, device)
    return r["xpsnr"], r["wsse"], _sizes(planes), xpsnr_grid(planes[0][0], planes[0][1])[0]


def frame_haarpsi(reference, encoded, layout="bgr24", height=None, width=None, engine=None, batch_size=64, device=None):
    """Per-frame HaarPSI per plane (Engine.haarpsi through the one-pass pipeline of frame_quality; both streams are uploaded
    once).  The definition is include/vqa.h's: a 2x2 mean at step 2, Haar coefficients of three scales and two orientations with
    a zero border, the local similarity of the two finer scales weighted by the coarsest, a sigmoid with alpha = 4.2 and its
    inverse - the grayscale index per plane, as recalled from the authors' HaarPSI.m and not pinned against it.
    Returns (haarpsi [n,p] float64 - exactly 1 for identical planes -, similarity [n,p] float64 - the weighted mean of the
    sigmoid -, plane sizes).  Every plane at least 16 x 16."""
    r, planes = _only_pass("haarpsi", (reference, encoded), layout, height, width, engine, batch_size, device)
    return r["haarpsi"], r["similarity"], _sizes(planes)


def frame_vca(reference, layout="yuv420p", height=None, width=None, engine=None, batch_size=64, device=None, blocks=False):
    """Per-frame VCA texture features per plane of the REFERENCE stream (Engine.vca through the one-pass pipeline of
    frame_quality; the stream is uploaded once, there is no distorted stream, and every chunk after the first sees the frame
    before it).  The definition is include/vqa.h's: per whole 32 x 32 block the orthonormal DCT-II, H_k = the sum of
    exp(|(u v / 1024)^2 - 1|) |D(u, v)| without the DC, and the block's sample sum - the paper's method, not pinned against the
    VCA tool, whose integer transform and normalisation of L differ.
    Returns (e [n,p] float64 - the spatial texture energy -, h [n,p] float64 - its temporal gradient, 0 for frame 0 and exactly 0
    for a repeated frame -, l [n,p] float64 - the brightness -, plane sizes), all on the 8-bit scale; with blocks=True also the
    block maps: per plane dict(qh, s as uint64 [n, nby, nbx]), qh in steps of 2^-(24 - depth).  Planar layouts (bgr24 is a
    ValueError); every plane at least 32 x 32."""
    last, planes = _only_pass("vca", (reference,), layout, height, width, engine, batch_size, device, vca_blocks=blocks)
    r, maps = last if blocks else (last, None)
    out = (r["e"], r["h"], r["l"], _sizes(planes))
    return out + (maps,) if blocks else out


def frame_artifacts(frames, layout="bgr24", height=None, width=None, engine=None, batch_size=64, device=None):
    """Per-frame no-reference blockiness, blur and noise per plane of ONE stream (Engine.artifacts through the one-pass pipeline of
    frame_quality; the stream is uploaded once, there is no second stream).  The definition is include/vqa.h's: the boundary
    steps of Wang, Sheikh and Bovik resolved by the phase of an 8 x 8 grid, the blur measure of Crete-Roffet et al. with a 9-tap
    mean, Immerkaer's noise estimate on the 8-bit scale - integers up to the last division, no tool compared.
    Returns (dict of [n,p] arrays: blockiness, blockiness_max, blur, noise as float64 and phase_h, phase_v as int32; plane
    sizes).  Every plane at least 16 x 16; packed bgr24 is measured per channel."""
    r, planes = _only_pass("artifacts", (frames,), layout, height, width, engine, batch_size, device)
    keys = ("blockiness", "blockiness_max", "phase_h", "phase_v", "blur", "noise")
    return {k: r[k] for k in keys}, _sizes(planes)


def frame_brisque(frames, layout="bgr24", height=None, width=None, engine=None, batch_size=64, device=None):
    """Per-frame BRISQUE natural-scene statistics per plane of ONE stream (Engine.brisque through the one-pass pipeline of
    frame_quality; the stream is uploaded once, there is no second stream).  The definition is include/vqa.h's: the MSCN field
    and its four neighbour products at two scales, a GGD and four AGGD fits per scale - after Mittal, Moorthy and Bovik's
    code as recalled, not pinned against it.
    Returns (features [n, p, 36] float64, flags [n, p] uint32, plane sizes).  Every plane at least 16 x 16; packed bgr24 is
    measured per channel."""
    r, planes = _only_pass("brisque", (frames,), layout, height, width, engine, batch_size, device)
    return np.ascontiguousarray(r["features"]), np.ascontiguousarray(r["flags"]), _sizes(planes)


def frame_mdsi(reference, encoded, layout="bgr24", height=None, width=None, engine=None, batch_size=64, device=None):
    """Per-frame MDSI, the mean deviation similarity index (Engine.mdsi through the one-pass pipeline of frame_quality; both
    streams are uploaded once): the planes of a pixel taken together, by the definition in include/vqa.h - gradient similarity
    of the luminance with the fused-image term, chromaticity similarity of two opponent channels, the mean absolute deviation of
    the complex quarter power; bgr24 as B, G, R, the planar YUV layouts as BT.709 limited range with replicated chroma, gray as
    luma alone - the authors' MDSI.m with the "sum" combination as recalled, not pinned against it.  (reference, encoded) is
    ordered: the metric is not symmetric.
    Returns (mdsi [n] float64 - exactly 0 for identical frames, larger is worse -, dev [n] float64, the deviation before the last
    quarter power).  Plane 0 at least 16 x 16."""
    r, _ = _only_pass("mdsi", (reference, encoded), layout, height, width, engine, batch_size, device)
    return np.ascontiguousarray(r["mdsi"]), np.ascontiguousarray(r["dev"])


def frame_delta_itp(reference, encoded, layout="bgr24", height=None, width=None, transfer="pq", full_range=False, engine=None,
                    batch_size=64, device=None):
    """Per-frame dE_ITP, the HDR colour difference of ITU-R BT.2124 (Engine.itp through the one-pass pipeline of frame_quality;
    both streams are uploaded once): the three planes of a pixel taken together, by the definition in include/vqa.h - the planar
    YUV layouts as BT.2020 non-constant luminance with replicated chroma, bgr24 as B, G, R; transfer "pq" or "hlg" (BT.2100, HLG
    on a 1000 cd/m2 display); full_range False (limited) or True (ignored for bgr24).  1 is about one just-noticeable difference.
    Returns (delta_itp [n] float64, the mean over the luma grid - exactly 0 for identical frames -, delta_itp_max [n] float64,
    the largest value of a pixel).  Luma at least 16 x 16; a one-plane layout, an unknown transfer or range is a ValueError."""
    r, _ = _only_pass("itp", (reference, encoded), layout, height, width, engine, batch_size, device,
                      delta_itp_transfer=transfer, delta_itp_full_range=full_range)
    return np.ascontiguousarray(r["de_mean"]), np.ascontiguousarray(r["de_max"])


def frame_pu21(reference, encoded, layout="bgr24", height=None, width=None, transfer="pq", full_range=False, engine=None,
               batch_size=64, device=None):
    """Per-frame PU21-PSNR and PU21-SSIM (Engine.pu21 through the one-pass pipeline of frame_quality; both streams are uploaded
    once): the three planes of a pixel taken together and read as a BT.2020 signal, turned into display light and PU21-encoded, by
    the definition in include/vqa.h - the planar YUV layouts as BT.2020 non-constant luminance with replicated chroma, bgr24 as
    B, G, R; transfer "pq" or "hlg" (HLG on a 1000 cd/m2 display); full_range False (limited) or True (ignored for bgr24).
    Returns (pu_psnr [n], pu_psnr_rgb [n], pu_ssim [n], mse_y [n], mse_rgb [n]), float64: the PSNRs at a peak of 256 PU units (inf
    for identical frames, not capped here), the Gaussian SSIM of the PU-encoded luminance (exactly 1 for identical frames) and the
    mean squared errors in PU units.  Luma at least 16 x 16; a one-plane layout, an unknown transfer or range is a ValueError."""
    r, _ = _only_pass("pu21", (reference, encoded), layout, height, width, engine, batch_size, device,
                      pu21_transfer=transfer, pu21_full_range=full_range)
    return tuple(np.ascontiguousarray(r[k]) for k in ("pu_psnr", "pu_psnr_rgb", "pu_ssim", "mse_y", "mse_rgb"))


def frame_fsim(reference, encoded, layout="bgr24", height=None, width=None, engine=None, batch_size=64, device=None):
    """Per-frame FSIM and FSIMc (Engine.fsim through the one-pass pipeline of frame_quality; both streams are uploaded once): phase
    congruency and Scharr gradient similarity of the luminance, with the chromaticity of I and Q in the colour form, the planes of
    a pixel taken together by the definition in include/vqa.h - the planar YUV layouts as BT.709 limited range with replicated
    chroma, bgr24 as B, G, R, the gray layouts as luma alone (fsimc == fsim there) - the authors' FeatureSIM.m as recalled, not
    pinned against it.  Returns (fsim [n], fsimc [n]) float64, exactly 1 for identical frames, smaller is worse.  Plane 0 at least
    16 x 16; one- and three-plane layouts."""
    r, _ = _only_pass("fsim", (reference, encoded), layout, height, width, engine, batch_size, device)
    return np.ascontiguousarray(r["fsim"]), np.ascontiguousarray(r["fsimc"])


def frame_sigstats(frames, layout="bgr24", height=None, width=None, engine=None, batch_size=64, device=None, black_level=None,
                   crop_level=None):
    """Per-frame signal statistics per plane of ANY stream (Engine.sigstats through the one-pass pipeline of frame_quality; the
    stream is uploaded once, there is no second stream): the exact levels, order statistics, range counts, bit masks, the
    difference to the frame before and the dark-border box, by the definition in include/vqa.h.  black_level, crop_level: None
    (32 and 24 on the 8-bit scale) or integers in sample units.  Returns the records [n,p] (engine.SIGSTATS_DTYPE); frame 0 has
    no predecessor.  events.signal_events turns them into black / frozen runs, cuts and the crop box.  Every plane at least
    16 x 16."""
    return _only_pass("sigstats", (frames,), layout, height, width, engine, batch_size, device, sigstats_black=black_level,
                      sigstats_crop=crop_level)[0]


def frame_scale(frames, layout, height, width, out_height, out_width, filter="bicubic", engine=None, batch_size=64, device=None):
    """The stream resampled to out_height x out_width on the GPU (Engine.scale: Pillow's Image.resize arithmetic, include/vqa.h;
    filter "bilinear" | "bicubic" | "lanczos"; every plane of the layout over its own grid, chroma centre-sited) -> a host
    array [n, out frame samples] of the input's dtype, in chunks of batch_size frames.  frames: what frame_cambi takes; height
    and width are read off [N,H,W(,3)] arrays and needed for planar [N, samples] ones.  Every plane on both sides at least
    16 x 16, ratios within 1/4 .. 8 per axis (ValueError)."""
    from .engine import check_scale_planes, planes_span, scale_filter
    frames = _host_stream(frames, wide=True)
    scale_filter(filter)
    h, w = _geometry(frames, layout, height, width)
    planes, out_planes = LAYOUTS[layout][0](h, w), LAYOUTS[layout][0](int(out_height), int(out_width))
    check_scale_planes(planes, out_planes)
    wide = layout_depth(layout) > 8
    n = _frame_count(frames)
    out = np.zeros((n, planes_span(out_planes) // (2 if wide else 1)), np.uint16 if wide else np.uint8)
    if n == 0:
        return out
    eng = engine if engine is not None else stream.get_engine(device)
    with stream.pass_lock(eng.device):
        for a, b in _frame_windows(n, int(batch_size)):
            res = eng.scale(_frame_part(frames, a, b), planes, out_planes, filter)
            out[a:b] = eng.download(res)
            res._owner.free()
    return out


def frame_convert(frames, layout, out_layout, height=None, width=None, chroma="linear", siting="center", range="limited",
                  engine=None, batch_size=64, device=None):
    """The stream written at another sample depth and / or chroma layout on the GPU (Engine.convert: include/vqa.h's integer
    definition, one rounding per sample; chroma "box" | "linear", siting "center" | "left", range "limited" | "full") -> a host
    array [n, frame samples of out_layout] of out_layout's sample type, in chunks of batch_size frames.  frames: what
    frame_scale takes, at `layout`; height and width are needed for planar [N, samples] arrays.  Both layouts have the same
    number of planes (mono to mono, three planes to three planes; packed bgr24 is not built): ValueError otherwise."""
    from .engine import check_convert_planes, convert_options, planes_span
    frames = _host_stream(frames, wide=True)
    convert_options(chroma, siting, range)
    _check_convert_layouts(layout, out_layout, equal_ok=True)
    h, w = _geometry(frames, layout, height, width)
    planes, out_planes = LAYOUTS[layout][0](h, w), LAYOUTS[out_layout][0](h, w)
    check_convert_planes(planes, out_planes)
    wide = layout_depth(out_layout) > 8
    n = _frame_count(frames)
    out = np.zeros((n, planes_span(out_planes) // (2 if wide else 1)), np.uint16 if wide else np.uint8)
    if n == 0:
        return out
    eng = engine if engine is not None else stream.get_engine(device)
    with stream.pass_lock(eng.device):
        for a, b in _frame_windows(n, int(batch_size)):
            res = eng.convert(_frame_part(frames, a, b), planes, out_planes, chroma, siting, range)
            out[a:b] = eng.download(res)
            res._owner.free()
    return out


FIELDS_WINDOW = 1024   # the frames of one submit of frame_fields and frame_weave (the C limit is 32768)


def _fields_request(values):
    """the fields argument / config key -> whether the measurement is on; a ValueError for anything but a boolean"""
    fields = values.get("fields", False)
    if not isinstance(fields, (bool, np.bool_)):
        raise ValueError("fields must be true or false.")
    return bool(fields)


def frame_fields(frames, layout, height=None, width=None, plane=0, engine=None, device=None, window=FIELDS_WINDOW):
    """Interlace and 3:2 pulldown detection of ONE whole clip (Engine.fields, include/vqa.h): per frame the comb, forward,
    backward, SAD and changed words of planes[plane] per row parity, exact integers; then fields.analyse: idet's single-frame
    rule as recalled (NOT pinned against FFmpeg), the repeated fields and a 3:2 cadence with its phase, field order and breaks.
    The clip is walked in windows of `window` frames and the last frame of a window is the next one's prev0: any window size
    gives the same records.  -> (records [n] of N.FIELDS_DTYPE, the analysis).  The plane at least 16 x 16."""
    from . import fields as F
    window = int(window)
    if window < 1:
        raise ValueError("window must be a positive integer.")
    frames = _host_stream(frames, wide=True)
    h, w = _geometry(frames, layout, height, width)
    planes = LAYOUTS[layout][0](h, w)
    if not 0 <= int(plane) < len(planes):
        raise ValueError("plane must be 0 .. %d for %s (got %r)" % (len(planes) - 1, layout, plane))
    n = _frame_count(frames)
    if not n:
        raise ValueError("the clip must hold at least one frame")
    eng = engine if engine is not None else stream.get_engine(device)
    rec = np.zeros(n, N.FIELDS_DTYPE)
    with stream.pass_lock(eng.device):
        for a, b in _frame_windows(n, window):
            prev0 = None if a == 0 else (frames.frame(a - 1) if isinstance(frames, DeviceFrames) else _frame_part(frames, a - 1, a))
            rec[a:b] = eng.fields(_frame_part(frames, a, b), planes, prev0, int(plane))
    return rec, F.analyse(rec)


def frame_weave(frames, layout, top_index, bottom_index, height=None, width=None, engine=None, device=None, window=FIELDS_WINDOW):
    """Frames out of the fields of other frames on the GPU (Engine.weave): the even rows of every plane of output frame j from
    frame top_index[j], the odd rows from frame bottom_index[j] - fields.telecine_plan, ivtc_plan and field_plan give such
    pairs.  The source clip is uploaded once and the output walked in windows of `window` frames.  -> a host array [n_out, frame
    samples] of the input's dtype."""
    from .engine import planes_span
    window = int(window)
    if window < 1:
        raise ValueError("window must be a positive integer.")
    frames = _host_stream(frames, wide=True)
    h, w = _geometry(frames, layout, height, width)
    planes = LAYOUTS[layout][0](h, w)
    wide = layout_depth(layout) > 8
    top, bottom = (np.asarray(a, np.int64).reshape(-1) for a in (top_index, bottom_index))
    if top.size != bottom.size:
        raise ValueError("top_index and bottom_index must be equally long (got %d and %d)" % (top.size, bottom.size))
    n = _frame_count(frames)
    out = np.zeros((top.size, planes_span(planes) // (2 if wide else 1)), np.uint16 if wide else np.uint8)
    if top.size == 0:
        return out
    if min(top.min(), bottom.min()) < 0 or max(top.max(), bottom.max()) >= n:
        raise ValueError("top_index and bottom_index must name source frames 0 .. %d" % (n - 1))
    eng = engine if engine is not None else stream.get_engine(device)
    with stream.pass_lock(eng.device):
        for a, b in _frame_windows(top.size, window):
            # the source frames this window names, and the indices counted from the first of them
            lo, hi = int(min(top[a:b].min(), bottom[a:b].min())), int(max(top[a:b].max(), bottom[a:b].max())) + 1
            res = eng.weave(_frame_part(frames, lo, hi), planes, top[a:b] - lo, bottom[a:b] - lo)
            out[a:b] = eng.download(res)
            res._owner.free()
    return out


def fields_extra(ref_analysis, dist_analysis):
    """the two analyses of frame_fields -> the nine top-level keys of the log and the row (fields.FIELDS_KEYS, in that order).  A
    distorted stream that is not progressive, or streams that do not match, are also a warning in the log of this module"""
    import logging
    from . import fields as F
    extra = F.summary_keys(ref_analysis, dist_analysis)
    if extra["FIELDS_DIST_TYPE"] != "progressive" or extra["FIELDS_DIST_CADENCE"] != "none":
        logging.getLogger(__name__).warning(
            "the distorted stream is not progressive at the reference's cadence (type %s, cadence %s, %d combed frames, %d frames "
            "that repeat a field): frame i of it need not be frame i of the reference", extra["FIELDS_DIST_TYPE"],
            extra["FIELDS_DIST_CADENCE"], extra["FIELDS_DIST_COMBED"], extra["FIELDS_DIST_REPEATS"])
    if not extra["FIELDS_MATCH"]:
        logging.getLogger(__name__).warning(
            "the two streams differ in field structure (reference: %s, cadence %s; distorted: %s, cadence %s): nothing was changed, "
            "fields.ivtc_plan and Engine.weave undo a pulldown", extra["FIELDS_REF_TYPE"], extra["FIELDS_REF_CADENCE"],
            extra["FIELDS_DIST_TYPE"], extra["FIELDS_DIST_CADENCE"])
    return extra


def _fields_keys(on, ref, layout, h, w, dist, dist_layout, dh, dw, extra, device):
    """the fields measurement of an entry point, over the streams as given - the reference at its layout, the distorted stream
    at its own size and layout - before any pre-pass: extra (DIST_RES, SCALE, DIST_PIXFMT, CONVERT or None) with the nine keys
    behind it.  Off: extra as it is, and no stream is touched."""
    if not on:
        return extra
    ra = frame_fields(ref, layout, h, w, device=device)[1]
    da = frame_fields(dist, dist_layout, dh, dw, device=device)[1]
    return dict(extra or {}, **fields_extra(ra, da))


ALIGN_WINDOW = 4096   # the distorted frames of one submit of frame_align (the C limit is 32768)


def _align_request(align, scale=None):
    """the align argument / config key -> the radius, or None when alignment is off; a ValueError for anything else"""
    if align is None:
        return None
    if isinstance(align, bool) or not isinstance(align, (int, np.integer)) or not 1 <= align <= N.ALIGN_MAX_RADIUS:
        raise ValueError("align must be null or an integer radius from 1 to %d." % N.ALIGN_MAX_RADIUS)
    if scale is not None:
        raise ValueError("align and scale do not go together: a ladder rung is not aligned at its own size.")
    return int(align)


def frame_align(reference, encoded, layout, height=None, width=None, radius=8, engine=None, device=None, window=ALIGN_WINDOW):
    """Temporal alignment of two whole clips of any lengths (Engine.align, include/vqa.h): the squared error of plane 0 of the
    layout between encoded frame j and reference frame j + k, k = -radius .. radius, and what align.analyse reads off it.  The
    encoded stream is walked in windows of `window` frames; a window [a, b) submits the reference frames [a - radius, b + radius),
    clipped, with the matching offset, and the bands are joined - any window size gives the same array.  -> analyse's dict
    (offset, match, ref_index, dropped, repeated, mismatched, sse_given, sse_aligned, psnr_gain) plus "sse", uint64
    [n, 2 radius + 1] with align.NONE where the reference frame does not exist.  Nothing is re-paired."""
    from . import align as A
    R, window = int(radius), int(window)
    if not 0 <= R <= N.ALIGN_MAX_RADIUS:
        raise ValueError("radius must be an integer from 0 to %d." % N.ALIGN_MAX_RADIUS)
    if not 1 <= window <= N.ALIGN_MAX_DIST:
        raise ValueError("window must be an integer from 1 to %d." % N.ALIGN_MAX_DIST)
    ref, enc = _host_stream(reference, wide=True), _host_stream(encoded, wide=True)
    h, w = _geometry(ref, layout, height, width)
    planes = LAYOUTS[layout][0](h, w)
    n_ref, n = _frame_count(ref), _frame_count(enc)
    if not n_ref or not n:
        raise ValueError("both clips must hold at least one frame")
    sse = np.full((n, 2 * R + 1), A.NONE, np.uint64)
    eng = engine if engine is not None else stream.get_engine(device)
    with stream.pass_lock(eng.device):
        for a, b in _frame_windows(n, window):
            lo, hi = max(a - R, 0), min(b + R, n_ref)
            if hi > lo:   # (else: no reference frame near this window, its rows stay NONE)
                sse[a:b] = eng.align(_frame_part(ref, lo, hi), _frame_part(enc, a, b), planes, R, offset=a - lo)
    out = A.analyse(sse)
    out["sse"] = sse
    return out


def align_extra(result, radius):
    """frame_align's (align.analyse's) dict -> the five top-level keys of the log and the row; a clip that is not aligned is
    also a warning in the log of this module"""
    import logging
    from . import align as A
    extra = A.log_keys(result, radius)
    if extra["ALIGN_OFFSET"] or extra["ALIGN_DROPPED"] or extra["ALIGN_REPEATED"]:
        logging.getLogger(__name__).warning(
            "the distorted stream is not aligned with the reference: offset %d, %d dropped, %d repeated frame(s); pairing the "
            "frames as given costs %.2f dB of PSNR (the frames are NOT re-paired)", extra["ALIGN_OFFSET"], extra["ALIGN_DROPPED"],
            extra["ALIGN_REPEATED"], extra["ALIGN_PSNR_GAIN"])
    return extra


SYNC_WINDOW = 4096   # the frames of one submit of frame_sync's signatures (the C limit is 32768)


def _sync_request(sync, min_overlap=None, apply=False):
    """the sync arguments / config keys -> (min_overlap, apply), or None when sync is off; a ValueError for anything else"""
    if not isinstance(sync, (bool, np.bool_)):
        raise ValueError("sync must be true or false.")
    if not isinstance(apply, (bool, np.bool_)):
        raise ValueError("sync_apply must be true or false.")
    if min_overlap is not None and (isinstance(min_overlap, bool) or not isinstance(min_overlap, (int, np.integer))
                                    or min_overlap < 1):
        raise ValueError("sync_min_overlap must be null or an integer >= 1.")
    if apply and not sync:
        raise ValueError("sync_apply needs sync: nothing is trimmed by an offset that was not measured.")
    return (None if min_overlap is None else int(min_overlap), bool(apply)) if sync else None


def _sync_config(config):
    """the config keys "sync", "sync_min_overlap" and "sync_apply" -> _sync_request's answer"""
    return _sync_request(config.get("sync", False), config.get("sync_min_overlap"), config.get("sync_apply", False))


def _frame_count(a):
    return a.n if isinstance(a, DeviceFrames) else a.shape[0]


def _frame_slice(a, lo, length):
    """frames lo .. lo + length - 1 of a stream: a view of an array, DeviceFrames.slice of resident frames"""
    return a.slice(lo, lo + length) if isinstance(a, DeviceFrames) else a[lo:lo + length]


def _frame_part(a, lo, hi):
    """frames lo .. hi - 1 of a stream as ONE SUBMIT of a frame_* walk: DeviceFrames.slice of resident frames, a contiguous
    [hi - lo, samples] array of host frames"""
    return a.slice(lo, hi) if isinstance(a, DeviceFrames) else np.ascontiguousarray(a[lo:hi]).reshape(hi - lo, -1)


def _frame_windows(n, window):
    """the bounds (a, b) of the windows of `window` frames a clip of n frames is walked in"""
    return [(a, min(n, a + window)) for a in range(0, n, window)]


def frame_sync(reference, encoded, layout, height=None, width=None, dist_height=None, dist_width=None, min_overlap=None,
               refine=None, engine=None, device=None, window=SYNC_WINDOW):
    """Clip-wide sync of two whole clips of any lengths (Engine.signature, Engine.sig_cross, include/vqa.h): the 256-byte
    signature of plane 0 of every frame of both streams, taken in windows of `window` frames - any window size gives the same
    arrays - then ONE cross of all distorted against all reference signatures, and what sync.analyse reads off it.  The
    signature is a 16 x 16 grid whatever the size, so the encoded stream may have a geometry of its own (dist_height,
    dist_width: a ladder rung); nothing is scaled.  -> analyse's dict (offset, mean, overlap, runner_up, ambiguous, per_frame,
    frames_off, runs, trim) plus "ref_sig" and "dist_sig" (uint8 [n, 256]), "diag" and "best".  refine=R (streams of one
    geometry only): also "align", frame_align of radius R on the two streams trimmed to the found overlap - the exact band
    around the found offset.  Nothing is re-paired."""
    from . import sync as S
    window = int(window)
    if not 1 <= window <= N.SIG_MAX_BATCH:
        raise ValueError("window must be an integer from 1 to %d." % N.SIG_MAX_BATCH)
    own = dist_height is not None or dist_width is not None
    if refine is not None:
        if isinstance(refine, bool) or not isinstance(refine, (int, np.integer)) or not 0 <= refine <= N.ALIGN_MAX_RADIUS:
            raise ValueError("refine must be null or an integer radius from 0 to %d." % N.ALIGN_MAX_RADIUS)
        if own:
            raise ValueError("refine needs streams of one geometry: frame_align compares samples.")
    ref, enc = _host_stream(reference, wide=True), _host_stream(encoded, wide=True)
    h, w = _geometry(ref, layout, height, width)
    dh, dw = _geometry(enc, layout, dist_height or height, dist_width or width) if own else _geometry(enc, layout, h, w)
    planes_r, planes_d = LAYOUTS[layout][0](h, w), LAYOUTS[layout][0](dh, dw)
    n_ref, n = _frame_count(ref), _frame_count(enc)
    if not n_ref or not n:
        raise ValueError("both clips must hold at least one frame")
    if n_ref > N.SIG_MAX_FRAMES or n > N.SIG_MAX_FRAMES:
        raise ValueError("a clip of more than %d frames is not synchronised in one cross." % N.SIG_MAX_FRAMES)
    eng = engine if engine is not None else stream.get_engine(device)
    sigs = []
    with stream.pass_lock(eng.device):
        for a, count, planes in ((ref, n_ref, planes_r), (enc, n, planes_d)):
            sig = np.empty((count, N.SIG_BYTES), np.uint8)
            for lo, hi in _frame_windows(count, window):
                sig[lo:hi] = eng.signature(_frame_part(a, lo, hi), planes)
            sigs.append(sig)
        diag, best = eng.sig_cross(sigs[1], sigs[0])
    out = S.analyse(diag, best, n, n_ref, min_overlap)
    out.update(ref_sig=sigs[0], dist_sig=sigs[1], diag=diag, best=best)
    if refine is not None:
        ref_lo, dist_lo, length = out["trim"]
        out["align"] = frame_align(_frame_slice(ref, ref_lo, length), _frame_slice(enc, dist_lo, length), layout, h, w,
                                   int(refine), engine=engine, device=device)
    return out


def sync_extra(result, applied):
    """frame_sync's (sync.analyse's) dict -> the six top-level keys of the log and the row; an offset, frames that pair
    elsewhere, an ambiguous answer and a trim that was applied are also warnings in the log of this module"""
    import logging
    from . import sync as S
    extra = S.log_keys(result, applied)
    log = logging.getLogger(__name__)
    if result["ambiguous"]:
        log.warning("the sync of the two streams is ambiguous: offset %d and offset %d fit equally well (a static or looping "
                    "clip); the streams go on as given", extra["SYNC_OFFSET"], result["runner_up"][0])
    elif applied:
        log.warning("the streams were trimmed to their overlap: %d frame(s) from reference frame %d and distorted frame %d "
                    "(offset %d, %d frame(s) pair elsewhere)", result["trim"][2], result["trim"][0], result["trim"][1],
                    extra["SYNC_OFFSET"], extra["SYNC_FRAMES_OFF"])
    elif extra["SYNC_OFFSET"] or extra["SYNC_FRAMES_OFF"]:
        log.warning("the distorted stream is not in sync with the reference: offset %d over %d frame(s), %d frame(s) pair "
                    "elsewhere (the frames are NOT re-paired: sync_apply trims both streams to the overlap)",
                    extra["SYNC_OFFSET"], extra["SYNC_OVERLAP"], extra["SYNC_FRAMES_OFF"])
    return extra


def _sync_streams(request, ref, dist, layout, h, w, dh, dw, device):
    """the sync pre-pass of the two entry points: request is _sync_request's (min_overlap, apply).  -> (the six keys, the trim
    to apply or None, sync.analyse's dict).  The trim is applied only where the answer is not ambiguous, and counts as applied
    only where it cuts."""
    own = (dh, dw) != (h, w)
    res = frame_sync(ref, dist, layout, h, w, dh if own else None, dw if own else None, request[0], device=device)
    ref_lo, dist_lo, length = res["trim"]
    cuts = request[1] and not res["ambiguous"] and (ref_lo or dist_lo or length != _frame_count(_host_stream(ref, wide=True))
                                                    or length != _frame_count(_host_stream(dist, wide=True)))
    return sync_extra(res, bool(cuts)), (res["trim"] if cuts else None), res


SHIFT_WINDOW = 1024   # the frames of one submit of frame_shift (the C limit is 32768)


def _shift_request(shift, margin=None, scale=None):
    """the shift and shift_margin arguments / config keys -> (radius, margin), or None when the search is off; a ValueError
    for anything else"""
    def integer(v):
        return not isinstance(v, bool) and isinstance(v, (int, np.integer))

    if shift is None:
        if margin is not None:
            raise ValueError("shift_margin needs shift: nothing is searched without a radius.")
        return None
    if not integer(shift) or not 1 <= shift <= N.SHIFT_MAX_RADIUS:
        raise ValueError("shift must be null or an integer radius from 1 to %d." % N.SHIFT_MAX_RADIUS)
    if margin is not None and (not integer(margin) or margin < shift):
        raise ValueError("shift_margin must be null or an integer not below shift.")
    if scale is not None:
        raise ValueError("shift and scale do not go together: a ladder rung is not registered at its own size.")
    return int(shift), int(shift if margin is None else margin)


def frame_shift(reference, encoded, layout, height=None, width=None, radius=4, margin=None, engine=None, device=None,
                window=SHIFT_WINDOW):
    """Spatial registration of two whole clips of one length (Engine.shift, include/vqa.h): the squared error of plane 0 of the
    layout between encoded frame j and reference frame j read at every shift (dy, dx) of -radius .. radius, over the core
    `margin` (default: radius) samples inside the plane, and what shift.analyse reads off it.  The clip is walked in windows
    of `window` frames; a frame's grid depends on its own pair alone - any window size gives the same array.  -> analyse's dict
    (shift, per_frame, frames_off, edge, sse_given, sse_shifted, psnr_gain, subpixel) plus "sse", uint64
    [n, 2 radius + 1, 2 radius + 1].  Nothing is moved."""
    from . import shift as S
    window = int(window)
    R, M = _shift_request(radius, margin)
    if not 1 <= window <= N.SHIFT_MAX_FRAMES:
        raise ValueError("window must be an integer from 1 to %d." % N.SHIFT_MAX_FRAMES)
    ref, enc = _host_stream(reference, wide=True), _host_stream(encoded, wide=True)
    h, w = _geometry(ref, layout, height, width)
    planes = LAYOUTS[layout][0](h, w)
    n = _frame_count(enc)
    if not n or _frame_count(ref) != n:
        raise ValueError("both clips must hold the same number of frames, at least one")
    sse = np.zeros((n, 2 * R + 1, 2 * R + 1), np.uint64)
    eng = engine if engine is not None else stream.get_engine(device)
    with stream.pass_lock(eng.device):
        for a, b in _frame_windows(n, window):
            sse[a:b] = eng.shift(_frame_part(ref, a, b), _frame_part(enc, a, b), planes, R, M)
    out = S.analyse(sse)
    out["sse"] = sse
    return out


def shift_extra(result, radius):
    """frame_shift's (shift.analyse's) dict -> the five top-level keys of the log and the row; a clip that is not in place, or
    whose best shift lies on the band's border, is also a warning in the log of this module"""
    import logging
    from . import shift as S
    extra = S.log_keys(result, radius)
    if extra["SHIFT_DY"] or extra["SHIFT_DX"] or result["edge"]:
        logging.getLogger(__name__).warning(
            "the distorted picture is not in place: it shows at (y, x) what the reference shows at (y %+d, x %+d)%s; %d frame(s) "
            "have another best shift; comparing in place costs %.2f dB of PSNR (the frames are NOT moved)", extra["SHIFT_DY"],
            extra["SHIFT_DX"], ", which is the border of the band: the true shift may lie beyond radius %d" % radius
            if result["edge"] else "", extra["SHIFT_FRAMES_OFF"], extra["SHIFT_PSNR_GAIN"])
    return extra


COLORFIT_WINDOW = 1024   # the frames of one submit of frame_colorfit (the C limit is 32768, and n h w <= 2^31 with tables)


def _colorfit_request(colorfit, scale=None, layout=None):
    """the colorfit argument / config key -> whether the fit is on; a ValueError for anything else"""
    if not isinstance(colorfit, (bool, np.bool_)):
        raise ValueError("colorfit must be true or false.")
    if colorfit and scale is not None:
        raise ValueError("colorfit and scale do not go together: the fit is taken sample against sample on one grid, and a "
                         "ladder rung is not fitted at its own size.")
    if colorfit and layout is not None and len(LAYOUTS[layout][0](16, 16)) not in (1, 3):
        raise ValueError("colorfit takes one plane or the three planes of a pixel together: %s has %d"
                         % (layout, len(LAYOUTS[layout][0](16, 16))))
    return bool(colorfit)


def _colorfit_config(config):
    """the config keys "colorfit" and "scale" -> _colorfit_request's answer"""
    check_switch("colorfit", config)
    return _colorfit_request(config.get("colorfit", False), config.get("scale"))


def colorfit_model(layout):
    """the model colorfit.analyse reads a layout as: "bgr" for bgr24, "gray" for one plane, "yuv" otherwise"""
    return "bgr" if layout == "bgr24" else "gray" if len(LAYOUTS[layout][0](16, 16)) == 1 else "yuv"


def frame_colorfit(reference, encoded, layout, height=None, width=None, tables=True, engine=None, device=None,
                   window=COLORFIT_WINDOW):
    """Colour registration of two whole clips of one length (Engine.colorfit, include/vqa.h): per frame pair the joint integer
    moments of the planes of both streams on the luma grid and, with tables, per reference code the count, sum and sum of
    squares of the encoded samples over the whole clip; and what colorfit.analyse reads off them - the per-plane gain and
    offset, the best 3 x 3 matrix, the per-code tone curve, the error each would leave and whether a known mishap (a range
    mix-up, a BT.601 / BT.709 matrix swap) explains the error.  The clip is walked in windows of `window` frames, cut to
    2^31 // (h w) when tables are on, and the tables are summed in Python integers: any window size gives the same arrays.  The
    model and depth come from the layout: bgr24 is "bgr", one plane "gray", otherwise "yuv".  -> (records [n] of
    engine.COLORFIT_DTYPE, tables uint64 [planes, bins, 3] or None, analyse's dict).  Nothing is corrected."""
    from . import colorfit as CF
    from .engine import COLORFIT_DTYPE
    window = int(window)
    if not 1 <= window <= N.COLORFIT_MAX_FRAMES:
        raise ValueError("window must be an integer from 1 to %d." % N.COLORFIT_MAX_FRAMES)
    _colorfit_request(True, None, layout)
    ref, enc = _host_stream(reference, wide=True), _host_stream(encoded, wide=True)
    h, w = _geometry(ref, layout, height, width)
    planes = LAYOUTS[layout][0](h, w)
    if tables:
        window = max(1, min(window, N.COLORFIT_TABLE_POSITIONS // (h * w)))
    n = _frame_count(enc)
    if not n or _frame_count(ref) != n:
        raise ValueError("both clips must hold the same number of frames, at least one")
    rec = np.zeros(n, COLORFIT_DTYPE)
    total = None
    eng = engine if engine is not None else stream.get_engine(device)
    with stream.pass_lock(eng.device):
        for a, b in _frame_windows(n, window):
            rec[a:b], tab = eng.colorfit(_frame_part(ref, a, b), _frame_part(enc, a, b), planes, bool(tables))
            if tables:
                words = [int(v) for v in tab.reshape(-1)]
                total = words if total is None else [x + y for x, y in zip(total, words)]
    nested = None
    if tables:   # [planes][bins][3] in Python integers for the analysis; the array for the caller
        bins = len(total) // (3 * len(planes))
        nested = [[total[(p * bins + i) * 3:(p * bins + i) * 3 + 3] for i in range(bins)] for p in range(len(planes))]
    tab = np.array(nested, np.uint64) if tables else None
    return rec, tab, CF.analyse(rec, layout_depth(layout), colorfit_model(layout), nested)


def colorfit_extra(result, depth):
    """frame_colorfit's (colorfit.analyse's) dict -> the seven top-level keys of the log and the row; a named mishap, or a
    matrix fit that at least halves the error, is also a warning in the log of this module"""
    import logging
    import math
    from . import colorfit as CF
    extra = CF.log_keys(result, depth)
    if result["match"] != "none" or result["psnr_gain"] >= 10.0 * math.log10(2.0):
        found = ("the mishap '%s' explains it: putting it right would gain %.2f dB of PSNR" % (
            extra["COLORFIT_MATCH"], extra["COLORFIT_MATCH_PSNR_GAIN"])) if result["match"] != "none" else \
            "no known mishap explains it"
        logging.getLogger(__name__).warning(
            "a code value does not mean the same in both streams: %s; the best matrix and offset would gain %.2f dB (luma gain "
            "%.4f, offset %+.2f on the 8-bit scale; a per-code curve %.2f dB beyond that); %d frame(s) have another match; "
            "comparing as given costs that much (the frames are NOT corrected)", found, extra["COLORFIT_PSNR_GAIN"],
            extra["COLORFIT_GAIN_Y"], extra["COLORFIT_OFFSET_Y"], extra["COLORFIT_TONE_PSNR_GAIN"], extra["COLORFIT_FRAMES_OFF"])
    return extra


CONFORM_WINDOW = 256   # the output frames of one submit of frame_conform (the C limit is 32768)


def _conform_request(conform, color="match", sync=False, align=None, shift=None, colorfit=False, scale=None):
    """the conform and conform_color arguments / config keys next to the requests they build on -> the colour mode ("none" |
    "match" | "levels" | "matrix" | "tone"), or None when conform is off; a ValueError for anything else"""
    from .conform import COLOR_MODES
    if not isinstance(conform, (bool, np.bool_)):
        raise ValueError("conform must be true or false.")
    if not isinstance(color, str) or color not in COLOR_MODES:
        raise ValueError("conform_color must be one of %s." % ", ".join("'%s'" % m for m in COLOR_MODES))
    if not conform:
        return None
    if scale is not None:
        raise ValueError("conform and scale do not go together: a ladder rung is not registered at its own size.")
    if not (sync or align is not None or shift is not None or colorfit):
        raise ValueError("conform needs at least one of sync, align, shift and colorfit: nothing is applied that was not measured.")
    if color != "none" and not colorfit:
        raise ValueError("conform_color '%s' needs colorfit: no colour map is applied that was not fitted "
                         "(conform_color 'none' applies time and place alone)." % color)
    return color


def _conform_config(config):
    """the config keys "conform" and "conform_color" -> _conform_request's answer"""
    return _conform_request(config.get("conform", False), config.get("conform_color", "match"), config.get("sync", False),
                            config.get("align"), config.get("shift"), config.get("colorfit", False), config.get("scale"))


def _conform_tone_depth(mode, layout):
    """a tone table has one entry per code and colorfit's tables one bin per code up to 10 bits: refused before any pre-pass"""
    from .conform import TONE_MAX_DEPTH
    if mode == "tone" and layout_depth(layout) > TONE_MAX_DEPTH:
        raise ValueError("conform_color 'tone' is built up to %d bits (%s has %d): above, colorfit's bins hold several codes."
                         % (TONE_MAX_DEPTH, layout, layout_depth(layout)))


def _conform_plan(layout, height, width, **found):
    """conform.plan for a layout of this module: the plane builder, depth and colour model follow from it"""
    from . import conform as CO
    return CO.plan(LAYOUTS[layout][0], int(height), int(width), layout_depth(layout), colorfit_model(layout), **found)


def frame_conform(reference, encoded, layout, height=None, width=None, shift=(0, 0), offset=0, ref_index=None, color=None,
                  engine=None, device=None, window=CONFORM_WINDOW):
    """Both streams of a pair registered on the GPU (Engine.conform, include/vqa.h) by what align / sync, shift and colorfit
    found: the frames re-paired by the constant `offset` (or align's ref_index path; frames without a partner are dropped from
    both), the common window of the shift (dy, dx) cut out of both pictures, the colour map `color` applied to the ENCODED
    stream (conform.plan states all three).  -> (reference, encoded, summary): two host arrays [n, conformed frame samples] of
    the inputs' dtype and plan's summary (the CONFORM_* keys, chroma_half, frames).  The output is walked in windows of `window`
    frames; a frame's bytes depend on its own source frame alone - any window size gives the same arrays."""
    from .engine import planes_span
    window = int(window)
    if not 1 <= window <= N.CONFORM_MAX_OUT:
        raise ValueError("window must be an integer from 1 to %d." % N.CONFORM_MAX_OUT)
    ref, enc = _host_stream(reference, wide=True), _host_stream(encoded, wide=True)
    h, w = _geometry(ref, layout, height, width)
    n_ref, n_enc = _frame_count(ref), _frame_count(enc)
    if not n_ref or not n_enc:
        raise ValueError("both clips must hold at least one frame")
    plan = _conform_plan(layout, h, w, shift=shift, offset=offset, ref_index=ref_index, n_ref=n_ref, n_dist=n_enc, color=color)
    planes, out_planes = plan["planes"], plan["out_planes"]
    wide = layout_depth(layout) > 8
    n = plan["summary"]["frames"]
    eng = engine if engine is not None else stream.get_engine(device)
    outs = []
    with stream.pass_lock(eng.device):
        for src, count, side in ((ref, n_ref, plan["ref"]), (enc, n_enc, plan["dist"])):
            index = np.arange(count) if side["index"] is None else np.asarray(side["index"])
            out = np.zeros((n, planes_span(out_planes) // (2 if wide else 1)), np.uint16 if wide else np.uint8)
            for a, b in _frame_windows(n, window):
                ix = index[a:b]
                lo, hi = int(ix.min()), int(ix.max()) + 1   # the source frames this window names
                res = eng.conform(_frame_part(src, lo, hi), planes, out_planes, side["origin"], ix - lo, side["lut"], side["matrix"])
                out[a:a + len(ix)] = eng.download(res)
                res._owner.free()
            outs.append(out)
    return outs[0], outs[1], plan["summary"]


def _conform_offset(align_result, sync_result, trimmed):
    """the constant offset conform applies: align's where it ran (it ran after sync's trim), else sync's where the answer is
    not ambiguous and was not applied already, else 0"""
    if align_result is not None:
        return int(align_result["offset"])
    if sync_result is not None and not sync_result["ambiguous"] and not trimmed:
        return int(sync_result["offset"])
    return 0


def _conform_color(mode, ref, enc, layout, h, w, shift, device):
    """the colour-fit pre-pass of a conformed run: over the pair already registered in time (the caller's slices) and place
    (frame_conform by the found shift), with the roles SWAPPED where the mode applies a fit - frame_colorfit(enc, ref): its
    least-squares map r ~ b + M d is then directly the correction of the encoded stream.  -> (conform.plan's `color`, the
    colorfit result the COLORFIT_* keys are read off)"""
    cr, ce, _ = frame_conform(ref, enc, layout, h, w, shift=shift, device=device)
    place = _conform_plan(layout, h, w, shift=shift)
    oh, ow = place["out_height"], place["out_width"]
    swapped = mode in ("levels", "matrix", "tone")
    _rec, tab, res = frame_colorfit(ce, cr, layout, oh, ow, device=device) if swapped else \
        frame_colorfit(cr, ce, layout, oh, ow, device=device)
    if mode == "match":
        color = None if res["match"] == "none" else ("match", res["match"])
    elif mode == "levels":
        color = ("levels", res["gain"], res["offset"])
    elif mode == "matrix":
        color = ("matrix", res["matrix"], res["matrix_offset"])
    elif mode == "tone":
        color = ("tone", tab.tolist())
    else:
        color = None
    return color, res


def conform_extra(plan, frames, align_result=None, shift_result=None):
    """a plan of conform.plan and the frames the pass will pair -> the seven top-level keys of the log and the row; what conform
    does NOT put right is a warning in the log of this module"""
    import logging
    from . import conform as CO
    extra = CO.log_keys(dict(plan["summary"], CONFORM_FRAMES=int(frames)))
    log = logging.getLogger(__name__)
    if align_result is not None and (align_result["dropped"] or align_result["repeated"]):
        log.warning("conform applies the constant offset %d alone: %d dropped and %d repeated frame(s) stay where they are (a "
                    "per-frame path is frame_conform's)", extra["CONFORM_OFFSET"], align_result["dropped"], align_result["repeated"])
    if shift_result is not None and shift_result["edge"]:
        log.warning("conform applies a shift on the border of the searched band: the true shift may lie beyond it")
    if extra["CONFORM_CHROMA_HALF"]:
        log.warning("conform moved the picture by an odd shift on a subsampled axis: the chroma planes stay half a chroma "
                    "sample apart (nothing is interpolated)")
    return extra


LIGHT_WINDOW = 1024   # the frames of one submit of frame_light (a batch of any length goes out in slices by itself)


def _light_request(light, transfer="pq", full_range=False):
    """the light, light_transfer and light_full_range arguments (the config's "light_range" already turned into the last) ->
    (transfer, full_range), or None when the measurement is off; a ValueError for anything else.  The parameters are checked
    whether light is on or not."""
    if not isinstance(light, (bool, np.bool_)):
        raise ValueError("light must be true or false.")
    if transfer == "hlg":
        raise ValueError("light_transfer 'hlg' is not built: HLG's display light is not a per-channel function (the OOTF needs Ys) "
                         "and CTA-861.3's MaxCLL / MaxFALL are HDR10's; light_transfer must be 'pq'.")
    if transfer != "pq":
        raise ValueError("light_transfer must be 'pq'.")
    if not isinstance(full_range, (bool, np.bool_)):
        raise ValueError("light_full_range must be true or false.")
    return ("pq", bool(full_range)) if light else None


def _light_config(config):
    """the config keys "light", "light_transfer" and "light_range" -> _light_request's answer"""
    rng = config.get("light_range", "limited")
    if not (isinstance(rng, str) and rng in ITP_RANGES):
        raise ValueError('light_range must be "limited" or "full".')
    return _light_request(config.get("light", False), config.get("light_transfer", "pq"), ITP_RANGES[rng])


def frame_light(frames, layout, height=None, width=None, transfer="pq", full_range=False, engine=None, device=None,
                window=LIGHT_WINDOW, table=None, histogram=False):
    """HDR light levels and gamut QC of ONE whole clip (Engine.light, include/vqa.h): per frame the words behind MaxCLL and
    MaxFALL (CTA-861.3, as the header states it - not compared with any tool), the per-channel maxima, the BT.2020 luminance, ten
    percentiles of maxRGB and the counts of pixels outside BT.709 and P3 and of clamped pixels; the planar YUV layouts as BT.2020
    non-constant luminance with replicated chroma, bgr24 as B, G, R; transfer "pq" ("hlg" is a ValueError that says why), or a
    table of the caller's own.  The clip is walked in windows of `window` frames; a frame's record depends on its own samples
    alone - any window size gives the same records.  -> (records [n] of engine.LIGHT_DTYPE, light.summarise's dict), with
    histogram=True (records, summary, uint32 [n, 4096]).  Luma at least 16 x 16; a one-plane layout is a ValueError."""
    from . import light as L
    from .engine import LIGHT_DTYPE
    window = int(window)
    if window < 1:
        raise ValueError("window must be a positive integer.")
    if table is None:
        _light_request(True, transfer, full_range)
    if not isinstance(full_range, (bool, np.bool_)):
        raise ValueError("light_full_range must be true or false.")
    frames = _host_stream(frames, wide=True)
    h, w = _geometry(frames, layout, height, width)
    planes = LAYOUTS[layout][0](h, w)
    if len(planes) != 3:
        raise ValueError("light levels take the three planes of a pixel together: %s has %d" % (layout, len(planes)))
    n = _frame_count(frames)
    if not n:
        raise ValueError("the clip must hold at least one frame")
    eng = engine if engine is not None else stream.get_engine(device)
    if table is None:
        table = eng.light_table(transfer)
    rec = np.zeros(n, LIGHT_DTYPE)
    hist = np.zeros((n, N.LIGHT_BINS), np.uint32) if histogram else None
    with stream.pass_lock(eng.device):
        for a, b in _frame_windows(n, window):
            got = eng.light(_frame_part(frames, a, b), planes, None, transfer, bool(full_range), table, histogram)
            if histogram:
                rec[a:b], hist[a:b] = got
            else:
                rec[a:b] = got
    summary = L.summarise(rec)
    return (rec, summary, hist) if histogram else (rec, summary)


def light_extra(summary):
    """frame_light's summary -> the eight top-level keys of the log and the row (light.LIGHT_KEYS, in that order).  A MaxCLL
    above 10000 cd/m2 or a MaxFALL above MaxCLL is a bug and raises; clamped pixels are also a warning in the log of this module"""
    import logging
    from . import light as L
    L.check(summary)
    extra = {k: (int(summary[k]) if k == "LIGHT_MAXCLL_FRAME" else float(summary[k])) for k in L.LIGHT_KEYS}
    if extra["LIGHT_CLAMPED"] > 0:
        logging.getLogger(__name__).warning(
            "%.4f %% of the reference stream's pixels decode to R'G'B' outside [0, 1] (illegal Y'CbCr combinations or samples above "
            "the depth's peak): they were clamped and counted", 100.0 * extra["LIGHT_CLAMPED"])
    return extra


def _scale_request(scale, dist_height, dist_width):
    """the three arguments that turn scaling on -> whether it is on; a ValueError for a set that does not fit together"""
    for name, v in (("dist_height", dist_height), ("dist_width", dist_width)):
        if v is not None and (isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v <= 0):
            raise ValueError("%s must be a positive integer." % name)
    if scale is None:
        if dist_height is not None or dist_width is not None:
            raise ValueError("dist_height / dist_width need scale: nothing is scaled without a filter being named.")
        return False
    if not (isinstance(scale, str) and scale in N.SCALE_FILTERS):
        raise ValueError("scale must be \"bilinear\", \"bicubic\" or \"lanczos\".")
    if (dist_height is None) != (dist_width is None):
        raise ValueError("dist_height and dist_width go together.")
    return True


def _convert_request(values):
    """the four arguments of the conversion - run_ffmpeg_metrics' keywords or a config's keys, named alike - and the pre-passes
    named next to them -> (chroma, siting, range), or None when nothing is converted; a ValueError for a set that does not fit
    together"""
    from .engine import CONVERT_CHROMA, CONVERT_RANGE, CONVERT_SITING
    convert, dist_pixfmt = values.get("convert"), values.get("dist_pixfmt")
    siting, rng = values.get("convert_siting") or "center", values.get("convert_range") or "limited"
    if dist_pixfmt is not None and not (isinstance(dist_pixfmt, str) and dist_pixfmt in LAYOUTS):
        raise ValueError("dist_pixfmt must be null or one of the pixel layouts pixfmt takes.")
    if not (isinstance(siting, str) and siting in CONVERT_SITING):
        raise ValueError("convert_siting must be \"center\" or \"left\".")
    if not (isinstance(rng, str) and rng in CONVERT_RANGE):
        raise ValueError("convert_range must be \"limited\" or \"full\".")
    if convert is None:
        if dist_pixfmt is not None:
            raise ValueError("dist_pixfmt needs convert: nothing is converted without being named.")
        return None
    if not (isinstance(convert, str) and convert in CONVERT_CHROMA):
        raise ValueError("convert must be \"box\" or \"linear\".")
    for key, on in (("sync", values.get("sync")), ("align", values.get("align") is not None), ("shift", values.get("shift") is not None),
                    ("colorfit", values.get("colorfit")), ("conform", values.get("conform"))):
        if on:
            raise ValueError("%s and convert do not go together: the pair-reading pre-passes are not built on a pair of mixed pixel "
                             "layouts (Engine.convert's frames can be handed to them by the caller)." % key)
    return convert, siting, rng


def _check_convert_layouts(layout, dist_layout, converting=True, equal_ok=False):
    """the two layouts of a pair against the conversion asked for; a ValueError for a pair that does not fit it"""
    if not converting:
        if dist_layout != layout:
            raise ValueError("reference and distorted streams must share a pixel layout (%s and %s: name the conversion with "
                             "convert to measure them)" % (layout, dist_layout))
        return
    if dist_layout == layout and not equal_ok:
        raise ValueError("convert needs streams of different pixel layouts (both are %s): equal formats are measured as they are."
                         % layout)
    if "bgr24" in (layout, dist_layout):
        raise ValueError("convert between packed bgr24 and planar YUV is a colour-matrix question: not built.")
    if len(LAYOUTS[layout][1]) != len(LAYOUTS[dist_layout][1]):
        raise ValueError("convert needs as many planes on both sides (%s has %d, %s has %d): mono to or from three planes is not "
                         "built." % (layout, len(LAYOUTS[layout][1]), dist_layout, len(LAYOUTS[dist_layout][1])))


def _convert_planes(conv, scaling, scale, layout, dist_layout, planes, dh, dw, extra):
    """the distorted stream's own planes of a converting pass and the log's keys -> (dist_planes, extra): DIST_PIXFMT and CONVERT
    right after DIST_RES / SCALE where those exist"""
    from .engine import check_convert_planes, check_scale_planes
    dist_planes = LAYOUTS[dist_layout][0](dh, dw)
    mid = LAYOUTS[layout][0](dh, dw) if scaling else planes
    check_convert_planes(dist_planes, mid)
    if scaling:
        check_scale_planes(mid, planes)
    return dist_planes, dict(extra or {}, DIST_PIXFMT=dist_layout, CONVERT="/".join(conv))


# ---------------------------------------------------------------------------
# The pre-passes of the two entry points: one table, one request parser, one chain
# ---------------------------------------------------------------------------
# a pre-pass: its name, the top-level keys it adds to the log and the row, and its request parser - (values, config) -> what
# was asked, None / False when it is off; values: run_ffmpeg_metrics' keywords or a config, which name all but the light range
# alike.  The table's order is the order of the KEYS; the checks and the run have orders of their own (_requests, _prepass_chain)
Prepass = namedtuple("Prepass", "name keys request")
PREPASSES = (
    Prepass("light", LIGHT_KEYS, lambda v, config: _light_config(v) if config else
            _light_request(v["light"], v["light_transfer"], v["light_full_range"])),
    Prepass("sync", SYNC_KEYS, lambda v, config: _sync_config(v)),
    Prepass("colorfit", COLORFIT_KEYS, lambda v, config: _colorfit_config(v) if config else
            _colorfit_request(v["colorfit"], v["scale"])),
    Prepass("align", ALIGN_KEYS, lambda v, config: _align_request(v.get("align"), v.get("scale"))),
    Prepass("shift", SHIFT_KEYS, lambda v, config: _shift_request(v.get("shift"), v.get("shift_margin"), v.get("scale"))),
    Prepass("conform", CONFORM_KEYS, lambda v, config: _conform_config(v)),
)
# what was asked of a pass before it starts: whether the rung is scaled, align's radius, shift's (radius, margin), light's
# (transfer, full_range), sync's (min_overlap, apply), whether the colour fit is on, conform's colour mode
class Requests(namedtuple("Requests", "scaling radius search lit syn fit mode")):
    """the seven fields, and beside them `convert`: None or the (chroma, siting, range) of a converting pass - no pre-pass and no
    field, so that a request without it is the tuple it was - and `fields`: whether the field statistics of both streams are
    measured ahead of the chain"""
    convert = None
    fields = False


def _requests(values, config=False):
    """run_ffmpeg_metrics' keywords, or with config=True a config -> Requests.  The order of the checks, and so the first error
    of a bad combination: scale, align, shift, light, sync, colorfit, conform, convert, fields."""
    parse = {p.name: p.request for p in PREPASSES}
    req = Requests(_scale_request(values.get("scale"), values.get("dist_height"), values.get("dist_width")),
                   *(parse[name](values, config) for name in ("align", "shift", "light", "sync", "colorfit", "conform")))
    req.convert = _convert_request(values)
    req.fields = _fields_request(values)
    return req


def _prepass_keys(found, extra=None):
    """the log's further keys: extra (a scaled pass's DIST_RES and SCALE, or None) and then the keys the pre-passes found
    (name -> keys), in the table's order whatever order they ran in.  Nothing found: extra as it is."""
    if not found:
        return extra
    out = dict(extra or {})
    for p in PREPASSES:
        out.update(found.get(p.name, {}))
    return out


def _prepass_chain(req, ref, dist, also, layout, h, w, dist_hw, planes, sw, device, extra=None, same_shape=False):
    """The pre-passes of an entry point, in the order they run: sync and its trim, light over the reference, align, conform's
    constant offset by slicing the feeds, shift, the colour fit - over the trimmed pair, or with conform over the pair
    registered in time and place - and conform's plan.  ref, dist: the pair they read; also: further streams cut like dist;
    dist_hw: dist's own (height, width) under scale; planes: what the pass measures; sw: the switches, for the plane checks at the
    conformed size; extra: _prepass_keys'; same_shape: a pair of unequal shapes is an error once sync had its say.
    -> ([ref, dist] + also as they are left, the log's further keys, the plan or None, the planes to measure at, whether a
    pre-pass ran).  With everything off no stream is touched."""
    streams, found = [ref, dist] + list(also), {}
    trim = synced = aligned = moved = plan = None

    def cut(ref_lo, dist_lo, length):
        streams[0] = _frame_slice(_host_stream(streams[0], wide=True), ref_lo, length)
        streams[1:] = [_frame_slice(a, dist_lo, length) for a in streams[1:]]

    if req.syn is not None:   # before everything else: it may trim what everything else reads
        found["sync"], trim, synced = _sync_streams(req.syn, ref, dist, layout, h, w, dist_hw[0], dist_hw[1], device)
        if trim is not None:
            cut(*trim)
    if same_shape and not isinstance(streams[0], DeviceFrames) and streams[0].shape != streams[1].shape:
        raise ValueError("ref and dist must have the same shape")
    if req.lit is not None:
        found["light"] = light_extra(frame_light(streams[0], layout, h, w, req.lit[0], req.lit[1], device=device)[1])
    if req.radius is not None:
        aligned = frame_align(streams[0], streams[1], layout, h, w, req.radius, device=device)
        found["align"] = align_extra(aligned, req.radius)
    if req.mode is not None:   # conform, time: the constant offset by the feeds, before the shift is searched
        offset = _conform_offset(aligned, synced, trim is not None)
        streams[0] = _host_stream(streams[0], wide=True)
        length = max(0, min(_frame_count(streams[1]), _frame_count(streams[0]) - offset) - max(0, -offset))
        if length < 1:
            raise ValueError("the offset %d leaves no frame pair to conform" % offset)
        cut(max(0, offset), max(0, -offset), length)
    if req.search is not None:
        moved = frame_shift(streams[0], streams[1], layout, h, w, req.search[0], req.search[1], device=device)
        found["shift"] = shift_extra(moved, req.search[0])
    if req.mode is not None:   # conform, place and colour: the fit is taken over the pair registered so far
        place = tuple(moved["shift"]) if moved is not None else (0, 0)
        color = None
        if req.fit:
            color, fitted = _conform_color(req.mode, streams[0], streams[1], layout, h, w, place, device)
            found["colorfit"] = colorfit_extra(fitted, layout_depth(layout))
        plan = _conform_plan(layout, h, w, shift=place, offset=offset, color=color)
        found["conform"] = conform_extra(plan, _frame_count(streams[0]), aligned, moved)
        planes = plan["out_planes"]
        for f in FEATURES:
            if sw[f.kind] and f.plane_check is not None:
                f.plane_check(planes)
    elif req.fit:   # the colour-fit pre-pass over the (trimmed) pair
        found["colorfit"] = colorfit_extra(frame_colorfit(streams[0], streams[1], layout, h, w, device=device)[2],
                                           layout_depth(layout))
    return streams, _prepass_keys(found, extra), plan, planes, bool(found)


def _brisque_model(model_path, range_path):
    """the config's two paths -> a model or None; loaded before the pass starts, so a bad file costs no GPU time"""
    if model_path is None:
        if range_path is not None:
            raise ValueError("brisque_range_path needs a brisque_model_path")
        return None
    from . import brisque_model
    return brisque_model.load_model(model_path, range_path)


def _load_models(sw):
    """the model files the switches (features.switches) name -> (VMAF model or None, BRISQUE model or None); loaded before the pass
    starts, so a bad file costs no GPU time"""
    model = None
    if sw["vmaf_model_path"] is not None:
        from . import vmaf_model
        model = vmaf_model.load_model(sw["vmaf_model_path"])
    return model, _brisque_model(sw.get("brisque_model_path"), sw.get("brisque_range_path"))


def write_vif_log(vmaf_log, scale=None, adm=None, *, motion=None, model=None, siti=None, psnr_hvs=None, ciede=None, gmsd=None,
                  cambi=None, xpsnr=None, haarpsi=None, vca=None, artifacts=None, brisque=None, brisque_model=None, mdsi=None,
                  delta_itp=None, pu21=None, fsim=None, sigstats=None, sigstats_depth=8, extra=None):
    """libvmaf's JSON log, restricted to what is computed: frames[i].metrics.vif_scale0..3 and pooled_metrics.vif_scaleN
    .{min, max, mean, harmonic_mean} (libvmaf's harmonic mean: n / sum 1 / (x + 1) - 1).  No "vmaf" key without a model.
    scale: [n, 4], the first (luma) plane's values, or None when VIF was not measured.
    adm: None, or the first plane's ADM records [n] (engine.ADM_DTYPE): the log then also carries adm2 and adm_scale0..3, per
    frame and pooled in the same way.
    motion: None, or the first plane's motion records [n] (stream.MOTION_PASS_DTYPE): the log then also carries motion2 and
    motion, likewise.
    siti: None, or the first plane's SI/TI records [n] (engine.SITI_DTYPE): the log then also carries si and ti, after the motion
    keys and before vmaf, likewise (P.910's clip values are the pooled maxima).  The model never reads them.
    psnr_hvs: None, or the first plane's PSNR-HVS records [n] (engine.PSNR_HVS_DTYPE): the log then also carries psnr_hvs and
    psnr_hvsm in dB, after ti and before vmaf, likewise.  JSON has no infinity: the log writes min(value, 100.0) dB
    (PSNR_HVS_DB_CAP), so identical frames read 100.0.  The model never reads them.
    ciede: None, or the CIEDE2000 records [n] (engine.CIEDE_DTYPE, one per frame): the log then also carries ciede2000, after
    psnr_hvsm and before vmaf, likewise capped at 100.0.  The model never reads it.
    gmsd: None, or the first plane's GMSD records [n] (engine.GMSD_DTYPE): the log then also carries gmsd, after ciede2000 and
    before vmaf, likewise.  The model never reads it.
    cambi: None, or the first plane's CAMBI records [n] (engine.CAMBI_DTYPE) of the encoded stream: the log then also carries
    cambi, after gmsd and before vmaf, likewise.  The model never reads it.
    xpsnr: None, or the first plane's XPSNR records [n] (engine.XPSNR_DTYPE): the log then also carries xpsnr in dB, after cambi
    and before vmaf, likewise capped at 100.0.  The model never reads it.
    haarpsi: None, or the first plane's HaarPSI records [n] (engine.HAARPSI_DTYPE): the log then also carries haarpsi, after
    xpsnr and before vmaf, likewise.  The model never reads it.
    vca: None, or the first plane's VCA records [n] (engine.VCA_DTYPE) of the reference stream: the log then also carries vca_e,
    vca_h and vca_l, after haarpsi and before vmaf, likewise (frame 0's vca_h = 0 is part of the pooled values).  The model never
    reads them.
    artifacts: None, or the first plane's blockiness / blur / noise records [n] (engine.ARTIFACTS_DTYPE) of the encoded stream:
    the log then also carries blockiness, blur and noise, after vca_l and before vmaf, likewise.  The model never reads them.
    brisque: None, or the first plane's BRISQUE records [n] (engine.BRISQUE_DTYPE) of the encoded stream: the log then also
    carries brisque_00 .. brisque_35, after noise and before vmaf, likewise; with brisque_model (brisque_model.load_model) also
    "brisque" = the model's score over them, after brisque_35.  The VMAF model never reads them.
    mdsi: None, or the MDSI records [n] (engine.MDSI_DTYPE, one per frame): the log then also carries mdsi, after the BRISQUE
    keys and before vmaf, likewise.  The model never reads it.
    delta_itp: None, or the dE_ITP records [n] (engine.ITP_DTYPE, one per frame): the log then also carries delta_itp (the
    frame's mean) and delta_itp_max (its largest pixel), after mdsi and before vmaf, likewise.  The model never reads them.
    pu21: None, or the PU21 records [n] (engine.PU21_DTYPE, one per frame): the log then also carries pu_psnr, pu_psnr_rgb (each
    capped at 100.0: identical frames give inf, which JSON cannot hold and a mean cannot pool) and pu_ssim, after delta_itp_max
    and before vmaf, likewise.  The model never reads them.
    fsim: None, or the FSIM records [n] (engine.FSIM_DTYPE, one per frame): the log then also carries fsim and fsimc, after pu_ssim
    and before vmaf, likewise.  The model never reads them.
    sigstats: None, or the first plane's signal statistics [n] (engine.SIGSTATS_DTYPE) of the reference stream, whose samples have
    sigstats_depth bits: the log then also carries y_min, y_low, y_avg, y_high, y_max, y_dif, out_of_range ((under + over_luma) /
    N), black, frozen (0 or 1) and scene_score (events.signal_events at its defaults), after fsimc and before vmaf, likewise, and
    next to "frames" and "pooled_metrics" an object "signal": black_frames, frozen_frames, scene_cuts (counts) and crop ([top,
    bottom, left, right] over the frames that are not black, null when all are).  The model never reads them.
    extra: None, or a dict of further top-level keys, written last (a scaled pass: "DIST_RES" and "SCALE").
    model: None, or a vmaf_model.VmafModel: every frame then also carries "vmaf" = vmaf_model.predict over the frame's logged
    features (a feature the model names and the log lacks is a ValueError), pooled like the features."""
    import json
    given = dict(locals(), vif=scale)
    names, cols, top = [], [], {}
    for f in FEATURES:
        if given[f.flag] is not None:
            keys, columns, more = f.to_log(f, given[f.flag], given)
            names, cols = names + keys, cols + columns
            top.update(more)
    if model is not None:
        from . import vmaf_model
        score = vmaf_model.predict(model, vmaf_model.feature_matrix(model, dict(zip(names, cols))))
        names += ["vmaf"]
        cols += [score]
    scale = np.stack(cols, axis=1) if cols else np.zeros((0, 0))
    frames = [{"frameNum": i, "metrics": {k: float(v) for k, v in zip(names, row)}} for i, row in enumerate(scale)]
    pooled = {}
    for s, k in enumerate(names):
        x = scale[:, s]
        if len(x):
            pooled[k] = {"min": float(x.min()), "max": float(x.max()), "mean": float(x.mean()),
                         "harmonic_mean": float(len(x) / np.sum(1.0 / (x + 1.0)) - 1.0)}
    with open(vmaf_log, "w") as f:
        doc = {"frames": frames, "pooled_metrics": pooled}
        doc.update(top)
        if extra:
            doc.update(extra)
        json.dump(doc, f, indent=1)
        f.write("\n")


# ---------------------------------------------------------------------------
# FFmpeg-format stats lines, a chunk of frames at a time
# ---------------------------------------------------------------------------
def _db(x):
    """10 log10(x) with inf for x = inf (FFmpeg prints "inf")"""
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(x)


def _psnr(mse, peak=255.0):
    """FFmpeg vf_psnr.c get_psnr(): 10*log10(max^2 / mse); mse == 0 -> inf (the expression the stats lines use)"""
    with np.errstate(divide="ignore"):
        return float(_db(np.float64(peak * peak) / np.float64(mse)))


def psnr_stats_lines(n0, sse, sizes, comps, peak=255):
    """Lines n0.. of FFmpeg's psnr stats_file (vf_psnr.c) for sse [m,p]: per-component mse = sse/(w*h); mse_avg
    weights components by plane area; psnr = 10 log10(peak^2 / mse) (get_psnr(); mse 0 -> inf); 2-decimal text.
    peak: vf_psnr's max, (1 << depth) - 1 of the pixel format (255 for 8 bits, 1023 for 10)."""
    pk = float(peak)
    sse = np.asarray(sse, np.float64).reshape(-1, len(sizes))
    areas = [w * h for w, h in sizes]
    total = float(sum(areas))
    mse = sse / np.asarray(areas, np.float64)
    mse_avg = np.zeros(len(sse))
    for j, a in enumerate(areas):
        mse_avg = mse_avg + mse[:, j] * (a / total)
    with np.errstate(divide="ignore"):
        cols = [np.arange(n0, n0 + len(sse), dtype=np.float64), mse_avg] + [mse[:, j] for j in range(len(areas))]
        cols += [_db(pk * pk / mse_avg)] + [_db(pk * pk / mse[:, j]) for j in range(len(areas))]
    fmt = ("n:%d mse_avg:%0.2f " + "".join("mse_%c:%%0.2f " % c for c in comps) + "psnr_avg:%0.2f "
           + "".join("psnr_%c:%%0.2f " % c for c in comps) + "\n")
    return (fmt * len(sse)) % tuple(np.column_stack(cols).ravel().tolist())


def ssim_stats_lines(n0, ssim, sizes, comps):
    """Lines n0.. of FFmpeg's ssim stats_file (vf_ssim.c): 'n:1 Y:0.99 U:.. V:.. All:0.99 (20.0)'."""
    ssim = np.asarray(ssim, np.float64).reshape(-1, len(sizes))
    areas = [w * h for w, h in sizes]
    total = float(sum(areas))
    allv = np.zeros(len(ssim))
    for j, a in enumerate(areas):
        allv = allv + ssim[:, j] * (a / total)
    with np.errstate(divide="ignore", invalid="ignore"):
        db = np.where(allv < 1.0, _db(1.0 / (1.0 - allv)), np.inf)
    cols = [np.arange(n0, n0 + len(ssim), dtype=np.float64)] + [ssim[:, j] for j in range(len(areas))] + [allv, db]
    fmt = "n:%d " + "".join("%c:%%f " % c.upper() for c in comps) + "All:%f (%f)\n"
    return (fmt * len(ssim)) % tuple(np.column_stack(cols).ravel().tolist())


def psnr_stats_line(n, sse_row, sizes, comps, peak=255):
    return psnr_stats_lines(n, [list(sse_row)], sizes, comps, peak)


def ssim_stats_line(n, ssim_row, sizes, comps):
    return ssim_stats_lines(n, [list(ssim_row)], sizes, comps)


class _StatsWriter:
    """Writes the two stats files chunk by chunk (stream.run's on_quality), in FFmpeg's component order."""

    def __init__(self, psnr_log, ssim_log, layout, sizes):
        comps = LAYOUTS[layout][1]
        # FFmpeg lists rgb components in r,g,b order whatever the packing
        self.order = [2, 1, 0] if layout == "bgr24" else list(range(len(comps)))
        self.names = "rgb" if layout == "bgr24" else comps
        self.sizes = [sizes[j] for j in self.order]
        self.peak = (1 << layout_depth(layout)) - 1   # vf_psnr.c: max of the pixel format
        self.fp, self.fs = open(psnr_log, "w"), open(ssim_log, "w")

    def resize(self, sizes):
        """the planes' sizes changed before the first line was written (a conformed pass measures the common window)"""
        self.sizes = [sizes[j] for j in self.order]

    def __call__(self, first_frame, sse, ssim):
        self.fp.write(psnr_stats_lines(first_frame + 1, sse[:, self.order], self.sizes, self.names, self.peak))
        self.fs.write(ssim_stats_lines(first_frame + 1, ssim[:, self.order], self.sizes, self.names))

    def close(self):
        self.fp.close()
        self.fs.close()


def _open_quality_stream(src, layout, height, width):
    """-> (frames, layout, height, width).  .y4m paths select their layout by themselves (the header's C tag: yuv420p,
    yuv422p10le ...); headerless .yuv (planar: `layout` when it names a planar pix_fmt, else yuv420p) and .bgr / .bgr24
    (packed) files take their geometry from height / width."""
    if isinstance(src, str) and src.endswith(".y4m"):
        from .frames import open_y4m, y4m_pixfmt
        arr, h, w, _fps = open_y4m(src)     # a memory map: the pass pages in what it gathers, nothing is read up front
        return arr, y4m_pixfmt(src), h, w
    if isinstance(src, str) and src.endswith(".yuv"):
        fmt = layout if layout in PIXFMTS else "yuv420p"
        if not height or not width:
            raise ValueError("a raw %s stream needs height and width" % fmt)
        from .frames import read_raw_yuv
        return read_raw_yuv(src, height, width, fmt), fmt, height, width
    if layout == "bgr24":
        return _open_frames(src, height, width), layout, height, width
    if isinstance(src, str):
        raise ValueError("Unsupported file type. Please provide a .y4m / .yuv (yuv420p) or .npy / .bgr24 ([N,H,W,3] BGR) stream.")
    return src, layout, height, width


def run_ffmpeg_metrics(reference_video, distorted_video, psnr_log, ssim_log, vmaf_log, vmaf_model_path=None,
                       layout="bgr24", ssim_mode="gauss", height=None, width=None, batch_size=64, device=None, vif=False,
                       adm=False, motion=False, siti=False, psnr_hvs=False, ciede=False, ciede_weights=N.CIEDE_WEIGHTS_CIE,
                       gmsd=False, cambi=False, xpsnr=False, haarpsi=False, vca=False, artifacts=False, brisque=False,
                       brisque_model_path=None, brisque_range_path=None, mdsi=False, delta_itp=False,
                       delta_itp_transfer="pq", delta_itp_full_range=False, pu21=False, pu21_transfer="pq",
                       pu21_full_range=False, fsim=False, sigstats=False, sigstats_black=None, sigstats_crop=None,
                       dist_height=None, dist_width=None, scale=None, align=None, shift=None,
                       shift_margin=None, light=False, light_transfer="pq", light_full_range=False, sync=False,
                       sync_min_overlap=None, sync_apply=False, colorfit=False, conform=False, conform_color="match",
                       dist_pixfmt=None, convert=None, convert_siting="center", convert_range="limited", fields=False):
    """video_processing.py:270-297 — PSNR and SSIM between two streams, one stats line per frame.
    Streams: [N,H,W,3] BGR arrays / .npy (components r,g,b as FFmpeg labels RGB input), planar yuv420p
    arrays with height/width, or .y4m files (components y,u,v — what FFmpeg sees for an H.264 clip).
    vif=True: the same pass (one upload per chunk) also measures VIF on four scales and writes vmaf_log in libvmaf's JSON
    shape (write_vif_log: the first plane's vif_scale0..3 per frame and pooled; no vmaf value).  Without it vmaf_log is not
    written, as before.
    adm=True: likewise ADM on four scales (adm2 and adm_scale0..3 of the first plane, per frame and pooled, in the same log).
    motion=True: likewise VMAF's motion feature of the reference stream (motion2 and motion of the first plane).
    siti=True: likewise ITU-T P.910's spatial and temporal information of the reference stream (si and ti of the first plane; a
    model file does not turn it on).
    psnr_hvs=True: likewise PSNR-HVS and PSNR-HVS-M (psnr_hvs and psnr_hvsm of the first plane in dB, capped at 100.0 - JSON has
    no infinity; a model file does not turn it on).
    ciede=True: likewise CIEDE2000 of the three planes together (ciede2000 = 45 - 20 log10 of the frame's mean dE00, capped at
    100.0; three-plane layouts only; ciede_weights = (kL, kC, kH), default (1, 1, 1); a model file does not turn it on).
    gmsd=True: likewise GMSD (gmsd of the first plane; a model file does not turn it on).
    cambi=True: likewise CAMBI, the banding index of the ENCODED stream alone (cambi of the first plane; a model file does not
    turn it on).
    xpsnr=True: likewise XPSNR, the activity-weighted PSNR with block weights (xpsnr of the first plane in dB, capped at 100.0;
    planar layouts only - bgr24 is a ValueError; a model file does not turn it on).
    haarpsi=True: likewise HaarPSI, the Haar wavelet perceptual similarity (haarpsi of the first plane; a model file does not
    turn it on).
    vca=True: likewise VCA's texture features of the REFERENCE stream (vca_e, vca_h, vca_l of the first plane; planar layouts
    only - bgr24 is a ValueError; a model file does not turn it on).
    artifacts=True: likewise the no-reference blockiness, blur and noise of the ENCODED stream alone (blockiness, blur, noise of
    the first plane; a model file does not turn it on).
    brisque=True: likewise BRISQUE's 36 natural-scene statistics of the ENCODED stream alone (brisque_00 .. brisque_35 of the
    first plane; a VMAF model file does not turn it on).  brisque_model_path (libsvm's text model) and brisque_range_path
    (svm-scale's range file) turn it on and add "brisque", the score (brisque_model.py; loaded BEFORE the pass starts).
    mdsi=True: likewise MDSI, the mean deviation similarity index of the planes taken together (mdsi, one value per frame; one-
    or three-plane layouts; neither a VMAF nor a BRISQUE model file turns it on).
    delta_itp=True: likewise dE_ITP of ITU-R BT.2124, the three planes together read as a BT.2020 signal (delta_itp, the frame's
    mean, and delta_itp_max, its largest pixel; three-plane layouts only; delta_itp_transfer "pq" | "hlg", delta_itp_full_range
    False (limited) | True; a model file does not turn it on).
    pu21=True: likewise PU21-PSNR and PU21-SSIM, the three planes together read as a BT.2020 signal, as display light in PU21 units
    (pu_psnr and pu_psnr_rgb, capped at 100.0, and pu_ssim; three-plane layouts only; pu21_transfer "pq" | "hlg", pu21_full_range
    False (limited) | True; a model file does not turn it on).
    fsim=True: likewise FSIM and FSIMc of the planes taken together (fsim and fsimc, one value each per frame; one- and three-plane
    layouts; a model file does not turn it on).
    sigstats=True: likewise the signal statistics of the REFERENCE stream - the source SI/TI and VCA describe too - from the same
    upload (y_min .. scene_score of the first plane and the "signal" object, write_vif_log; sigstats_black, sigstats_crop: None or
    the black and the dark-border level in sample units; a model file does not turn it on).
    scale="bilinear" | "bicubic" | "lanczos": the distorted stream is a ladder rung of its OWN size, dist_height x dist_width (a
    .y4m file brings its size in its header, [N,H,W,3] arrays in their shape; the same layout and depth as the reference).
    Every chunk is uploaded at that size and resampled to the reference's on the GPU (stream.Quality's dist_planes / scale:
    what `[dist]scale=W:H:flags=bicubic` does before the filters in an FFmpeg graph, in Pillow's arithmetic), so EVERYTHING the
    pass says about the distorted stream - cambi, artifacts and brisque included - is said at the reference's geometry
    (frame_cambi and the other frame_* calls on the rung itself give the native figure).  vmaf_log, when written, gains the
    top-level keys "DIST_RES" ("1280x720") and "SCALE".  Without scale, streams of different sizes stay the error they were,
    dist_height / dist_width alone are a ValueError, and every file is byte for byte what it was.
    align=R (an integer radius 1 .. 32; default None): before the pass starts, a pass of its own (frame_align) measures whether
    the distorted stream holds the reference's frames in the reference's places - its answer is about how the frames are PAIRED,
    which is what the pass takes on trust.  vmaf_log is then written in any case and gains the top-level keys "ALIGN_RADIUS",
    "ALIGN_OFFSET", "ALIGN_DROPPED", "ALIGN_REPEATED" and "ALIGN_PSNR_GAIN" (align.analyse); a non-zero offset, drop or repeat is
    also logged as a warning.  The frames are NOT re-paired: nothing is changed silently.  align with scale is a ValueError.
    Without align every file is byte for byte what it was.
    shift=R (an integer radius 1 .. 16; default None) with shift_margin (default None: R): before the pass starts, a pass of its
    own (frame_shift) measures whether the distorted picture sits where the reference picture sits - the squared error of plane
    0 at every integer shift of -R .. R over the core shift_margin samples inside the plane.  vmaf_log is then written in any
    case and gains the top-level keys "SHIFT_RADIUS", "SHIFT_DY", "SHIFT_DX", "SHIFT_FRAMES_OFF" and "SHIFT_PSNR_GAIN"
    (shift.analyse), after the ALIGN_* keys when both are on; a non-zero shift, or a best shift on the band's border, is also
    logged as a warning.  The frames are NOT moved: nothing is changed silently.  shift with scale is a ValueError.  Without
    shift every file is byte for byte what it was.
    light=True (default False) with light_transfer ("pq"; "hlg" is a ValueError that says why) and light_full_range (False:
    limited): before the pass starts, a pass of its own over the REFERENCE stream (frame_light) measures the HDR10 light levels
    and the gamut - CTA-861.3's MaxCLL and MaxFALL as include/vqa.h states them, not compared with any tool.  vmaf_log is then
    written in any case and gains the top-level keys "LIGHT_MAXCLL", "LIGHT_MAXFALL", "LIGHT_MAXCLL_FRAME", "LIGHT_P9998",
    "LIGHT_Y_AVG", "LIGHT_OUT_709", "LIGHT_OUT_P3" and "LIGHT_CLAMPED" (light.summarise), BEFORE the ALIGN_* and SHIFT_* keys.  A
    one-plane layout is a ValueError.  Without light every file is byte for byte what it was.
    sync=True (default False) with sync_min_overlap (default None: half the shorter clip) and sync_apply (default False): before
    every other pre-pass, a pass of its own (frame_sync) finds where in the reference the distorted stream belongs, anywhere in
    the clip and for streams of unequal length - or, under scale, of unequal size.  vmaf_log is then written in any case and
    gains the top-level keys "SYNC_OFFSET", "SYNC_OVERLAP", "SYNC_DISTANCE", "SYNC_RUNNER_UP", "SYNC_FRAMES_OFF" and
    "SYNC_APPLIED" (sync.analyse), after the LIGHT_* and before the ALIGN_* / SHIFT_* keys.  With sync_apply and an answer that
    is not ambiguous, both streams are sliced to the found overlap BEFORE the equal-shape check, every later pre-pass and the
    pass, which is logged as a warning; SYNC_APPLIED is 1 only when something was cut.  An ambiguous answer (a static clip) is
    never applied: a warning, SYNC_APPLIED 0, and the streams go on as given.  sync_apply without sync is a ValueError.
    Without sync every file is byte for byte what it was.
    colorfit=True (default False): after the sync pre-pass - so with sync_apply over the trimmed pair - a pass of its own
    (frame_colorfit) measures whether a code value means the same in both streams: the joint integer moments of the planes and
    the per-code transfer tables, from which colorfit.analyse reads the per-plane gain and offset, the best 3 x 3 matrix, the tone
    curve and whether a known mishap (limited / full range, BT.601 / BT.709 matrix) explains the error.  vmaf_log is then written
    in any case and gains the top-level keys "COLORFIT_MATCH", "COLORFIT_MATCH_PSNR_GAIN", "COLORFIT_PSNR_GAIN",
    "COLORFIT_GAIN_Y", "COLORFIT_OFFSET_Y" (on the 8-bit scale), "COLORFIT_TONE_PSNR_GAIN" (plane 0) and "COLORFIT_FRAMES_OFF",
    after the SYNC_* and before the ALIGN_* / SHIFT_* keys; gains are capped at 100.0.  A named mishap, or a matrix fit worth
    10 log10(2) dB or more, is also logged as a warning.  The frames are NOT corrected.  colorfit with scale, and a two-plane
    layout, are a ValueError.  Without colorfit every file is byte for byte what it was.
    conform=True (default False) with conform_color ("none" | "match" (default) | "levels" | "matrix" | "tone"): what the
    pre-passes FOUND is applied on the GPU before anything is measured (conform.py, Engine.conform_submit), in this order: align's
    constant offset - after sync's trim with sync_apply; sync's own offset where align is off and nothing was trimmed - by
    slicing both streams right after the alignment pre-pass, so the shift search already sees the re-paired frames; the clip's
    shift (dy, dx), as the common window of both pictures; the colour mode, on the distorted stream.  The colour-fit pre-pass then
    runs over the pair ALREADY registered in time and place, with the roles swapped for "levels", "matrix" and "tone" (its
    least-squares map is then the correction itself): the COLORFIT_* keys of such a run describe the registered pair.  "match"
    applies the inverse of the named mishap and nothing when COLORFIT_MATCH is "none"; an ambiguous sync applies no offset.  Every
    chunk of both streams is uploaded as given and conformed on the engine that measures it (stream.Quality's conform), so the
    psnr / ssim stats lines and every feature are those of the conformed pair, at the conformed size.  vmaf_log gains, as its
    LAST top-level keys, "CONFORM_OFFSET", "CONFORM_DY", "CONFORM_DX", "CONFORM_COLOR" ("none", "match:<mishap>", "levels",
    "matrix", "tone"), "CONFORM_RES" ("1918x1078"), "CONFORM_FRAMES" and "CONFORM_CHROMA_HALF" (1: an odd shift on a subsampled
    axis left the chroma planes half a chroma sample apart; nothing is interpolated).  A non-zero ALIGN_DROPPED / ALIGN_REPEATED
    (only the constant offset is applied in the pass), a shift on the band's border and CONFORM_CHROMA_HALF are warnings.
    conform needs at least one of sync, align, shift and colorfit, a colour mode other than "none" needs colorfit, "tone" needs a
    depth of at most 10 bits, and conform with scale is a ValueError.  Without conform every file is byte for byte what it was.
    convert="box" | "linear": the distorted stream has its OWN pixel layout - another sample depth and / or chroma layout than
    the reference, a 10-bit 4:2:2 mezzanine against its 8-bit 4:2:0 encode.  A .y4m pair brings its two layouts in its headers;
    arrays and raw .yuv take the distorted one from dist_pixfmt (layout names the reference's).  Every chunk is uploaded as it is
    and converted to the reference's layout on the GPU (stream.Quality's convert; include/vqa.h's integer definition: what an
    auto-inserted `format=` does in an FFmpeg graph, NOT swscale's arithmetic), convert_siting "center" | "left" and
    convert_range "limited" | "full" with it.  With scale the conversion runs first, at the rung's size.  vmaf_log gains the
    top-level keys "DIST_PIXFMT" and "CONVERT" ("linear/center/limited"), right after DIST_RES / SCALE where those exist.
    Layouts that differ without convert stay the error they were; dist_pixfmt without convert, convert on equal layouts, on a
    differing plane count or packed bgr24, and convert with sync, align, shift, colorfit or conform are ValueErrors (light reads
    the reference only and stays allowed).  Without the keywords every file is byte for byte what it was.
    fields=True: before every pre-pass frame_fields reads both streams as given - the reference at its layout, the distorted
    stream at its own size and layout, so it goes with scale and with convert - and vmaf_log, written in any case, gains nine
    top-level keys before every pre-pass key: FIELDS_REF_TYPE, FIELDS_REF_COMBED (frames classed tff or bff), FIELDS_REF_CADENCE,
    FIELDS_REF_REPEATS, the same four as FIELDS_DIST_*, and FIELDS_MATCH (1 when type, cadence and phase agree).  A distorted
    stream that is not progressive, or FIELDS_MATCH 0, is also a logged warning.  The frames are NOT changed: applying a plan
    (fields.ivtc_plan) is the caller's Engine.weave.  idet's rule as recalled, not pinned against FFmpeg.
    vmaf_model_path: a libvmaf JSON model or a bare libsvm model (vmaf_model.load_model; loaded BEFORE the pass starts, so a bad
    file costs no GPU time).  It turns vif, adm and motion on; the log then also carries frames[i].metrics.vmaf and
    pooled_metrics.vmaf.{min, max, mean, harmonic_mean}, which extract_metrics_from_logs reads as the reference does."""
    given = dict(locals())
    sw = switches(given)
    models = _load_models(sw)
    req = _requests(given)
    scaling = req.scaling
    ref, layout, height, width = _open_quality_stream(reference_video, layout, height, width)
    # (a scaled pass never borrows the reference's size for the rung: a .y4m header, the array's shape or the two arguments say it)
    dist, layout_d, dist_h, dist_w = _open_quality_stream(distorted_video, (dist_pixfmt or layout) if req.convert else layout,
                                                          dist_height or (None if scaling else height),
                                                          dist_width or (None if scaling else width))
    _check_convert_layouts(layout, layout_d, req.convert is not None)
    h, w = _geometry(ref, layout, height, width)
    planes = LAYOUTS[layout][0](h, w)
    _colorfit_request(req.fit, scale, layout)
    _conform_tone_depth(req.mode, layout)
    dist_planes = extra = None
    dh, dw = h, w
    if scaling:
        from .engine import check_scale_planes
        dh, dw = _geometry(_host_stream(dist, wide=True), layout_d, dist_h, dist_w)
        if not dh or not dw:
            raise ValueError("scale needs the distorted stream's size: dist_height and dist_width")
        dist_planes = LAYOUTS[layout][0](dh, dw)
        if not req.convert:
            check_scale_planes(dist_planes, planes)
        extra = {"DIST_RES": "%dx%d" % (dw, dh), "SCALE": scale}
    if req.convert:
        dist_planes, extra = _convert_planes(req.convert, scaling, scale, layout, layout_d, planes, dh, dw, extra)
    wr = _StatsWriter(psnr_log, ssim_log, layout, _sizes(planes))
    try:
        for f in FEATURES:
            if sw[f.kind]:
                _check_request(f, layout, given)
                if f.plane_check is not None:
                    f.plane_check(planes)
        extra = _fields_keys(req.fields, ref, layout, h, w, dist, layout_d, dh, dw, extra, device)
        (rs, ds), extra, plan, planes, ran = _prepass_chain(
            req, _host_stream(ref, wide=True), _host_stream(dist, wide=True), (), layout, h, w, (dh, dw), planes, sw, device,
            extra=extra, same_shape=not scaling and not req.convert)
        if plan is not None:
            wr.resize(_sizes(planes))
        _measure(ds, rs, sw, models, planes, _SSIM_MODES[ssim_mode], layout, dist_planes, scale, extra, vmaf_log,
                 ran=ran or req.fields, batch_size=batch_size, on_quality=wr, device=device, conform=plan, convert=req.convert)
    finally:
        wr.close()
    return None


_csv_lock = threading.Lock()


def thread_safe_update_csv(metrics, csv_file="video_quality_data.csv"):
    """video_processing.py:44-68 — append one row, header only when the file is new (no pandas needed).  The "is the file
    new" test sits INSIDE the lock (the reference tests at :56 before taking it at :62, so two threads can both write a header)."""
    import csv
    with _csv_lock:
        exists = os.path.isfile(csv_file) and os.path.getsize(csv_file) > 0
        with open(csv_file, "a", newline="") as f:
            wr = csv.writer(f)
            if not exists:
                wr.writerow(list(metrics.keys()))
            wr.writerow(list(metrics.values()))


# the keys this build adds to the reference's config.json (config.json:1-7 keeps its five; SURVEY.md section 5 "Config / flag system")
MODE_KEYS = {
    # key: (allowed values, message in the reference's validate_config style)
    # (the message names the modes of ABI 7; "msssim", multi-scale SSIM over the Gaussian window, is accepted as well)
    "ssim_mode": (("gauss", "ffmpeg", "msssim"), "ssim_mode must be 'gauss' or 'ffmpeg'."),
    # (the message names the layouts of ABI 7; the planar pix_fmts of frames.PIXFMTS - yuv422p, yuv420p10le ... - are
    # accepted as well)
    "pixfmt": ((None, "bgr24") + tuple(PIXFMTS), "pixfmt must be 'bgr24', 'yuv420p' or 'gray'."),
    "dct_mode": ((None, "auto", "block8", "full"), "dct_mode must be 'auto', 'block8' or 'full'."),
    "motion": ((None, "sad", "farneback"), "motion must be 'sad' or 'farneback'."),
}


def _write_feature_log(vmaf_log, q, on, *, model=None, brisque_model=None, sigstats_depth=8, extra=None):
    """a pass's records (stream.run's quality tuple, whose elements stream.records_by_kind names) -> vmaf_log: the first plane's of
    the per-plane kinds, the frame's of the per-frame ones.  on: flag (FEATURES) -> switch, the flags that are off may be missing.
    model: the VMAF model, which scores a pass that measured motion (with it, its other features)."""
    on = {f.kind: bool(on.get(f.flag)) for f in FEATURES}
    rec = stream.records_by_kind(q, on)
    log = {f.flag: rec[f.kind] if KINDS[f.kind].per_frame else rec[f.kind][:, 0] for f in FEATURES if on[f.kind]}
    write_vif_log(vmaf_log, log.pop("vif", None), model=model if on["motion"] else None, brisque_model=brisque_model,
                  sigstats_depth=sigstats_depth, extra=extra, **log)


def _measure(dist, ref, sw, models, planes, ssim_mode, layout, dist_planes, scale, extra, vmaf_log, conform=None, ran=False,
             convert=None, **run):
    """One pass (stream.run with its further arguments `run`) whose Quality the switches sw (features.switches) spell, and the feature
    log of what it measured, when a kind is on.  models: _load_models(sw).  conform: None or the plan the pass applies (planes
    are then its out_planes).  ran: a pre-pass ran (_prepass_chain).  convert: None or the (chroma, siting, range) of a converting
    pass.  -> stream.run's pair"""
    quality = stream.Quality(planes, ssim_mode, dist_planes=dist_planes, scale=scale, conform=conform, convert=convert,
                             **{k: v for k, v in sw.items() if k not in MODEL_PATHS})
    q, series = stream.run(dist, ref, quality=quality, **run)
    on = {f.flag: sw[f.kind] for f in FEATURES}
    if any(on.values()) or ran:   # (a pre-pass always has something to say; DIST_RES and SCALE alone do not ask for a log)
        _write_feature_log(vmaf_log, q, on, model=models[0], brisque_model=models[1], sigstats_depth=layout_depth(layout),
                           extra=extra)
    return q, series


def _check_mode_keys(config):
    for key, (allowed, message) in MODE_KEYS.items():
        if key in config and config[key] not in allowed:
            raise ValueError(message)
    dev = config.get("device")
    if dev is not None and (isinstance(dev, bool) or not isinstance(dev, int) or dev < 0):
        raise ValueError("device must be a non-negative integer.")
    for f in FEATURES:   # every kind's switch, then its parameters (validated whether the kind is on or not)
        check_switch(f.config_key, config)
        for p in f.params:
            p.check(p.config, config)
    mp = config.get("vmaf_model_path")
    if mp is not None and not (isinstance(mp, str) and os.path.isfile(mp) and os.access(mp, os.R_OK)):
        raise ValueError("vmaf_model_path must be null or the path of a readable model file.")
    bs = config.get("batch_size", 100)
    if isinstance(bs, bool) or not isinstance(bs, int) or bs <= 0:
        raise ValueError("batch_size must be a positive integer.")
    for key in ("height", "width"):   # the geometry of headerless inputs (.yuv, .bgr24)
        v = config.get(key)
        if v is not None and (isinstance(v, bool) or not isinstance(v, int) or v <= 0):
            raise ValueError("height and width must be positive integers.")
    _requests(config, config=True)


def process_video_and_extract_metrics(input_video, encoded_video, config, csv_file="video_quality_data.csv",
                                      bitrate=0, frame_rate=30.0, column_order="reference", encoded_bgr=None,
                                      height=None, width=None):
    """video_processing.py:180-267 minus the libx264 encode and ffprobe steps (external codec, out of
    scope): both streams arrive decoded.  Quality metrics compare input vs encoded (:216); complexity is
    computed on the ENCODED stream (:242-247).  ONE pass (stream.run) serves both.

    input_video / encoded_video   the pair the quality filters compare:
        [N,H,W,3] BGR frames (.npy, array, torch tensor, DeviceFrames) - the complexity kernels then read the same
            encoded frames, every chunk is uploaded once; or
        the decoded planes FFmpeg's psnr / ssim filters see (:274-276): .y4m files or planar [N, H*W*3/2] yuv420p
            arrays (config pixfmt "yuv420p") - together with
    encoded_bgr                   the encoded stream as cv2.VideoCapture decodes it ([N,H,W,3] BGR: .npy, array, tensor,
        DeviceFrames; complexity_metrics.py:100), which the complexity half reads.  Per chunk the planar pair and the chunk's
        selected BGR frames are uploaded, each byte once.
    config   the reference's keys (crf, resize_width, resize_height, frame_interval, vmaf_model_path; config.json:1-7) plus
        batch_size, ssim_mode ("gauss" north_star's 11x11 Gaussian, default | "ffmpeg" vf_ssim's 8x8 integer windows |
        "msssim" multi-scale SSIM over the Gaussian window: the ssim stats lines and the SSIM column then carry MS-SSIM),
        vif (true: the row gains VIF_scale0..3, the pooled means of the first plane's VIF on four scales; default false),
        adm (true: the row gains ADM2 and ADM_scale0..3, the pooled means of the first plane's ADM; default false),
        motion_feature (true: the row gains MOTION2 and MOTION, the pooled means of the first plane's VMAF motion feature of the
        INPUT stream; default false; the reference's vmaf_model_path, when not null, names a libvmaf model file: it turns vif, adm
        and motion_feature on and the row gains VMAF, the pooled mean of the per-frame scores, right after SSIM),
        siti (true: the row gains SI and TI, ITU-T P.910's spatial and temporal information of the INPUT stream's first plane -
        the pooled MAXIMA over the frames -, after MOTION; default false; a model file does not turn it on),
        psnr_hvs (true: the row gains PSNR_HVS and PSNR_HVSM, the pooled means of the first plane's per-frame PSNR-HVS and
        PSNR-HVS-M in dB, each frame's value capped at 100.0 - JSON and the row have no infinity -, after TI; default false; a
        model file does not turn it on),
        ciede (true: the row gains CIEDE2000, the pooled mean of the per-frame 45 - 20 log10(mean dE00) of the three planes taken
        together, each frame's value capped at 100.0, after PSNR_HVSM; three-plane pixfmts only; default false; a model file does
        not turn it on), ciede_weights ([kL, kC, kH], default [1, 1, 1], the CIE standard),
        gmsd (true: the row gains GMSD, the pooled mean of the first plane's per-frame gradient magnitude similarity deviation,
        after CIEDE2000; default false; a model file does not turn it on),
        cambi (true: the row gains CAMBI, the pooled mean of the first plane's per-frame banding index of the ENCODED stream,
        after GMSD; default false; a model file does not turn it on),
        xpsnr (true: the row gains XPSNR, the pooled mean of the first plane's per-frame activity-weighted PSNR in dB, each
        frame's value capped at 100.0, after CAMBI; planar pixfmts only; default false; a model file does not turn it on),
        haarpsi (true: the row gains HAARPSI, the pooled mean of the first plane's per-frame Haar wavelet perceptual similarity,
        after XPSNR; default false; a model file does not turn it on),
        vca (true: the row gains VCA_E, VCA_H and VCA_L, the pooled means of the first plane's per-frame VCA texture energy, its
        temporal gradient - frame 0's 0 included - and brightness of the INPUT stream, after HAARPSI; planar pixfmts only; default
        false; a model file does not turn it on),
        artifacts (true: the row gains BLOCKINESS, BLUR and NOISE, the pooled means of the first plane's per-frame no-reference
        blockiness, blur and noise of the ENCODED stream, after VCA_L; default false; a model file does not turn it on),
        brisque (true: the row gains BRISQUE_ALPHA and BRISQUE_SIGMA2, the pooled means of features 0 and 1 - the GGD shape and
        variance of the first plane's MSCN field at scale 0 - of the ENCODED stream, after NOISE; the log carries all 36 features;
        default false; a VMAF model file does not turn it on), brisque_model_path and brisque_range_path (libsvm's text model and
        svm-scale's range file, brisque_model.py: both turn brisque on, and the row gains BRISQUE, the pooled mean of the score,
        after BRISQUE_SIGMA2; no model ships),
        mdsi (true: the row gains MDSI, the pooled mean of the per-frame mean deviation similarity index of the planes taken
        together - 0 for identical frames, larger is worse -, after the BRISQUE columns; one- or three-plane pixfmts; default
        false; a model file does not turn it on),
        delta_itp (true: the row gains DELTA_ITP, the pooled mean of the per-frame mean dE_ITP of ITU-R BT.2124 - the three planes
        taken together, read as a BT.2020 signal; 1 is about one just-noticeable difference -, and DELTA_ITP_MAX, the largest
        pixel's value over all frames, after MDSI; three-plane pixfmts only; default false; a model file does not turn it on),
        delta_itp_transfer ("pq" default | "hlg": BT.2100's transfer function, HLG on a 1000 cd/m2 display), delta_itp_range
        ("limited" default | "full"; no effect on bgr24),
        pu21 (true: the row gains PU_PSNR and PU_PSNR_RGB, the pooled means of the per-frame PU21-PSNR of the luminance and of the
        three channels - display light in PU21 units, peak 256, each frame capped at 100.0 -, and PU_SSIM, the pooled mean of the
        per-frame PU21-SSIM, after DELTA_ITP_MAX; three-plane pixfmts only; default false; a model file does not turn it on),
        pu21_transfer ("pq" default | "hlg"), pu21_range ("limited" default | "full"; no effect on bgr24),
        fsim (true: the row gains FSIM and FSIMC, the pooled means of the per-frame feature similarity index of the luminance and of
        its colour form, the planes taken together, after PU_SSIM; one- and three-plane pixfmts; default false; a model file does
        not turn it on),
        sigstats (true: the row gains, after FSIMC and from the INPUT stream's first plane, Y_LOW - the minimum over the frames of
        the 10 % order statistic -, Y_HIGH - the maximum of the 90 % one -, OUT_OF_RANGE - the mean share of samples below 16 s or
        above 235 s -, BLACK_FRAMES, FROZEN_FRAMES and SCENE_CUTS - counts of frames, events.signal_events at its defaults - and
        CROP_TOP, CROP_BOTTOM, CROP_LEFT, CROP_RIGHT, the union box over the frames that are not black, -1 each when all are;
        default false; a model file does not turn it on), sigstats_black and sigstats_crop (null or 0 .. 65535: the black and the
        dark-border level in sample units; default 32 and 24 on the 8-bit scale),
        pixfmt (None: by input | "bgr24" | "yuv420p" | "gray" | FFmpeg's other planar names: yuv422p, yuv444p, yuv420p10le,
        yuv422p10le, yuv444p10le, the 12-bit three, yuv420p16le, yuv444p16le, gray10le, gray12le, gray16le - uint16
        [N, samples] arrays above 8 bits; .y4m inputs take theirs from the header), dct_mode ("auto" default: full-frame up to 128x128, 8x8 blocks
        above | "block8" | "full" the reference's cv2.dct at any size), motion ("sad" north_star's block-SAD | "farneback" the
        reference's own; default: set_motion_mode / VQA_MOTION), device (GPU index; default VQA_DEVICE, LOCAL_RANK, 0) and
        height / width (the geometry of headerless inputs: raw .yuv planar pairs, raw .bgr24 streams),
        scale ("bilinear" | "bicubic" | "lanczos"; default null) with dist_height / dist_width (the size of the ENCODED pair
        stream when it is a ladder rung smaller or larger than the input; .y4m files bring theirs): the rung is uploaded at its
        own size and resampled to the input's on the GPU before anything measures it (run_ffmpeg_metrics), encoded_bgr stays at
        the rung's size for the complexity half, and the row gains DIST_RES ("1280x720") and SCALE as its LAST columns; needs
        encoded_bgr next to a planar pair (one BGR stream cannot serve both halves at two sizes: ValueError),
        align (null default | an integer radius 1 .. 32): a pre-pass of its own (frame_align) measures, before the pass starts,
        whether the encoded pair stream holds the input's frames in the input's places, and the row gains ALIGN_RADIUS,
        ALIGN_OFFSET, ALIGN_DROPPED, ALIGN_REPEATED and ALIGN_PSNR_GAIN as its LAST columns; an offset, drop or repeat is also
        a warning; the frames are not re-paired; with scale it is a ValueError,
        shift (null default | an integer radius 1 .. 16) with shift_margin (null default: the radius | an integer not below it):
        a pre-pass of its own (frame_shift) measures, before the pass starts, whether the encoded pair stream's picture sits
        where the input's sits, and the row gains SHIFT_RADIUS, SHIFT_DY, SHIFT_DX, SHIFT_FRAMES_OFF and SHIFT_PSNR_GAIN as its
        LAST columns, after the ALIGN_* columns when both are on; a non-zero shift or a best shift on the band's border is also
        a warning; the frames are not moved; with scale it is a ValueError,
        light (false default | true) with light_transfer ("pq" default; "hlg" is a ValueError that says why) and light_range
        ("limited" default | "full"): a pre-pass of its own over the INPUT stream (frame_light) measures, before the pass starts,
        the HDR10 light levels and the gamut, and the row gains LIGHT_MAXCLL, LIGHT_MAXFALL, LIGHT_MAXCLL_FRAME, LIGHT_P9998,
        LIGHT_Y_AVG, LIGHT_OUT_709, LIGHT_OUT_P3 and LIGHT_CLAMPED BEFORE the ALIGN_* and SHIFT_* columns, which stay the last;
        three-plane pixfmts only,
        sync (false default | true) with sync_min_overlap (null default: half the shorter clip | an integer >= 1) and sync_apply
        (false default | true): a pre-pass of its own over the quality pair (frame_sync), before every other pre-pass, finds
        where in the input the encoded stream belongs - anywhere in the clip, for streams of unequal length and, under scale,
        of unequal size - and the row gains SYNC_OFFSET, SYNC_OVERLAP, SYNC_DISTANCE, SYNC_RUNNER_UP, SYNC_FRAMES_OFF and
        SYNC_APPLIED before the ALIGN_* / SHIFT_* columns; with sync_apply and an answer that is not ambiguous the input is
        sliced by the reference side's trim and BOTH the encoded BGR stream and the encoded pair stream by the distorted
        side's, so both halves of the pass see the same frames; an ambiguous answer is a warning and is never applied;
        sync_apply without sync is a ValueError,
        colorfit (false default | true): a pre-pass of its own over the quality pair (frame_colorfit), after the sync pre-pass
        and so over the trimmed pair, measures whether a code value means the same in both streams, and the row gains
        COLORFIT_MATCH, COLORFIT_MATCH_PSNR_GAIN, COLORFIT_PSNR_GAIN, COLORFIT_GAIN_Y, COLORFIT_OFFSET_Y,
        COLORFIT_TONE_PSNR_GAIN and COLORFIT_FRAMES_OFF after the SYNC_* and before the ALIGN_* / SHIFT_* columns; a named
        mishap or a matrix fit worth 10 log10(2) dB or more is also a warning; the frames are not corrected; with scale, and
        for a two-plane pixfmt, it is a ValueError,
        conform (false default | true) with conform_color ("none" | "match" default | "levels" | "matrix" | "tone"): what sync,
        align, shift and colorfit found is APPLIED to the quality pair on the GPU before anything is measured, as
        run_ffmpeg_metrics states it - the constant offset by slicing the input, the encoded quality stream AND its BGR frames
        alike, the shift as the common window, the colour mode on the encoded quality stream; PSNR, SSIM and every feature of the
        row are then those of the conformed pair, the COLORFIT_* columns describe the registered pair, and the row gains
        CONFORM_OFFSET, CONFORM_DY, CONFORM_DX, CONFORM_COLOR, CONFORM_RES, CONFORM_FRAMES and CONFORM_CHROMA_HALF as its LAST
        columns; the complexity half reads the BGR frames as they are.  It needs at least one of sync, align, shift and
        colorfit, a colour mode other than "none" needs colorfit, and a quality pair of its own (planar streams next to
        encoded_bgr); with scale it is a ValueError,
        convert (null | "box" | "linear"; default null) with dist_pixfmt (the ENCODED pair stream's own pixel layout, one of
        pixfmt's names; a .y4m pair brings both in its headers), convert_siting ("center" | "left") and convert_range ("limited" |
        "full"): the encoded pair stream differs from the input in sample depth and / or chroma layout; every chunk is uploaded
        as it is and converted to the input's layout on the GPU (run_ffmpeg_metrics' convert; include/vqa.h's integer definition,
        not swscale's), ahead of scale where both are named.  The row gains DIST_PIXFMT and CONVERT ("linear/center/limited")
        right after DIST_RES / SCALE where those exist.  It needs a quality pair of its own (planar streams next to encoded_bgr);
        dist_pixfmt without convert, convert on equal layouts, on a differing plane count or bgr24, and convert with sync, align,
        shift, colorfit or conform are ValueErrors; light stays allowed,
        fields (true | false; default false): frame_fields reads both streams of the quality pair as given, ahead of every
        pre-pass, and the row gains FIELDS_REF_TYPE, FIELDS_REF_COMBED, FIELDS_REF_CADENCE, FIELDS_REF_REPEATS, the same four as
        FIELDS_DIST_* and FIELDS_MATCH right after DIST_RES / SCALE / DIST_PIXFMT / CONVERT where those exist and before every
        pre-pass column (run_ffmpeg_metrics' fields).  The frames are not changed; it goes with every other key.
    column_order="reference" keeps the reference's unpacking of the 8-tuple (:235-242), which shifts five labels
    (SURVEY.md §3.2); "fixed" uses the tuple's true order."""
    import tempfile
    import uuid
    from . import complexity_metrics as cm
    _check_mode_keys(config)
    crf = config.get("crf", 23)
    rw, rh = config.get("resize_width", 64), config.get("resize_height", 64)
    interval = config.get("frame_interval", 10)
    batch_size = config.get("batch_size", 100)
    ssim_mode = _SSIM_MODES[config.get("ssim_mode", "gauss")]
    sw = _config_switches(config)
    models = _load_models(sw)   # before the pass starts: a bad file costs no GPU time
    scale = config.get("scale")
    req = _requests(config, config=True)
    scaling = req.scaling
    dct_mode = cm._DCT_MODES[config.get("dct_mode")]
    motion_mode = cm.motion_mode_of(config.get("motion"))
    device = config.get("device")
    layout = config.get("pixfmt") or "bgr24"
    height, width = height or config.get("height"), width or config.get("width")   # (raw .yuv / .bgr24 files carry no header)
    uid = uuid.uuid4().hex
    tmp = tempfile.gettempdir()
    psnr_log, ssim_log, vmaf_log = (os.path.join(tmp, "%s_%s.log" % (k, uid)) for k in ("psnr", "ssim", "vmaf"))
    try:
        ref, layout, qh, qw = _open_quality_stream(input_video, layout, height, width)
        qenc, layout_d, dqh, dqw = _open_quality_stream(encoded_video, (config.get("dist_pixfmt") or layout) if req.convert else layout,
                                                        config.get("dist_height") or (None if scaling else qh),
                                                        config.get("dist_width") or (None if scaling else qw))
        _check_convert_layouts(layout, layout_d, req.convert is not None)
        if scaling and (layout == "bgr24" and encoded_bgr is None):
            raise ValueError("scaling needs a distorted stream of the quality half's own: pass the rung as a planar pair next to "
                             "encoded_bgr (one BGR stream serves both halves at one size)")
        if not scaling:
            dqh, dqw = qh, qw
        if layout == "bgr24" and encoded_bgr is None:
            enc, qdist = qenc, None       # (:216 and :242 read the same encoded stream: every chunk is uploaded once)
        else:
            if encoded_bgr is None:
                raise ValueError("a %s quality pair needs the encoded stream's BGR frames for the complexity half "
                                 "(complexity_metrics.py:100 reads cv2's BGR decode): pass encoded_bgr=" % layout)
            enc, qdist = _open_frames(encoded_bgr, dqh or height, dqw or width), _host_stream(qenc, wide=True)
            ref = _host_stream(ref, wide=True)
        eh, ew = (enc.h, enc.w) if isinstance(enc, DeviceFrames) else (enc.shape[1], enc.shape[2])
        if qdist is None:
            h, w = eh, ew
        else:
            h, w = _geometry(ref, layout, (qh or eh) if not scaling else qh, (qw or ew) if not scaling else qw)
            if scaling and (not h or not w):
                raise ValueError("scale needs the input stream's size: height and width")
            dh, dw = _geometry(qdist, layout_d, dqh or eh, dqw or ew) if scaling else (h, w)   # (the BGR stream has the rung's size)
            for a, lay, (ah, aw) in ((ref, layout, (h, w)), (qdist, layout_d, (dh, dw))):   # (layout_d is layout unless converting)
                if lay == "yuv420p":
                    from .frames import frame_bytes_yuv420p
                    if not isinstance(a, DeviceFrames) and (a.ndim != 2 or a.shape[1] != frame_bytes_yuv420p(ah, aw)):
                        raise ValueError("yuv420p streams must be planar [N, H*W*3/2] uint8 arrays of the frames' geometry "
                                         "(%dx%d: %d bytes per frame)" % (aw, ah, frame_bytes_yuv420p(ah, aw)))
                elif lay in PIXFMTS and lay != "gray":
                    dt = np.uint16 if layout_depth(lay) > 8 else np.uint8
                    if not isinstance(a, DeviceFrames) and (a.ndim != 2 or a.shape[1] != frame_samples(ah, aw, lay)
                                                            or a.dtype != dt):
                        raise ValueError("%s streams must be planar [N, %d] %s arrays of the frames' geometry (%dx%d)"
                                         % (lay, frame_samples(ah, aw, lay), np.dtype(dt).name, aw, ah))
        _conform_tone_depth(req.mode, layout)
        planes = LAYOUTS[layout][0](h, w)
        dist_planes = extra = None
        if scaling:
            from .engine import check_scale_planes
            dist_planes = LAYOUTS[layout][0](dh, dw)
            if not req.convert:
                check_scale_planes(dist_planes, planes)
            extra = {"DIST_RES": "%dx%d" % (dw, dh), "SCALE": scale}
        if req.convert:
            if qdist is None:
                raise ValueError("converting needs a distorted stream of the quality half's own: pass the quality pair as planar "
                                 "streams next to encoded_bgr (one BGR stream serves both halves as it is)")
            dist_planes, extra = _convert_planes(req.convert, scaling, scale, layout, layout_d, planes, dh, dw, extra)
        for f in FEATURES:
            if sw[f.kind] and f.plane_check is not None:
                f.plane_check(planes)
        if req.mode is not None and qdist is None:
            raise ValueError("conform needs a distorted stream of the quality half's own: pass the quality pair as planar "
                             "streams next to encoded_bgr (one BGR stream serves both halves as it is)")
        extra = _fields_keys(req.fields, ref, layout, h, w, enc if qdist is None else qdist, layout_d,
                             *((dh, dw) if scaling else (h, w)), extra, device)
        # the pre-passes read the quality pair; the BGR frames beside it are cut with it, so both halves see the same frames
        streams, extra, plan, planes, ran = _prepass_chain(
            req, ref, enc if qdist is None else qdist, () if qdist is None else (enc,), layout, h, w,
            (dh, dw) if scaling else (h, w), planes, sw, device, extra=extra)
        ran = ran or req.fields
        ref, enc, qdist = (streams[0], streams[1], None) if qdist is None else (streams[0], streams[2], streams[1])
        wr = _StatsWriter(psnr_log, ssim_log, layout, _sizes(planes))
        try:
            _q, series = _measure(enc, ref, sw, models, planes, ssim_mode, layout, dist_planes, scale, extra, vmaf_log,
                                  complexity=stream.Complexity((rw, rh), interval, dct_mode=dct_mode, motion_mode=motion_mode),
                                  ran=ran, batch_size=batch_size, on_quality=wr, qdist=qdist, device=device, conform=plan,
                                  convert=req.convert)
        finally:
            wr.close()
        resolution = "%dx%d" % (ew, eh)
        metrics = extract_metrics_from_logs(psnr_log, ssim_log, vmaf_log, input_video, crf, bitrate, resolution, frame_rate)
        t = cm.pool_series(series, enc, interval, batch_size=batch_size, fps=frame_rate)
        if column_order == "reference":   # (:235-242) motion, dct, temporal, hist, edge, orb, colour, fps
            names = ("Advanced Motion Complexity", "DCT Complexity", "Temporal DCT Complexity", "Histogram Complexity",
                     "Edge Detection Complexity", "ORB Feature Complexity", "Color Histogram Complexity",
                     "Framerate Variation")
        else:                             # (:301-310) the order the tuple really has
            names = ("Advanced Motion Complexity", "DCT Complexity", "Histogram Complexity", "Edge Detection Complexity",
                     "ORB Feature Complexity", "Color Histogram Complexity", "Temporal DCT Complexity",
                     "Framerate Variation")
        metrics.update(dict(zip(names, t)))
        if scaling or req.convert or req.fields:
            metrics.update(extra)
        if ran:   # (extract_metrics_from_logs read the pre-passes' keys off the log: they go last)
            metrics.update((k, metrics.pop(k)) for k in list(extra))
        thread_safe_update_csv(metrics, csv_file)
        return metrics
    finally:
        for p in (psnr_log, ssim_log, vmaf_log):
            if os.path.exists(p):
                os.remove(p)


def extract_metrics_from_logs(psnr_log, ssim_log, vmaf_log, video_file, crf, bitrate, resolution, frame_rate):
    """video_processing.py:145-177 — same keys, same regular expressions, first match only."""
    metrics = {"Bitrate (kbps)": bitrate, "Resolution (px)": resolution, "Frame Rate (fps)": frame_rate, "CRF": crf}
    if os.path.isfile(psnr_log):
        with open(psnr_log) as f:
            match = re.search(r"psnr_avg:(\s*\d+\.\d+)", f.read())
            if match:
                metrics["PSNR"] = float(match.group(1))
    if os.path.isfile(ssim_log):
        with open(ssim_log) as f:
            match = re.search(r"All:(\s*\d+\.\d+)", f.read())
            if match:
                metrics["SSIM"] = float(match.group(1))
    if os.path.isfile(vmaf_log):   # this build's JSON (write_vif_log): the pooled means; VMAF when a model scored the frames
        import json
        try:
            with open(vmaf_log) as f:
                doc = json.load(f)
            pooled, signal, doc_top = doc.get("pooled_metrics", {}), doc.get("signal"), doc
        except (ValueError, AttributeError):   # not a JSON log (libvmaf writes XML by default): nothing to add
            pooled, signal, doc_top = {}, None, None
        if "vmaf" in pooled:       # (:172-173), placed where the reference puts it: right after SSIM
            metrics["VMAF"] = float(pooled["vmaf"]["mean"])
        for f in FEATURES:         # (per-frame dB values were capped by the log's writer)
            f.to_row(f, pooled, signal, metrics)
        for p in PREPASSES:        # a pre-pass's keys, when the log holds them all: the row's last columns, in the table's order
            if isinstance(doc_top, dict) and all(k in doc_top for k in p.keys):
                metrics.update((k, doc_top[k]) for k in p.keys)
    return metrics


def load_config(config_file):
    """video_processing.py:71-85 — JSON config, validated; same keys as the reference's config.json."""
    import json
    with open(config_file, "r") as f:
        config = json.load(f)
    validate_config(config)
    return config


def validate_config(config):
    """video_processing.py:87-98 — same range checks, same messages; then this build's added keys in the same style."""
    if not (1 <= config.get("crf", 23) <= 51):
        raise ValueError("CRF value must be between 1 and 51.")
    if config.get("resize_width", 0) <= 0 or config.get("resize_height", 0) <= 0:
        raise ValueError("Resize dimensions must be positive integers.")
    if config.get("frame_interval", 10) <= 0:
        raise ValueError("Frame interval must be a positive integer.")
    if not isinstance(config.get("num_workers", (os.cpu_count() or 2) // 2), int):
        raise ValueError("num_workers must be an integer.")
    # this build's keys: MODE_KEYS, device, batch_size, height / width, the scale, align, shift, light, sync and colorfit requests and every config key of FEATURES (the
    # kinds' switches and their parameters); and that a vmaf_model_path names a readable file
    _check_mode_keys(config)


def main(argv=None):
    """video_processing.py:300-321 with decoded streams instead of a container + encode step:
        python -m rtvqa_amd.video_processing config.json input.npy encoded.npy [--csv out.csv]"""
    import argparse
    ap = argparse.ArgumentParser(description="Quality + complexity metrics of an (input, encoded) stream pair -> CSV row.")
    ap.add_argument("config_file")
    ap.add_argument("input_video", help="reference stream: .npy [N,H,W,3] BGR")
    ap.add_argument("encoded_video", help="distorted stream, same geometry (.npy BGR, or .y4m with --encoded-bgr)")
    ap.add_argument("--encoded-bgr", default=None, help="with a .y4m quality pair: the encoded stream's BGR frames (.npy) for the complexity half")
    ap.add_argument("--csv", default="video_quality_data.csv")
    ap.add_argument("--column-order", default="reference", choices=["reference", "fixed"])
    a = ap.parse_args(argv)
    m = process_video_and_extract_metrics(a.input_video, a.encoded_video, load_config(a.config_file), csv_file=a.csv,
                                          column_order=a.column_order, encoded_bgr=a.encoded_bgr)
    print(m)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
