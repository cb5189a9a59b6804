"""The feature table: what video_processing knows about each plane-batch kind of stream.PLANE_KINDS - ONE entry per kind, in that
table's order, which is the order of the log's keys and of the row's columns.

FEATURES says per kind under which names the entry points and the config switch it on, which record fields become which keys of
the JSON log and under which cap, which pooled statistic becomes which CSV column, and which parameters it has.
video_processing's write_vif_log, _write_feature_log, run_ffmpeg_metrics, process_video_and_extract_metrics, _check_mode_keys,
extract_metrics_from_logs and frame_* calls read it and name no kind themselves; a new kind is a row here, next to its row in
PLANE_KINDS ("Adding a metric").
"""
import collections
import os

import numpy as np

from . import _native as N
from . import stream
from .engine import check_vca_planes, check_xpsnr_planes

PSNR_HVS_DB_CAP = 100.0   # JSON has no infinity: the log and the row carry min(dB, 100); the C record keeps the infinity
PU21_PSNR_CAP = 100.0   # the row's PU_PSNR and PU_PSNR_RGB: a frame's value (inf for identical frames) is capped here before pooling
ITP_RANGES = {"limited": False, "full": True}   # the config's "delta_itp_range" / "pu21_range" -> full_range


# ---- the config's checks, check(key, config), in the reference's validate_config style
def check_switch(key, config):
    if key in config and not isinstance(config[key], bool):
        raise ValueError("%s must be true or false." % key)


def _cfg_choice(allowed, text):
    def check(key, config):
        if key in config and not (isinstance(config[key], str) and config[key] in allowed):
            raise ValueError("%s must be %s." % (key, text))
    return check


def _cfg_weights(key, config):
    if key in config:
        k = config[key]
        if not (isinstance(k, (list, tuple)) and len(k) == 3 and
                all(isinstance(x, (int, float)) and not isinstance(x, bool) and np.isfinite(x) and x > 0 for x in k)):
            raise ValueError("%s must be three positive numbers [kL, kC, kH]." % key)


def _cfg_level(key, config):
    v = config.get(key)
    if v is not None and (isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= N.SIGSTATS_MAX_LEVEL):
        raise ValueError("%s must be null or an integer from 0 to %d." % (key, N.SIGSTATS_MAX_LEVEL))


def _cfg_file(key, config):
    bp = config.get(key)
    if bp is not None and not (isinstance(bp, str) and os.path.isfile(bp) and os.access(bp, os.R_OK)):
        raise ValueError("%s must be null or the path of a readable file." % key)


def _cfg_range_file(key, config):
    _cfg_file(key, config)
    if config.get(key) is not None and config.get("brisque_model_path") is None:
        raise ValueError("%s needs a brisque_model_path." % key)


_cfg_transfer, _cfg_range = _cfg_choice(N.ITP_TRANSFERS, '"pq" or "hlg"'), _cfg_choice(ITP_RANGES, '"limited" or "full"')


# ---- records -> the log's columns: to_log(feature, records, given) -> (keys, columns [n] float64, top-level keys of the log);
# given: write_vif_log's arguments by name
def _field_columns(f, rec, given):
    rec = np.asarray(rec).reshape(-1)
    cols = [(field(rec) if callable(field) else rec[field]).astype(np.float64) for _, field, _ in f.log]
    return [key for key, _, _ in f.log], [c if cap is None else np.minimum(c, cap) for c, (_, _, cap) in zip(cols, f.log)], {}


def _vif_columns(f, rec, given):
    """rec: write_vif_log's `scale`, the [n, 4] array - or the records whose field of that name it is"""
    rec = np.asarray(rec)
    scale = np.asarray(rec["scale"] if rec.dtype.names else rec, np.float64).reshape(-1, N.VIF_LEVELS)
    return [key for key, _, _ in f.log], [scale[:, s] for s in range(N.VIF_LEVELS)], {}


def _brisque_columns(f, rec, given):
    """the 36 features and, with a model (brisque_model.load_model), its score over them"""
    feats = np.asarray(rec).reshape(-1)["features"].astype(np.float64).reshape(-1, 36)
    names, cols = [key for key, _, _ in f.log[:36]], [feats[:, k] for k in range(36)]
    if given["brisque_model"] is not None:
        from . import brisque_model as bm
        names, cols = names + [f.log[36][0]], cols + [bm.predict(given["brisque_model"], feats)]
    return names, cols, {}


def _sigstats_columns(f, rec, given):
    """the levels, the out-of-range share and events.signal_events' per-frame answers; the clip's events as the "signal" object"""
    from . import events
    rec = np.asarray(rec).reshape(-1)
    ev = events.signal_events(rec, given["sigstats_depth"])
    count = rec["count"].astype(np.float64)
    cols = [rec[k].astype(np.float64) for k in ("min", "low", "mean", "high", "max", "dif")]
    cols += [(rec["under"].astype(np.float64) + rec["over_luma"].astype(np.float64)) / count,
             ev["black"].astype(np.float64), ev["frozen"].astype(np.float64), ev["scene_score"]]
    signal = {"black_frames": int(ev["black"].sum()), "frozen_frames": int(ev["frozen"].sum()),
              "scene_cuts": len(ev["cuts"]), "crop": None if ev["crop"] is None else list(ev["crop"])}
    return [key for key, _, _ in f.log], cols, {"signal": signal}


# ---- the log's pooled values -> the row's columns: to_row(feature, pooled, signal, metrics) adds to metrics
def _pooled_columns(f, pooled, signal, metrics):
    for column, key, stat in f.row:
        if key in pooled:
            metrics[column] = float(pooled[key][stat])


SIGNAL_COLUMNS = (("BLACK_FRAMES", "black_frames"), ("FROZEN_FRAMES", "frozen_frames"), ("SCENE_CUTS", "scene_cuts"))
CROP_COLUMNS = ("CROP_TOP", "CROP_BOTTOM", "CROP_LEFT", "CROP_RIGHT")


def _sigstats_row(f, pooled, signal, metrics):
    """the source's signal statistics: extremes, a mean share and - integers, from the "signal" object - event counts and the box"""
    if "y_low" in pooled and signal is not None:
        _pooled_columns(f, pooled, signal, metrics)
        for column, key in SIGNAL_COLUMNS:
            metrics[column] = int(signal[key])
        for column, v in zip(CROP_COLUMNS, signal["crop"] if signal["crop"] is not None else (-1, -1, -1, -1)):
            metrics[column] = int(v)


# kind          the name in stream.PLANE_KINDS (Quality's switch)
# flag          the keyword of run_ffmpeg_metrics and write_vif_log: the kind's name, but for dE_ITP's
# config_key    the config's boolean key: the flag, but for motion's (the config's "motion" is the complexity half's motion mode)
# log           (log key, record field or function of the records, cap or None), in the log's order
# row           (CSV column, log key, pooled statistic), in the row's order
# params        Param(config key, run_ffmpeg_metrics keyword, Quality keyword, config check, config value -> Quality value or None,
#               early); without a Quality keyword the parameter is a model file's path, which turns the kind on; early: the
#               entry points check the value under THEIR name for it (by PLANE_KINDS' check) before a stream is opened
# three_planes  the entry points refuse a one-plane layout under the flag's name before a stream is opened
# plane_check   check(planes), run by the two log-writing entry points before a stream is opened
# to_log, to_row   the functions above, where "field -> column" does not say it
Param = collections.namedtuple("Param", "config flag quality check convert early", defaults=(None, False))
Feature = collections.namedtuple("Feature", "kind log row flag config_key params three_planes plane_check to_log to_row",
                                 defaults=(None, None, (), False, None, _field_columns, _pooled_columns))


def _same(*keys, cap=None):
    """log columns named as their record fields"""
    return tuple((k, k, cap) for k in keys)


def _means(*keys, stat="mean"):
    """row columns named as their log keys, in capitals"""
    return tuple((k.upper(), k, stat) for k in keys)


def _level(s):
    return lambda rec: rec["scale"][:, s]


_VIF_KEYS = tuple("vif_scale%d" % s for s in range(N.VIF_LEVELS))
_ADM_KEYS = tuple("adm_scale%d" % s for s in range(N.ADM_LEVELS))
_BRISQUE_KEYS = tuple("brisque_%02d" % k for k in range(36)) + ("brisque",)
_SIGSTATS_KEYS = ("y_min", "y_low", "y_avg", "y_high", "y_max", "y_dif", "out_of_range", "black", "frozen", "scene_score")
FEATURES = tuple(f._replace(flag=f.flag or f.kind, config_key=f.config_key or f.flag or f.kind) for f in (
    Feature("vif", tuple((k, None, None) for k in _VIF_KEYS), tuple((k.replace("vif", "VIF"), k, "mean") for k in _VIF_KEYS),
            to_log=_vif_columns),
    Feature("adm", _same("adm2") + tuple((k, _level(s), None) for s, k in enumerate(_ADM_KEYS)),
            _means("adm2") + tuple((k.replace("adm", "ADM"), k, "mean") for k in _ADM_KEYS)),
    Feature("motion", _same("motion2", "motion"), _means("motion2", "motion"), config_key="motion_feature"),
    Feature("siti", _same("si", "ti"), _means("si", "ti", stat="max")),   # ITU-T P.910: the clip's value is the maximum over its frames
    Feature("psnr_hvs", _same("psnr_hvs", "psnr_hvsm", cap=PSNR_HVS_DB_CAP), _means("psnr_hvs", "psnr_hvsm")),
    Feature("ciede", _same("ciede2000", cap=PSNR_HVS_DB_CAP), _means("ciede2000"), three_planes=True,
            params=(Param("ciede_weights", "ciede_weights", "ciede_weights", _cfg_weights, tuple),)),
    Feature("gmsd", _same("gmsd"), _means("gmsd")),
    Feature("cambi", _same("cambi"), _means("cambi")),
    Feature("xpsnr", _same("xpsnr", cap=PSNR_HVS_DB_CAP), _means("xpsnr"), plane_check=check_xpsnr_planes),
    Feature("haarpsi", _same("haarpsi"), _means("haarpsi")),
    Feature("vca", (("vca_e", "e", None), ("vca_h", "h", None), ("vca_l", "l", None)),   # (frame 0's vca_h = 0 is pooled too)
            _means("vca_e", "vca_h", "vca_l"), plane_check=check_vca_planes),
    Feature("artifacts", _same("blockiness", "blur", "noise"), _means("blockiness", "blur", "noise")),
    Feature("brisque", tuple((k, None, None) for k in _BRISQUE_KEYS),
            (("BRISQUE_ALPHA", "brisque_00", "mean"), ("BRISQUE_SIGMA2", "brisque_01", "mean"), ("BRISQUE", "brisque", "mean")),
            params=(Param("brisque_model_path", "brisque_model_path", None, _cfg_file),
                    Param("brisque_range_path", "brisque_range_path", None, _cfg_range_file)), to_log=_brisque_columns),
    Feature("mdsi", _same("mdsi"), _means("mdsi")),
    Feature("itp", (("delta_itp", "de_mean", None), ("delta_itp_max", "de_max", None)),
            (("DELTA_ITP", "delta_itp", "mean"), ("DELTA_ITP_MAX", "delta_itp_max", "max")), flag="delta_itp", three_planes=True,
            params=(Param("delta_itp_transfer", "delta_itp_transfer", "itp_transfer", _cfg_transfer, early=True),
                    Param("delta_itp_range", "delta_itp_full_range", "itp_full_range", _cfg_range, ITP_RANGES.__getitem__,
                          early=True))),
    Feature("pu21", _same("pu_psnr", "pu_psnr_rgb", cap=PU21_PSNR_CAP) + _same("pu_ssim"),
            _means("pu_psnr", "pu_psnr_rgb", "pu_ssim"), three_planes=True,
            params=(Param("pu21_transfer", "pu21_transfer", "pu21_transfer", _cfg_transfer, early=True),
                    Param("pu21_range", "pu21_full_range", "pu21_full_range", _cfg_range, ITP_RANGES.__getitem__,
                          early=True))),
    Feature("fsim", _same("fsim", "fsimc"), _means("fsim", "fsimc")),
    Feature("sigstats", tuple((k, None, None) for k in _SIGSTATS_KEYS),
            (("Y_LOW", "y_low", "min"), ("Y_HIGH", "y_high", "max"), ("OUT_OF_RANGE", "out_of_range", "mean")),
            params=(Param("sigstats_black", "sigstats_black", "sigstats_black", _cfg_level),
                    Param("sigstats_crop", "sigstats_crop", "sigstats_crop", _cfg_level)),
            to_log=_sigstats_columns, to_row=_sigstats_row),
))
KINDS = {k.name: k for k in stream.PLANE_KINDS}
PARAM_CHECKS = {name: check for k in stream.PLANE_KINDS for name, check in k.params}   # Quality keyword -> check(name, value)
# what a switches dict holds besides Quality's keywords: the model files' paths
MODEL_PATHS = ("vmaf_model_path",) + tuple(p.flag for f in FEATURES for p in f.params if p.quality is None)


def switches(values, config=False):
    """run_ffmpeg_metrics' arguments by name - or, config=True, a validated config - -> stream.Quality's keywords for the kinds
    and their parameters, plus the model files' paths under their own names.  Pure: no file and no device is touched."""
    sw = {}
    for f in FEATURES:
        sw[f.kind] = bool(values.get(f.config_key if config else f.flag, False))
        for p in f.params:
            name = p.config if config else p.flag
            if name in values:
                v = values[name]
                sw[p.quality or name] = p.convert(v) if config and p.convert else v
                if p.quality is None and v is not None:
                    sw[f.kind] = True
    sw["vmaf_model_path"] = values.get("vmaf_model_path")
    if sw["vmaf_model_path"] is not None:   # VMAF's features
        sw.update(vif=True, adm=True, motion=True)
    return sw
