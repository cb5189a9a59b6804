"""The VMAF score from a libvmaf model file: an RBF support-vector regression over per-frame features, on the host.

This restates, in vectorised float64 NumPy, what libvmaf's predict.c does with a model of type LIBSVMNUSVR and what libsvm's
svm_predict computes for an (epsilon- or nu-) SVR with an RBF kernel:

    x'_j  = slopes[j + 1] * f_j + intercepts[j + 1]                 (norm_type "linear_rescale"; j = 0 .. k - 1)
    y     = sum_i coef_i * exp(-gamma * |x' - sv_i|^2) - rho        (svm_predict)
    score = (y - intercepts[0]) / slopes[0], clipped to score_clip  (index 0 of slopes / intercepts belongs to the score)

Two file formats are accepted (load_model):

  * libvmaf's JSON model: key "model_dict" with model_type "LIBSVMNUSVR", norm_type "linear_rescale", feature_names
    ("VMAF_feature_adm2_score", "VMAF_feature_motion2_score", "VMAF_feature_vif_scale0_score" ...), slopes and intercepts of
    length 1 + features, an optional score_clip [lo, hi] and "model": libsvm's text model as ONE string.
    "score_transform" is IGNORED, as libvmaf ignores it by default (its enable_transform option is off); so is
    "feature_opts_dicts" when every entry is empty.  Every other key this module does not know is refused.
  * a bare libsvm text model: no normalisation (slopes 1, intercepts 0), no clip, and the features in vmaf_v0.6.1's order
    (FEATURES_V061).

The libsvm text model: header lines "svm_type nu_svr|epsilon_svr", "kernel_type rbf", "gamma G", "nr_class 2" (optional, not
used), "total_sv N", "rho R", then "SV" and N lines "coef idx:val idx:val ..." with 1-based, ascending, SPARSE indices (an
absent index is 0).  Anything else - another kernel type, an unknown feature name, a length mismatch, an unknown header line -
is a ValueError that names what was met.

The predictor is a few thousand flops per frame (about 200 support vectors x 6 features for vmaf_v0.6.1) next to the other
host float tails: it is not a kernel and not part of the C ABI (include/vqa.h says so).  No libvmaf model file ships with this
project and none was available when it was written: the module follows the formats as stated above and is tested with models
the tests construct; it is NOT pinned against libvmaf's binary or against the real vmaf_v0.6.1.json.

predict() forms every row on its own (reductions over the last axis of C-contiguous arrays, no BLAS), so a frame's score does
not depend on which other frames are in the call.
"""
import json

import numpy as np

# vmaf_v0.6.1's features, in its order: what a bare libsvm model is fed
FEATURES_V061 = ("adm2", "motion2", "vif_scale0", "vif_scale1", "vif_scale2", "vif_scale3")
# every per-frame feature this project measures (the keys of the JSON log)
KNOWN_FEATURES = ("adm2", "adm_scale0", "adm_scale1", "adm_scale2", "adm_scale3", "motion", "motion2",
                  "vif_scale0", "vif_scale1", "vif_scale2", "vif_scale3")
_MODEL_KEYS = ("model_type", "norm_type", "feature_names", "slopes", "intercepts", "score_clip", "score_transform", "model",
               "feature_opts_dicts")


class VmafModel:
    """features (names as in the JSON log), slopes / intercepts [1 + k], score_clip (lo, hi) or None, gamma, rho,
    coef [n_sv], sv [n_sv, k]"""

    def __init__(self, features, slopes, intercepts, score_clip, gamma, rho, coef, sv):
        self.features = tuple(features)
        self.slopes = np.asarray(slopes, np.float64)
        self.intercepts = np.asarray(intercepts, np.float64)
        self.score_clip = None if score_clip is None else (float(score_clip[0]), float(score_clip[1]))
        self.gamma, self.rho = float(gamma), float(rho)
        self.coef = np.ascontiguousarray(coef, np.float64)
        self.sv = np.ascontiguousarray(sv, np.float64)


def parse_libsvm(text, n_features):
    """libsvm's text model -> (gamma, rho, coef [n_sv], sv [n_sv, n_features])"""
    lines = [ln.strip() for ln in text.splitlines()]
    lines = [ln for ln in lines if ln]
    head = {}
    at = None
    for i, ln in enumerate(lines):
        if ln == "SV":
            at = i + 1
            break
        key, _, val = ln.partition(" ")
        if key not in ("svm_type", "kernel_type", "gamma", "nr_class", "total_sv", "rho"):
            raise ValueError("libsvm model: unsupported header line %r" % ln)
        if key in head:
            raise ValueError("libsvm model: header line %r twice" % key)
        head[key] = val.strip()
    if at is None:
        raise ValueError("libsvm model: no 'SV' line")
    for key in ("svm_type", "kernel_type", "gamma", "total_sv", "rho"):
        if key not in head:
            raise ValueError("libsvm model: no %r line" % key)
    if head["svm_type"] not in ("nu_svr", "epsilon_svr"):
        raise ValueError("libsvm model: svm_type must be nu_svr or epsilon_svr (got %r)" % head["svm_type"])
    if head["kernel_type"] != "rbf":
        raise ValueError("libsvm model: kernel_type must be rbf (got %r)" % head["kernel_type"])
    try:
        gamma, rho, total = float(head["gamma"]), float(head["rho"]), int(head["total_sv"])
    except ValueError:
        raise ValueError("libsvm model: gamma, rho and total_sv must be numbers (got %r, %r, %r)"
                         % (head["gamma"], head["rho"], head["total_sv"]))
    rows = lines[at:]
    if len(rows) != total:
        raise ValueError("libsvm model: total_sv says %d support vectors, %d follow 'SV'" % (total, len(rows)))
    coef = np.zeros(total, np.float64)
    sv = np.zeros((total, n_features), np.float64)
    for r, ln in enumerate(rows):
        parts = ln.split()
        try:
            coef[r] = float(parts[0])
            for item in parts[1:]:
                idx, _, val = item.partition(":")
                j = int(idx)
                if not 1 <= j <= n_features:
                    raise ValueError("libsvm model: support vector %d has index %d, the model has %d features" % (r, j, n_features))
                sv[r, j - 1] = float(val)
        except ValueError as e:
            if str(e).startswith("libsvm model:"):
                raise
            raise ValueError("libsvm model: cannot read support vector line %r" % ln)
    return gamma, rho, coef, sv


def _feature_of(name):
    """'VMAF_feature_adm2_score' -> 'adm2'"""
    short = name
    if short.startswith("VMAF_feature_"):
        short = short[len("VMAF_feature_"):]
    if short.endswith("_score"):
        short = short[:-len("_score")]
    if short not in KNOWN_FEATURES:
        raise ValueError("model: unknown feature name %r (known: %s)" % (name, ", ".join(KNOWN_FEATURES)))
    return short


def model_from_dict(doc):
    """libvmaf's JSON model, parsed -> VmafModel"""
    if not isinstance(doc, dict) or not isinstance(doc.get("model_dict"), dict):
        raise ValueError("model: a JSON model needs a 'model_dict' object")
    md = doc["model_dict"]
    for key in md:
        if key not in _MODEL_KEYS:
            raise ValueError("model: unsupported key %r in model_dict" % key)
    if md.get("model_type") != "LIBSVMNUSVR":
        raise ValueError("model: model_type must be LIBSVMNUSVR (got %r)" % (md.get("model_type"),))
    if md.get("norm_type") != "linear_rescale":
        raise ValueError("model: norm_type must be linear_rescale (got %r)" % (md.get("norm_type"),))
    if any(md.get("feature_opts_dicts") or ()):
        raise ValueError("model: feature options are not supported (got %r)" % (md["feature_opts_dicts"],))
    names = md.get("feature_names")
    if not isinstance(names, list) or not names:
        raise ValueError("model: feature_names must be a non-empty list")
    features = [_feature_of(nm) for nm in names]
    k = len(features)
    for key in ("slopes", "intercepts"):
        v = md.get(key)
        if not isinstance(v, list) or len(v) != 1 + k:
            raise ValueError("model: %s must have 1 + %d entries (got %r)" % (key, k, None if v is None else len(v)))
    if md["slopes"][0] == 0:
        raise ValueError("model: slopes[0] must not be 0")
    clip = md.get("score_clip")
    if clip is not None and (not isinstance(clip, list) or len(clip) != 2):
        raise ValueError("model: score_clip must be [lo, hi] (got %r)" % (clip,))
    if not isinstance(md.get("model"), str):
        raise ValueError("model: 'model' must be libsvm's text model as one string")
    gamma, rho, coef, sv = parse_libsvm(md["model"], k)
    return VmafModel(features, md["slopes"], md["intercepts"], clip, gamma, rho, coef, sv)


def load_model(path):
    """A libvmaf JSON model or a bare libsvm text model (the module docstring states both) -> VmafModel."""
    with open(path, "r") as f:
        text = f.read()
    if text.lstrip().startswith("{"):
        try:
            doc = json.loads(text)
        except ValueError as e:
            raise ValueError("model: %s is not valid JSON (%s)" % (path, e))
        return model_from_dict(doc)
    k = len(FEATURES_V061)
    gamma, rho, coef, sv = parse_libsvm(text, k)
    return VmafModel(FEATURES_V061, np.ones(1 + k), np.zeros(1 + k), None, gamma, rho, coef, sv)


def predict(model, features):
    """features [n, k] (columns in model.features' order; [k]: one frame) -> scores [n], float64."""
    f = np.asarray(features, np.float64)
    if f.ndim == 1:
        f = f[None]
    k = len(model.features)
    if f.ndim != 2 or f.shape[1] != k:
        raise ValueError("the model takes %d features per frame (got an array of shape %s)" % (k, f.shape))
    x = np.ascontiguousarray(f * model.slopes[1:] + model.intercepts[1:])
    d = x[:, None, :] - model.sv[None, :, :]                     # [n, n_sv, k]
    d2 = np.sum(d * d, axis=2)
    y = np.sum(model.coef[None, :] * np.exp(-model.gamma * d2), axis=1) - model.rho
    score = (y - model.intercepts[0]) / model.slopes[0]
    if model.score_clip is not None:
        score = np.clip(score, model.score_clip[0], model.score_clip[1])
    return score


def feature_matrix(model, columns):
    """columns: feature name -> [n] -> the [n, k] matrix predict takes; a feature the model names and `columns` lacks is a
    ValueError."""
    missing = [nm for nm in model.features if nm not in columns]
    if missing:
        raise ValueError("the model needs features that were not measured: %s" % ", ".join(missing))
    return np.stack([np.asarray(columns[nm], np.float64) for nm in model.features], axis=1)
