"""libvmaf's SVR prediction in float64 by plain loops, written from the docstring of rtvqa_amd/vmaf_model.py - not from its code.

    x'_j  = slopes[j + 1] * f_j + intercepts[j + 1]
    y     = sum_i coef_i * exp(-gamma * |x' - sv_i|^2) - rho
    score = (y - intercepts[0]) / slopes[0], clipped to score_clip

and the two file formats the tests write: libvmaf's JSON model and libsvm's text model (sparse 1-based indices)."""
import json
import math

FEATURES_V061 = ("adm2", "motion2", "vif_scale0", "vif_scale1", "vif_scale2", "vif_scale3")


def predict_one(f, slopes, intercepts, clip, gamma, rho, coef, sv):
    x = [slopes[j + 1] * f[j] + intercepts[j + 1] for j in range(len(f))]
    y = 0.0
    for c, v in zip(coef, sv):
        d2 = 0.0
        for j in range(len(x)):
            d2 += (x[j] - v[j]) ** 2
        y += c * math.exp(-gamma * d2)
    y -= rho
    s = (y - intercepts[0]) / slopes[0]
    if clip is not None:
        s = min(max(s, clip[0]), clip[1])
    return s


def predict(features, slopes, intercepts, clip, gamma, rho, coef, sv):
    return [predict_one(list(f), slopes, intercepts, clip, gamma, rho, coef, sv) for f in features]


def libsvm_text(gamma, rho, coef, sv, svm_type="nu_svr", kernel_type="rbf", nr_class=True, sparse=True):
    """libsvm's text model; sparse: zero components are left out (the indices stay 1-based and ascending)"""
    lines = ["svm_type %s" % svm_type, "kernel_type %s" % kernel_type, "gamma %r" % float(gamma)]
    if nr_class:
        lines.append("nr_class 2")
    lines += ["total_sv %d" % len(coef), "rho %r" % float(rho), "SV"]
    for c, v in zip(coef, sv):
        items = ["%d:%r" % (j + 1, float(x)) for j, x in enumerate(v) if not (sparse and float(x) == 0.0)]
        lines.append(" ".join(["%r" % float(c)] + items))
    return "\n".join(lines) + "\n"


def json_model(gamma, rho, coef, sv, slopes, intercepts, clip=None, features=FEATURES_V061, **extra):
    md = {"model_type": "LIBSVMNUSVR", "norm_type": "linear_rescale",
          "feature_names": ["VMAF_feature_%s_score" % f for f in features],
          "slopes": [float(x) for x in slopes], "intercepts": [float(x) for x in intercepts],
          "model": libsvm_text(gamma, rho, coef, sv)}
    if clip is not None:
        md["score_clip"] = [float(clip[0]), float(clip[1])]
    md.update(extra)
    return json.dumps({"model_dict": md}, indent=1)
