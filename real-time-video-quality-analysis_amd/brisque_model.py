"""The BRISQUE score from the 36 features of include/vqa.h (vqa_brisque_submit): libsvm's epsilon-SVR with an RBF kernel over
features that svm-scale has rescaled linearly - on the host, in float64, through vmaf_model's parser and predictor.

Two files make a model:
  model   libsvm's text model (svm_type epsilon_svr or nu_svr, kernel_type rbf), read with vmaf_model.parse_libsvm at 36 features
  range   svm-scale's range file:  a line `x`, a line `lower upper`, then lines `index min max` (index 1 .. 36; a feature without
          a line is left as it is).  x' = lower + (upper - lower)(f - min) / (max - min); a feature with max == min maps to lower.
The score is vmaf_model.predict over x', not clipped.  Anything malformed is a ValueError that names what was met.

No BRISQUE model ships with this project and none was at hand when this was written: the path is tested with models made by the
tests themselves, and the features feeding it are not pinned against the authors' MATLAB (README, "Parity")."""
import numpy as np

from . import vmaf_model

N_FEATURES = 36
FEATURE_NAMES = tuple("brisque_%02d" % k for k in range(N_FEATURES))


def parse_range(text, n_features=N_FEATURES):
    """svm-scale's range file -> (slopes [n], intercepts [n]) with x' = f * slope + intercept"""
    lines = [ln.strip() for ln in text.splitlines()]
    lines = [ln for ln in lines if ln]
    if not lines or lines[0] != "x":
        raise ValueError("range file: the first line must be 'x' (got %r)" % (lines[0] if lines else ""))
    if len(lines) < 2:
        raise ValueError("range file: no 'lower upper' line")
    parts = lines[1].split()
    try:
        if len(parts) != 2:
            raise ValueError
        lower, upper = float(parts[0]), float(parts[1])
    except ValueError:
        raise ValueError("range file: the second line must be 'lower upper' (got %r)" % lines[1])
    if not (np.isfinite(lower) and np.isfinite(upper)) or upper <= lower:
        raise ValueError("range file: lower and upper must be finite and lower < upper (got %r)" % lines[1])
    slopes, intercepts = np.ones(n_features, np.float64), np.zeros(n_features, np.float64)
    seen = set()
    for ln in lines[2:]:
        parts = ln.split()
        try:
            if len(parts) != 3:
                raise ValueError
            j, lo, hi = int(parts[0]), float(parts[1]), float(parts[2])
        except ValueError:
            raise ValueError("range file: cannot read the line %r as 'index min max'" % ln)
        if not 1 <= j <= n_features:
            raise ValueError("range file: index %d, the model has %d features" % (j, n_features))
        if j in seen:
            raise ValueError("range file: index %d twice" % j)
        if not (np.isfinite(lo) and np.isfinite(hi)) or hi < lo:
            raise ValueError("range file: min and max of index %d must be finite and min <= max (got %r)" % (j, ln))
        seen.add(j)
        if hi == lo:                         # svm-scale skips such a feature; here it maps to lower
            slopes[j - 1], intercepts[j - 1] = 0.0, lower
        else:
            slopes[j - 1] = (upper - lower) / (hi - lo)
            intercepts[j - 1] = lower - lo * slopes[j - 1]
    return slopes, intercepts


def load_model(model_path, range_path=None):
    """-> vmaf_model.VmafModel over FEATURE_NAMES, with the range file's slopes and intercepts (none: the features as they
    are) and no clip"""
    with open(model_path, "r") as f:
        gamma, rho, coef, sv = vmaf_model.parse_libsvm(f.read(), N_FEATURES)
    slopes, intercepts = np.ones(N_FEATURES), np.zeros(N_FEATURES)
    if range_path is not None:
        with open(range_path, "r") as f:
            slopes, intercepts = parse_range(f.read(), N_FEATURES)
    return vmaf_model.VmafModel(FEATURE_NAMES, np.concatenate([[1.0], slopes]), np.concatenate([[0.0], intercepts]), None,
                                gamma, rho, coef, sv)


def predict(model, features):
    """features [n, 36] (or [36]) -> scores [n], float64"""
    return vmaf_model.predict(model, features)
