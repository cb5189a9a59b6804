#!/usr/bin/env python3
"""Freeze what video_processing.write_vif_log writes and what extract_metrics_from_logs reads back, for seeded records of every
plane-batch kind, into tests/golden/feature_logs.json.

These pin the LOG'S AND THE ROW'S LAYOUT - which keys, in which order, under which cap, which pooled statistic in which
column - not any metric: the records are random numbers.  The file was written ONCE, by the commit before the feature table
(video_processing.FEATURES) replaced the per-kind chains, so tests/test_feature_table_host.py compares the table against the
code it replaced.  Re-run only when the log or the row changes on purpose:  python oracle/gen_feature_logs.py

The cases: every kind at once ("all"), every kind alone (under write_vif_log's keyword for it), and vif + adm + motion with a
small VMAF model ("vmaf").  The model's gamma is 0, so every kernel value is exp(-0) = 1 and the score is sum(coef) - rho in
exact arithmetic: the text does not depend on how a machine's exp() rounds.
"""
import json
import os
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from rtvqa_amd import engine, stream, vmaf_model  # noqa: E402
from rtvqa_amd import video_processing as vp  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "feature_logs.json")
FRAMES = 3
# write_vif_log's keyword -> the dtype of the records it takes, in the order of stream.PLANE_KINDS
DTYPES = (("vif", engine.VIF_DTYPE), ("adm", engine.ADM_DTYPE), ("motion", stream.MOTION_PASS_DTYPE), ("siti", engine.SITI_DTYPE),
          ("psnr_hvs", engine.PSNR_HVS_DTYPE), ("ciede", engine.CIEDE_DTYPE), ("gmsd", engine.GMSD_DTYPE),
          ("cambi", engine.CAMBI_DTYPE), ("xpsnr", engine.XPSNR_DTYPE), ("haarpsi", engine.HAARPSI_DTYPE), ("vca", engine.VCA_DTYPE),
          ("artifacts", engine.ARTIFACTS_DTYPE), ("brisque", engine.BRISQUE_DTYPE), ("mdsi", engine.MDSI_DTYPE),
          ("delta_itp", engine.ITP_DTYPE), ("pu21", engine.PU21_DTYPE), ("fsim", engine.FSIM_DTYPE),
          ("sigstats", engine.SIGSTATS_DTYPE))
# one infinity each, so that the caps are exercised: (keyword, field, frame)
INFINITE = (("psnr_hvs", "psnr_hvs", 0), ("ciede", "ciede2000", 1), ("xpsnr", "xpsnr", 2), ("pu21", "pu_psnr", 0))


def records():
    """keyword -> [FRAMES] seeded records: integer fields small integers, float fields finite uniforms (RandomState: a frozen
    stream, the same numbers under every NumPy)"""
    rng = np.random.RandomState(20261020)
    out = {}
    for name, dtype in DTYPES:
        rec = np.zeros(FRAMES, dtype)
        for field in dtype.names:
            shape = rec[field].shape
            if rec[field].dtype.kind == "f":
                rec[field] = rng.uniform(0.0625, 60.0, shape)
            else:
                rec[field] = rng.randint(0, 100, shape)
        out[name] = rec
    out["sigstats"]["count"] = rng.randint(1000, 2000, FRAMES)
    for name, field, frame in INFINITE:
        out[name][field][frame] = np.inf
    return out


def model():
    k = len(vmaf_model.FEATURES_V061)
    sv = np.arange(3 * k, dtype=np.float64).reshape(3, k) / 8.0
    return vmaf_model.VmafModel(vmaf_model.FEATURES_V061, np.ones(1 + k), np.zeros(1 + k), (0.0, 100.0), 0.0, -4.0,
                                [30.5, 20.25, 10.125], sv)


def cases():
    """case name -> write_vif_log's keyword arguments"""
    rec = records()
    rec["scale"] = rec.pop("vif")["scale"]     # write_vif_log takes VIF's [n, 4] array, under `scale`
    out = {"all": dict(rec)}
    for name in rec:
        out[name] = {name: rec[name]}
    out["vmaf"] = {k: rec[k] for k in ("scale", "adm", "motion")}
    out["vmaf"]["model"] = model()
    return out


def render(kwargs, tmp):
    """-> (the log's text, the row as a list of [column, value])"""
    psnr_log, ssim_log, vmaf_log = (os.path.join(tmp, n) for n in ("psnr.log", "ssim.log", "vmaf.json"))
    with open(psnr_log, "w") as f:
        f.write("n:1 mse_avg:1.00 psnr_avg:48.13 \n")
    with open(ssim_log, "w") as f:
        f.write("n:1 Y:0.990000 All:0.990000 (20.000000)\n")
    vp.write_vif_log(vmaf_log, **kwargs)
    with open(vmaf_log, newline="") as f:
        text = f.read()
    row = vp.extract_metrics_from_logs(psnr_log, ssim_log, vmaf_log, "x", 23, 1000, "64x64", 30.0)
    return text, [[k, v] for k, v in row.items()]


def main():
    doc = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, kwargs in cases().items():
            text, row = render(kwargs, tmp)
            doc[name] = {"log": text, "row": row}
    with open(OUT, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print("wrote %s: %d cases, %d bytes" % (OUT, len(doc), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
