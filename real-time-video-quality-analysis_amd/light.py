"""HDR10 static metadata and gamut QC read off the records of Engine.light / video_processing.frame_light: pure host code.

records is [n] of engine.LIGHT_DTYPE (or any sequence of mappings with the same fields), one per frame: the integer words the
GPU formed and the doubles vqa_light_wait made of them (include/vqa.h, vqa_light_submit).  CTA-861.3: MaxCLL is the largest
max(R, G, B) of any pixel of the clip, MaxFALL the largest frame average of it, both in cd/m2 - as stated in the header, not
compared with any tool.  Shares are exact ratios of summed pixel counts, formed in Python integers and divided once."""

LIGHT_KEYS = ("LIGHT_MAXCLL", "LIGHT_MAXFALL", "LIGHT_MAXCLL_FRAME", "LIGHT_P9998", "LIGHT_Y_AVG", "LIGHT_OUT_709",
              "LIGHT_OUT_P3", "LIGHT_CLAMPED")
P9998 = 9   # pct_nits' index of the 99.98 % value
PEAK_NITS = 10000.0   # what a PQ signal can say


def summarise(records):
    """-> dict with LIGHT_KEYS, in that order: LIGHT_MAXCLL (the max over frames of max_nits), LIGHT_MAXFALL (the max of
    avg_nits), LIGHT_MAXCLL_FRAME (the first frame that reaches MaxCLL), LIGHT_P9998 (the max over frames of the 99.98 % value:
    the robust MaxCLL; a bin's lower edge), LIGHT_Y_AVG (the mean of y_avg), LIGHT_OUT_709, LIGHT_OUT_P3 and LIGHT_CLAMPED (the
    clip's pixel shares).  At least one record."""
    n = len(records)
    if not n:
        raise ValueError("records must hold at least one frame")
    max_nits = [float(r["max_nits"]) for r in records]
    cll = max(max_nits)
    pixels = sum(int(r["count"]) for r in records)
    if pixels <= 0:
        raise ValueError("records must count at least one pixel")

    def share(field):
        return sum(int(r[field]) for r in records) / pixels

    return {"LIGHT_MAXCLL": cll, "LIGHT_MAXFALL": max(float(r["avg_nits"]) for r in records),
            "LIGHT_MAXCLL_FRAME": max_nits.index(cll), "LIGHT_P9998": max(float(r["pct_nits"][P9998]) for r in records),
            "LIGHT_Y_AVG": sum(float(r["y_avg"]) for r in records) / n, "LIGHT_OUT_709": share("out_709"),
            "LIGHT_OUT_P3": share("out_p3"), "LIGHT_CLAMPED": share("clamped")}


def check(summary, peak=PEAK_NITS):
    """what cannot be: a MaxCLL above the table's peak (10000 cd/m2 for PQ), a MaxFALL above MaxCLL - a ValueError, since either
    is a bug and not a property of a clip"""
    if summary["LIGHT_MAXCLL"] > peak:
        raise ValueError("MaxCLL %r is above %r cd/m2" % (summary["LIGHT_MAXCLL"], peak))
    if summary["LIGHT_MAXFALL"] > summary["LIGHT_MAXCLL"]:
        raise ValueError("MaxFALL %r is above MaxCLL %r" % (summary["LIGHT_MAXFALL"], summary["LIGHT_MAXCLL"]))
    return summary
