#!/usr/bin/env python3
"""Freeze what the two entry points of video_processing do with the six pre-passes - which frame_* call sees which frames, in
which order, what stream.run is handed, which keys the log and the row gain - into tests/golden/prepass_trace.json.

The file was written ONCE, by commit f21e14170dd34e3fcba20a3c4923086f4315e5a7: the last one in which run_ffmpeg_metrics and
process_video_and_extract_metrics each carried the chain of pre-passes written out by hand.  tests/test_prepass_chain_host.py
compares the one chain that replaced them against it.  Both sides run the same stand-ins, tests/prepass_chain_cases.py: no
device is touched.  Re-run only when the chain changes on purpose:  python oracle/gen_prepass_trace.py

The cases: sync off / on / applied x light x align x shift x colorfit x conform off / "none" / "match" / "matrix", through both
entry points, over clips of 12 and 10 frames and, where nothing is trimmed, of 10 and 10 (prepass_chain_cases.cases); a combination
the request parser refuses is recorded with its message.  The file holds every distinct call, log value and error once
(prepass_chain_cases.pack).
"""
import logging
import os
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

import prepass_chain_cases as PC  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "prepass_trace.json")


def main():
    commit = subprocess.check_output(["git", "-C", REPO, "rev-parse", "HEAD"]).decode().strip()
    traces = []
    logging.disable(logging.WARNING)   # (what the pre-passes found is a warning each, a few thousand in all)
    with tempfile.TemporaryDirectory() as tmp:
        for counts, kw in PC.cases():
            traces.append({entry: PC.trace(entry, kw, tmp, setattr, counts) for entry in PC.ENTRY_POINTS})
    assert PC.unpack(PC.pack(traces)) == traces
    with open(OUT, "w") as f:
        PC.dump(dict(PC.pack(traces), commit=commit), f)
    print("wrote %s at %s: %d cases, %d bytes" % (OUT, commit, len(traces), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
