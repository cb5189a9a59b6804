#!/usr/bin/env python3
"""Writes tests/golden/scale_pins.json: Pillow's Image.resize on small planes, the pins of tests/test_scale_host.py.
The inputs are regenerated from the recorded seed (tests/scale_reference.pin_input); the outputs are Pillow's, zlib + base64.
Mode L for the three filters on ten geometries and two contents; mode I;16 (depth 16) for bicubic and lanczos on two, on
noise in the middle half of the range: where a pass overshoots, Pillow's 16-bit path saturates the HIGH byte only and lets the
low byte wrap (65536 + 3 is stored as 0xff03), which is no clip to compare a clip against.
Run from the repository root with Pillow installed: python scripts/gen_scale_pins.py"""
import base64
import json
import os
import sys
import zlib

import numpy as np
import PIL
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import scale_reference as sr  # noqa: E402

SEED = 20261020
# (in h, in w, out h, out w): up, down, odd sizes, one axis unchanged, 4x down, 8x up
GEOMETRIES_L = [(9, 16, 14, 24), (14, 24, 9, 16), (2, 3, 16, 24), (32, 48, 8, 12), (8, 11, 16, 22), (5, 7, 15, 21),
                (12, 24, 12, 16), (10, 13, 15, 13), (15, 12, 10, 19), (25, 35, 8, 11)]
GEOMETRIES_I16 = [(9, 16, 14, 24), (15, 12, 10, 19)]
RESAMPLE = {"bilinear": Image.Resampling.BILINEAR, "bicubic": Image.Resampling.BICUBIC, "lanczos": Image.Resampling.LANCZOS}


def main():
    cases = []
    for mode, depth, geos, filters in (("L", 8, GEOMETRIES_L, sr.FILTERS), ("I;16", 16, GEOMETRIES_I16, ("bicubic", "lanczos"))):
        for h, w, oh, ow in geos:
            for filt in filters:
                for content in (("noise", "binary") if mode == "L" else ("midnoise",)):
                    a = sr.pin_input(SEED, len(cases), h, w, content, depth)
                    out = np.asarray(Image.fromarray(a).resize((ow, oh), RESAMPLE[filt]))
                    assert out.shape == (oh, ow) and out.dtype == a.dtype
                    cases.append({"mode": mode, "depth": depth, "filter": filt, "content": content, "in": [h, w], "out": [oh, ow],
                                  "data": base64.b64encode(zlib.compress(out.astype("<u%d" % a.itemsize).tobytes(), 9)).decode()})
    doc = {"tool": "Pillow %s Image.resize" % PIL.__version__, "seed": SEED, "cases": cases}
    path = os.path.join(ROOT, "tests", "golden", "scale_pins.json")
    with open(path, "w") as f:
        f.write('{"tool": %s, "seed": %d, "cases": [\n' % (json.dumps(doc["tool"]), SEED))   # one case a line
        f.write(",\n".join(json.dumps(c) for c in cases))
        f.write("\n]}\n")
    print("%d cases -> %s (%d bytes)" % (len(cases), path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
