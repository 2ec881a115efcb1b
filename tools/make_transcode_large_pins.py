#!/usr/bin/env python3
"""Writes tests/golden/transcode_large_pins.json: length and SHA-256 of what tests/transcode_ref.transcode makes of the
large sources of tests/transcode_cases.large(), for every (source, options) pair of LARGE_PAIRS whose expected file is not
one of Pillow's own (the photos' progressive file and baseline twin are each other's expected files and need no pin).

The pins are the RESTATEMENT's output, not Pillow's: for the camera file (tests/golden/IMG_6510.JPG) no Pillow file of the
same coefficients exists -- re-encoding its pixels would quantise again. tests/test_transcode_ref.py recomputes every
entry but the camera file's two, over which the restatement takes half a minute: those are recomputed only here.

    python tools/make_transcode_large_pins.py          (no Pillow needed)
"""
import hashlib
import json
import os
import platform
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def entry(data):
    return dict(size=len(data), sha256=hashlib.sha256(data).hexdigest())


def main():
    from tests import transcode_cases as T
    from tests import transcode_ref as R

    if sys.argv[1:]:
        raise SystemExit(__doc__)
    files = T.large()
    pins = {}
    for source, label, options, expected in T.LARGE_PAIRS:
        t = time.time()
        out = R.transcode(files[source], **options)
        if expected is not None:  # Pillow's file: checked, not pinned
            assert out == files[expected], (source, label)
        else:
            pins["%s/%s" % (source, label)] = entry(out)
        print("%-16s %-12s %8d bytes  %5.1f s" % (source, label, len(out), time.time() - t))
    for name in ("photo", "photo_rst"):  # the two source kinds hold the same coefficients
        for label in ("plain", "row"):
            assert pins["%s/%s" % (name, label)] == pins["%s_twin/%s" % (name, label)], (name, label)
    doc = dict(versions=dict(python=platform.python_version(), numpy=np.__version__),
               sources={k: entry(v) for k, v in sorted(files.items())}, pins=pins)
    with open(T.LARGE_PINS, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%s: %d pins" % (T.LARGE_PINS, len(pins)))


if __name__ == "__main__":
    main()
