#!/usr/bin/env python3
"""Writes tests/golden/transcode_frame_pins.npz: for every source of tests/transcode_frame_cases.sources() the files Pillow
(on libjpeg-turbo) writes for its pixels with each kind of options -- S_<name>-<kind>, where kind A is the source of the
transcode and the others what the transcode with those options has to be. And for oriented() the source O_<name>-1 and
Pillow's files of the turned pixels O_<name>-<o>, o = 2..8.

    python tools/make_transcode_frame_pins.py
"""
import io
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import PIL
    from PIL import Image, features

    from tests import transcode_frame_cases as K
    from tests import transcode_orient_ref as X

    if not features.check_feature("libjpeg_turbo"):
        raise SystemExit("the pins are libjpeg-turbo's: this Pillow is built on another libjpeg")
    if sys.argv[1:]:
        raise SystemExit(__doc__)
    versions = dict(pillow=PIL.__version__, libjpeg_turbo=features.version_feature("libjpeg_turbo"), jpeglib=features.version("jpg"))

    def save(img, mode, params, **more):
        f = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(img), mode).save(f, "JPEG", **params, **more)
        return np.frombuffer(f.getvalue(), np.uint8)

    out = {}
    for name, (img, mode, params) in K.sources().items():
        for kind, more in K.KINDS.items():
            out["S_%s-%s" % (name, kind)] = save(img, mode, params, **more)
    for name, (img, mode, params) in K.oriented().items():
        for o in range(1, 9):
            out["O_%s-%d" % (name, o)] = save(X.orient_pixels(img, o), mode, params)
    out["meta"] = np.frombuffer(json.dumps(versions).encode(), np.uint8)
    np.savez_compressed(K.GOLDEN, **out)
    print("%s: %d files, %d bytes" % (K.GOLDEN, len(out) - 1, os.path.getsize(K.GOLDEN)))


if __name__ == "__main__":
    main()
