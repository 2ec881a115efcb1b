#!/usr/bin/env python3
"""Writes tests/golden/transcode_orient_pins.npz: for every case of tests/transcode_orient_cases.pin_cases() the file Pillow
(on libjpeg-turbo) writes for the case's pixels -- S_<name>, the source of an oriented transcode -- and, for every
orientation 1..8 the rules allow, without and with `trim`, the files it writes for Image.transpose of the (cut) pixels,
plain (A), with optimize=True (B) and with progressive=True (C): P_<name>-<o>-<trim>-<kind>. An entry with trim 1 is
written only where the trim cuts something.

    python tools/make_transcode_orient_pins.py
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
    from PIL import Image, ImageFile, features

    from tests import transcode_orient_cases as K

    if not features.check_feature("libjpeg_turbo"):
        raise SystemExit("the pins are libjpeg-turbo's: this Pillow is built on another libjpeg")
    if sys.argv[1:]:
        raise SystemExit(__doc__)
    ImageFile.MAXBLOCK = 1 << 24
    versions = dict(pillow=PIL.__version__, libjpeg_turbo=features.version_feature("libjpeg_turbo"), jpeglib=features.version("jpg"))

    def save(im, params, **more):
        f = io.BytesIO()
        im.save(f, "JPEG", **params, **more)
        return f.getvalue()

    out, names = {}, []
    for case in K.pin_cases():
        img, params = K.cell_image(case), K.save_params(case)
        out["S_" + case["name"]] = np.frombuffer(save(Image.fromarray(img), params), np.uint8)
        names.append(case["name"])
        for o in range(1, 9):
            for trim in (False, True):
                size = K.allowed(case, o, trim)
                if size is None or (trim and size == (case["w"], case["h"])):
                    continue
                im = Image.fromarray(img[:size[1], :size[0]])
                if o != 1:
                    im = im.transpose(getattr(Image.Transpose, K.PIL_METHOD[o]))
                for kind, more in K.KINDS.items():
                    out["P_%s-%d-%d-%s" % (case["name"], o, trim, kind)] = np.frombuffer(save(im, params, **more), np.uint8)
    out["meta"] = np.frombuffer(json.dumps(dict(versions, cases=names)).encode(), np.uint8)
    np.savez_compressed(K.GOLDEN, **out)
    print("%s: %d cases, %d files, %d bytes" % (K.GOLDEN, len(names), len(out) - 1, os.path.getsize(K.GOLDEN)))


if __name__ == "__main__":
    main()
