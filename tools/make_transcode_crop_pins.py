#!/usr/bin/env python3
"""Writes tests/golden/transcode_crop_pins.npz: for every case of tests/transcode_crop_cases.pin_cases() the file Pillow (on
libjpeg-turbo) writes for the case's pixels -- S_<name>, the source of a cropped transcode -- and for every window of
transcode_crop_cases.windows() the file it writes for the cropped pixels with the same quality and subsampling, plain (A),
with optimize=True (B) or with progressive=True (C), one kind per window in turn: P_<name>-<window>-<kind>. And for
oriented_pin_cases(), whose sources are those of transcode_orient_pins.npz, Pillow's file of the rectangle of
Image.transpose of the (cut) cell image: O_<name>-<o>-<trim>-<x>_<y>_<w>_<h>-<kind>.

    python tools/make_transcode_crop_pins.py
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

    from tests import transcode_crop_cases as W
    from tests import transcode_orient_cases as K
    from tests import transcode_orient_ref as X

    if not features.check_feature("libjpeg_turbo"):
        raise SystemExit("the pins are libjpeg-turbo's: this Pillow is built on another libjpeg")
    if sys.argv[1:]:
        raise SystemExit(__doc__)
    ImageFile.MAXBLOCK = 1 << 24
    versions = dict(pillow=PIL.__version__, libjpeg_turbo=features.version_feature("libjpeg_turbo"), jpeglib=features.version("jpg"))

    def save(img, params, **more):
        f = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(img)).save(f, "JPEG", **params, **more)
        return np.frombuffer(f.getvalue(), np.uint8)

    out, names = {}, []
    for ci, case in enumerate(W.pin_cases()):
        img, params = W.image(case["w"], case["h"], case["sampling"], case["content"]), W.save_params(case["sampling"])
        out["S_" + case["name"]] = save(img, params)
        names.append(case["name"])
        for wi, (window, (x, y, w, h)) in enumerate(W.windows(case["w"], case["h"], *W.imcu(case["sampling"])).items()):
            kind = W.pin_kind(ci, wi)
            out["P_%s-%s-%s" % (case["name"], window, kind)] = save(img[y:y + h, x:x + w], params, **W.KINDS[kind])
    for n, (name, o, trim, (x, y, w, h)) in enumerate(W.oriented_pin_cases()):
        case = next(c for c in K.pin_cases() if c["name"] == name)
        size = K.allowed(case, o, trim)
        turned = X.orient_pixels(K.cell_image(case)[:size[1], :size[0]], o)
        kind = "ABC"[n % 3]
        out["O_%s-%d-%d-%d_%d_%d_%d-%s" % (name, o, trim, x, y, w, h, kind)] = save(turned[y:y + h, x:x + w], K.save_params(case), **W.KINDS[kind])
    out["meta"] = np.frombuffer(json.dumps(dict(versions, cases=names)).encode(), np.uint8)
    np.savez_compressed(W.GOLDEN, **out)
    print("%s: %d cases, %d files, %d bytes" % (W.GOLDEN, len(names), len(out) - 1, os.path.getsize(W.GOLDEN)))


if __name__ == "__main__":
    main()
