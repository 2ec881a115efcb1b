#!/usr/bin/env python3
"""Writes tests/golden/transcode_pins.npz: for every case of tests/transcode_cases.cases() the files Pillow (on
libjpeg-turbo) writes for the case's pixels with Image.fromarray(a).save(f, "JPEG", quality= | qtables=, subsampling=,
restart_marker_blocks=) -- A as it stands, B with optimize=True, C with progressive=True and, where the case names
`restart_to`, R with that restart interval. All files are stored whole: they are the sources of the transcode tests as
well as what those expect, and the tests never need Pillow.

    python tools/make_transcode_pins.py
"""
import io
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PILLOW_SUBSAMPLING = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}


def save(Image, img, case, restart, **more):
    f = io.BytesIO()
    params = dict(subsampling=case["grey_subsampling"] if case["sampling"] == "grey" else PILLOW_SUBSAMPLING[case["sampling"]], restart_marker_blocks=restart)
    if case["quality"]:
        params["quality"] = case["quality"]
    else:
        params["qtables"] = case["qtables"][:1 if case["sampling"] == "grey" else 2]
    Image.fromarray(img).save(f, "JPEG", **params, **more)
    return f.getvalue()


def main():
    import PIL
    from PIL import Image, ImageFile, features

    from tests import transcode_cases

    if not features.check_feature("libjpeg_turbo"):
        raise SystemExit("the pins are libjpeg-turbo's: this Pillow is built on another libjpeg")
    if sys.argv[1:]:
        raise SystemExit(__doc__)
    ImageFile.MAXBLOCK = 1 << 24  # (an optimised or progressive file leaves libjpeg at once)
    versions = dict(pillow=PIL.__version__, libjpeg_turbo=features.version_feature("libjpeg_turbo"), jpeglib=features.version("jpg"))
    out, names = {}, []
    for case in transcode_cases.cases():
        img, name, r = transcode_cases.image(case), case["name"], case["restart_interval"]
        files = dict(A=save(Image, img, case, r), B=save(Image, img, case, r, optimize=True), C=save(Image, img, case, r, progressive=True))
        if case["restart_to"] is not None:
            files["R"] = save(Image, img, case, case["restart_to"])
        for k, data in files.items():
            out["%s_%s" % (k, name)] = np.frombuffer(data, np.uint8)
        names.append(name)
    out["meta"] = np.frombuffer(json.dumps(dict(versions, cases=names)).encode(), np.uint8)
    path = os.path.join(ROOT, "tests", "golden", "transcode_pins.npz")
    np.savez_compressed(path, **out)
    print("%s: %d cases, %d files, %d bytes" % (path, len(names), len(out) - 1, os.path.getsize(path)))


if __name__ == "__main__":
    main()
