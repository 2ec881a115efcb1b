#!/usr/bin/env python3
"""Writes tests/golden/coefficients_pins.npz: for every case of tests/coefficients_ref.cases() the files Pillow (on
libjpeg-turbo) writes for the case's pixels with Image.fromarray(a).save(f, "JPEG", quality=, subsampling=) -- A as it
stands, B with optimize=True, C with progressive=True -- and the SHA-256 of each component's expected coefficient tensor
(tests/coefficients_ref.read of A: int16 [blocks_y, blocks_x, 64] over the real grid). The files lie end to end in one
array, which compresses their common headers; the tests read the pins and never need Pillow to have them.

    python tools/make_coefficients_pins.py
"""
import io
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PILLOW_SUBSAMPLING = {"grey": 0, "4:4:4": 0, "4:2:2": 1, "4:2:0": 2}


def main():
    import PIL
    from PIL import Image, ImageFile, features

    from tests import coefficients_ref as K

    if not features.check_feature("libjpeg_turbo"):
        raise SystemExit("the pins are libjpeg-turbo's: this Pillow is built on another libjpeg")
    if sys.argv[1:]:
        raise SystemExit(__doc__)
    ImageFile.MAXBLOCK = 1 << 24  # (an optimised or progressive file leaves libjpeg at once)
    versions = dict(pillow=PIL.__version__, libjpeg_turbo=features.version_feature("libjpeg_turbo"), jpeglib=features.version("jpg"))
    blob, index = bytearray(), {}
    for case in K.cases():
        img, entry = K.image(case), dict(files={})
        for kind, more in K.KINDS.items():
            f = io.BytesIO()
            Image.fromarray(img).save(f, "JPEG", quality=case["quality"], subsampling=PILLOW_SUBSAMPLING[case["sampling"]], **more)
            entry["files"][kind] = (len(blob), len(blob) + len(f.getvalue()))
            blob += f.getvalue()
        first = entry["files"]["A"]
        entry["sha"] = [K.sha(c) for c in K.read(bytes(blob[first[0]:first[1]])).coef]
        index[case["name"]] = entry
    path = os.path.join(ROOT, "tests", "golden", "coefficients_pins.npz")
    np.savez_compressed(path, files=np.frombuffer(bytes(blob), np.uint8), meta=np.frombuffer(json.dumps(dict(versions=versions, cases=index)).encode(), np.uint8))
    print("%s: %d cases, %d bytes of files, %d bytes" % (path, len(index), len(blob), os.path.getsize(path)))


if __name__ == "__main__":
    main()
