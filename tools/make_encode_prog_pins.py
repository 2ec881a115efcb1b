#!/usr/bin/env python3
"""Writes tests/golden/encode_prog_pins.npz: what Pillow (on libjpeg-turbo) makes of every case of tests/encode_cases.cases()
and of tests/encode_prog_ref.edge_cases() with Image.fromarray(a).save(f, "JPEG", quality=, subsampling=,
restart_marker_blocks=, progressive=True). The format is encode_opt_pins.npz's: files of up to WHOLE_FILE_LIMIT bytes are
stored whole, larger ones as length and SHA-256, beside the versions of the libraries. The tests read the pins and never need
Pillow.

    python tools/make_encode_prog_pins.py
"""
import hashlib
import io
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WHOLE_FILE_LIMIT = 4096
PILLOW_SUBSAMPLING = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}


def main():
    import PIL
    from PIL import Image, ImageFile, features

    from tests import encode_cases, encode_prog_ref

    if not features.check_feature("libjpeg_turbo"):
        raise SystemExit("the pins are libjpeg-turbo's: this Pillow is built on another libjpeg")
    if sys.argv[1:]:
        raise SystemExit(__doc__)
    # a progressive file leaves libjpeg at once, as an optimised one does, and Pillow's buffer for it is too small for noise
    # at quality 97, 4:4:4 ("broken data stream")
    ImageFile.MAXBLOCK = 1 << 24
    versions = dict(pillow=PIL.__version__, libjpeg_turbo=features.version_feature("libjpeg_turbo"), jpeglib=features.version("jpg"))
    out, index = {}, []
    todo = [(c, encode_cases.image(c)) for c in encode_cases.cases()] + encode_prog_ref.edge_cases()
    for case, img in todo:
        f = io.BytesIO()
        Image.fromarray(img).save(f, "JPEG", quality=case["quality"], subsampling=PILLOW_SUBSAMPLING[case["subsampling"]],
                                  restart_marker_blocks=case["restart_interval"], progressive=True)
        data = f.getvalue()
        entry = dict(name=case["name"], length=len(data), sha256=hashlib.sha256(data).hexdigest(), whole=len(data) <= WHOLE_FILE_LIMIT)
        if entry["whole"]:
            out["file_" + case["name"]] = np.frombuffer(data, np.uint8)
        index.append(entry)
    out["meta"] = np.frombuffer(json.dumps(dict(versions, cases=index)).encode(), np.uint8)
    path = os.path.join(ROOT, "tests", "golden", "encode_prog_pins.npz")
    np.savez_compressed(path, **out)
    print("%s: %d cases, %d whole files, %d bytes" % (path, len(index), sum(e["whole"] for e in index), os.path.getsize(path)))


if __name__ == "__main__":
    main()
