#!/usr/bin/env python3
"""Writes tests/golden/encode_pins.npz: what Pillow (on libjpeg-turbo) makes of every case of tests/encode_cases.py with
Image.fromarray(a).save(f, "JPEG", quality=, subsampling=, restart_marker_blocks=). Files of up to WHOLE_FILE_LIMIT bytes are
stored whole, larger ones as length and SHA-256. The tests read the pins and never import Pillow.

    python tools/make_encode_pins.py
"""
import hashlib
import io
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

WHOLE_FILE_LIMIT = 4096
PILLOW_SUBSAMPLING = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}


def main():
    import PIL
    from PIL import Image, features

    import encode_cases

    if not features.check_feature("libjpeg_turbo"):
        raise SystemExit("the pins are libjpeg-turbo's: this Pillow is built on another libjpeg")
    out, index = {}, []
    for case in encode_cases.cases():
        f = io.BytesIO()
        Image.fromarray(encode_cases.image(case)).save(f, "JPEG", quality=case["quality"], subsampling=PILLOW_SUBSAMPLING[case["subsampling"]],
                                                        restart_marker_blocks=case["restart_interval"])
        data = f.getvalue()
        entry = dict(name=case["name"], length=len(data), sha256=hashlib.sha256(data).hexdigest(), whole=len(data) <= WHOLE_FILE_LIMIT)
        if entry["whole"]:
            out["file_" + case["name"]] = np.frombuffer(data, np.uint8)
        index.append(entry)
    meta = dict(pillow=PIL.__version__, libjpeg_turbo=features.version_feature("libjpeg_turbo"), jpeglib=features.version("jpg"), cases=index)
    out["meta"] = np.frombuffer(json.dumps(meta).encode(), np.uint8)
    path = os.path.join(ROOT, "tests", "golden", "encode_pins.npz")
    np.savez_compressed(path, **out)
    print("%s: %d cases, %d whole files, %d bytes" % (path, len(index), sum(e["whole"] for e in index), os.path.getsize(path)))


if __name__ == "__main__":
    main()
