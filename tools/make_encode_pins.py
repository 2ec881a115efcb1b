#!/usr/bin/env python3
"""Writes tests/golden/encode_pins.npz: what Pillow (on libjpeg-turbo) makes of every case of tests/encode_cases.py with
Image.fromarray(a).save(f, "JPEG", quality=, subsampling=, restart_marker_blocks=). Files of up to WHOLE_FILE_LIMIT bytes are
stored whole, larger ones as length and SHA-256. The tests read the pins and never import Pillow.

    python tools/make_encode_pins.py            # encode_pins.npz: encode_cases.cases()
    python tools/make_encode_pins.py --sweep    # only encode_sweep_pins.npz: encode_cases.new_cases(), every file by length and
                                                # SHA-256; the versions must be those encode_pins.npz records
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
    only_sweep = sys.argv[1:] == ["--sweep"]
    if sys.argv[1:] and not only_sweep:
        raise SystemExit(__doc__)
    versions = dict(pillow=PIL.__version__, libjpeg_turbo=features.version_feature("libjpeg_turbo"), jpeglib=features.version("jpg"))
    if only_sweep and versions != encode_cases.pins()[1]:
        raise SystemExit("encode_pins.npz was written by %s, this is %s: the two files must come from the same libraries" % (encode_cases.pins()[1], versions))
    whole_file_limit = 0 if only_sweep else WHOLE_FILE_LIMIT
    out, index = {}, []
    for case in encode_cases.new_cases() if only_sweep else encode_cases.cases():
        f = io.BytesIO()
        Image.fromarray(encode_cases.image(case)).save(f, "JPEG", quality=case["quality"], subsampling=PILLOW_SUBSAMPLING[case["subsampling"]],
                                                        restart_marker_blocks=case["restart_interval"])
        data = f.getvalue()
        entry = dict(name=case["name"], length=len(data), sha256=hashlib.sha256(data).hexdigest(), whole=len(data) <= whole_file_limit)
        if entry["whole"]:
            out["file_" + case["name"]] = np.frombuffer(data, np.uint8)
        index.append(entry)
    meta = dict(versions, cases=index)
    out["meta"] = np.frombuffer(json.dumps(meta).encode(), np.uint8)
    path = os.path.join(ROOT, "tests", "golden", "encode_sweep_pins.npz" if only_sweep else "encode_pins.npz")
    np.savez_compressed(path, **out)
    print("%s: %d cases, %d whole files, %d bytes" % (path, len(index), sum(e["whole"] for e in index), os.path.getsize(path)))


if __name__ == "__main__":
    main()
