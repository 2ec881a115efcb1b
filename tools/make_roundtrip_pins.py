#!/usr/bin/env python3
"""Writes tests/golden/roundtrip_pins.npz: what Pillow (on libjpeg-turbo) makes of every case of tests/roundtrip_ref.cases()
with  Image.fromarray(a).save(buf, "JPEG", quality=, subsampling=)  and then  np.asarray(Image.open(buf)).

    cases      int64 [n, 7]: width, height, channels, pattern index, subsampling index, quality, seed (roundtrip_ref.case_table)
    sha256     uint8 [n, 32]: the SHA-256 of every output
    small      uint8: the outputs of the cases of at most roundtrip_ref.STORED_PIXELS pixels, one after the other
    small_off  int64 [n + 1]: case i's output is small[small_off[i]:small_off[i + 1]] (empty for a larger case)
    meta       JSON: the versions of Pillow and libjpeg-turbo

The tests read the pins and never import Pillow.

    python tools/make_roundtrip_pins.py
"""
import hashlib
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

    from tests import roundtrip_ref as R

    if not features.check_feature("libjpeg_turbo"):
        raise SystemExit("the pins are libjpeg-turbo's: this Pillow is built on another libjpeg")
    cases = R.cases()
    sha, small, off = [], [], [0]
    for case in cases:
        _, w, h, ch, _, ss, q, _ = case
        buf = io.BytesIO()
        Image.fromarray(R.case_input(case)).save(buf, "JPEG", quality=q, subsampling=R.SUBSAMPLINGS.index(ss))
        got = np.asarray(Image.open(io.BytesIO(buf.getvalue())))
        assert got.dtype == np.uint8 and got.shape == ((h, w) if ch == 1 else (h, w, 3)), case
        sha.append(np.frombuffer(hashlib.sha256(np.ascontiguousarray(got).tobytes()).digest(), np.uint8))
        if w * h <= R.STORED_PIXELS:
            small.append(got.ravel())
        off.append(off[-1] + (got.size if w * h <= R.STORED_PIXELS else 0))
    meta = dict(pillow=PIL.__version__, libjpeg_turbo=features.version_feature("libjpeg_turbo"), jpeglib=features.version("jpg"))
    path = os.path.join(ROOT, "tests", "golden", "roundtrip_pins.npz")
    np.savez_compressed(path, cases=R.case_table(cases), sha256=np.stack(sha), small=np.concatenate(small), small_off=np.array(off, np.int64),
                        meta=np.frombuffer(json.dumps(meta).encode(), np.uint8))
    print("%s: %d cases, %d stored as arrays, %d bytes" % (path, len(cases), len(small), os.path.getsize(path)))


if __name__ == "__main__":
    main()
