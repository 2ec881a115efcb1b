"""Writes tests/golden/slow_sync_pins.json: for every file of tests/cases.slow_sync(), the SHA-256 of its bytes and of
what Pillow (its bundled libjpeg-turbo) decodes from it, after checking that this equals the numpy restatement of
libjpeg (tests/libjpeg_ref.py) applied to the CPU oracle's coefficients. tests/test_slow_sync_host.py then checks the
corpus against the pins without Pillow.

    python tools/make_slow_sync_pins.py

One- and three-component files: np.asarray(Image.open(f).convert("RGB")). The four-component file is CMYK to Pillow,
which hands out the inverted samples: 255 - np.asarray(im) must equal the restatement's planes, fancy-upsampled to
the image size; the planes are pinned."""
import hashlib
import io
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import oracle  # noqa: E402
from tests import cases, libjpeg_ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "slow_sync_pins.json")


def sha256(b):
    return hashlib.sha256(np.ascontiguousarray(b).tobytes() if isinstance(b, np.ndarray) else b).hexdigest()


def main():
    from PIL import Image

    pins = {}
    for name, case in cases.slow_sync().items():
        dec = oracle.decode(case.data)
        pin = {"jpeg_sha256": sha256(case.data)}
        if dec.ncomp in (1, 3):
            want = libjpeg_ref.libjpeg_rgb_of(dec)
            got = libjpeg_ref.pillow_rgb(case.data)
            assert np.array_equal(got, want), name
            pin["rgb_sha256"] = sha256(got)
        else:
            im = Image.open(io.BytesIO(case.data))
            im.load()
            assert im.mode == "CMYK" and im.size == (dec.width, dec.height), name
            planes = libjpeg_ref.islow_planes_of(dec)
            got = np.asarray(im)
            for c in range(dec.ncomp):
                up = libjpeg_ref.upsample_fancy(planes[c], max(dec.hs) // dec.hs[c], max(dec.vs) // dec.vs[c], dec.width, dec.height)
                assert np.array_equal(255 - got[:, :, c], up), (name, c)
            pin["planes_sha256"] = [sha256(p) for p in planes]
        pins[name] = pin
        print(name, "ok")
    with open(OUT, "w") as f:
        json.dump(pins, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
