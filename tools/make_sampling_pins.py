"""Writes tests/golden/sampling_pins.json: for every file of tests/cases.sampling_sweep(), the SHA-256 of its bytes and of
what Pillow (its bundled libjpeg-turbo) decodes from it, after checking that this equals the numpy restatement of
libjpeg (tests/libjpeg_ref.py) applied to the CPU oracle's coefficients. tests/test_sampling_host.py then checks the
corpus against the pins without Pillow.

    python tools/make_sampling_pins.py

Integral one- and three-component files: np.asarray(Image.open(f).convert("RGB")) ("rgb_sha256"). The four-component
file is CMYK to Pillow, which hands out the inverted samples: 255 - np.asarray(im) must equal the restatement's planes,
fancy-upsampled to the image size. Every other file that the oracle decodes has its ISLOW planes pinned
("planes_sha256"). A file Pillow cannot open or decode is pinned as "pillow": "refused"."""
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

OUT = os.path.join(ROOT, "tests", "golden", "sampling_pins.json")


def sha256(b):
    return hashlib.sha256(np.ascontiguousarray(b).tobytes() if isinstance(b, np.ndarray) else b).hexdigest()


def pillow_image(data):
    """The decoded PIL image, or None where Pillow refuses the file."""
    from PIL import Image, UnidentifiedImageError

    try:
        im = Image.open(io.BytesIO(data))
        im.load()
        return im
    except (OSError, UnidentifiedImageError):
        return None


def main():
    pins = {}
    for name, data in cases.sampling_sweep().items():
        pin = {"jpeg_sha256": sha256(data)}
        im = pillow_image(data)
        if im is None:
            pin["pillow"] = "refused"
        if cases.sweep_is_refused(name):
            assert im is None, name
            pins[name] = pin
            print(name, "refused")
            continue
        dec = oracle.decode(data)
        if not cases.sweep_is_planes_only(name):
            assert dec.ncomp in (1, 3) and im is not None, name
            want = libjpeg_ref.libjpeg_rgb_of(dec)
            got = np.asarray(im.convert("RGB"))
            assert np.array_equal(got, want), name
            pin["rgb_sha256"] = sha256(got)
        else:
            planes = libjpeg_ref.islow_planes_of(dec)
            if dec.ncomp == 4:
                assert im is not None and im.mode == "CMYK" and im.size == (dec.width, dec.height), name
                got = np.asarray(im)
                for c in range(dec.ncomp):
                    up = libjpeg_ref.upsample_fancy(planes[c], max(dec.hs) // dec.hs[c], max(dec.vs) // dec.vs[c], dec.width, dec.height)
                    assert np.array_equal(255 - got[:, :, c], up), (name, c)
            else:
                assert im is None, name
            pin["planes_sha256"] = [sha256(p) for p in planes]
        pins[name] = pin
        print(name, "ok")
    with open(OUT, "w") as f:
        json.dump(pins, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
