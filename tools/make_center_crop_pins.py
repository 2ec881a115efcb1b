"""Writes tests/golden/center_crop_pins.npz: what Pillow makes of torchvision's Resize + CenterCrop, so that
tests/test_center_crop_host.py and tests/test_gpu_center_crop.py can check the restatement (tests/center_crop_ref.py) and
jpeggpu_ext_resize_view_to_tensor without Pillow.

    python tools/make_center_crop_pins.py

The pipeline is Pillow's alone: im = Image.open(f) (after im.draft("RGB", (W // d, H // d)) for a scale d > 1)
.convert("RGB").resize((rw, rh), filter).crop((x, y, x + cw, y + ch)) -- Image.crop fills what lies outside the image with
zeros, which is CenterCrop's padding. (rw, rh) and (x, y) come from tests/center_crop_ref.py, the contract's two rules.
Inputs: the small Pillow-encoded files of tests/golden/libjpeg_pins.npz (jpeg/<name>), tests/cases.matrix()["ss_2x1"] and
tests/golden/IMG_6510.JPG ("photo").
Arrays: out/<name>/<d>/<resize>/<ch>x<cw>/<filter>, or out_sha256/... (the SHA-256 of that array in C order) when it has
more than 256 pixels; <resize> is the int of Resize(int).
"""
import hashlib
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import center_crop_ref as CC  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "center_crop_pins.npz")
MAX_PINNED_PIXELS = 256
FILTERS = ("bilinear", "bicubic")
SMALL_CASES = ((24, (16, 16)), (48, (40, 40)), (32, (40, 40)), (20, (12, 30)))  # (resize, (ch, cw)): down, up, padded, odd
MATRIX_CASES = (("ss_2x1", 8, 48, (40, 40)), ("ss_2x1", 1, 64, (37, 37)))  # (name, d, resize, crop)
PHOTO_CASES = ((1, 256, (224, 224)), (8, 256, (224, 224)))  # (d, resize, crop)


def sha256(a):
    return np.array(hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest())


def key(name, d, resize, crop, filt):
    return "%s/%d/%d/%dx%d/%s" % (name, d, resize, crop[0], crop[1], filt)


def pillow_center_crop(im, resize, crop, f):
    ch, cw = crop
    rw, rh = CC.resized_size(im.size[0], im.size[1], resize)
    x, y = CC.center_crop_window(rw, rh, cw, ch)
    return np.asarray(im.resize((rw, rh), f).crop((x, y, x + cw, y + ch)))


def opened(data, d):
    from PIL import Image

    im = Image.open(io.BytesIO(data))
    if d != 1:
        im.draft("RGB", (im.size[0] // d, im.size[1] // d))
    return im.convert("RGB")


def main():
    from PIL import Image

    from tests import cases

    res = {"bilinear": Image.Resampling.BILINEAR, "bicubic": Image.Resampling.BICUBIC}
    arrays = {}

    def pin(name, d, im, resize, crop):
        for filt in FILTERS:
            a = pillow_center_crop(im, resize, crop, res[filt])
            assert a.shape == (crop[0], crop[1], 3)
            kind = "out/" if crop[0] * crop[1] <= MAX_PINNED_PIXELS else "out_sha256/"
            arrays[kind + key(name, d, resize, crop, filt)] = a if kind == "out/" else sha256(a)

    pins = np.load(os.path.join(ROOT, "tests", "golden", "libjpeg_pins.npz"))
    for k in pins.files:
        if k.startswith("jpeg/"):
            for resize, crop in SMALL_CASES:
                pin(k[len("jpeg/"):], 1, opened(pins[k].tobytes(), 1), resize, crop)
    matrix = cases.matrix()
    for name, d, resize, crop in MATRIX_CASES:
        pin(name, d, opened(matrix[name], d), resize, crop)
    with open(os.path.join(ROOT, "tests", "golden", "IMG_6510.JPG"), "rb") as f:
        photo = f.read()
    for d, resize, crop in PHOTO_CASES:
        pin("photo", d, opened(photo, d), resize, crop)
    np.savez_compressed(OUT, **arrays)
    print("%s: %d arrays, %d bytes" % (OUT, len(arrays), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
