"""Writes tests/golden/resize_pins.npz: what Pillow's Image.resize makes of crops of Pillow-decoded JPEGs, so that
tests/test_resize_host.py and tests/test_gpu_resize.py can check the restatement (tests/pillow_resample_ref.py) and
jpeggpu_ext_resize_to_rgb without Pillow.

    python tools/make_resize_pins.py

Inputs: the small Pillow-encoded files of tests/golden/libjpeg_pins.npz (jpeg/<name>) and tests/golden/IMG_6510.JPG.
Arrays: out/<name>/<x0,y0,x1,y1>/<W>x<H>/<filter> = np.asarray(Image.open(f).convert("RGB").crop(box).resize((W, H),
filter)), or out_sha256/... (the SHA-256 of that array in C order) when it has more than 256 pixels; the photo's
outputs are pinned by SHA-256 only.
"""
import hashlib
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "tests", "golden", "resize_pins.npz")
MAX_PINNED_PIXELS = 256
FILTERS = ("bilinear", "bicubic")


def boxes_and_sizes(w, h):
    """(box, (W, H)) of one image: the whole image and an inner crop, each downscaled, upscaled and with one direction
    unchanged."""
    out = []
    for box in ((0, 0, w, h), (3, 2, w - 4, h - 3)):
        bw, bh = box[2] - box[0], box[3] - box[1]
        for size in ((24, 16), (48, 30), (bw, 9), (11, bh), (1, 1)):
            out.append((box, size))
    return out


PHOTO_CASES = (  # (box, (W, H)): RandomResizedCrop-like rectangles, a Resize(256) of the whole image, an upscale
    ((500, 300, 2900, 2100), (224, 224)),
    ((0, 0, 4032, 3024), (341, 256)),
    ((1000, 1000, 1017, 1011), (224, 224)),
    ((1904, 1400, 2128, 1624), (224, 224)),  # 224 x 224 centre crop: both directions skipped
    ((100, 7, 3001, 1000), (224, 160)),
)


def sha256(a):
    return np.array(hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest())


def key(name, box, size, filt):
    return "%s/%s/%dx%d/%s" % (name, ",".join(str(v) for v in box), size[0], size[1], filt)


def main():
    from PIL import Image

    res = {"bilinear": Image.Resampling.BILINEAR, "bicubic": Image.Resampling.BICUBIC}
    pins = np.load(os.path.join(ROOT, "tests", "golden", "libjpeg_pins.npz"))
    arrays = {}
    for k in pins.files:
        if not k.startswith("jpeg/"):
            continue
        name = k[len("jpeg/"):]
        im = Image.open(io.BytesIO(pins[k].tobytes())).convert("RGB")
        for box, size in boxes_and_sizes(*im.size):
            for filt in FILTERS:
                a = np.asarray(im.crop(box).resize(size, res[filt]))
                if size[0] * size[1] <= MAX_PINNED_PIXELS:
                    arrays["out/" + key(name, box, size, filt)] = a
                else:
                    arrays["out_sha256/" + key(name, box, size, filt)] = sha256(a)
    im = Image.open(os.path.join(ROOT, "tests", "golden", "IMG_6510.JPG")).convert("RGB")
    for box, size in PHOTO_CASES:
        for filt in FILTERS:
            arrays["out_sha256/" + key("photo", box, size, filt)] = sha256(np.asarray(im.crop(box).resize(size, res[filt])))
    np.savez_compressed(OUT, **arrays)
    print("%s: %d arrays, %d bytes" % (OUT, len(arrays), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
