"""Writes tests/golden/exif_pins.npz: what Pillow gives for the files of tests/exif_ref.gpu_files() with an Exif segment of
every orientation 1..8 -- ImageOps.exif_transpose(im).convert("RGB"), after im.draft("RGB", (W // d, H // d)) at d = 2 and 8
-- and for the resize cases: ....crop(box).resize(size, filter). tests/test_exif_host.py checks the numpy restatement
against them where Pillow is present, tests/test_gpu_exif.py the library without it.

    python tools/make_exif_pins.py          (needs Pillow; written with Pillow 12.2)

Arrays:
  * jpeg_sha256/<name>: the SHA-256 of the file without Exif, which the tests regenerate and check;
  * rgb/<name>/<o>/<d> or rgb_sha256/<name>/<o>/<d>: Pillow's displayed RGB at d = 1, 2, 8 (an array of more than 1024 pixels
    by its SHA-256 only). Left out: sizes for which draft() does not return the image at 1 / d (color_ref.draft_comparable);
  * resize/<name>/<o>/<x,y,w,h>/<WxH>/<filter>: the displayed rectangle resized -- for every orientation the whole 53 x 37
    and 300 x 20 files to 24 x 16 and 16 x 24, and the eight seeded crops of exif_ref.batch_cases() to 24 x 16.
"""
import hashlib
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import color_ref, exif_ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "exif_pins.npz")
MAX_PINNED_PIXELS = 1024


def sha256(a):
    return np.array(hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest())


def displayed(data, d=1):
    """ImageOps.exif_transpose of the file after draft() at 1 / d, as an RGB image."""
    from PIL import Image, ImageOps

    im = Image.open(io.BytesIO(data))
    w, h = im.size
    if d > 1:
        im.draft("RGB", (max(w // d, 1), max(h // d, 1)))
    return ImageOps.exif_transpose(im).convert("RGB")


def resized(im, box, size, filt):
    from PIL import Image

    f = {"bilinear": Image.Resampling.BILINEAR, "bicubic": Image.Resampling.BICUBIC}[filt]
    x, y, w, h = box
    return np.asarray(im.crop((x, y, x + w, y + h)).resize(size, f))


def main():
    arrays = {}
    files = exif_ref.gpu_files()
    for name, (data, _twin) in files.items():
        arrays["jpeg_sha256/" + name] = sha256(np.frombuffer(data, np.uint8))
        W, H = exif_ref.frame_size(data)
        for o in range(1, 9):
            f = exif_ref.with_orientation(data, o)
            for d in exif_ref.SCALES:
                if d > 1 and not color_ref.draft_comparable(W, H, d):
                    continue
                a = np.asarray(displayed(f, d))
                w, h = exif_ref.orient_size(o, -(-W // d), -(-H // d))
                assert a.shape == (h, w, 3), (name, o, d, a.shape)
                key = "%s/%d/%d" % (name, o, d)
                if w * h <= MAX_PINNED_PIXELS:
                    arrays["rgb/" + key] = a
                else:
                    arrays["rgb_sha256/" + key] = sha256(a)
    for name in exif_ref.RESIZE_FILES:
        for o in range(1, 9):
            im = displayed(exif_ref.with_orientation(files[name][0], o))
            box = (0, 0) + im.size
            for size in exif_ref.RESIZE_SIZES:
                for filt in exif_ref.FILTERS:
                    arrays["resize/%s/%d/%s/%dx%d/%s" % (name, o, ",".join(map(str, box)), size[0], size[1], filt)] = resized(im, box, size, filt)
    for name, o, box in exif_ref.batch_cases():
        im = displayed(exif_ref.with_orientation(files[name][0], o))
        for filt in exif_ref.FILTERS:
            arrays["resize/%s/%d/%s/24x16/%s" % (name, o, ",".join(map(str, box)), filt)] = resized(im, box, (24, 16), filt)
    np.savez_compressed(OUT, **arrays)
    print("%d arrays, %d bytes" % (len(arrays), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
