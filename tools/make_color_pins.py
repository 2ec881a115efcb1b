"""Writes tests/golden/color_pins.npz: what Pillow returns for the RGB-, CMYK- and YCCK-coded files of
tests/color_ref.cases() -- Image.open(f).convert("RGB"), after im.draft("RGB", (W // d, H // d)) at d = 2, 4, 8 -- so that
tests/test_color_ref.py and tests/test_gpu_color.py can check the numpy restatement (tests/color_ref.py) and the library's
colour-aware RGB calls without Pillow.

    python tools/make_color_pins.py

Arrays:
  * jpeg_sha256/<name>: the SHA-256 of the input, which the tests regenerate and check against it;
  * model/<name>: the colour model (enum jpeggpu_ext_color_space) the case list gives the file;
  * rgb/<name>/<d> or rgb_sha256/<name>/<d>: Pillow's RGB at d = 1, 2, 4, 8. An array of more than 4 k pixels is pinned by
    its SHA-256 (C order) only, which keeps the file small.

Excluded (tests/color_ref.comparable): the 3 x 5 files at d > 1, for which draft() does not return the image at 1 / d.
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import color_ref, draft_ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "color_pins.npz")
MAX_PINNED_PIXELS = 4 * 1024


def sha256(a):
    return np.array(hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest())


def main():
    arrays = {}
    pinned = skipped = 0
    for name, (data, model) in color_ref.cases().items():
        arrays["jpeg_sha256/" + name] = sha256(np.frombuffer(data, np.uint8))
        arrays["model/" + name] = np.array(model, np.int32)
        width, height = color_ref.frame_size(data)
        for d in color_ref.SCALES:
            if not color_ref.comparable(name, d):
                skipped += 1
                continue
            rgb, size = color_ref.pillow_rgb(data, d)
            assert size == (draft_ref.ceil_div(width, d), draft_ref.ceil_div(height, d)), (name, d, size)
            key = "%s/%d" % (name, d)
            if rgb.shape[0] * rgb.shape[1] <= MAX_PINNED_PIXELS:
                arrays["rgb/" + key] = rgb
            else:
                arrays["rgb_sha256/" + key] = sha256(rgb)
            pinned += 1
    np.savez_compressed(OUT, **arrays)
    print("%d cases pinned, %d not comparable with Pillow, %d bytes" % (pinned, skipped, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
