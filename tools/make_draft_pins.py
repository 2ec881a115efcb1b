"""Writes tests/golden/draft_pins.npz: what Pillow (its bundled libjpeg-turbo) returns for a scaled decode,
im.draft("RGB", (W // d, H // d)); im.convert("RGB"), so that tests/test_draft_ref.py and tests/test_gpu_draft.py can
check the numpy restatement (tests/draft_ref.py) and the library's JPEGGPU_EXT_SCALE_LIBJPEG mode without Pillow.

    python tools/make_draft_pins.py

Arrays:
  * jpeg_sha256/<name>: the SHA-256 of the input -- a file of tests/cases.matrix(), of tests/cases.sampling_sweep()
    ("sweep:<name>") or the photo -- which the tests regenerate and check against it;
  * rgb/<name>/<d> or rgb_sha256/<name>/<d>: Pillow's RGB at d = 2, 4, 8 of every one- and three-component file with
    integral sampling ratios;
  * resize/<name>/<d>/<x0>,<y0>,<x1>,<y1>/<w>x<h>/<filter>: Pillow's draft + convert("RGB") + crop(box) + resize for a few
    files and seeded rectangles (the box in pixels of the image at 1 / d);
  * draft_scale: int32 [n, 5] rows (width, height, requested width, requested height, the scale JpegImageFile.draft picked).
An array of more than 4 k pixels is pinned by its SHA-256 (C order) only, which keeps the file small.

Excluded (tests/draft_ref.pillow_comparable): dense_escapes at 1/2, where libjpeg-turbo's SIMD jpeg_idct_4x4 differs from
jidctred.c (as its SIMD ISLOW does at full size), and files smaller than d in a direction, for which draft() cannot be
made to pick that scale.
"""
import hashlib
import io
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import draft_ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "draft_pins.npz")
MAX_PINNED_PIXELS = 4 * 1024
RESIZE_FILES = ("ss_2x2", "ss_2x1", "ss_1x2", "gray", "sweep:y4x2_a", "photo")
REQUESTS = ((1, 1), (3, 2), (7, 9), (16, 16), (25, 19), (33, 40), (50, 38), (64, 64), (100, 76), (101, 77), (199, 151), (224, 224),
            (500, 400), (1008, 756), (2016, 1512), (5000, 5000))


def sha256(a):
    return np.array(hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest())


def resize_cases(name, width, height, d):
    """[(box, (w, h))]: seeded rectangles of the image at 1 / d and output sizes, small enough to pin as arrays."""
    rng = np.random.default_rng(zlib.crc32(("%s/%d" % (name, d)).encode()))
    W, H = draft_ref.ceil_div(width, d), draft_ref.ceil_div(height, d)
    out = [((0, 0, W, H), (min(W, 31), min(H, 23)))]
    for _ in range(2):
        w, h = int(rng.integers(max(1, W // 4), W + 1)), int(rng.integers(max(1, H // 4), H + 1))
        x, y = int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1))
        out.append(((x, y, x + w, y + h), (int(rng.integers(8, 40)), int(rng.integers(8, 40)))))
    return out


def main():
    from oracle import oracle
    from PIL import Image

    arrays, rows = {}, []
    files = draft_ref.inputs()
    pinned = skipped = 0
    for name, data in files.items():
        dec = oracle.decode(data)
        arrays["jpeg_sha256/" + name] = sha256(np.frombuffer(data, np.uint8))
        for req in REQUESTS if draft_ref.has_rgb(dec) else ():
            im = Image.open(io.BytesIO(data))
            got = im.draft("RGB", req)
            scale = 1 if got is None else int(round(dec.width / got[1][2]))
            rows.append((dec.width, dec.height, req[0], req[1], scale))
        for d in draft_ref.SCALES:
            if not draft_ref.pillow_comparable(name, dec, d):
                skipped += 1
                continue
            rgb, size = draft_ref.pillow_draft_rgb(data, d)
            assert size == (draft_ref.ceil_div(dec.width, d), draft_ref.ceil_div(dec.height, d)), (name, d, size)
            key = "%s/%d" % (name, d)
            if rgb.shape[0] * rgb.shape[1] <= MAX_PINNED_PIXELS:
                arrays["rgb/" + key] = rgb
            else:
                arrays["rgb_sha256/" + key] = sha256(rgb)
            pinned += 1
            if name in RESIZE_FILES:
                im = Image.open(io.BytesIO(data))
                im.draft("RGB", (dec.width // d, dec.height // d))
                full = im.convert("RGB")
                for box, (w, h) in resize_cases(name, dec.width, dec.height, d):
                    for filt, f in (("bilinear", Image.BILINEAR), ("bicubic", Image.BICUBIC)):
                        out = np.asarray(full.crop(box).resize((w, h), f))
                        arrays["resize/%s/%d/%s/%dx%d/%s" % (name, d, ",".join(str(v) for v in box), w, h, filt)] = out
    arrays["draft_scale"] = np.array(sorted(set(rows)), np.int32)
    np.savez_compressed(OUT, **arrays)
    print("%d cases pinned, %d not comparable with Pillow, %d draft_scale rows, %d bytes" %
          (pinned, skipped, len(arrays["draft_scale"]), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
