"""Writes tests/golden/libjpeg_pins.npz: what Pillow (its bundled libjpeg-turbo) decodes at full size, so that
tests/test_libjpeg_ref.py and tests/test_gpu_libjpeg.py can check the numpy restatement (tests/libjpeg_ref.py) and the
library's ISLOW mode without Pillow.

    python tools/make_libjpeg_pins.py

Arrays:
  * jpeg/<name>: the input file, for the small Pillow-encoded images (q50 / q90 / q100, subsampling 0, 1, 2 -- 4:4:4,
    4:2:2, 4:2:0 -- at odd sizes, and grayscale); jpeg_sha256/<name>: the SHA-256 of the input, for the files of
    tests/cases.matrix(), which the tests regenerate (tests/libjpeg_ref.pinned_jpeg checks that they still match);
  * planes/<name>/<c> or planes_sha256/<name>/<c>: Pillow's planes (Image.draft("YCbCr" | "L", im.size): no colour
    conversion, no upsampling) of the 4:4:4 and grayscale files;
  * rgb/<name> or rgb_sha256/<name>: np.asarray(Image.open(f).convert("RGB")) of the one- and three-component files;
  * photo_rgb_sha256: the SHA-256 of Pillow's RGB of tests/golden/IMG_6510.JPG.
An array of more than 4 k pixels is pinned by its SHA-256 (C order) only, which keeps the file small.

Excluded: dense_escapes. libjpeg-turbo runs its SIMD ISLOW IDCT there, whose arithmetic differs from jidctint.c's for
that file's coefficients (63 of magnitude 512..1023 with quantisers of 1); the restatement, and the library, follow
jidctint.c.
"""
import hashlib
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import cases, libjpeg_ref, scaled_ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "libjpeg_pins.npz")
EXCLUDED = {"dense_escapes"}
MAX_PINNED_PIXELS = 4 * 1024


def sha256(a):
    return np.array(hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest())


def pillow_inputs():
    from PIL import Image

    rng = np.random.default_rng(2026)
    out = {}
    for q in (50, 90, 100):
        for sub in (0, 1, 2):
            for w, h in ((61, 45), (33, 17)):
                smooth = np.cumsum(np.cumsum(rng.integers(-6, 7, (h, w, 3)), 0), 1)
                a = np.clip(128 + smooth + rng.integers(-20, 21, (h, w, 3)), 0, 255).astype(np.uint8)
                buf = io.BytesIO()
                Image.fromarray(a, "RGB").save(buf, "JPEG", quality=q, subsampling=sub)
                out["pil_q%d_s%d_%dx%d" % (q, sub, w, h)] = buf.getvalue()
        buf = io.BytesIO()
        Image.fromarray(rng.integers(0, 256, (23, 37), dtype=np.uint8), "L").save(buf, "JPEG", quality=q)
        out["pil_l_q%d_37x23" % q] = buf.getvalue()
    return out


def _pin(arrays, key, a):
    if a.shape[0] * a.shape[1] <= MAX_PINNED_PIXELS:
        arrays[key] = a
    else:
        kind, _, rest = key.partition("/")
        arrays[kind + "_sha256/" + rest] = sha256(a)


def main():
    from oracle import oracle

    arrays = {}
    inputs = {}
    for name, data in cases.matrix().items():
        if name in EXCLUDED:
            continue
        if oracle.decode(data).ncomp in (1, 3):
            inputs[name] = data
            arrays["jpeg_sha256/" + name] = sha256(np.frombuffer(data, np.uint8))
    for name, data in pillow_inputs().items():
        inputs[name] = data
        arrays["jpeg/" + name] = np.frombuffer(data, np.uint8)
    for name, data in inputs.items():
        dec = oracle.decode(data)
        if dec.ncomp == 1 or (set(dec.hs) == {1} and set(dec.vs) == {1}):
            for c, p in enumerate(scaled_ref.pillow_draft(data, 1)):
                _pin(arrays, "planes/%s/%d" % (name, c), p)
        _pin(arrays, "rgb/" + name, libjpeg_ref.pillow_rgb(data))
    with open(os.path.join(ROOT, "tests", "golden", "IMG_6510.JPG"), "rb") as f:
        arrays["photo_rgb_sha256"] = sha256(libjpeg_ref.pillow_rgb(f.read()))
    np.savez_compressed(OUT, **arrays)
    print("%s: %d arrays, %d bytes" % (OUT, len(arrays), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
