"""Writes tests/golden/scaled_pins.npz: Pillow's (bundled libjpeg-turbo's) scaled decodes -- Image.draft at (W // d, H // d),
d = 2, 4, 8 -- of the 4:4:4, grayscale and non-interleaved 4:4:4 files of tests/cases.matrix() and of a few small
Pillow-encoded images at q50 / q90 / q100, stored with their JPEG bytes so that tests/test_scaled_ref.py can check the
numpy restatement of the reduced IDCTs (tests/scaled_ref.py) without Pillow.

    python tools/make_scaled_pins.py

draft() picks the power-of-two scale s with W // s >= the requested width; the planes it returns are ceil(W / d) wide.
Excluded: dense_escapes at d = 2. libjpeg-turbo runs its SIMD jsimd_idct_4x4 there, whose arithmetic differs from
jidctred.c's for its coefficients (63 of magnitude 512..1023 with quantisers of 1) in 270 of 7680 samples; the
restatement, and the library, follow jidctred.c.
"""
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import cases, scaled_ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "scaled_pins.npz")
MATRIX_CASES = ("ss_1x1", "gray", "gray_hdr_2x2", "ni_444", "dense_escapes", "cfg4_small")
EXCLUDED = {("dense_escapes", 2)}


def pillow_inputs():
    from PIL import Image

    rng = np.random.default_rng(2024)
    out = {}
    for q in (50, 90, 100):
        for mode, (w, h) in (("RGB", (61, 45)), ("L", (48, 40))):
            smooth = np.cumsum(np.cumsum(rng.integers(-6, 7, (h, w, 3)), 0), 1)
            a = np.clip(128 + smooth + rng.integers(-20, 21, (h, w, 3)), 0, 255).astype(np.uint8)
            im = Image.fromarray(a, "RGB")
            if mode == "L":
                im = im.convert("L")
            buf = io.BytesIO()
            im.save(buf, "JPEG", quality=q, subsampling=0)  # 4:4:4
            out["pil_%s_q%d" % (mode.lower(), q)] = buf.getvalue()
    return out


def main():
    m = cases.matrix()
    inputs = {name: m[name] for name in MATRIX_CASES}
    inputs.update(pillow_inputs())
    arrays = {}
    for name, data in inputs.items():
        arrays["jpeg/" + name] = np.frombuffer(data, np.uint8)
        for d in (2, 4, 8):
            if (name, d) in EXCLUDED:
                continue
            for c, p in enumerate(scaled_ref.pillow_draft(data, d)):
                arrays["planes/%s/%d/%d" % (name, d, c)] = p
    np.savez_compressed(OUT, **arrays)
    print("%s: %d arrays, %d bytes" % (OUT, len(arrays), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
