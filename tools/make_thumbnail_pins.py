"""Writes tests/golden/thumbnail_pins.npz: what Pillow's Image.thumbnail makes of the cases of tests/thumbnail_cases.py, so
that tests/test_thumbnail_ref.py and tests/test_gpu_thumbnail.py can check the restatement (tests/thumbnail_ref.py),
jpeggpu_ext_thumbnail_to_rgb and thumbnail_jpeg without Pillow.

    python tools/make_thumbnail_pins.py

The pipeline is Pillow's alone: im = Image.open(f); im.thumbnail((req_w, req_h), filter, reducing_gap=gap); np.asarray(im).
Arrays:
  src/<name>                      the source files (uint8), made as tests/thumbnail_cases.SOURCES says
  out/<case>/<filter>             the thumbnail, (h, w, 3) or (h, w) for a grey file; out_sha256/... (the SHA-256 of that
                                  array in C order) and size/<case>/<filter> = (w, h) when it has more than 1024 pixels
  jpeg/<case>/<filter>/<mode>     im.save(f, "JPEG", **arguments, **mode) after the thumbnail (thumbnail_cases.JPEG_CASES)
  exif/<o>/<filter>               np.asarray(ImageOps.exif_transpose(im)) after the thumbnail, of the EXIF source with
                                  orientation o = 1..8 (tests/exif_ref.with_orientation)
"""
import hashlib
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import thumbnail_cases as TC  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "thumbnail_pins.npz")


def sha256(a):
    return np.array(hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest())


def make_source(spec):
    from PIL import Image

    from tests import color_ref
    from tools import jpegsynth

    if spec[0] in ("synth", "rgb_ids"):
        _, w, h, sampling, seed = spec
        data = jpegsynth.encode(w, h, sampling, quality=60, noise=6, seed=seed)
        return color_ref.patch_ids(data, color_ref.IDS_RGB) if spec[0] == "rgb_ids" else data
    _, kind, w, h, save = spec
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "white":
        im = Image.fromarray(np.full((h, w, 3), 255, np.uint8))
    elif kind == "checker":
        im = Image.fromarray((((xx + yy) & 1) * 255).astype(np.uint8))  # grey: chroma subsampling would blur it
    else:  # smooth colour with some texture
        rng = np.random.default_rng(77)
        a = np.stack([xx * 255 // (w - 1), yy * 255 // (h - 1), (xx + yy) * 255 // (w + h - 2)], axis=-1) + rng.integers(-20, 21, (h, w, 3))
        im = Image.fromarray(np.clip(a, 0, 255).astype(np.uint8))
    f = io.BytesIO()
    im.save(f, "JPEG", **save)
    return f.getvalue()


def main():
    from PIL import Image, ImageOps

    from tests import exif_ref

    res = {"bilinear": Image.Resampling.BILINEAR, "bicubic": Image.Resampling.BICUBIC}
    arrays = {}
    srcs = {name: make_source(spec) for name, spec in TC.SOURCES.items()}
    for name, data in srcs.items():
        arrays["src/" + name] = np.frombuffer(data, np.uint8)

    def thumb(data, req, filt, gap):
        im = Image.open(io.BytesIO(data))
        im.thumbnail(req, res[filt], reducing_gap=gap)
        return im

    for case, src, req, gap in TC.CASES:
        for filt in TC.FILTERS:
            a = np.asarray(thumb(srcs[src], req, filt, gap))
            if a.shape[0] * a.shape[1] <= TC.MAX_PINNED_PIXELS:
                arrays["out/" + TC.key(case, filt)] = a
            else:
                arrays["out_sha256/" + TC.key(case, filt)] = sha256(a)
                arrays["size/" + TC.key(case, filt)] = np.array([a.shape[1], a.shape[0]])
    by_name = {c[0]: c for c in TC.CASES}
    for case, filt, save in TC.JPEG_CASES:
        _, src, req, gap = by_name[case]
        assert b"\xff\xfe" not in srcs[src][:600], "a COM segment would be copied across"
        for mode, extra in TC.JPEG_MODES.items():
            f = io.BytesIO()
            thumb(srcs[src], req, filt, gap).save(f, "JPEG", **save, **extra)
            arrays["jpeg/%s/%s" % (TC.key(case, filt), mode)] = np.frombuffer(f.getvalue(), np.uint8)
    for o in range(1, 9):
        for filt in TC.FILTERS:
            im = thumb(exif_ref.with_orientation(srcs[TC.EXIF_SOURCE], o), TC.EXIF_REQUEST, filt, TC.EXIF_GAP)
            arrays["exif/%d/%s" % (o, filt)] = np.asarray(ImageOps.exif_transpose(im))
    np.savez_compressed(OUT, **arrays)
    print("%s: %d arrays, %d bytes" % (OUT, len(arrays), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
