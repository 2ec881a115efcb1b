"""The sources and windows of the cropped-transcode tests.

    SIZES, SAMPLINGS      the sources of the live sweep: noise and photograph-like images (transcode_orient_cases.sweep_image)
                          at 75 x 53 and 80 x 64 in every sampling, saved by Pillow at quality 85
    image(w, h, sampling, content)  the pixels
    windows(w, h, ux, uy) the rectangles Pillow's file of the cropped pixels must equal, for an image of w x h and an iMCU of
                          ux x uy: name -> (x, y, w, h). They start on an iMCU boundary and each extent is a multiple of the
                          iMCU or reaches the image's edge
    ragged(w, h, ux, uy)  rectangles that end inside the image off a block boundary: the last blocks keep the source's
                          samples, so only a decode compares (grey and 4:4:4)
    pin_cases()           the subset pinned in tests/golden/transcode_crop_pins.npz (tools/make_transcode_crop_pins.py): dicts
                          name, w, h, sampling, content; each with all of windows(), the output kinds A, B, C in turn
    oriented_pin_cases()  (source name of transcode_orient_pins.npz, orientation, trim, rect): Pillow's file of the crop of
                          Image.transpose of the (cut) cell image, a rectangle that is not centred
    source_of_kind(...)   a source written by the repository's own writers: baseline interleaved, a scan per component, or
                          progressive (the GPU and host tests)
    pins() -> (sources name -> bytes, expected key -> bytes, versions); keys (name, window, kind) and (name, o, trim, rect, kind)
"""
import json
import os

import numpy as np

from tests import transcode_orient_cases as K

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transcode_crop_pins.npz")
SIZES = [(75, 53), (80, 64)]
SAMPLINGS = K.SAMPLINGS
CONTENTS = ("noise", "photo")
QUALITY = 85
KINDS = K.KINDS


def image(w, h, sampling, content):
    return K.sweep_image(w, h, sampling == "grey", content, 11)


def save_params(sampling, restart_blocks=0):
    p = dict(quality=QUALITY, subsampling=K.PILLOW_SUBSAMPLING[sampling])
    if restart_blocks:
        p["restart_marker_blocks"] = restart_blocks
    return p


def imcu(sampling):
    hs, vs = K.FACTORS[sampling]
    return 8 * hs, 8 * vs


def windows(w, h, ux, uy):
    return {
        "interior": (ux, uy, 2 * ux, 2 * uy),
        "right": (2 * ux, uy, w - 2 * ux, uy),
        "bottom": (ux, 2 * uy, 2 * ux, h - 2 * uy),
        "corner": (2 * ux, 2 * uy, w - 2 * ux, h - 2 * uy),
        "one": (ux, uy, ux, uy),
        "whole": (0, 0, w, h),
    }


def ragged(w, h, ux, uy):
    return [(ux, uy, ux + 5, uy + 3), (0, 2 * uy, 3 * ux - 1, 2 * uy), (2 * ux, 0, 13, h), (ux, uy, w - ux - 3, 7), (0, 0, 1, 1), (3 * ux, 2 * uy, 20, 9)]


def pin_cases():
    out = []
    for k, sampling in enumerate(SAMPLINGS):
        for j, (w, h) in enumerate(SIZES):
            content = CONTENTS[(k + j) % 2]
            out.append(dict(name="%dx%d_%s_%s" % (w, h, sampling.replace(":", ""), content), w=w, h=h, sampling=sampling, content=content))
    return out


def pin_kind(case_index, window_index):
    return "ABC"[(case_index + window_index) % 3]


def oriented_pin_cases():
    out = []
    for name, rects in (("48x32_420_q100", ((16, 0, 16, 16), (0, 16, 32, 16))), ("64x48_444_q100", ((8, 16, 24, 16), (40, 0, 24, 40))),
                        ("35x21_444_q100", ((8, 8, 16, 8), (0, 8, 16, 8))), ("17x40_grey_sym", ((8, 0, 8, 16), (0, 24, 16, 16))),
                        ("32x32_422_q100", ((16, 8, 16, 24),))):
        case = next(c for c in K.pin_cases() if c["name"] == name)
        for o in range(2, 9):
            trim = K.allowed(case, o, False) is None
            size = K.allowed(case, o, trim)
            if size is None:
                continue
            tw, th = size[::-1] if o >= 5 else size
            for rect in rects:
                x, y, w, h = (rect[1], rect[0], rect[3], rect[2]) if o >= 5 else rect  # (the rectangle turns with the image)
                if x + w <= tw and y + h <= th:
                    out.append((name, o, trim, (x, y, w, h)))
    return out


def source_of_kind(kind, sampling, w, h, content, seed, restart, quality=80):
    """A source written by the repository's own writers: the quantised coefficients of a seeded image as a baseline
    interleaved file ("interleaved"), a baseline file with each component in a scan of its own ("own_scans", unit
    quantisers) or a progressive file ("progressive"), as the oriented sweep writes them."""
    from oracle import oracle
    from tests import encode_ref as E
    from tests import progressive_ref as P
    from tests import transcode_ref as R

    grey = sampling == "grey"
    a = E.encode(K.sweep_image(w, h, grey, content, seed), quality, "4:4:4" if grey else sampling, restart)
    if kind == "interleaved":
        return a
    grids = [np.asarray(g) for g in oracle.decode(a).coef]
    factors = [(1, 1)] if grey else [K.FACTORS[sampling], (1, 1), (1, 1)]
    nc = len(factors)
    if kind == "own_scans":
        from tools import jpegsynth

        return jpegsynth.encode_custom(w, h, factors, grids, [P._flat_table(16, 5)[:2]], [P._flat_table(256, 9)[:2]], tables=[(0, 0)] * nc, interleaved=False,
                                       restart_interval=restart)
    inverse = np.argsort(E.ZIGZAG)
    qtabs = {t: np.array(q)[inverse] for t, q in R.parse(a)["qtabs"].items()}
    return P.encode(w, h, factors, qtabs, [0, 1, 1][:nc], grids, P.script_pillow_like(nc), restart=restart)


_pins = None


def pins():
    global _pins
    if _pins is None:
        with np.load(GOLDEN) as z:
            meta = json.loads(z["meta"].tobytes().decode())
            sources = {name: z["S_" + name].tobytes() for name in meta["cases"]}
            want = {}
            for key in z.files:
                if key.startswith("P_"):
                    name, window, kind = key[2:].rsplit("-", 2)
                    want[name, window, kind] = z[key].tobytes()
                elif key.startswith("O_"):
                    name, o, t, rect, kind = key[2:].rsplit("-", 4)
                    want[name, int(o), bool(int(t)), tuple(int(v) for v in rect.split("_")), kind] = z[key].tobytes()
        _pins = sources, want, {k: v for k, v in meta.items() if k != "cases"}
    return _pins

