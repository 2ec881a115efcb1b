"""The pinned cases of the transcode that keeps its source's frame (tests/transcode_frame_ref.py): what Pillow writes outside
the pixel encoder's layouts. tools/make_transcode_frame_pins.py saves Pillow's files, so that the tests never need Pillow.

    sources()      name -> (image, mode, save parameters): CMYK at quality 80, RGB-coded (keep_rgb), YCbCr 4:4:4 / 4:2:2 /
                   4:2:0 with three quantisation tables (Cb's is not Cr's), and the same with an entry above 255 (SOF1,
                   Pq = 1); each at 75 x 53 and 80 x 64
    KINDS          the options of Pillow's second file of the same pixels: "A" plain, "B" optimize=True, "C" progressive=True
                   (18 scans for CMYK, 14 for RGB, 10 for YCbCr), each also with a restart interval of RESTART MCUs ("Ar",
                   "Br", "Cr"). The transcode of A with a kind's options must be that file.
    oriented()     name -> (cell image, mode, save parameters): 80 x 64 sources with 4:4:4 chroma whose orientation 2..8
                   Pillow writes too -- images constant over 16 x 16 cells with tables symmetric in natural order (quality
                   100, or such `qtables`), for which turning the pixels turns the coefficients exactly
                   (tests/transcode_orient_cases.py)
    renumbered(data, by)   a file with other quantisation-table numbers: still one the default mode takes
    pins()         the npz as a dict"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transcode_frame_pins.npz")
SIZES = ((75, 53), (80, 64))
RESTART = 3
KINDS = {"A": dict(), "B": dict(optimize=True), "C": dict(progressive=True), "Ar": dict(restart_marker_blocks=RESTART),
         "Br": dict(optimize=True, restart_marker_blocks=RESTART), "Cr": dict(progressive=True, restart_marker_blocks=RESTART)}
OPTIONS = {"A": dict(restart_interval=0), "B": dict(optimize=True, restart_interval=0), "C": dict(progressive=True, restart_interval=0),
           "Ar": dict(restart_interval=RESTART), "Br": dict(optimize=True, restart_interval=RESTART), "Cr": dict(progressive=True, restart_interval=RESTART)}
# natural order, as Pillow takes them; Cb's table is not Cr's
TABLES_8 = [[min(255, 3 + (k % 8) + 2 * (k // 8) + 2 * t) for k in range(64)] for t in range(3)]
TABLES_16 = [[300 + t if k == 63 else 2 + (k % 8) + (k // 8) + t for k in range(64)] for t in range(3)]
# q[8 v + u] == q[8 u + v]
SYMMETRIC = [[2 + t + (k % 8) + (k // 8) for k in range(64)] for t in range(3)]


def image(w, h, channels, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([(xx * (3 + k) + yy * (2 * k + 1)) % 256 for k in range(channels)], -1).astype(np.int64)
    return np.clip(base + rng.integers(-6, 7, (h, w, channels)), 0, 255).astype(np.uint8)


def cell_image(w, h, channels, seed):
    rng = np.random.default_rng(seed)
    cells = rng.integers(0, 256, (-(-h // 16), -(-w // 16), channels), dtype=np.uint8)
    return np.ascontiguousarray(np.repeat(np.repeat(cells, 16, 0), 16, 1)[:h, :w])


def sources():
    out = {}
    for n, (w, h) in enumerate(SIZES):
        size = "%dx%d" % (w, h)
        out["cmyk_" + size] = (image(w, h, 4, 10 + n), "CMYK", dict(quality=80))
        out["rgb_" + size] = (image(w, h, 3, 20 + n), "RGB", dict(quality=75, keep_rgb=True))
        for s, name in enumerate(("444", "422", "420")):
            out["t3_%s_%s" % (name, size)] = (image(w, h, 3, 30 + 3 * n + s), "RGB", dict(qtables=TABLES_8, subsampling=s))
            out["t16_%s_%s" % (name, size)] = (image(w, h, 3, 40 + 3 * n + s), "RGB", dict(qtables=TABLES_16, subsampling=s))
    return out


def oriented():
    w, h = 80, 64
    return {"cmyk": (cell_image(w, h, 4, 50), "CMYK", dict(quality=100)), "rgb": (cell_image(w, h, 3, 51), "RGB", dict(quality=100, keep_rgb=True)),
            "t3": (cell_image(w, h, 3, 52), "RGB", dict(qtables=SYMMETRIC, subsampling=0))}


def renumbered(data, by):
    """A baseline file with every quantisation-table number raised by `by`, in its DQT segments and in its frame header."""
    data = bytearray(data)
    at = 2
    while data[at + 1] != 0xDA:
        if data[at + 1] == 0xDB:
            data[at + 4] += by
        if data[at + 1] in (0xC0, 0xC1, 0xC2):
            for c in range(data[at + 9]):
                data[at + 12 + 3 * c] += by
        at += 2 + int.from_bytes(data[at + 2:at + 4], "big")
    return bytes(data)


def pins():
    z = np.load(GOLDEN)
    return {k: z[k].tobytes() for k in z.files if k != "meta"}
