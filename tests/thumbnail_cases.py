"""The thumbnail cases that tests/golden/thumbnail_pins.npz pins (tools/make_thumbnail_pins.py writes it with Pillow) and that
tests/test_thumbnail_ref.py and tests/test_gpu_thumbnail.py run: the smallest sources and requests at which each step of
Pillow's Image.thumbnail can go wrong, each with both filters. The sources live in the pins (src/<name>), so the tests
need neither Pillow nor an encoder; SOURCES says how the tool makes them.

The seeded sweep of tests/test_thumbnail_ref.py (live Pillow only) is here too.
"""
import os

import numpy as np

FILTERS = ("bilinear", "bicubic")
MAX_PINNED_PIXELS = 1024  # larger thumbnails are pinned by their SHA-256

S444 = ((1, 1),) * 3
S420 = ((2, 2), (1, 1), (1, 1))
S422 = ((2, 1), (1, 1), (1, 1))
S440 = ((1, 2), (1, 1), (1, 1))
GRAY = ((1, 1),)

# name -> how the tool makes it: ("synth", width, height, sampling, seed) through tools/jpegsynth.py, "rgb_ids" the same
# with the component ids 'R', 'G', 'B' (an RGB-coded file), ("pillow", kind, width, height, save arguments) through Pillow
SOURCES = {
    "small": ("synth", 40, 30, S420, 901),
    "g641": ("synth", 641, 479, GRAY, 902),
    "c420": ("synth", 640, 480, S420, 903),
    "big": ("synth", 700, 500, S420, 904),
    "c422": ("synth", 333, 251, S422, 905),
    "c440": ("synth", 201, 153, S440, 906),
    "c444": ("synth", 203, 155, S444, 907),
    "wide": ("synth", 696, 40, S420, 908),
    "rgb": ("rgb_ids", 69, 37, S444, 909),
    "white": ("pillow", "white", 200, 160, dict(quality=90)),
    "checker": ("pillow", "checker", 128, 96, dict(quality=100)),
    "prog": ("pillow", "smooth", 320, 240, dict(quality=80, progressive=True)),
}

# (case, source, (req_w, req_h), gap) -- what each is here for; the plans are asserted in tests/test_thumbnail_ref.py
CASES = (
    ("noop", "small", (64, 64), 2.0),            # an image smaller than the request: the full-scale decode
    ("rw_only", "small", (64, 20), 2.0),         # req_w >= W only: 40 x 30 -> 27 x 20, no draft
    ("draft2", "c422", (48, 48), 2.0),           # draft only, 1/2: 167 x 126 from the box 166.5 x 125.5
    ("draft4", "c440", (16, 16), 2.0),           # draft only, 1/4: 51 x 39 from 50.25 x 38.25
    ("draft8", "big", (24, 24), 2.0),            # draft only, 1/8: 88 x 63 from 87.5 x 62.5
    ("hit8", "c420", (80, 60), 1.0),             # the draft hits the size: 1/8 of 640 x 480
    ("hit4", "prog", (80, 60), 1.0),             # the same at 1/4, a progressive source
    ("reduce_eq", "c444", (10, 10), 2.0),        # 1/4, then reduce (2, 2) of 51 x 39: both edges ragged
    ("reduce_ne", "c420", (10, 10), 2.0),        # the issue's example: 1/8, factors (4, 3), 80 x 60 divides
    ("reduce_ne_gray", "g641", (10, 10), 2.0),   # grey, 1/8 = 81 x 60, factors (4, 3): a ragged last column
    ("reduce_440", "c440", (10, 10), 2.0),       # 4:4:0 at 1/4, reduce (2, 2)
    ("reduce_422_8", "c422", (5, 5), 2.0),       # 4:2:2 at 1/8 -- libjpeg replicates the chroma -- then reduce (4, 3)
    ("reduce_deep", "c422", (96, 4), 2.0),       # no draft, factors (33, 31) of 333 x 251: boxes over several staged rounds
    ("reduce_rgb", "rgb", (10, 10), 2.0),        # an RGB-coded file, reduce (3, 3)
    ("reduce_fy1", "prog", (10, 10), 2.0),       # 1/8 = 40 x 30, factors (2, 1)
    ("one", "wide", (10, 10), 2.0),              # a final height of 1: 696 x 40 -> 10 x 1, 1/2 then reduce (17, 10)
    ("white_reduce", "white", (10, 96), 2.0),    # all-255 source at full size, reduce (10, 10): the sums saturate
    ("white_draft", "white", (10, 10), 1.0),     # all 255 through 1/8 and reduce (2, 2) of 25 x 20
    ("checker", "checker", (10, 96), 2.0),       # one-pixel black and white squares at full size, reduce (6, 6), ragged
    ("gap_none", "c420", (48, 48), None),        # no draft and no reduce: 640 x 480 straight to 48 x 36
    ("gap_none_big", "big", (96, 96), None),     # the same, 700 x 500 -> 96 x 69: the widest canvas here
    ("gap3", "g641", (24, 24), 3.0),             # gap 3: 1/4, reduce (2, 2) of 161 x 120
    ("gap1", "c444", (24, 24), 1.0),             # gap 1: 1/4 = 51 x 39, reduce (2, 2)
)

# thumbnail_jpeg against Pillow's files: (case, filter, save arguments)
JPEG_CASES = (
    ("reduce_ne", "bicubic", dict(quality=75)),
    ("gap_none", "bilinear", dict(quality=90, subsampling="4:4:4")),
    ("reduce_ne_gray", "bicubic", dict(quality=85)),
    ("draft8", "bicubic", dict(quality=60, subsampling="4:2:2")),
)
JPEG_MODES = {"plain": dict(), "optimize": dict(optimize=True), "progressive": dict(progressive=True)}

EXIF_SOURCE, EXIF_REQUEST, EXIF_GAP = "c444", (16, 16), 2.0  # the eight orientations: 203 x 155 -> 16 x 12 (or 12 x 16)


def key(case, filt):
    return "%s/%s" % (case, filt)


def load_pins():
    here = os.path.dirname(os.path.abspath(__file__))
    return np.load(os.path.join(here, "golden", "thumbnail_pins.npz"))


def source(pins, name):
    return pins["src/" + name].tobytes()


def sweep(n_files=320, seed=2024):
    """The seeded sweep: (jpeg bytes, width, height, (req_w, req_h), filter, gap, layout name) of one thumbnail for each
    of n_files synthetic files of 40 x 30 .. 700 x 500 pixels, the five layouts in turn; the kind of request changes
    every five files."""
    from tools import jpegsynth

    layouts = (GRAY, S444, S420, S422, S440)
    gaps = (None, 1.0, 2.0, 2.0, 3.0)
    rng = np.random.default_rng(seed)
    for i in range(n_files):
        w, h = int(rng.integers(40, 701)), int(rng.integers(30, 501))
        data = jpegsynth.encode(w, h, layouts[i % 5], quality=60, noise=6, seed=1000 + i)
        k = (i // 5) % 5
        gap = gaps[int(rng.integers(0, len(gaps)))]
        if k == 0 and i % 3:  # a request that holds the image, in one direction only for some
            req = (int(rng.integers(w, 900)), int(rng.integers(h if i % 2 else 4, 900)))
        elif k == 1:  # the draft may hit the size: a request of the image at 1/2, 1/4 or 1/8, gap 1
            s = (2, 4, 8)[(i // 25) % 3]
            req, gap = (-(-w // s), -(-h // s)), 1.0
        elif k == 2 and i % 2:  # the draft at 1/8 alone: with gap 2 that is a request in (W / 32, W / 16]
            req, gap = (max(w // 16, 1), max(h // 16, 1)), 2.0
        elif k == 3 and i % 5 >= 3:  # 4:2:2 and 4:4:0 at 1/8, where libjpeg replicates, and a reduction behind it
            req, gap = (max(w // 40, 1), max(h // 40, 1)), 2.0
        else:
            req = (int(rng.integers(1, 97)), int(rng.integers(1, 97)))
        yield data, w, h, req, FILTERS[(i + i // 5) % 2], gap, ("gray", "444", "420", "422", "440")[i % 5]
