"""The sources of the oriented-transcode tests.

The PINS (tests/golden/transcode_orient_pins.npz, written by tools/make_transcode_orient_pins.py; the tests read them and
never need Pillow): images that are constant over 16 x 16 cells, so that every 8 x 8 block of every component is constant
at every sampling and at every edge, saved at quality 100 (quantisers of 1) or with a pair of tables that is symmetric in
natural order. For such an image a flip, a turn or a transposition of the PIXELS gives exactly the flipped, turned or
transposed coefficients, so Pillow's file of Image.transpose of the (cut) pixels is, byte for byte, what an oriented
transcode of Pillow's file of the pixels has to be: block permutation, sizes, sampling swap, trim and dummy blocks against
libjpeg.

    pin_cases()  -> list of dicts: name, w, h, sampling, tables ("q100" | "sym")
    cell_image(case) -> the uint8 pixels
    allowed(case, o, trim) -> the (w, h) of the trimmed source, or None where the rules refuse
    pins()       -> (sources name -> bytes, expected (name, o, trim, kind) -> bytes with kind in "ABC", versions). An entry
                    with trim=True is there only where the trim cuts something; otherwise the file is the trim=False one.
    expected(name, o, trim, kind) -> the pinned file

The SWEEP sources (the GPU tests): seeded noise and photograph-like images as baseline interleaved files, baseline files
with each component in a scan of its own and progressive files, written by the repository's own writers."""
import json
import os

import numpy as np

from tests import transcode_orient_ref as X

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transcode_orient_pins.npz")
SIZES = [(32, 32), (48, 32), (16, 64), (35, 21), (8, 8), (17, 40), (64, 48), (5, 3)]
SAMPLINGS = ["grey", "4:4:4", "4:2:0", "4:2:2"]
FACTORS = {"grey": (1, 1), "4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}
PILLOW_SUBSAMPLING = {"grey": 0, "4:4:4": 0, "4:2:2": 1, "4:2:0": 2}
KINDS = {"A": dict(), "B": dict(optimize=True), "C": dict(progressive=True)}
# symmetric in natural order (Pillow takes `qtables` in natural order): q[8 v + u] == q[8 u + v]
SYM_TABLES = [[1 + 2 * (u + v) + (u * v) % 5 for v in range(8) for u in range(8)], [3 + 5 * max(u, v) for v in range(8) for u in range(8)]]
# Image.transpose's method for an orientation (ImageOps.exif_transpose)
PIL_METHOD = {2: "FLIP_LEFT_RIGHT", 3: "ROTATE_180", 4: "FLIP_TOP_BOTTOM", 5: "TRANSPOSE", 6: "ROTATE_270", 7: "TRANSVERSE", 8: "ROTATE_90"}


def pin_cases():
    out = []
    for w, h in SIZES:
        for sampling in SAMPLINGS:
            out.append(dict(name="%dx%d_%s_q100" % (w, h, sampling.replace(":", "")), w=w, h=h, sampling=sampling, tables="q100"))
    for (w, h), sampling in (((48, 32), "4:2:0"), ((35, 21), "4:4:4"), ((17, 40), "grey")):
        out.append(dict(name="%dx%d_%s_sym" % (w, h, sampling.replace(":", "")), w=w, h=h, sampling=sampling, tables="sym"))
    return out


def cell_image(case):
    w, h = case["w"], case["h"]
    rng = np.random.default_rng([w, h, SAMPLINGS.index(case["sampling"]), case["tables"] == "sym"])
    cells = rng.integers(0, 256, (-(-h // 16), -(-w // 16)) + (() if case["sampling"] == "grey" else (3,)), dtype=np.uint8)
    return np.ascontiguousarray(np.repeat(np.repeat(cells, 16, 0), 16, 1)[:h, :w])


def save_params(case):
    p = dict(subsampling=PILLOW_SUBSAMPLING[case["sampling"]])
    if case["tables"] == "sym":
        p["qtables"] = SYM_TABLES[:1 if case["sampling"] == "grey" else 2]
    else:
        p["quality"] = 100
    return p


def allowed(case, o, trim):
    hs, vs = FACTORS[case["sampling"]]
    if o in X.TRANSPOSED and (hs, vs) == (2, 1):
        return None
    try:
        return X.target_size(case["w"], case["h"], hs, vs, o, trim)
    except X.Unsupported:
        return None


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
                    name, o, t, kind = key[2:].rsplit("-", 3)
                    want[name, int(o), bool(int(t)), kind] = z[key].tobytes()
        _pins = sources, want, {k: v for k, v in meta.items() if k != "cases"}
    return _pins


def expected(name, o, trim, kind):
    want = pins()[1]
    return want[name, o, True, kind] if (name, o, True, kind) in want and trim else want[name, o, False, kind]


# ---- the sweep ----

SWEEP_SIZES = [(16, 16), (48, 32), (32, 48), (17, 40), (35, 21)]
SWEEP_LARGE = (128, 112)  # in 4:2:0: 336 blocks, two gather tiles, and a tile boundary on the transposed side
SOURCE_KINDS = ("interleaved", "own_scans", "progressive")


def sweep_image(w, h, grey, kind, seed):
    rng = np.random.default_rng([w, h, int(grey), kind == "noise", seed])
    shape = (h, w) if grey else (h, w, 3)
    if kind == "noise":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    base = 128 + 80 * np.sin(x / 9.0 + seed) * np.cos(y / 6.0) + 0.4 * x - 0.3 * y
    if not grey:
        base = np.stack([base, np.roll(base, 5, 1), 240 - base], -1)
    return np.clip(base + rng.normal(0, 3, shape), 0, 255).astype(np.uint8)
