"""The sources of the transcode tests: a seeded sample over sizes, samplings, qualities (and one pair of custom tables) and
restart intervals, each with the files Pillow writes for the SAME pixels and parameters -- A plain, B with optimize=True, C
with progressive=True, and for some R with another restart interval. The files hold the same coefficients, so every
direction of a transcode has a byte-exact expected file (tests/golden/transcode_pins.npz, written by
tools/make_transcode_pins.py; the tests read the pins and never need Pillow).

    cases() -> list of dicts: name, w, h, sampling ("grey" | "4:4:4" | "4:2:2" | "4:2:0"), quality or None with `qtables`,
               restart_interval, restart_to (None: no R file), kind ("noise" | "smooth"), grey_subsampling (Pillow's value for
               a grey file: it only sets the sampling byte of the frame header)
    image(case) -> the uint8 pixels
    pins() -> name -> dict(A=bytes, B=bytes, C=bytes, R=bytes or None), and the versions that wrote them
    DIRECTIONS: (source, options, expected) over the files of a case"""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transcode_pins.npz")
SIZES = [(1, 1), (8, 8), (17, 13), (33, 17), (136, 120)]
SAMPLINGS = ["grey", "4:4:4", "4:2:2", "4:2:0"]
FACTORS = {"grey": (1, 1), "4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}
# a pair of tables that no quality gives: luma with quantisers of 1 in the low frequencies (categories of 10 at noise), a
# flat chroma table
QTABLES = [[1] * 10 + [3] * 22 + [7] * 32, [9] * 64]
# every direction between the files of a case: A plain, B optimised, C progressive
DIRECTIONS = [("A", dict(optimize=True), "B"), ("A", dict(progressive=True), "C"), ("C", dict(), "A"), ("B", dict(), "A"), ("A", dict(), "A"),
              ("C", dict(progressive=True), "C"), ("B", dict(optimize=True), "B"), ("C", dict(optimize=True), "B")]


def mcus_x(case):
    return -(-case["w"] // (8 * FACTORS[case["sampling"]][0]))


def _case(w, h, sampling, quality, restart, kind, restart_to=None, grey_subsampling=0):
    c = dict(w=w, h=h, sampling=sampling, quality=quality, qtables=None if quality else QTABLES, restart_interval=restart, restart_to=restart_to,
             kind=kind, grey_subsampling=grey_subsampling)
    for key in ("restart_interval", "restart_to"):
        if c[key] == "row":
            c[key] = mcus_x(c)
    c["name"] = "%dx%d_%s_%s_r%d_%s" % (w, h, sampling.replace(":", ""), "q%d" % quality if quality else "qtab", c["restart_interval"], kind)
    return c


def cases():
    out = [
        # what must be there whatever the sample draws: dummy blocks both ways, a tile boundary in the middle of an MCU row
        # (432 blocks), escapes (categories of 10 and above at quality 100 on noise), the custom tables, every restart interval
        _case(17, 13, "4:2:0", 75, 0, "noise", restart_to=1),
        _case(17, 13, "4:2:0", 100, 1, "noise", restart_to=0),
        _case(136, 120, "4:2:0", 75, 0, "smooth", restart_to="row"),
        _case(136, 120, "4:2:0", 1, 3, "noise", restart_to=0),
        _case(136, 120, "4:2:2", 75, "row", "smooth", restart_to=3),
        _case(136, 120, "grey", 75, 0, "smooth", restart_to=1),
        _case(33, 17, "4:4:4", 100, 0, "noise", restart_to=3),
        _case(33, 17, "4:2:2", None, 0, "noise", restart_to="row"),
        _case(33, 17, "grey", 100, 3, "noise", grey_subsampling=2),
        _case(1, 1, "4:2:0", 75, 0, "noise", restart_to=1),
        _case(1, 1, "grey", 1, 0, "noise"),
        _case(8, 8, "4:4:4", 75, 1, "smooth"),
    ]
    rng = np.random.default_rng(20261020)
    names = {c["name"] for c in out}
    while len(out) < 40:
        w, h = SIZES[int(rng.integers(0, 4))]  # (the sample stays below the largest size: the pins stay small)
        c = _case(w, h, SAMPLINGS[int(rng.integers(0, 4))], [1, 75, 100][int(rng.integers(0, 3))], [0, 1, 3, "row"][int(rng.integers(0, 4))],
                  ["noise", "smooth"][int(rng.integers(0, 2))], restart_to=[None, None, 0, 1, 3, "row"][int(rng.integers(0, 6))])
        if c["name"] not in names and c["restart_to"] != c["restart_interval"]:
            names.add(c["name"])
            out.append(c)
    return out


def image(case):
    rng = np.random.default_rng([case["w"], case["h"], SAMPLINGS.index(case["sampling"]), case["quality"] or 0, case["restart_interval"]])
    shape = (case["h"], case["w"]) if case["sampling"] == "grey" else (case["h"], case["w"], 3)
    if case["kind"] == "noise":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    y, x = np.mgrid[0:case["h"], 0:case["w"]]
    base = 128 + 90 * np.sin(x / 11.0) * np.cos(y / 7.0)
    if len(shape) == 3:
        base = np.stack([base, np.roll(base, 3, 1), 255 - base], -1)
    return np.clip(base + rng.normal(0, 4, shape), 0, 255).astype(np.uint8)


_pins = None


def pins():
    global _pins
    if _pins is None:
        with np.load(GOLDEN) as z:
            meta = json.loads(z["meta"].tobytes().decode())
            files = {}
            for name in meta["cases"]:
                files[name] = {k: (z["%s_%s" % (k, name)].tobytes() if "%s_%s" % (k, name) in z else None) for k in "ABCR"}
        _pins = files, {k: v for k, v in meta.items() if k != "cases"}
    return _pins
