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


# ---- sources beyond Pillow's small files (tests/test_gpu_transcode_scale.py, tests/test_transcode_ref.py) ----

LARGE_PINS = os.path.join(os.path.dirname(GOLDEN), "transcode_large_pins.json")
CAMERA = os.path.join(os.path.dirname(GOLDEN), "IMG_6510.JPG")
TILE_BLOCKS = 256  # blocks per workgroup of the gather and of the encoder's block stage

_large = None


def large():
    """name -> file. The files of tests/golden/progressive_large.npz -- photo (1024 x 768, 4:2:0, 18 432 blocks) and photo_rst
    (512 x 384, restart interval 1), each progressive and as its baseline twin (`<name>_twin`, Pillow's optimize=True file
    of the same pixels); eob_cap and eob_ladder (grey, 1456 x 1448, 32 942 blocks, progressive) -- and the camera file
    tests/golden/IMG_6510.JPG (4032 x 3024, 4:2:0, DRI 252, EXIF; 285 768 blocks)."""
    global _large
    if _large is None:
        from tests import progressive_cases

        big = progressive_cases.large()
        _large = {"photo": big["photo"].prog, "photo_twin": big["photo"].twin, "photo_rst": big["photo_rst"].prog,
                  "photo_rst_twin": big["photo_rst"].twin, "eob_cap": big["eob_cap"].prog, "eob_ladder": big["eob_ladder"].prog}
        with open(CAMERA, "rb") as f:
            _large["camera"] = f.read()
    return _large


LARGE_ROW = {"photo": 64, "photo_rst": 32}  # MCUs per MCU row
# (source, option label, options, expected): expected names another file of large() -- Pillow's own -- or is None: the pin
# LARGE_PINS holds under "<source>/<label>", which is tests/transcode_ref.transcode's output (tools/make_transcode_large_pins.py)
LARGE_PAIRS = []
for _n in ("photo", "photo_rst"):
    LARGE_PAIRS += [(_n, "optimize", dict(optimize=True), _n + "_twin"), (_n + "_twin", "progressive", dict(progressive=True), _n)]
    for _s in (_n, _n + "_twin"):
        LARGE_PAIRS += [(_s, "plain", dict(), None), (_s, "row", dict(restart_interval=LARGE_ROW[_n]), None)]
for _n in ("eob_cap", "eob_ladder"):
    LARGE_PAIRS += [(_n, "plain", dict(), None), (_n, "progressive", dict(progressive=True), None)]
LARGE_PAIRS += [("camera", "optimize", dict(optimize=True), None), ("camera", "progressive", dict(progressive=True), None)]

_large_pins = None


def large_pins():
    """"<source>/<label>" -> dict(size, sha256) for the pairs of LARGE_PAIRS without a file of Pillow's, and the versions."""
    global _large_pins
    if _large_pins is None:
        with open(LARGE_PINS) as f:
            doc = json.load(f)
        _large_pins = doc["pins"], doc["versions"]
    return _large_pins


def blocks_of(w, h, sampling):
    """Blocks of the MCU stream a target codes, and its tiles of TILE_BLOCKS."""
    hs, vs = FACTORS[sampling]
    n = -(-w // (8 * hs)) * -(-h // (8 * vs)) * (1 if sampling == "grey" else hs * vs + 2)
    return n, -(-n // TILE_BLOCKS)


# the crafted progressive files that hold exactly the coefficients of the baseline file they were made from, in every block a
# target codes (the others: non-interleaved scans leave dummy blocks uncoded, early_stop leaves bits unsent, sixty_four_scans
# never codes chroma's AC coefficients)
CRAFTED_EQUAL = ("plain_gray_rst", "three_refinements_rst", "escapes", "two_large_444", "threshold_420", "threshold_420_below", "deep_levels")
CRAFTED_REFUSED = "pillow_like_four"  # four components: JPEGGPU_NOT_SUPPORTED


def crafted_progressive():
    """name -> (progressive file, the baseline file its coefficients come from): tests/progressive_cases.crafted() and
    structure(), scan scripts Pillow cannot write."""
    from tests import progressive_cases

    out = dict(progressive_cases.crafted())
    out.update(progressive_cases.structure())
    return out


# ---- the coding limits (jpeggpu_ext.h: an AC coefficient of category above 10, a DC difference of category above 11) ----

S420 = ((2, 2), (1, 1), (1, 1))
AC_CODABLE, AC_UNCODABLE = (1023, -1023), (1024, -1024, 2047, 16383, -16384)
_limits = None


def _limit_file(route, w, h, sampling, grids, restart=0):
    """One file of the given per-component coefficient grids [by, bx, 64] (natural order, DC absolute), unit quantisers."""
    from tests import progressive_ref as P
    from tools import jpegsynth

    if route == "progressive":
        return P.encode(w, h, list(sampling), {0: np.ones(64, np.int64)}, [0] * len(sampling), grids, P.script_three_refinements(len(sampling)), restart=restart)
    if len(sampling) == 1:
        return jpegsynth.encode_blocks(grids[0].reshape(-1, 64), grids[0].shape[1], np.ones(64, np.uint8), restart, optimize=True)
    dc, ac = P._flat_table(16, 5)[:2], P._flat_table(256, 9)[:2]  # a code for every symbol a 16-bit coefficient can need
    return jpegsynth.encode_custom(w, h, sampling, grids, [dc], [ac], tables=[(0, 0)] * 3, restart_interval=restart)


def limit_sources():
    """The sources at the coding limits, each built both ways -- a baseline file (tools/jpegsynth: the symbol-stream branch
    of the gather) and a progressive one (tests/progressive_ref.encode, three refinement levels: the coefficient-array
    branch). A list of dicts:
        name, route ("baseline" | "progressive"), data, w, h, sampling ("grey" | "4:2:0"),
        codable   {restart interval of the target: bool}; every source is tried at 0, the restart pair also at 1
        where     (block of the target's MCU stream, zigzag index, value) of the coefficient the case is about (for a DC
                  case the second block of the pair, or the lone block)
    Zigzag index 1 is natural index 1, zigzag 63 natural 63."""
    global _limits
    if _limits is not None:
        return _limits
    out = []

    def background(by, bx, seed):
        rng = np.random.default_rng(seed)
        g = np.zeros((by, bx, 64), np.int16)
        g[..., 0] = rng.integers(-20, 21, (by, bx))
        g[..., 1] = rng.integers(-3, 4, (by, bx))
        g[..., 8] = rng.integers(-2, 3, (by, bx))
        return g

    def add(name, w, h, sampling, grids, codable, where, restart=0):
        for route in ("baseline", "progressive"):
            out.append(dict(name="%s_%s" % (name, route), route=route, data=_limit_file(route, w, h, FACTOR_LISTS[sampling], grids, restart), w=w, h=h,
                            sampling=sampling, codable=codable, where=where))

    # AC: the last codable magnitude and values beyond it, at both ends of the zigzag, in block 2 of a 2 x 2 grey file
    for v in AC_CODABLE + AC_UNCODABLE:
        for zz in (1, 63):
            g = background(2, 2, 1)
            g[1, 0, zz] = v
            add("ac_%d_zz%d" % (v, zz), 16, 16, "grey", [g], {0: abs(v) < 1024}, (2, zz, v))
    # ... in a luma and in a chroma block of a 4:2:0 source (2 x 2 MCUs of 6 blocks)
    for comp, block, at in (("luma", 6 + 3, (0, 1, 3)), ("chroma", 12 + 5, (2, 1, 0))):
        for v in (1023, 1024):
            grids = [background(4, 4, 2), background(2, 2, 3), background(2, 2, 4)]
            grids[at[0]][at[1], at[2], 63] = v
            add("ac_%s_%d" % (comp, v), 32, 32, "4:2:0", grids, {0: v < 1024}, (block, 63, v))
    # ... in a block of the item's second tile: grey 136 x 136, 289 blocks
    for v in (-1023, -1024):
        g = background(17, 17, 5)
        g[16, 8, 1] = v
        add("ac_second_tile_%d" % v, 136, 136, "grey", [g], {0: abs(v) < 1024}, (16 * 17 + 8, 1, v))
    # DC differences of 2047 and 2048, both signs: the first block (against 0), the second, across an MCU row's end
    for sign in (1, -1):
        for d in (2047, 2048):
            g = background(2, 2, 6)
            g[0, 0, 0] = sign * d
            g[0, 1, 0] = sign * (d - 1024)  # (the difference behind it stays small)
            g[1, 0, 0] = sign * (d - 1030)
            add("dc_first_%d" % (sign * d), 16, 16, "grey", [g], {0: d < 2048}, (0, 0, sign * d))
            lo, hi = (-1024, d - 1024) if sign > 0 else (1023, 1023 - d)
            g = background(2, 2, 7)
            g[0, 0, 0], g[0, 1, 0] = lo, hi
            add("dc_second_%d" % (sign * d), 16, 16, "grey", [g], {0: d < 2048}, (1, 0, hi))
            g = background(2, 2, 8)
            g[0, 1, 0], g[1, 0, 0] = lo, hi
            add("dc_row_%d" % (sign * d), 16, 16, "grey", [g], {0: d < 2048}, (2, 0, hi))
            grids = [background(4, 4, 9), background(2, 2, 10), background(2, 2, 11)]  # Cr of MCU 0 and of MCU 1
            grids[2][0, 0, 0], grids[2][0, 1, 0] = lo, hi
            add("dc_chroma_%d" % (sign * d), 32, 32, "4:2:0", grids, {0: d < 2048}, (6 + 5, 0, hi))
    # the restart dependence: 1023 and -1025 in neighbouring MCUs; with an interval of 1 every difference is the DC itself
    g = background(2, 2, 12)
    g[0, 0, 0], g[0, 1, 0] = 1023, -1025
    add("dc_restart_pair", 16, 16, "grey", [g], {0: False, 1: True}, (1, 0, -1025))
    grids = [background(4, 4, 13), background(2, 2, 14), background(2, 2, 15)]
    grids[1][0, 1, 0], grids[1][1, 0, 0] = 1023, -1025  # Cb of MCUs 1 and 2
    add("dc_restart_pair_chroma", 32, 32, "4:2:0", grids, {0: False, 1: True}, (12 + 4, 0, -1025))
    _limits = out
    return out


FACTOR_LISTS = {"grey": ((1, 1),), "4:2:0": S420}
