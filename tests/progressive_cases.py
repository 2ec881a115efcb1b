"""The inputs of the progressive tests, shared by the host and the GPU tests: Pillow's pinned files
(tests/golden/progressive_pins.npz, tools/make_progressive_pins.py) and the files tests/progressive_ref.encode writes
from the coefficients of tests/cases.matrix() files, with scan scripts no encoder at hand produces; the large files of
tests/golden/progressive_large.npz (tools/make_progressive_large.py) and small files at the edges of the work list and
of the level structure (STRUCTURE)."""
import functools
import os

import numpy as np

from tests import progressive_ref as pr
from tests.conftest import GOLDEN

SCALES = (1, 2, 4, 8)


@functools.lru_cache(maxsize=1)
def pins():
    """name -> (progressive file, baseline twin, {d: Pillow's RGB})."""
    z = np.load(os.path.join(GOLDEN, "progressive_pins.npz"))
    return {str(n): (z["prog/%s" % n].tobytes(), z["twin/%s" % n].tobytes(), {d: z["rgb/%s/%d" % (n, d)] for d in SCALES})
            for n in z["names"]}


# (case name, file of tests/cases.matrix(), scan script, restart interval in MCUs of each scan, AC code length)
CRAFTED = (
    ("plain_420", "odd_17x9", "plain", 0, 9),                 # non-interleaved DC scans, Al = 0 throughout
    ("plain_gray_rst", "gray", "plain", 3, 11),               # ... with restart intervals; AC codes longer than the look-up
    ("three_refinements_420", "ss_2x2", "three_refinements", 0, 9),
    ("three_refinements_rst", "odd_partial_mcu", "three_refinements", 2, 10),
    ("single_bands_420", "ss_2x2", "single_bands", 0, 11),    # bands of one coefficient; EOB runs over the whole scan
    ("single_bands_rst", "ss_2x1", "single_bands", 5, 9),     # ... cut at every restart
    ("pillow_like_four", "four_comp_opt", "pillow_like", 4, 9),
    ("escapes", "dense_escapes", "three_refinements", 0, 9),  # |coefficient| >= 512: the escape entries of the hand-over; ZRLs in refinement
    ("early_stop_420", "ss_2x2", "early_stop", 0, 9),         # unrefined bits, a band never coded
    ("early_stop_gray_rst", "gray", "early_stop", 7, 11),
)
COMPLETE = tuple(c[0] for c in CRAFTED if not c[0].startswith("early_stop"))


class Large:
    """One file of tests/golden/progressive_large.npz: `prog`; for the photos also `twin` and `rgb`, {d: (SHA-256 of
    Pillow's RGB bytes, its shape)}."""

    def __init__(self, prog, twin=None, rgb=None):
        self.prog, self.twin, self.rgb = prog, twin, rgb


@functools.lru_cache(maxsize=1)
def large():
    """name -> Large (tools/make_progressive_large.py): eob_ladder, eob_cap, photo, photo_rst."""
    z = np.load(os.path.join(GOLDEN, "progressive_large.npz"))
    out = {}
    for n in map(str, z["names"]):
        if "twin/" + n in z.files:
            rgb = {d: (z["rgb_sha256/%s/%d" % (n, d)].tobytes(), tuple(int(v) for v in z["rgb_shape/%s/%d" % (n, d)])) for d in SCALES}
            out[n] = Large(z["prog/" + n].tobytes(), z["twin/" + n].tobytes(), rgb)
        else:
            out[n] = Large(z["prog/" + n].tobytes())
    return out


def script_sixty_four(nc):
    """The most scans the decoder takes, all of one level: the DC scan and a band per AC coefficient of component 0 (the
    other components' AC coefficients are never coded)."""
    return [(tuple(range(nc)), 0, 0, 0, 0)] + [((0,), k, k, 0, 0) for k in range(1, 64)]


def script_deep_levels(nc):
    """The longest ladder of refinements: DC from Al = 13 down (14 levels), AC from Al = 3 down."""
    out = [(tuple(range(nc)), 0, 0, 0, 13)] + [((c,), 1, 63, 0, 3) for c in range(nc)]
    out += [(tuple(range(nc)), 0, 0, al + 1, al) for al in range(12, -1, -1)]
    for al in (2, 1, 0):
        out += [((c,), 1, 63, al + 1, al) for c in range(nc)]
    return out


S420, S444, GREY = ((2, 2), (1, 1), (1, 1)), ((1, 1), (1, 1), (1, 1)), ((1, 1),)
# (case name, width, height, sampling, scan script, restart interval): the work list's and the level structure's edges
STRUCTURE = (
    ("two_large_444", 72, 72, S444, "plain", 1),         # 81 segments in every scan: several large scans in one level
    ("threshold_420", 128, 64, S420, "plain", 2),        # luma scans of exactly 64 segments, chroma 16
    ("threshold_420_below", 128, 64, S420, "plain", 3),  # ... of 43 and 11: nothing is large
    ("sixty_four_scans", 40, 24, S420, "sixty_four", 0),
    ("deep_levels", 40, 24, GREY, "deep_levels", 0),
)


@functools.lru_cache(maxsize=1)
def structure():
    """name -> (progressive file, the baseline file its coefficients come from), as crafted()."""
    from oracle import oracle
    from tools import jpegsynth

    out = {}
    for k, (name, w, h, sampling, script, restart) in enumerate(STRUCTURE):
        dense = name == "sixty_four_scans"  # every one of its 63 bands is to hold a coefficient
        src = jpegsynth.encode(w, h, sampling, quality=100 if dense else 90, noise=40 if dense else 10, seed=900 + k)
        o = oracle.decode(src)
        script = globals().get("script_" + script) or getattr(pr, "script_" + script)
        f = pr.encode(o.width, o.height, list(zip(o.hs, o.vs)), {q: o.qtab[q] for q in set(o.qidx)}, o.qidx, o.coef, script(o.ncomp),
                      restart=restart, ac_len=10 if k % 2 else 9)
        out[name] = (f, src)
    return out


@functools.lru_cache(maxsize=None)
def restated(data):
    """progressive_ref.decode of a file with its statistics, (Decoded, stats): computed once per file and shared (read-only)."""
    stats = []
    return pr.decode(data, stats), stats


@functools.lru_cache(maxsize=1)
def crafted():
    """name -> (progressive file, the baseline file its coefficients come from)."""
    from oracle import oracle
    from tests import cases

    m = cases.matrix()
    out = {}
    for name, src, script, restart, ac_len in CRAFTED:
        o = oracle.decode(m[src])
        sampling = list(zip(o.hs, o.vs))
        f = pr.encode(o.width, o.height, sampling, {q: o.qtab[q] for q in set(o.qidx)}, o.qidx, o.coef,
                      getattr(pr, "script_" + script)(o.ncomp), restart=restart, ac_len=ac_len, jfif=o.ncomp != 4)
        out[name] = (f, m[src])
    return out
