"""The inputs of the progressive tests, shared by the host and the GPU tests: Pillow's pinned files
(tests/golden/progressive_pins.npz, tools/make_progressive_pins.py) and the files tests/progressive_ref.encode writes
from the coefficients of tests/cases.matrix() files, with scan scripts no encoder at hand produces."""
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
