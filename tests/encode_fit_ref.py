"""CPU restatement of encoding to a byte budget (jpeggpu_ext_encode_fit_batch), on top of tests/encode_ref.py and
tests/encode_opt_ref.py: the rule that picks the quality, word for word as include/jpeggpu/jpeggpu_ext.h states it, over the
restated encoder's file sizes. tools/make_encode_fit_pins.py runs the same rule over Pillow's files
(tests/golden/encode_fit_pins.npz); tests/test_encode_fit_ref.py compares the two, tests/test_gpu_encode_fit.py runs the device.

    choose(size, lo, hi, budget) -> quality, or None when even `lo` is over budget;  size: q -> bytes
    largest_fitting(size, lo, hi, budget) -> the largest quality of lo..hi that fits, or None: NOT what the call promises
    evaluations(lo, hi) -> how many sizes the rule looks at, at most
    budgets(table, lo, hi) -> the budgets the tests place on a table of sizes: its ends, its median, its dips
    cases(), image(case), encode(case, quality), pins()
"""
import hashlib
import json
import os

import numpy as np

from tests import encode_cases as K
from tests import encode_opt_ref as O

OVER_BUDGET = 5  # JPEGGPU_EXT_ENCODE_OVER_BUDGET


def choose(size, lo, hi, budget):
    """The contract. `size(q)` is the length of the encoder's file at quality q; it is not monotone in q."""
    if size(hi) <= budget:
        return hi
    if size(lo) > budget:
        return None
    best, a, b = lo, lo + 1, hi - 1
    while a <= b:
        m = (a + b) // 2
        if size(m) <= budget:
            best, a = m, m + 1
        else:
            b = m - 1
    return best


def largest_fitting(size, lo, hi, budget):
    fits = [q for q in range(lo, hi + 1) if size(q) <= budget]
    return max(fits) if fits else None


def evaluations(lo, hi):
    """The most sizes choose() asks for: 1, 2, or quality_max, quality_min and a bisection of hi - lo - 1 values."""
    w = hi - lo + 1
    return w if w <= 2 else 2 + (w - 2).bit_length()


def launches(lo, hi, optimize):
    """What the header states for a call whose widest range is lo..hi."""
    p = evaluations(lo, hi)
    return 12 + 10 * p if optimize else 10 + 8 * p


def dips(table, lo, hi):
    """The qualities q of lo..hi - 1 with size(q + 1) < size(q). `table`: {q: bytes} or a sequence indexed by q."""
    return [q for q in range(lo, hi) if table[q + 1] < table[q]]


def budgets(table, lo, hi, max_dips=None):
    """The budgets the tests place on a table: size(hi) and a byte less, size(lo) and a byte less (over budget), the median
    of the table, and in every dip (the first `max_dips` of them) the size at its bottom: q + 1 fits, q does not."""
    sizes = sorted(table[q] for q in range(lo, hi + 1))
    out = [table[hi], table[hi] - 1, table[lo], table[lo] - 1, sizes[len(sizes) // 2]]
    for q in dips(table, lo, hi)[:max_dips]:
        out.append(table[q + 1])
    seen, uniq = set(), []
    for b in out:
        if b not in seen and b >= 0:
            seen.add(b)
            uniq.append(b)
    return uniq


# (w, h): a single sample, one block, partial blocks and MCUs at both edges under every subsampling, dummy blocks, a few
# hundred blocks
SIZES = [(1, 1), (8, 8), (17, 9), (37, 39), (59, 24), (65, 11), (120, 80)]
SUBSAMPLINGS = ["4:4:4", "4:2:2", "4:2:0"]
INTERVALS = [0, 1, 3]
CONTENTS = ["gradient", "noise", "photo"]
# beside the full range: two qualities, one quality, and a range that starts and ends inside
RANGES = [(1, 100), (1, 100), (1, 95), (40, 41), (50, 50), (10, 90)]


def cases():
    """42 cases: every size with six combinations that rotate through colour, content, subsampling, restart interval,
    `optimize` and the range of qualities."""
    out = []
    for si, (w, h) in enumerate(SIZES):
        for t in range(6):
            k = 6 * si + t
            grey = k % 4 == 3
            c = K._case("", h, w, grey, CONTENTS[(si + t) % 3], 75, SUBSAMPLINGS[(k + si) % 3], INTERVALS[(k // 2) % 3], seed=500 + k)
            c["optimize"] = (t + si) % 2 == 1
            c["lo"], c["hi"] = RANGES[(t + si) % 6]
            c["name"] = "fit_%dx%d_%s_%s_%s_r%d_%s_q%d_%d" % (w, h, c["content"], "grey" if grey else "rgb", c["subsampling"].replace(":", ""),
                                                            c["restart_interval"], "opt" if c["optimize"] else "std", c["lo"], c["hi"])
            out.append(c)
    # the standing example of a table that is not monotone: a 37 x 39 gradient at 4:2:0 over the whole range
    c = K._case("fit_37x39_gradient_rgb_420_r0_std_q1_100_example", 39, 37, False, "gradient", 75, "4:2:0", 0, seed=0)
    c["optimize"], c["lo"], c["hi"] = False, 1, 100
    out.append(c)
    return out


def image(case):
    return K.image(case)


def encode(case, quality, img=None):
    """The restated encoder's file of a case at a quality."""
    return O.encode(image(case) if img is None else img, quality, case["subsampling"], case["restart_interval"], optimize=case["optimize"])


def fit(case, budget, lo=None, hi=None):
    """(quality or None, file or None) by the rule over the restated encoder."""
    img, files = image(case), {}

    def size(q):
        if q not in files:
            files[q] = encode(case, q, img)
        return len(files[q])

    q = choose(size, case["lo"] if lo is None else lo, case["hi"] if hi is None else hi, budget)
    return q, None if q is None else files[q]


_pins = None


def pins():
    """({case name: dict(table={q: bytes} for q 1..100, budgets=[dict(budget, quality (-1: over budget), length, sha256)],
    files={quality: bytes} of the files stored whole)}, versions) from tests/golden/encode_fit_pins.npz."""
    global _pins
    if _pins is None:
        z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encode_fit_pins.npz"))
        meta = json.loads(z["meta"].tobytes().decode())
        table = {}
        for e in meta["cases"]:
            sizes = z["sizes_" + e["name"]]
            table[e["name"]] = dict(table={q: int(sizes[q - 1]) for q in range(1, 101)}, budgets=e["budgets"],
                                    files={int(q): z["file_%s_q%d" % (e["name"], q)].tobytes() for q in e["whole"]})
        _pins = (table, {k: v for k, v in meta.items() if k != "cases"})
    return _pins


def equals_pin(name, budget_entry, data):
    """Whether `data` is the pinned file of a budget entry: its bytes where the pin holds them, its length and SHA-256 otherwise."""
    whole = pins()[0][name]["files"].get(budget_entry["quality"])
    if whole is not None:
        return data == whole
    return len(data) == budget_entry["length"] and hashlib.sha256(data).hexdigest() == budget_entry["sha256"]
