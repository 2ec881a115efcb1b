"""The restatement of encoding with optimised Huffman tables (tests/encode_opt_ref.py) against Pillow's pinned
optimize=True files (tests/golden/encode_opt_pins.npz), against a live Pillow where one on libjpeg-turbo is importable, and
jpeg_gen_optimal_table on crafted counts. No GPU needed."""
import io

import numpy as np
import pytest

from tests import encode_cases as K
from tests import encode_opt_ref as R
from tests import encode_ref as E

CASES = K.cases()


def _kraft(bits):
    return sum(n * 2 ** (16 - (i + 1)) for i, n in enumerate(bits))


def test_restatement_equals_every_pin():
    """All cases of encode_cases.cases() and the edge images, none left out."""
    todo = [(c, K.image(c)) for c in CASES] + R.edge_cases()
    pins = R.pins()[0]
    assert len(todo) == len(pins) == len(CASES) + 5
    wrong = [c["name"] for c, img in todo if not R.equals_pin(c["name"], R.encode(img, c["quality"], c["subsampling"], c["restart_interval"]))]
    assert not wrong, wrong
    assert R.pins()[1] == K.pins()[1], "both pin files come from the same Pillow and libjpeg-turbo"


def test_optimised_files_are_not_longer_and_differ():
    pins, plain = R.pins()[0], K.pins()[0]
    assert all(pins[c["name"]]["length"] <= plain[c["name"]]["length"] for c in CASES)
    assert sum(pins[c["name"]]["length"] < plain[c["name"]]["length"] for c in CASES) == len(CASES)


def test_the_cases_reach_the_hard_paths():
    """Length limiting (code lengths of 17 and more before it) and tables of a single symbol, as the case list promises."""
    limited, single = [], 0
    for c, img in [(c, K.image(c)) for c in CASES if c["name"] in ("scan_lanes_plus", "scan_lanes_plus_420_r11", "real_640x427_grey_r3", "real_640x427")] + R.edge_cases()[4:]:
        hs, vs = E.SUBSAMPLINGS[c["subsampling"]]
        co = E.coefficients(img, hs, vs, c["quality"])
        counts = R.symbol_counts(co, c["restart_interval"])
        deepest = max(R.depth_before_limiting(counts[t, cls]) for t in range(1 if c["grey"] else 2) for cls in (0, 1))
        if deepest > 16:
            limited.append(c["name"])
    assert limited == ["scan_lanes_plus", "scan_lanes_plus_420_r11", "real_640x427_grey_r3", "opt_fibonacci_664_grey"]
    for c, img in R.edge_cases()[:2]:
        t = R.tables(img, c["quality"], c["subsampling"], c["restart_interval"])
        single += sum(len(x[1]) == 1 for x in t if x is not None)
    assert single == 4 + 2  # every table of the flat RGB image, both of the zero grey one


def test_live_pillow_on_a_seeded_subset():
    Image = pytest.importorskip("PIL.Image")
    from PIL import ImageFile, features

    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("this Pillow is not built on libjpeg-turbo")
    rng = np.random.default_rng(99)
    saved = ImageFile.MAXBLOCK
    ImageFile.MAXBLOCK = 1 << 24
    try:
        for _ in range(20):
            h, w = (int(v) for v in rng.integers(1, 60, 2))
            grey = bool(rng.integers(0, 2))
            img = rng.integers(0, 256, (h, w) if grey else (h, w, 3), dtype=np.uint8)
            if rng.integers(0, 2):
                img = (img // 64 * 64).astype(np.uint8)
            q, s, r = int(rng.integers(1, 101)), ["4:4:4", "4:2:2", "4:2:0"][int(rng.integers(0, 3))], [0, 1, 5][int(rng.integers(0, 3))]
            f = io.BytesIO()
            Image.fromarray(img).save(f, "JPEG", quality=q, subsampling=E.PILLOW_SUBSAMPLING[E.SUBSAMPLINGS[s]], restart_marker_blocks=r, optimize=True)
            assert R.encode(img, q, s, r) == f.getvalue(), (h, w, grey, q, s, r)
    finally:
        ImageFile.MAXBLOCK = saved


def _one(symbol, count=5):
    c = np.zeros(256, np.int64)
    c[symbol] = count
    return c


def test_gen_optimal_table_one_symbol():
    bits, values, status = R.gen_optimal_table(_one(0x21))
    assert status == R.OK and values == [0x21]
    assert bits == [1] + [0] * 15, "one bit: the pseudo-symbol took the other code of that length and left"


def test_gen_optimal_table_two_equal():
    c = _one(3) + _one(9)
    bits, values, status = R.gen_optimal_table(c)
    assert status == R.OK and values == [3, 9]
    assert bits == [1, 1] + [0] * 14, "the pseudo-symbol merges with symbol 9 first (the largest index among the least counts)"


def test_gen_optimal_table_256_equal():
    bits, values, status = R.gen_optimal_table(np.full(256, 7))
    assert status == R.OK and sorted(values) == list(range(256))
    assert sum(bits) == 256 and _kraft(bits) + 2 ** (16 - max(i + 1 for i, n in enumerate(bits) if n)) <= 2 ** 16, "room for the all-ones code"
    assert bits[7] == 255 and bits[8] == 1  # 255 codes of 8 bits, one of 9 whose sibling was the pseudo-symbol
    assert values[-1] == 255, "symbol 255 merged with the pseudo-symbol"


def test_gen_optimal_table_fibonacci_20_is_limited():
    c = R.fib_counts(20)
    assert R.depth_before_limiting(c) == 20
    bits, values, status = R.gen_optimal_table(c)
    assert status == R.OK and sum(bits) == 20 and len(values) == 20
    assert values == list(range(19, -1, -1)), "by code length before limiting: the most frequent first"
    assert _kraft(bits) < 2 ** 16, "a prefix code of at most 16 bits with the all-ones code free"


def test_gen_optimal_table_fibonacci_33_overflows():
    assert R.depth_before_limiting(R.fib_counts(32)) == 32
    assert R.gen_optimal_table(R.fib_counts(32))[2] == R.OK
    assert R.depth_before_limiting(R.fib_counts(33)) == 33
    assert R.gen_optimal_table(R.fib_counts(33)) == (None, None, R.OVERFLOW)


def test_gen_optimal_table_tie_rule_on_merged_sums():
    """Counts 1, 1, 2, 2 (and the pseudo-symbol's 1): after two merges a sum equals a symbol's count, and which of them is
    taken decides the lengths. libjpeg takes the LARGEST index among equals."""
    c = np.zeros(256, np.int64)
    c[[10, 20, 30, 40]] = [1, 1, 2, 2]
    bits, values, status = R.gen_optimal_table(c)
    assert status == R.OK
    # 256 + 20 -> 2 at 256; then the least is 10 (1) and, among the 2s, 256 (the largest index): 10 + 256 -> 3 at 10;
    # then 40 + 30 -> 4 at 40; then 10 (3) + 40 (4). With the smallest index among equals 30 would have met the sum of 2
    # instead, and 10 would be a bit longer than 40.
    assert values == [10, 30, 40, 20]
    assert bits == [0, 3, 1] + [0] * 13  # 10, 30, 40: 2 bits; 20 and the pseudo-symbol: 3, and the pseudo-symbol leaves
    assert R.gen_optimal_table(np.zeros(256, np.int64))[2] == R.EMPTY


def test_symbol_counts_agree_with_the_entropy_coder():
    """The counted symbols, coded with the Annex K tables, are the bits of the standard stream (value bits counted apart)."""
    for name in ("37x53_noise_rgb_q95_422_r3", "zrl_sparse_rgb", "dc11_black_white_blocks"):
        c = next(c for c in CASES if c["name"] == name)
        hs, vs = E.SUBSAMPLINGS[c["subsampling"]]
        co = E.coefficients(K.image(c), hs, vs, c["quality"])
        counts = R.symbol_counts(co, c["restart_interval"])
        assert counts[:, 0].sum() == len(co["coefs"]), "one DC symbol per block"
        nz = np.count_nonzero(co["coefs"][:, 1:])
        assert counts[:, 1].sum() - counts[:, 1, 0].sum() - counts[:, 1, 0xF0].sum() == nz
        assert counts[:, 0, 12:].sum() == 0 and (c["grey"] or counts[1].sum() > 0)
