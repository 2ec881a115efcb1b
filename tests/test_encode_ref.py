"""The encoder's CPU restatement (tests/encode_ref.py) against Pillow's files (tests/golden/encode_pins.npz), and the case
list's coverage: every symbol and edge case the device must get right occurs in it. No GPU, no Pillow."""
import functools

import numpy as np
import pytest

from tests import encode_cases as K
from tests import encode_ref as E

CASES = K.cases()


@functools.lru_cache(maxsize=None)
def _encoded(i):
    c, stats = CASES[i], {}
    data = E.encode(K.image(c), c["quality"], c["subsampling"], c["restart_interval"], stats)
    return data, stats


def test_case_names_are_unique_and_pinned():
    names = [c["name"] for c in CASES]
    assert len(set(names)) == len(names)
    assert set(names) == set(K.pins()[0])
    assert K.pins()[1]["libjpeg_turbo"], "the pins record the library that wrote them"


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c["name"] for c in CASES])
def test_restatement_equals_pin(i):
    data, _ = _encoded(i)
    assert K.equals_pin(CASES[i]["name"], data)


def test_quantisation_tables_follow_jpeg_set_quality():
    """The DQT payloads of the pinned files at every quality are the rule's tables, in zigzag order."""
    for q in range(1, 101):
        data = K.pins()[0]["qsweep_q%d" % q]["data"]
        p = data.index(b"\xff\xdb")
        assert data[p + 5:p + 69] == bytes(int(E.quant_table(E.BASE_LUMA, q)[z]) for z in E.ZIGZAG)
        assert data[p + 69 + 5:p + 69 + 69] == bytes(int(E.quant_table(E.BASE_CHROMA, q)[z]) for z in E.ZIGZAG)


def test_case_list_covers_every_symbol_and_edge():
    total = {}
    for i in range(len(CASES)):
        for k, v in _encoded(i)[1].items():
            total[k] = max(total.get(k, 0), v)
    assert total["zrl"] >= 1
    assert total["no_eob"] >= 1, "a block whose last coefficient is coded ends without EOB"
    assert total["max_dc_category"] == 11
    assert total["max_ac_category"] == 10
    assert total["stuffed_bytes"] >= 1
    assert total["stuffed_padding_bytes"] >= 1, "a 0xFF completed by the padding ones is stuffed too"
    assert total["restart_markers"] > 8, "the restart counter wraps past RST7"
    assert total["dummy_right"] >= 1 and total["dummy_bottom"] >= 1 and total["dummy_corner"] >= 1


def test_corner_chain_of_three():
    """An MCU of which only the first luma block is real: the three others copy its DC, each from the one before."""
    c = next(c for c in CASES if c["name"].startswith("37x53") and c["subsampling"] == "4:2:0" and not c["grey"])
    co = E.coefficients(K.image(c), 2, 2, c["quality"])
    last = co["coefs"][-6:]  # the bottom-right MCU
    assert list(co["dummy"][-6:-2]) == [0, 1, 2, 3]
    assert (last[1:4, 0] == last[0, 0]).all() and not last[1:4, 1:].any()


def test_sizes_at_the_kernels_tiles():
    by_name = {c["name"]: i for i, c in enumerate(CASES)}
    st = _encoded(by_name["tile_plus_one_block"])[1]
    assert st["blocks"] == K.TILE_BLOCKS + 1
    st = _encoded(by_name["chunk_plus_few_bytes"])[1]
    assert K.CHUNK_BYTES < st["unstuffed_bytes"] <= K.CHUNK_BYTES + 64
    st = _encoded(by_name["scan_lanes_plus"])[1]
    assert st["blocks"] > K.SCAN_THREADS * K.TILE_BLOCKS and st["unstuffed_bytes"] > K.SCAN_THREADS * K.CHUNK_BYTES
    st = _encoded(by_name["scan_lanes_plus_420_r11"])[1]
    assert st["unstuffed_bytes"] > K.SCAN_THREADS * K.CHUNK_BYTES and st["restart_markers"] > 8


def test_even_height_bottom_rule_matters():
    """4:2:0, an even height that is no multiple of 16: padding the input to the MCU height BEFORE downsampling is not what
    libjpeg does, and gives other bytes."""
    differ = 0
    for c in CASES:
        if c["name"].endswith("_bottom"):
            img = K.image(c)
            right = E.encode(img, c["quality"], c["subsampling"], c["restart_interval"])
            wrong = E.encode(img, c["quality"], c["subsampling"], c["restart_interval"], bottom_rule="mcu_first")
            assert K.equals_pin(c["name"], right)
            differ += right != wrong
    assert differ >= 1


def test_forward_dct_is_eight_times_the_dct():
    rng = np.random.default_rng(5)
    b = rng.integers(-128, 128, (20, 8, 8)).astype(np.int64)
    k = np.arange(8)
    m = np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / 16) * np.where(k[:, None] == 0, np.sqrt(1 / 8), np.sqrt(2 / 8))
    true = m @ b.astype(np.float64) @ m.T
    assert np.abs(E.fdct_islow(b) - 8 * true).max() < 1.5
