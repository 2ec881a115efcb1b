"""The encoder's CPU restatement (tests/encode_ref.py) against Pillow's files (tests/golden/encode_pins.npz), and the case
list's coverage: every symbol and edge case the device must get right occurs in it. The same for the sweep, the edge cases and
the big calls of tests/test_gpu_encode_scale.py (tests/golden/encode_sweep_pins.npz): what the draw covers, which coefficients
the edge images reach, and the tile and chunk structure the two big calls are there for. No GPU, no Pillow."""
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


# ------------------------------------------------------------------------------------------------
# the sweep, the edge cases and the big calls of tests/test_gpu_encode_scale.py (tests/golden/encode_sweep_pins.npz)
# ------------------------------------------------------------------------------------------------

NEW = K.new_cases()
NEW_INDEX = {c["name"]: i for i, c in enumerate(NEW)}


@functools.lru_cache(maxsize=None)
def _encoded_new(i):
    c, stats = NEW[i], {}
    data = E.encode(K.image(c), c["quality"], c["subsampling"], c["restart_interval"], stats)
    return len(data), K.equals_pin(c["name"], data), stats  # (not the files: the lattice's are megabytes)


def test_new_case_names_are_unique_and_pinned():
    names = [c["name"] for c in NEW]
    assert len(set(names)) == len(names) and not set(names) & set(K.pins()[0])
    assert set(names) == set(K.sweep_pins()[0])
    assert K.sweep_pins()[1] == K.pins()[1], "both pin files come from the same Pillow and libjpeg-turbo"
    assert all(p["data"] is None for p in K.sweep_pins()[0].values())
    assert [int(c["name"].split("_")[1]) for c in K.sweep()] == list(range(K.SWEEP_COUNT)), "a sweep case's name carries its index"


@pytest.mark.parametrize("i", range(len(NEW)), ids=[c["name"] for c in NEW])
def test_restatement_equals_new_pin(i):
    length, equal, _ = _encoded_new(i)
    assert length == K.pin_of(NEW[i]["name"])["length"] and equal


def test_sweep_covers_geometry_and_parameters():
    sweep = K.sweep()
    rgb = lambda s: [c for c in sweep if not c["grey"] and c["subsampling"] == s]  # noqa: E731
    assert {c["w"] % 16 for c in rgb("4:2:0")} == set(range(16))
    assert {c["w"] % 16 for c in rgb("4:2:2")} == set(range(16))
    assert {c["h"] % 16 for c in rgb("4:2:0")} == set(range(16))
    for group in [[c for c in sweep if c["grey"]]] + [rgb(s) for s in K.SUBSAMPLINGS]:
        assert {c["restart_interval"] for c in group} == set(K.SWEEP_INTERVALS)
    assert any(c["restart_interval"] > K.counts(c)["mcus"] for c in sweep), "an interval no MCU count reaches: one segment, but a DRI"
    assert any(c["restart_interval"] == 65535 for c in sweep)
    assert any(c["restart_interval"] and K.counts(c)["mcus_x"] % c["restart_interval"] and K.counts(c)["segments"] > 8 for c in sweep), \
        "segments that begin in the middle of an MCU row, more of them than there are RSTn"
    assert len({c["quality"] for c in sweep}) >= 60
    assert {c["content"] for c in sweep} == set(K.SWEEP_CONTENTS)
    for c in sweep:  # the restated counts are the census's
        st = _encoded_new(NEW_INDEX[c["name"]])[2]
        assert st["blocks"] == K.counts(c)["blocks"] and st["restart_markers"] == K.counts(c)["segments"] - 1


def test_edge_cases_reach_the_largest_coefficients():
    """Over the basis images: an AC coefficient of category 10 at 40 or more zigzag positions, of either sign, and a DC
    difference of category 11 -- and nothing beyond, as kMaxBlockBits assumes."""
    positive, negative, dc = set(), set(), 0
    for c in K.edge_cases():
        st = _encoded_new(NEW_INDEX[c["name"]])[2]
        assert st["max_ac_category"] <= 10 and st["max_dc_category"] <= 11
        dc = max(dc, st["max_dc_category"])
        if c["content"] == "basis":
            hs, vs = E.SUBSAMPLINGS[c["subsampling"]]
            ac = E.coefficients(K.image(c), hs, vs, c["quality"])["coefs"][:, 1:].astype(np.int64)
            positive |= set(np.nonzero((ac >= 512).any(0))[0] + 1)
            negative |= set(np.nonzero((ac <= -512).any(0))[0] + 1)
    assert dc == 11
    assert len(positive) >= 40 and len(negative) >= 40, (len(positive), len(negative))


def test_lattice_holds_every_colour():
    img = K.lattice_image()
    colours = {tuple(img[8 * by, 8 * bx]) for by in range(img.shape[0] // 8) for bx in range(img.shape[1] // 8)}
    assert len(colours) == len(K.LATTICE_LEVELS) ** 3
    assert (img.reshape(97, 8, 97, 8, 3) == img.reshape(97, 8, 97, 8, 3)[:, :1, :, :1]).all(), "every block is flat"


def test_medium_items_have_several_tiles():
    assert all(100 <= min(c["h"], c["w"]) and max(c["h"], c["w"]) <= 260 and 2 <= K.counts(c)["tiles"] <= 12 for c in K.medium())
    assert any(c["grey"] for c in K.medium()) and len({c["subsampling"] for c in K.medium()}) == 3 and len({c["restart_interval"] for c in K.medium()}) > 4


@pytest.mark.parametrize("reverse", [False, True])
def test_many_call_has_runs_with_item_boundaries(reverse):
    items = K.many_call(reverse)
    assert sorted(c["name"] for c in items) == sorted(c["name"] for c in K.sweep() + K.medium())
    first = K.starts(items, "tiles")
    tiles = first[-1]
    assert tiles > 4 * K.SCAN_THREADS and len(items) > 500
    per = -(-tiles // K.SCAN_THREADS)  # scan_before: a lane's run
    assert per >= 4
    run = lambda tile: tile // per  # noqa: E731
    n = [K.counts(c)["tiles"] for c in items]
    # a run that holds a multi-tile item's last tile, a whole one-tile item and another item's first tile: a kConst cursor in
    # the middle of a lane's run and one at its end or further in, behind kRound / kAdd tiles
    assert any(n[i] > 1 and n[i + 1] == 1 and run(first[i + 1] - 1) == run(first[i + 2]) for i in range(len(items) - 2))
    assert any(run(first[i]) != run(first[i + 1] - 1) for i in range(len(items))), "a run boundary inside an item"


def test_grid_call_lies_beyond_the_grid():
    call = K.grid_call()
    items = call["items"]
    assert len({c["name"] for c in items}) <= 8 and all((c["h"], c["w"]) == (256, 256) for c in items)
    assert K.counts(items[0])["chunks"] == 78 and K.counts(next(c for c in items if c["subsampling"] == "4:2:0"))["chunks"] == 39
    first = K.starts(items, "chunks")
    assert first[-1] > K.CHUNK_GRID
    beyond = [i for i in range(len(items)) if first[i] >= K.CHUNK_GRID]
    assert len(beyond) >= 3
    stats = lambda i: _encoded_new(NEW_INDEX[items[i]["name"]])[2]  # noqa: E731
    below, short = call["short"]
    assert first[below + 1] <= K.CHUNK_GRID and short in beyond and call["zero"] not in call["short"]
    intact = [i for i in beyond if i not in call["short"] and i != call["zero"]]
    assert any(stats(i)["restart_markers"] > 8 and stats(i)["stuffed_bytes"] > 0 for i in intact)
    assert any(stats(i)["unstuffed_bytes"] > K.CHUNK_BYTES for i in intact)
    assert stats(short)["unstuffed_bytes"] > K.CHUNK_BYTES, "the refused item's chunks behind the grid would all have been written"
    assert any(first[i] < K.CHUNK_GRID < first[i + 1] for i in range(len(items))), "and one item straddles the grid's end"
    assert {"noise", "photo"} <= {c["content"] for c in items} and any(c["grey"] for c in items)


def test_difference_report_names_the_stage(monkeypatch):
    """tests/encode_diff.py on crafted files: a changed coefficient is named by block, component and zigzag index; a fill byte
    in front of EOI leaves the coefficients equal; a truncated stream cannot be read; and an oracle that raises leaves the
    byte offset."""
    from oracle import oracle
    from tests.encode_diff import where_files_differ

    c = K.medium()[0]
    hs, vs = E.SUBSAMPLINGS[c["subsampling"]]
    co = E.coefficients(K.image(c), hs, vs, c["quality"])
    head = E.header(co["w"], co["h"], co["ncomp"], hs, vs, c["quality"], c["restart_interval"])
    want = head + E.entropy_code(co, c["restart_interval"]) + b"\xff\xd9"
    assert K.equals_pin(c["name"], want)
    co["coefs"][5, 7] += 1  # MCU 0 of a 4:2:0 image: four luma blocks, Cb, Cr
    report = where_files_differ(head + E.entropy_code(co, c["restart_interval"]) + b"\xff\xd9", want)
    assert "block 5 (MCU 0, component 2) at zigzag index 7" in report and "encode_blocks" in report and "1 of 546 blocks" in report
    report = where_files_differ(want[:-2] + b"\xff" + want[-2:], want)
    assert "coefficients are equal" in report and "packing, stuffing or markers" in report
    assert "cannot read" in where_files_differ(want[:len(head) + 3], want)
    assert "too small" in where_files_differ(None, want)

    def broken(data):
        raise RuntimeError("no oracle")

    monkeypatch.setattr(oracle, "decode", broken)
    report = where_files_differ(want[:700] + b"\x00" + want[701:], want)
    assert "first difference at byte 700" in report and "no oracle" in report
