"""The CPU restatement of a JPEG round trip (tests/roundtrip_ref.py) against Pillow's pinned outputs
(tests/golden/roundtrip_pins.npz, written by tools/make_roundtrip_pins.py): every case, exactly. No GPU and no Pillow needed."""
import os

import numpy as np
import pytest

from tests import roundtrip_ref as R

PINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "roundtrip_pins.npz")


@pytest.fixture(scope="module")
def pins():
    return np.load(PINS)


def test_the_pins_hold_the_cases(pins):
    cases = R.cases()
    assert np.array_equal(pins["cases"], R.case_table(cases))
    assert pins["sha256"].shape == (len(cases), 32) and pins["small_off"].shape == (len(cases) + 1,)
    stored = np.diff(pins["small_off"]) > 0
    assert np.array_equal(stored, np.array([w * h <= R.STORED_PIXELS for _, w, h, *_ in cases]))
    assert int(pins["small_off"][-1]) == pins["small"].size
    assert os.path.getsize(PINS) <= os.path.getsize(os.path.join(os.path.dirname(PINS), "encode_pins.npz"))
    # what the cases are chosen for: sides below a block, a downsampled width of at most 2, odd sides under 4:2:0, several MCU rows
    sizes = set((w, h) for _, w, h, *_ in cases)
    assert {(1, 1), (3, 2), (9, 17), (250, 131)} <= sizes and len(cases) == 12 * (30 + 90)


@pytest.mark.parametrize("size", R.SIZES, ids=lambda s: "%dx%d" % s)
def test_restatement_equals_every_pin(pins, size):
    n = 0
    for i, case in enumerate(R.cases()):
        name, w, h, _, _, ss, q, _ = case
        if (w, h) != size:
            continue
        assert R.matches_pin(pins, i, R.roundtrip(R.case_input(case), q, ss)), name
        n += 1
    assert n == 120


def test_wrap_block_needs_the_range_limits_wrap(monkeypatch):
    """R.WRAP_BLOCK keeps its purpose: with jidctint.c's range limit the sample at R.WRAP_AT is 255, with a plain clamp 0,
    and nothing else differs."""
    from tests import libjpeg_ref as L

    exact = R.roundtrip(R.WRAP_BLOCK, 1)
    monkeypatch.setattr(L, "range_limit", lambda x: np.clip(np.asarray(x) + 128, 0, 255).astype(np.uint8))
    clamped = R.roundtrip(R.WRAP_BLOCK, 1)
    assert exact[R.WRAP_AT] == 255 and clamped[R.WRAP_AT] == 0
    assert [tuple(p) for p in np.argwhere(exact != clamped)] == [R.WRAP_AT]


def test_a_pin_notices_one_wrong_sample(pins):
    for i in (0, len(R.cases()) - 1):  # one stored as an array, one by its SHA-256
        case = R.cases()[i]
        a = R.roundtrip(R.case_input(case), case[6], case[5]).copy()
        assert R.matches_pin(pins, i, a)
        a.flat[-1] ^= 1
        assert not R.matches_pin(pins, i, a)
