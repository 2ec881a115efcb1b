"""tests/coefficients_ref.py against Pillow, independently of the library: on every pinned source
(tests/golden/coefficients_pins.npz: grey and the three samplings at 17 x 9 and 75 x 53, qualities 30 / 75 / 95) the write of
the read is Pillow's own file byte for byte -- plain, and with optimize=True and progressive=True Pillow's file of the same
pixels --, and libjpeg's IDCT, upsampling and colour conversion of the read coefficients are Pillow's pixels."""
import io

import numpy as np
import pytest

from tests import coefficients_ref as K
from tests import libjpeg_ref as L

CASES = K.cases()
NAMES = [c["name"] for c in CASES]


def test_pins_cover_the_cases():
    files, versions = K.pins()
    assert sorted(files) == sorted(NAMES) and len(NAMES) == 24
    assert {(c["w"], c["h"]) for c in CASES} == {(17, 9), (75, 53)} and {c["quality"] for c in CASES} == {30, 75, 95}
    assert {c["sampling"] for c in CASES} == {"grey", "4:4:4", "4:2:2", "4:2:0"}
    assert all(set(f) == {"A", "B", "C", "sha"} for f in files.values()) and "libjpeg_turbo" in versions


@pytest.mark.parametrize("name", NAMES)
def test_write_of_read_is_pillows_file(name):
    f = K.pins()[0][name]
    co = K.read(f["A"])
    assert [K.sha(c) for c in co.coef] == f["sha"]
    for kind, options in K.KINDS.items():
        assert K.write(co, **options) == f[kind], kind
    # the three files hold the same coefficients, whichever is read
    for kind in "BC":
        other = K.read(f[kind])
        assert all(np.array_equal(a, b) for a, b in zip(co.coef, other.coef)) and all(np.array_equal(a, b) for a, b in zip(co.qtables, other.qtables))
        assert other.progressive == (kind == "C")


@pytest.mark.parametrize("name", NAMES)
def test_read_coefficients_decode_to_pillows_pixels(name):
    pytest.importorskip("PIL.Image")
    f = K.pins()[0][name]
    assert np.array_equal(K.rgb(K.read(f["A"])), L.pillow_rgb(f["A"]))


def test_grids_are_the_real_ones():
    """The real grid, not the MCU-padded one: 17 x 9 in 4:2:0 is 3 x 2 luma blocks (its MCUs hold 4 x 2) and 2 x 1 of chroma (9 x 5 samples)."""
    files = K.pins()[0]
    assert [c.shape for c in K.read(files["17x9_420_q75"]["A"]).coef] == [(2, 3, 64), (1, 2, 64), (1, 2, 64)]
    assert [c.shape for c in K.read(files["17x9_422_q75"]["A"]).coef] == [(2, 3, 64), (2, 2, 64), (2, 2, 64)]
    assert [c.shape for c in K.read(files["75x53_420_q75"]["A"]).coef] == [(7, 10, 64), (4, 5, 64), (4, 5, 64)]
    assert [c.shape for c in K.read(files["75x53_grey_q75"]["A"]).coef] == [(7, 10, 64)]


def test_uncodable_values_are_refused():
    co = K.read(K.pins()[0]["17x9_420_q75"]["A"])
    bad = co.copy()
    bad.coef[0][1, 2, 5] = 1024
    with pytest.raises(K.Unsupported):
        K.write(bad)
    bad = co.copy()
    bad.coef[1][0, 0, 0] = 2048  # the first block of Cb: predicted from 0
    with pytest.raises(K.Unsupported):
        K.write(bad)
    ok = co.copy()
    ok.coef[0][1, 2, 5], ok.coef[1][0, 0, 0] = -1023, -2047
    got = K.read(K.write(ok))
    assert all(np.array_equal(a, b) for a, b in zip(ok.coef, got.coef))


def test_live_pillow_restart_intervals():
    """Pillow's restart_marker_blocks file from the plain file's coefficients, where there is a Pillow on libjpeg-turbo."""
    Image = pytest.importorskip("PIL.Image")
    from PIL import features

    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("this Pillow is not built on libjpeg-turbo")
    sub = {"grey": 0, "4:4:4": 0, "4:2:2": 1, "4:2:0": 2}
    for case in CASES[::5]:
        co = K.read(K.pins()[0][case["name"]]["A"])
        for r in (1, 3):
            f = io.BytesIO()
            Image.fromarray(K.image(case)).save(f, "JPEG", quality=case["quality"], subsampling=sub[case["sampling"]], restart_marker_blocks=r)
            assert K.write(co, restart_interval=r) == f.getvalue(), (case["name"], r)
