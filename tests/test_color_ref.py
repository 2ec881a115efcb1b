"""The numpy restatement of Pillow's convert("RGB") of RGB-, CMYK- and YCCK-coded JPEGs (tests/color_ref.py) against
Pillow: live on the whole case list at scales 1, 1/2, 1/4 and 1/8, and the pins of tests/golden/color_pins.npz against
live Pillow. No GPU needed; needs Pillow."""
import hashlib
import os

import numpy as np
import pytest

from tests import color_ref, draft_ref
from tests.conftest import GOLDEN

pytest.importorskip("PIL")


@pytest.fixture(scope="module")
def pins():
    return np.load(os.path.join(GOLDEN, "color_pins.npz"))


@pytest.fixture(scope="module")
def decoded():
    from oracle import oracle

    return {name: (data, model, oracle.decode(data)) for name, (data, model) in color_ref.cases().items()}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def test_case_list_covers_what_it_should(decoded):
    models = [m for _, m, _ in decoded.values()]
    assert len(decoded) == 6 * 3 + 4 * 3 + 2
    assert models.count(color_ref.CMYK) == 12 and models.count(color_ref.YCCK) == 8 and models.count(color_ref.RGB) == 8
    assert models.count(color_ref.YCBCR) == 4
    for name, (data, model, dec) in decoded.items():
        assert color_ref.model_of_file(data) == model, name
        assert (dec.width, dec.height) == color_ref.frame_size(data), name
    assert decoded["ycck_ni"][2].ncomp == 4 and decoded["ycck_dri"][2].ncomp == 4
    # the only exclusion: the 3 x 5 files below full size
    excluded = [(n, d) for n in decoded for d in color_ref.SCALES if not color_ref.comparable(n, d)]
    assert excluded and all(color_ref.frame_size(decoded[n][0]) == (3, 5) and d > 1 for n, d in excluded), excluded
    assert all(color_ref.comparable(n, d) for n in decoded for d in color_ref.SCALES if color_ref.frame_size(decoded[n][0]) != (3, 5))


def test_muldiv255_is_the_rounded_division():
    a, b = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64))
    assert np.array_equal(color_ref.muldiv255(a, b), (2 * a * b + 255) // 510)  # round(a b / 255), halves up


def test_restatement_equals_live_pillow(decoded):
    n = 0
    for name, (data, model, dec) in decoded.items():
        for d in color_ref.SCALES:
            if not color_ref.comparable(name, d):
                continue
            want, size = color_ref.pillow_rgb(data, d)
            assert size == (draft_ref.ceil_div(dec.width, d), draft_ref.ceil_div(dec.height, d)), (name, d, size)
            got = color_ref.color_rgb_of(dec, model, d)
            assert got.shape == want.shape and np.array_equal(got, want), (name, d, int((got != want).sum()) if got.shape == want.shape else got.shape)
            n += 1
    assert n == 4 * len(decoded) - 12  # the six 3 x 5 files at 1/4 and 1/8


def test_the_models_differ_on_these_files(decoded):
    """A file read as the wrong model gives other pixels: the cases tell the models apart."""
    for name in ("s444_adobe0", "s420_ids"):
        _, _, dec = decoded[name]
        assert not np.array_equal(color_ref.color_rgb_of(dec, color_ref.RGB), color_ref.color_rgb_of(dec, color_ref.YCBCR)), name
    for name in ("c444_adobe2", "c22_plain"):
        _, _, dec = decoded[name]
        assert not np.array_equal(color_ref.color_rgb_of(dec, color_ref.CMYK), color_ref.color_rgb_of(dec, color_ref.YCCK)), name


def test_pins_equal_live_pillow(pins, decoded):
    names = {k.partition("/")[2] for k in pins.files if k.startswith("jpeg_sha256/")}
    assert names == set(decoded)
    n = 0
    for name, (data, model, dec) in decoded.items():
        assert hashlib.sha256(data).hexdigest() == str(pins["jpeg_sha256/" + name]), (name, "input differs from the pinned one")
        assert int(pins["model/" + name]) == model, name
        for d in color_ref.SCALES:
            key = "%s/%d" % (name, d)
            if not color_ref.comparable(name, d):
                assert "rgb/" + key not in pins.files and "rgb_sha256/" + key not in pins.files
                continue
            want, _ = color_ref.pillow_rgb(data, d)
            if "rgb/" + key in pins.files:
                assert np.array_equal(pins["rgb/" + key], want), key
            else:
                assert str(pins["rgb_sha256/" + key]) == sha(want), key
            n += 1
    assert n == sum(k.startswith(("rgb/", "rgb_sha256/")) for k in pins.files) == 4 * len(decoded) - 12
