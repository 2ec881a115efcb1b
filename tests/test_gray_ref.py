"""The grey restatement (tests/gray_ref.py) against Pillow, where Pillow is importable, and against Pillow's pinned outputs
(tests/golden/gray_pins.npz) everywhere. No GPU needed."""
import numpy as np
import pytest

from tests import color_ref, exif_ref, gray_ref

FILES = gray_ref.files()
NAMES = gray_ref.names(FILES)


@pytest.fixture(scope="module")
def pins():
    return gray_ref.load_pins()


def test_the_pins_are_complete(pins):
    assert sorted(k for k, _ in gray_ref.pin_keys(FILES)) == sorted(k for k in pins.files if k != "pillow_version")
    for name in ("s444", "s422", "s420", "s440", "s411", "gray", "rgb", "prog", "luma_small"):
        assert all("L/%s/%d" % (name, d) in pins.files for d in gray_ref.SCALES), name


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_pins(pins, name):
    for d in gray_ref.SCALES:
        key = "L/%s/%d" % (name, d)
        if key in pins.files:
            assert gray_ref.matches_pin(gray_ref.gray(gray_ref.twin(FILES, name), d), pins[key]), key


def test_orientations_and_resizes_equal_the_pins(pins):
    base = gray_ref.gray(FILES[gray_ref.ORIENT_FILE], gray_ref.ORIENT_SCALE)
    for o in range(1, 9):
        assert gray_ref.matches_pin(exif_ref.apply(base, o), pins["exif/%d" % o]), o
    a = gray_ref.gray(FILES[gray_ref.RESIZE_FILE])
    for filt in gray_ref.FILTERS:
        for ow, oh in gray_ref.RESIZES:
            assert gray_ref.matches_pin(gray_ref.resize(a, ow, oh, filt), pins["resize/%s/%dx%d" % (filt, ow, oh)]), (filt, ow, oh)


def test_progressive_is_its_baseline_twin(pins):
    for d in gray_ref.SCALES:
        assert gray_ref.matches_pin(gray_ref.gray(FILES["prog_twin"], d), pins["L/prog/%d" % d])


def test_rgb_coded_files_take_rgb_gray_convert():
    from oracle import oracle

    from tests import draft_ref

    dec = oracle.decode(FILES["rgb"])
    assert color_ref.model_of_file(FILES["rgb"]) == color_ref.RGB
    r, g, b = (p.astype(np.int64) for p in draft_ref.draft_planes_of(dec, 1))
    assert np.array_equal(gray_ref.gray(FILES["rgb"]), (19595 * r + 38470 * g + 7471 * b + 32768) >> 16)
    assert not np.array_equal(gray_ref.gray(FILES["rgb"]), draft_ref.draft_planes_of(dec, 1)[0])


def test_no_grey_of_four_components():
    from oracle import oracle

    data = exif_ref.gpu_files()["ycck"][0]
    with pytest.raises(ValueError):
        gray_ref.gray_of(oracle.decode(data), color_ref.model_of_file(data))


def test_pillow_agrees_where_it_is_importable(pins):
    pytest.importorskip("PIL")
    for key, make in gray_ref.pin_keys(FILES):
        assert gray_ref.matches_pin(make(), pins[key]), key
    # CMYK and YCCK: draft("L") leaves the file as it is
    assert gray_ref.pillow_gray(exif_ref.gpu_files()["ycck"][0], 2)[1] == "CMYK"
