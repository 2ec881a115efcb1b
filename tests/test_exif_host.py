"""EXIF orientation on the host: jpeggpu_ext_get_orientation on the whole case list of tests/exif_ref.py, the pure
jpeggpu_ext_orient_size / jpeggpu_ext_orient_rect against numpy slicing of an index image, orient_rect followed by
set_crop, the refusals -- and the pins of tests/golden/exif_pins.npz against the numpy restatement (color_ref's RGB, then
exif_ref's table, then pillow_resample_ref) and, where Pillow is present, against Pillow again. No GPU needed."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import jpeggpu_amd
from jpeggpu_amd import JpegGpuError, Status
from jpeggpu_amd import build as jbuild
from tests import color_ref, exif_ref
from tests import pillow_resample_ref as R
from tests.conftest import GOLDEN


@pytest.fixture(scope="module")
def L():
    jbuild.build()
    return jpeggpu_amd.lib()


@pytest.fixture(scope="module")
def bases():
    from tools import jpegsynth

    return {"baseline": jpegsynth.encode(40, 24, ((2, 2), (1, 1), (1, 1)), restart_interval=2, seed=3),
            "progressive": np.load(os.path.join(GOLDEN, "progressive_pins.npz"))["prog/p420"].tobytes()}


@pytest.fixture(scope="module")
def pins():
    return np.load(os.path.join(GOLDEN, "exif_pins.npz"))


def orientation_of(data, **kw):
    dec = jpeggpu_amd.Decoder()
    try:
        dec.set_progressive(True)
        if kw.get("device_scan"):
            dec.set_device_scan(True)
        dec.parse_header(data)
        return dec.orientation()
    finally:
        dec.cleanup()


@pytest.mark.parametrize("kind", ("baseline", "progressive"))
def test_get_orientation_equals_the_rule_on_the_case_list(L, bases, kind):
    plain = orientation_of(bases[kind])
    assert plain == 1
    for name, (data, want) in exif_ref.cases(bases[kind]).items():
        assert exif_ref.orientation_of_file(data) == want, name
        assert orientation_of(data) == want, name
        assert orientation_of(data, device_scan=True) == want, (name, "device scan")


def test_the_exif_segment_changes_nothing_else(L, bases):
    def parse(data):
        dec = jpeggpu_amd.Decoder()
        try:
            info = dec.parse_header(data)
            lay = dec.layout()
            return ([info.sizes_x[c] for c in range(4)], [info.sizes_y[c] for c in range(4)], info.num_components, lay.num_scans,
                    lay.scans[0].num_subsequences, lay.scans[0].num_segments, int(dec.color_space()))
        finally:
            dec.cleanup()

    want = parse(bases["baseline"])
    for name, (data, _) in exif_ref.cases(bases["baseline"]).items():
        assert parse(data) == want, name


def test_arguments_of_get_orientation(L, bases):
    dec = jpeggpu_amd.Decoder()
    try:
        o = C.c_int(77)
        assert L.jpeggpu_ext_get_orientation(dec._h, C.byref(o)) == Status.INVALID_ARGUMENT  # nothing parsed yet
        assert L.jpeggpu_ext_get_orientation(None, C.byref(o)) == Status.INVALID_ARGUMENT
        dec.parse_header(exif_ref.with_orientation(bases["baseline"], 6))
        assert L.jpeggpu_ext_get_orientation(dec._h, None) == Status.INVALID_ARGUMENT
        assert o.value == 77
        assert dec.orientation() == 6
        dec.parse_header(bases["baseline"])  # the last parsed image's
        assert dec.orientation() == 1
    finally:
        dec.cleanup()


def rectangles(ow, oh):
    """Every corner, 1 x 1, a full row, a full column, the whole image, and some in between."""
    out = [(0, 0, ow, oh), (0, 0, 1, 1), (ow - 1, 0, 1, 1), (0, oh - 1, 1, 1), (ow - 1, oh - 1, 1, 1), (0, 2, ow, 1), (3, 0, 1, oh)]
    out += [(0, 0, 3, 2), (ow - 3, 0, 3, 2), (0, oh - 2, 3, 2), (ow - 3, oh - 2, 3, 2), (1, 1, ow - 2, oh - 3), (2, 1, 3, 4)]
    return out


def test_orient_size_and_rect_equal_numpy_slicing(L):
    w, h = 11, 7
    index = np.arange(w * h).reshape(h, w)
    for o in range(1, 9):
        shown = exif_ref.apply(index, o)
        ow, oh = jpeggpu_amd.orient_size(o, w, h)
        assert (oh, ow) == shown.shape and (ow, oh) == exif_ref.orient_size(o, w, h)
        for x, y, rw, rh in rectangles(ow, oh):
            sx, sy, sw, sh = jpeggpu_amd.orient_rect(o, w, h, (x, y, rw, rh))
            assert (sx, sy, sw, sh) == exif_ref.orient_rect(o, w, h, x, y, rw, rh), (o, x, y, rw, rh)
            assert np.array_equal(exif_ref.apply(index[sy:sy + sh, sx:sx + sw], o), shown[y:y + rh, x:x + rw]), (o, x, y, rw, rh)


def test_orient_rect_then_set_crop(L, bases):
    """The mapped rectangle is what a cropped parse reports, so a displayed-coordinate crop decodes only its segments."""
    w, h = 40, 24
    for o in range(1, 9):
        data = exif_ref.with_orientation(bases["baseline"], o)
        ow, oh = jpeggpu_amd.orient_size(o, w, h)
        for rect in ((0, 0, 5, 3), (ow - 7, oh - 9, 7, 9), (3, 1, 1, 1), (0, 0, ow, oh)):
            stored = jpeggpu_amd.orient_rect(o, w, h, rect)
            dec = jpeggpu_amd.Decoder()
            try:
                dec.set_crop(*stored)
                dec.parse_header(data)
                ci = dec.crop_info()
                assert (ci.x, ci.y, ci.width, ci.height) == stored, (o, rect)
                assert dec.orientation() == o
            finally:
                dec.cleanup()


def test_refusals(L):
    a, b, c, d = (C.c_int(v) for v in (0, 0, 2, 2))
    for o in (0, 9, -1, 65536):
        ow, oh = C.c_int(5), C.c_int(5)
        assert L.jpeggpu_ext_orient_size(o, 8, 8, C.byref(ow), C.byref(oh)) == Status.INVALID_ARGUMENT
        assert (ow.value, oh.value) == (5, 5)
        assert L.jpeggpu_ext_orient_rect(o, 8, 8, C.byref(a), C.byref(b), C.byref(c), C.byref(d)) == Status.INVALID_ARGUMENT
        info, img = jpeggpu_amd.api.ImgInfo(), jpeggpu_amd.api.Img()
        assert L.jpeggpu_ext_planes_to_rgbi_oriented(C.byref(info), 2, o, 0, C.byref(img), None, 0, 8, 8, None) == Status.INVALID_ARGUMENT
        ci = jpeggpu_amd.api.CropInfo()
        assert L.jpeggpu_ext_crop_to_rgbi_oriented(C.byref(info), 2, o, 0, C.byref(ci), C.byref(img), None, 0, None) == Status.INVALID_ARGUMENT
    assert (a.value, b.value, c.value, d.value) == (0, 0, 2, 2)
    with pytest.raises(JpegGpuError):
        jpeggpu_amd.orient_rect(6, 8, 4, (0, 0, 5, 1))  # the displayed image is 4 wide
    with pytest.raises(JpegGpuError):
        jpeggpu_amd.orient_rect(1, 8, 4, (0, 0, 0, 1))
    assert L.jpeggpu_ext_orient_size(6, 0, 4, C.byref(a), C.byref(b)) == Status.INVALID_ARGUMENT
    assert L.jpeggpu_ext_orient_size(6, 8, 4, None, C.byref(b)) == Status.INVALID_ARGUMENT


# ------------------------------------------------------------------------------------------------
# the pins
# ------------------------------------------------------------------------------------------------

def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def stored_rgb():
    """name, d -> the numpy restatement of Pillow's stored RGB (of the baseline twin: the same coefficients)."""
    files = exif_ref.gpu_files()
    cache = {}

    def get(name, d):
        if (name, d) not in cache:
            cache[name, d] = color_ref.color_rgb(files[name][1], d)
        return cache[name, d]

    return get


def test_the_pins_are_of_these_files(pins):
    for name, (data, _) in exif_ref.gpu_files().items():
        assert sha(np.frombuffer(data, np.uint8)) == str(pins["jpeg_sha256/" + name]), name


def test_the_restatement_reproduces_every_rgb_pin(pins, stored_rgb):
    n = 0
    for key in pins.files:
        kind, *rest = key.split("/")
        if kind not in ("rgb", "rgb_sha256"):
            continue
        name, o, d = rest[0], int(rest[1]), int(rest[2])
        shown = exif_ref.apply(stored_rgb(name, d), o)
        if kind == "rgb":
            assert np.array_equal(shown, pins[key]), key
        else:
            assert sha(shown) == str(pins[key]), key
        n += 1
    assert n >= 14 * 8 * 2


def test_the_restatement_reproduces_every_resize_pin_and_the_pass_order_shows(pins, stored_rgb):
    n = 0
    for key in pins.files:
        if not key.startswith("resize/"):
            continue
        _, name, o, box, size, filt = key.split("/")
        x, y, w, h = (int(v) for v in box.split(","))
        ow, oh = (int(v) for v in size.split("x"))
        shown = exif_ref.apply(stored_rgb(name, 1), int(o))[y:y + h, x:x + w]
        assert np.array_equal(R.resize(shown, ow, oh, filt), pins[key]), key
        if name in exif_ref.RESIZE_FILES and (w, h) == shown.shape[1::-1] and (x, y) == (0, 0):
            # the case proves the order of the passes only if the other order gives other pixels
            assert not np.array_equal(exif_ref.resize_swapped(shown, ow, oh, filt), pins[key]), key
        n += 1
    assert n == 2 * 8 * 2 * 2 + 8 * 2


def test_pillow_still_gives_the_pins(pins):
    pytest.importorskip("PIL")
    import importlib.util

    spec = importlib.util.spec_from_file_location("make_exif_pins", os.path.join(os.path.dirname(GOLDEN), "..", "tools", "make_exif_pins.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    files = exif_ref.gpu_files()
    n = 0
    for key in pins.files:
        kind, *rest = key.split("/")
        if kind in ("rgb", "rgb_sha256"):
            a = np.asarray(gen.displayed(exif_ref.with_orientation(files[rest[0]][0], int(rest[1])), int(rest[2])))
            assert np.array_equal(a, pins[key]) if kind == "rgb" else sha(a) == str(pins[key]), key
        elif kind == "resize":
            name, o, box, size, filt = rest
            im = gen.displayed(exif_ref.with_orientation(files[name][0], int(o)))
            a = gen.resized(im, tuple(int(v) for v in box.split(",")), tuple(int(v) for v in size.split("x")), filt)
            assert np.array_equal(a, pins[key]), key
            n += 1
    assert n == 2 * 8 * 2 * 2 + 8 * 2
