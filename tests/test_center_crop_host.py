"""Resize + CenterCrop on the host (jpeggpu_ext_resize_view_*): the two rules against a hand-written table, the numpy
restatement (tests/center_crop_ref.py) against Pillow's own pipeline, the library's window tables and rectangles against
the restatement, argument checks, and the pins against the restatement. No GPU needed."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import jpeggpu_amd
from jpeggpu_amd import Status
from jpeggpu_amd import build as jbuild
from jpeggpu_amd.api import ResizeView, TensorSpec
from tests import center_crop_ref as CC
from tests import exif_ref
from tests import pillow_resample_ref as R
from tests.conftest import GOLDEN
from tests.test_resize_host import FAKE, arr, item

BILINEAR, BICUBIC = 0, 1


@pytest.fixture(scope="module")
def L():
    jbuild.build()
    return jpeggpu_amd.lib()


# (w, h, size) -> (rw, rh): worked by hand from "short side = size, long side = int(size * long / short)"
RESIZE_TABLE = (
    ((500, 375, 256), (341, 256)),    # 256 * 500 / 375 = 341.33
    ((640, 227, 256), (721, 256)),    # 256 * 640 / 227 = 721.76: truncated, not rounded
    ((375, 500, 256), (256, 341)),
    ((300, 300, 256), (256, 256)),
    ((4032, 3024, 256), (341, 256)),
    ((504, 378, 256), (341, 256)),
    ((17, 9, 24), (45, 24)),          # 24 * 17 / 9 = 45.33: an upscale
    ((1, 1000, 3), (3, 3000)),
    ((200, 152, (120, 152)), (152, 120)),  # a pair is (height, width), used as given
)
# (resized side, crop side) -> the window's corner: int(round((r - c) / 2.0)), Python's round; padded: -((c - r) // 2)
CORNER_TABLE = (
    ((341, 224), 58),    # 58.5 -> 58: half to even
    ((343, 224), 60),    # 59.5 -> 60
    ((256, 224), 16),
    ((224, 224), 0),
    ((225, 224), 0),     # 0.5 -> 0
    ((227, 224), 2),     # 1.5 -> 2
    ((200, 224), -12),   # an even difference: 12 left, 12 right
    ((201, 224), -11),   # an odd one: 11 left, 12 right
    ((9, 24), -7),       # 15: 7 left, 8 right
    ((17, 24), -3),      # 7: 3 left, 4 right
)


def test_the_two_rules_by_hand():
    for (w, h, size), want in RESIZE_TABLE:
        assert jpeggpu_amd.resized_size(w, h, size) == want, (w, h, size)
        assert CC.resized_size(w, h, size) == want, (w, h, size)
    for (r, c), want in CORNER_TABLE:
        assert jpeggpu_amd.center_crop_window(r, 1000, (7, c)) == (want, int(round((1000 - 7) / 2.0))), (r, c)
        assert jpeggpu_amd.center_crop_window(1000, r, (c, 7))[1] == want, (r, c)
        assert jpeggpu_amd.center_crop_window(r, r, c) == (want, want), (r, c)
        assert CC.center_crop_window(r, r, c, c) == (want, want), (r, c)
        if want < 0:  # the padding on the two sides adds up, the larger share on the right
            left, right = -want, c - r + want
            assert (left, right) == ((c - r) // 2, (c - r + 1) // 2)


def pipeline_cases():
    """(h, w, resize, crop): a downscale, a padded case (both directions, rows only), an identity direction (the resize
    leaves the height / both as they are), an upscale, odd everything; and seeded ones."""
    fixed = [(375, 500, 256, 224), (45, 61, 32, 40), (152, 200, 32, (40, 30)), (152, 200, 152, 120), (120, 152, (120, 152), 100),
             (152, 200, 176, 150), (9, 17, 9, 24), (9, 17, 24, 24), (227, 640, 256, 224), (33, 77, (50, 31), (37, 41)), (1, 1, 4, 8)]
    rng = np.random.default_rng(21)
    rand = [(int(rng.integers(1, 200)), int(rng.integers(1, 200)), int(rng.integers(1, 120)), (int(rng.integers(1, 100)), int(rng.integers(1, 100))))
            for _ in range(40)]
    return fixed + rand


@pytest.mark.parametrize("filt", R.FILTERS)
def test_restatement_equals_pillows_pipeline(filt):
    pytest.importorskip("PIL")
    from PIL import Image

    f = {"bilinear": Image.Resampling.BILINEAR, "bicubic": Image.Resampling.BICUBIC}[filt]
    rng = np.random.default_rng(4)
    padded = identity = up = 0
    for h, w, size, crop in pipeline_cases():
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        ch, cw = (crop, crop) if isinstance(crop, int) else crop
        rw, rh = CC.resized_size(w, h, size)
        x, y = CC.center_crop_window(rw, rh, cw, ch)
        # Pillow's pipeline: resize, then the crop where the image is large enough and an explicit zero pad where not
        r = np.asarray(Image.fromarray(a).resize((rw, rh), f))
        want = np.zeros((ch, cw, 3), np.uint8)
        x0, x1, y0, y1 = max(x, 0), min(x + cw, rw), max(y, 0), min(y + ch, rh)
        want[y0 - y:y1 - y, x0 - x:x1 - x] = np.asarray(Image.fromarray(r).crop((x0, y0, x1, y1)))
        got = CC.resize_center_crop(a, size, crop, filt)
        assert np.array_equal(got, want), (filt, h, w, size, crop)
        # Image.crop with a box beyond the image pads with zeros too: the pins tool's one-liner
        assert np.array_equal(np.asarray(Image.fromarray(r).crop((x, y, x + cw, y + ch))), want)
        padded += x < 0 or y < 0
        identity += rw == w or rh == h
        up += rw > w
    assert padded >= 4 and identity >= 3 and up >= 4


def window_cases():
    """(in, resized, x0, count): downscale, upscale and identity; windows inside, starting before 0, ending behind
    `resized`, doing both, and lying wholly outside."""
    out = []
    for i, r in ((375, 256), (500, 341), (9, 24), (17, 45), (152, 152), (200, 176), (4032, 341), (3, 300), (40, 1)):
        for x0, n in ((0, r), (r // 3, max(1, r // 2)), (-5, r // 2 + 5), (r // 2, r), (-7, r + 15), (-1, 1), (r, 3), (-9, 4)):
            out.append((i, r, x0, n))
    rng = np.random.default_rng(6)
    for _ in range(120):
        i, r = int(rng.integers(1, 900)), int(rng.integers(1, 400))
        out.append((i, r, int(rng.integers(-40, r + 20)), int(rng.integers(1, 300))))
    return out


@pytest.mark.parametrize("filt", R.FILTERS)
def test_window_tables_equal_the_restatements_slices(L, filt):
    front = behind = whole_empty = 0
    for i, r, x0, n in window_cases():
        for origin in (0, 3):
            first, count, w = jpeggpu_amd.resize_view_weights(i, r, x0, n, origin, filt)
            rf, rc, rw, inside = CC.window_tables(i, r, x0, n, filt)
            assert np.array_equal(count, rc) and np.array_equal(w, rw), (i, r, x0, n, filt)
            assert np.array_equal(first[inside], rf[inside] - origin), (i, r, x0, n, filt)
            assert (count[~inside] == 0).all() and (w[~inside] == 0).all()
            if not inside.any():
                assert (first == 0).all()
                whole_empty += 1
                continue
            # what the empty entries carry: in front the first of the first entry with taps, behind first + count of the last
            k0, k1 = np.flatnonzero(inside)[[0, -1]]
            assert (first[:k0] == first[k0]).all() and (first[k1 + 1:] == first[k1] + count[k1]).all(), (i, r, x0, n)
            # so that first and first + count never decrease: resize_h_tile reads a tile's input range off its ends
            assert (np.diff(first) >= 0).all() and (np.diff(first + count) >= 0).all(), (i, r, x0, n, filt)
            front += k0 > 0
            behind += k1 < n - 1
    assert front >= 40 and behind >= 40 and whole_empty >= 10


def test_the_whole_window_is_the_resize_table(L):
    for i, o in ((375, 256), (9, 24), (152, 152), (4032, 224)):
        for filt in R.FILTERS:
            a, b = jpeggpu_amd.resize_view_weights(i, o, 0, o, 0, filt), jpeggpu_amd.resize_weights(i, o, filt)
            assert all(np.array_equal(x, y) for x, y in zip(a, b)), (i, o, filt)


def test_view_weights_arguments(L):
    f, c, w = (C.c_int * 8)(), (C.c_int * 8)(), (C.c_int * 72)()
    call = L.jpeggpu_ext_resize_view_weights
    assert call(8, 4, -2, 8, 0, BILINEAR, f, c, w, 5) == Status.SUCCESS
    assert call(8, 4, -2, 8, 0, BILINEAR, f, c, w, 4) == Status.INVALID_ARGUMENT
    assert call(8, 4, -2, 8, 0, BICUBIC, f, c, w, 8) == Status.INVALID_ARGUMENT  # needs 9
    assert call(8, 4, 0, 4, 0, 2, f, c, w, 9) == Status.NOT_SUPPORTED
    assert call(0, 4, 0, 4, 0, BILINEAR, f, c, w, 9) == Status.INVALID_ARGUMENT
    assert call(8, 0, 0, 4, 0, BILINEAR, f, c, w, 9) == Status.INVALID_ARGUMENT
    assert call(8, 4, 0, 0, 0, BILINEAR, f, c, w, 9) == Status.INVALID_ARGUMENT
    assert call(8, 4, 0, 4, 0, BILINEAR, None, c, w, 9) == Status.INVALID_ARGUMENT
    assert call(8, 4, 0, 4, 0, BILINEAR, f, None, w, 9) == Status.INVALID_ARGUMENT
    assert call(8, 4, 0, 4, 0, BILINEAR, f, c, None, 9) == Status.INVALID_ARGUMENT


def rect_cases():
    """(w, h, resize, crop) of displayed images: the issue's shapes, padded and upscaled ones, seeded ones."""
    fixed = [(500, 375, 256, 224), (375, 500, 256, 224), (640, 227, 256, 224), (200, 152, 48, 40), (200, 152, 64, 37), (200, 152, 176, 150),
             (200, 152, (120, 152), 120), (200, 152, 32, 40), (17, 9, 9, 24), (4032, 3024, 256, 224), (53, 37, 24, (16, 30))]
    rng = np.random.default_rng(9)
    return fixed + [(int(rng.integers(1, 700)), int(rng.integers(1, 700)), int(rng.integers(1, 300)), (int(rng.integers(1, 260)), int(rng.integers(1, 260))))
                    for _ in range(60)]


@pytest.mark.parametrize("filt", R.FILTERS)
def test_view_rect_is_the_union_of_the_taps(L, filt):
    n = smaller = 0
    for w, h, size, crop in rect_cases():
        ch, cw = (crop, crop) if isinstance(crop, int) else crop
        rw, rh = CC.resized_size(w, h, size)
        x, y = CC.center_crop_window(rw, rh, cw, ch)
        cols, rows = CC.tap_range(w, rw, x, cw, filt), CC.tap_range(h, rh, y, ch, filt)
        assert cols is not None and rows is not None  # a centre window always overlaps the image
        shown = (cols[0], rows[0], cols[1] - cols[0], rows[1] - rows[0])
        assert jpeggpu_amd.resize_view_rect(w, h, (rw, rh, x, y), (ch, cw), filt) == shown, (w, h, size, crop)
        smaller += shown[2] * shown[3] < w * h
        for o in range(1, 9):  # the view is in displayed pixels; the stored image is the displayed one turned back
            sw, sh = exif_ref.orient_size(o, w, h)
            want = exif_ref.orient_rect(o, sw, sh, *shown)
            assert jpeggpu_amd.resize_view_rect(sw, sh, (rw, rh, x, y), (ch, cw), filt, o) == want, (w, h, size, crop, o)
            assert want == jpeggpu_amd.orient_rect(o, sw, sh, shown)
            n += 1
    assert n >= 8 * 70 and smaller >= 30


def test_view_rect_arguments(L):
    v = [C.c_int() for _ in range(4)]
    p = [C.byref(a) for a in v]
    view = ResizeView(341, 256, 58, 16, 0)
    call = L.jpeggpu_ext_resize_view_rect
    assert call(500, 375, 1, C.byref(view), 224, 224, BILINEAR, *p) == Status.SUCCESS
    assert call(500, 375, 0, C.byref(view), 224, 224, BILINEAR, *p) == Status.INVALID_ARGUMENT
    assert call(500, 375, 9, C.byref(view), 224, 224, BILINEAR, *p) == Status.INVALID_ARGUMENT
    assert call(0, 375, 1, C.byref(view), 224, 224, BILINEAR, *p) == Status.INVALID_ARGUMENT
    assert call(500, 375, 1, None, 224, 224, BILINEAR, *p) == Status.INVALID_ARGUMENT
    assert call(500, 375, 1, C.byref(view), 0, 224, BILINEAR, *p) == Status.INVALID_ARGUMENT
    assert call(500, 375, 1, C.byref(view), 224, 224, 2, *p) == Status.NOT_SUPPORTED
    assert call(500, 375, 1, C.byref(view), 224, 224, BILINEAR, None, *p[1:]) == Status.INVALID_ARGUMENT
    for bad in (ResizeView(0, 256, 0, 0, 0), ResizeView(341, -1, 0, 0, 0), ResizeView(341, 256, 341, 0, 0), ResizeView(341, 256, 0, -224, 0),
                ResizeView(341, 256, -224, 16, 0)):  # no size; a window beside the resized image
        assert call(500, 375, 1, C.byref(bad), 224, 224, BILINEAR, *p) == Status.INVALID_ARGUMENT


def views_of(*vs):
    a = (ResizeView * len(vs))()
    for i, v in enumerate(vs):
        a[i] = ResizeView(*v)
    return a


def spec_of(type_=0, std=1.0):
    s = TensorSpec()
    s.type = type_
    s.mean[:] = [0.0] * 3
    s.std[:] = [std] * 3
    return s


def call(L, items, views, n=None, w=40, h=40, filt=BILINEAR, layout=0, spec=None, dst=FAKE, scratch=FAKE, size=None, colors=None,
         orients=None):
    n = len(items) if n is None else n
    spec = spec_of() if spec is None else spec
    if size is None:
        size = L.jpeggpu_ext_resize_view_scratch_size(items, colors, orients, views, n, w, h, filt) if items is not None else 0
    return L.jpeggpu_ext_resize_view_to_tensor(items, colors, orients, views, n, w, h, filt, layout, C.byref(spec) if spec else None, dst,
                                               scratch, size, None)


def test_view_call_arguments(L):
    """Every call here is refused before anything is enqueued: the plane addresses are fake."""
    good = arr(item(size=(200, 152)), item(((1, 1),), size=(200, 152)))
    v = views_of((63, 48, 12, 4, 0), (63, 48, 12, 4, 0))
    size = L.jpeggpu_ext_resize_view_scratch_size(good, None, None, v, 2, 40, 40, BILINEAR)
    assert size > 0
    # the tensor call's own checks come first, then the resize call's, with their statuses
    assert L.jpeggpu_ext_resize_view_to_tensor(good, None, None, v, 2, 40, 40, BILINEAR, 0, None, FAKE, FAKE, size, None) == Status.INVALID_ARGUMENT
    assert call(L, good, v, spec=spec_of(7)) == Status.INVALID_ARGUMENT
    assert call(L, good, v, spec=spec_of(1, std=0.0)) == Status.INVALID_ARGUMENT
    assert call(L, good, None, size=1 << 30) == Status.INVALID_ARGUMENT
    assert L.jpeggpu_ext_resize_view_scratch_size(good, None, None, None, 2, 40, 40, BILINEAR) == 0
    assert call(L, None, v, n=1) == Status.INVALID_ARGUMENT
    assert call(L, good, v, n=0) == Status.INVALID_ARGUMENT
    assert call(L, good, v, w=0) == Status.INVALID_ARGUMENT
    assert call(L, good, v, filt=2, size=1 << 30) == Status.NOT_SUPPORTED
    assert call(L, good, v, layout=2) == Status.INVALID_ARGUMENT
    assert call(L, good, v, dst=None) == Status.INVALID_ARGUMENT
    assert call(L, good, v, scratch=None) == Status.INVALID_ARGUMENT
    assert call(L, good, v, size=size - 1) == Status.INVALID_ARGUMENT
    assert call(L, good, v, spec=spec_of(1), dst=FAKE + 2) == Status.INVALID_ARGUMENT  # not aligned to the element
    assert call(L, good, v, orients=(C.c_int * 2)(1, 9), size=1 << 30) == Status.INVALID_ARGUMENT
    # an item's own checks, as in the resize call
    a = arr(item(size=(200, 152)), item(((2, 1), (1, 1)), size=(200, 152)))
    assert call(L, a, v, size=1 << 30) == Status.NOT_SUPPORTED
    # the views: no size, a window that overlaps no pixel of the resized image
    for bad in ((0, 48, 0, 0, 0), (63, 0, 0, 0, 0), (63, 48, 63, 4, 0), (63, 48, -40, 4, 0), (63, 48, 12, 48, 0), (63, 48, 12, -40, 0)):
        vb = views_of((63, 48, 12, 4, 0), bad)
        assert L.jpeggpu_ext_resize_view_scratch_size(good, None, None, vb, 2, 40, 40, BILINEAR) == 0
        assert call(L, good, vb, size=1 << 30) == Status.INVALID_ARGUMENT, bad
    # windows that reach over the image's edges are padding, not errors
    assert L.jpeggpu_ext_resize_view_scratch_size(good, None, None, views_of((30, 22, -5, -9, 0), (63, 48, 30, 20, 1)), 2, 40, 40, BILINEAR) > 0


@pytest.mark.parametrize("filt", (BILINEAR, BICUBIC))
@pytest.mark.parametrize("o", (1, 3, 6))
def test_a_rectangle_one_column_short_is_refused(L, filt, o):
    """The rectangle must hold every pixel the window's taps read: resize_view_rect's is accepted, and so is a larger
    one (asked of the host-only size call: an accepted call would enqueue work on the fake planes); one column or one row
    less on any side is JPEGGPU_INVALID_ARGUMENT."""
    sw, sh = 200, 152
    dw, dh = exif_ref.orient_size(o, sw, sh)
    rw, rh = CC.resized_size(dw, dh, 64)
    x, y = CC.center_crop_window(rw, rh, 40, 40)
    view = (rw, rh, x, y)
    rx, ry, rwid, rhei = jpeggpu_amd.resize_view_rect(sw, sh, view, 40, R.FILTERS[filt], o)
    assert 0 < rx and 0 < ry and rx + rwid < sw and ry + rhei < sh  # strictly inside: every side can be cut and grown
    orients = (C.c_int * 1)(o)
    v = views_of(view + (0,))

    def status(rect):
        a = arr(item(size=(sw, sh), crop=rect))
        return call(L, a, v, filt=filt, orients=orients, size=1 << 30)

    for rect in ((rx + 1, ry, rwid - 1, rhei), (rx, ry, rwid - 1, rhei), (rx, ry + 1, rwid, rhei - 1), (rx, ry, rwid, rhei - 1)):
        assert status(rect) == Status.INVALID_ARGUMENT, rect
        a = arr(item(size=(sw, sh), crop=rect))
        assert L.jpeggpu_ext_resize_view_scratch_size(a, None, orients, v, 1, 40, 40, filt) == 0
    for rect in ((rx, ry, rwid, rhei), (rx - 1, ry - 1, rwid + 2, rhei + 2), (0, 0, sw, sh)):  # accepted: by the host-only size call
        a = arr(item(size=(sw, sh), crop=rect))
        assert L.jpeggpu_ext_resize_view_scratch_size(a, None, orients, v, 1, 40, 40, filt) > 0, rect


def test_identity_view_has_the_resize_calls_scratch(L):
    """{resized = out, 0, 0} on whole items is the resize call: the same plan, so the same scratch size."""
    its = arr(item(size=(200, 152)), item(((1, 1),), size=(333, 251)), item(((2, 1), (1, 1), (1, 1)), size=(64, 90)))
    for w, h in ((40, 40), (200, 152), (333, 90), (500, 400)):
        for filt in (BILINEAR, BICUBIC):
            v = views_of(*[(w, h, 0, 0, 0)] * 3)
            assert L.jpeggpu_ext_resize_view_scratch_size(its, None, None, v, 3, w, h, filt) == L.jpeggpu_ext_resize_scratch_size(its, 3, w, h, filt) > 0


def pinned_rgb(name, d):
    """Pillow's RGB of a pinned input at scale d, if a golden file holds it as an array (H, W, 3)."""
    if d == 1:
        pins, k = np.load(os.path.join(GOLDEN, "libjpeg_pins.npz")), "rgb/" + name
    else:
        pins, k = np.load(os.path.join(GOLDEN, "draft_pins.npz")), "rgb/%s/%d" % (name, d)
    if k not in pins.files:
        return None
    a = pins[k]
    return np.repeat(a[:, :, None], 3, 2) if a.ndim == 2 else a


def test_pins_are_pillow():
    """tests/golden/center_crop_pins.npz holds Pillow's outputs for tools/make_center_crop_pins.py's inputs: the
    restatement applied to the pinned Pillow RGB gives them (the photo and files pinned by hash only: on the GPU)."""
    pins = np.load(os.path.join(GOLDEN, "center_crop_pins.npz"))
    assert os.path.getsize(os.path.join(GOLDEN, "center_crop_pins.npz")) < os.path.getsize(os.path.join(GOLDEN, "draft_pins.npz"))
    n = 0
    for key in pins.files:
        kind, name, d, resize, crop, filt = key.split("/")
        rgb = pinned_rgb(name, int(d))
        if rgb is None:
            continue
        ch, cw = (int(v) for v in crop.split("x"))
        got = CC.resize_center_crop(rgb, int(resize), (ch, cw), filt)
        if kind == "out":
            assert np.array_equal(got, pins[key]), key
        else:
            assert hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest() == str(pins[key]), key
        n += 1
    assert n >= 160
