"""tests/transcode_crop_ref.py against the Pillow at hand, live, and against the pins: the cropped transcode of Pillow's file of
an image is Pillow's file of the cropped pixels where the window starts on an iMCU boundary and each extent is a multiple of
the iMCU or reaches the image's edge; a window that ends inside the image off a block boundary keeps the source's samples
(grey and 4:4:4: Pillow's decode of it is the crop of Pillow's decode of the source); with an orientation the same holds
on cell images. And the rules: what is refused, jpegtran's expansion, the source rectangle."""
import io

import numpy as np
import pytest

import jpeggpu_amd
from tests import transcode_crop_cases as W
from tests import transcode_crop_ref as Z
from tests import transcode_orient_cases as K
from tests import transcode_orient_ref as X
from tests import transcode_ref as R


@pytest.fixture(scope="module")
def pillow():
    Image = pytest.importorskip("PIL.Image")
    from PIL import ImageFile, features

    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("this Pillow is not built on libjpeg-turbo")
    saved = ImageFile.MAXBLOCK
    ImageFile.MAXBLOCK = 1 << 24

    def save(img, params, **more):
        f = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(img)).save(f, "JPEG", **params, **more)
        return f.getvalue()

    save.decode = lambda data: np.asarray(Image.open(io.BytesIO(data)))
    yield save
    ImageFile.MAXBLOCK = saved


def test_rules():
    assert Z.target_geometry(75, 53, 2, 2, 1) == (75, 53, 2, 2) and Z.target_geometry(80, 64, 2, 2, 6) == (64, 80, 2, 2)
    assert Z.target_geometry(75, 53, 2, 2, 3, True) == (64, 48, 2, 2) and Z.target_geometry(40, 16, 2, 1, 2, True) == (32, 16, 2, 1)
    with pytest.raises(Z.Unsupported):
        Z.target_geometry(32, 32, 2, 1, 5)
    g = (75, 53, 2, 2)
    assert Z.checked((16, 32, 59, 21), *g) == (16, 32, 59, 21) and Z.checked((0, 0, 1, 1), *g) == (0, 0, 1, 1)
    for rect in ((-16, 0, 16, 16), (0, 0, 0, 16), (0, 0, 16, 0), (16, 32, 60, 21), (16, 32, 59, 22), (0, 0, 16, -1)):
        with pytest.raises(Z.Invalid):
            Z.checked(rect, *g)
    for rect in ((8, 0, 16, 16), (0, 8, 16, 16), (17, 16, 8, 8)):
        with pytest.raises(Z.Unsupported):
            Z.checked(rect, *g)
    assert Z.checked((8, 16, 8, 8), 75, 53, 1, 2) == (8, 16, 8, 8)  # the TARGET's factors: 4:2:2 turned
    assert Z.expanded((17, 9, 10, 10), 2, 2) == (16, 0, 11, 19) and Z.expanded((17, 9, 10, 10), 1, 1) == (16, 8, 11, 11)
    assert Z.expanded((32, 16, 5, 5), 2, 2) == (32, 16, 5, 5)


def test_source_rectangle_is_the_pixels():
    """source_rect names the stored pixels a displayed rectangle shows, and jpeggpu_amd.transcode_crop_rects agrees with the
    restatement on both rectangles, trim and expansion included."""
    rng = np.random.default_rng(5)
    n = 0
    for sw, sh, hs, vs in ((75, 53, 2, 2), (80, 64, 2, 2), (40, 17, 2, 1), (35, 21, 1, 1)):
        s = np.arange(sw * sh).reshape(sh, sw)
        for o in range(1, 9):
            for trim in (False, True):
                try:
                    tw, th, ths, tvs = Z.target_geometry(sw, sh, hs, vs, o, trim)
                except Z.Unsupported:
                    if not (o >= 5 and (hs, vs) == (2, 1)):
                        with pytest.raises(ValueError):
                            jpeggpu_amd.transcode_crop_rects(sw, sh, hs, vs, (0, 0, 1, 1), o, trim)
                    continue
                cut = X.target_size(sw, sh, hs, vs, o, trim)
                shown = X.orient_pixels(s[:cut[1], :cut[0]], o)
                assert shown.shape == (th, tw)
                for _ in range(8):
                    x, y = int(rng.integers(0, tw)), int(rng.integers(0, th))
                    rect = (x, y, int(rng.integers(1, tw - x + 1)), int(rng.integers(1, th - y + 1)))
                    for expand in (False, True):
                        want = Z.expanded(rect, ths, tvs) if expand else rect
                        sx, sy, w, h = Z.source_rect(want, tw, th, o)
                        assert (X.orient_pixels(s[sy:sy + h, sx:sx + w], o) == shown[want[1]:want[1] + want[3], want[0]:want[0] + want[2]]).all()
                        assert jpeggpu_amd.transcode_crop_rects(sw, sh, hs, vs, rect, o, trim, expand) == (want, (sx, sy, w, h))
                        n += 1
                for bad in ((0, 0, tw + 1, 1), (0, 0, 1, th + 1), (-1, 0, 1, 1), (0, 0, 0, 1), (tw, 0, 1, 1)):
                    with pytest.raises(ValueError):
                        jpeggpu_amd.transcode_crop_rects(sw, sh, hs, vs, bad, o, trim)
    assert n > 500


@pytest.mark.parametrize("sampling", W.SAMPLINGS)
def test_live_windows_equal_pillow(pillow, sampling):
    """Noise and photograph-like images at 75 x 53 and 80 x 64, orientation 1: the six windows, plain, optimised and
    progressive, and with the source's restart interval and another one."""
    ux, uy = W.imcu(sampling)
    equal = 0
    for w, h in W.SIZES:
        for content in W.CONTENTS:
            img = W.image(w, h, sampling, content)
            for blocks in (0, 3):
                params = W.save_params(sampling, blocks)
                src = pillow(img, params)
                assert Z.transform(src, None) == src
                for window, (x, y, cw, ch) in W.windows(w, h, ux, uy).items():
                    for kind, options in W.KINDS.items():
                        assert Z.transform(src, (x, y, cw, ch), **options) == pillow(img[y:y + ch, x:x + cw], params, **options), (w, h, content, blocks, window, kind)
                        equal += 1
                    if blocks == 0:  # a second restart interval, from a source without one
                        other = dict(W.save_params(sampling, 2))
                        assert Z.transform(src, (x, y, cw, ch), restart_interval=2) == pillow(img[y:y + ch, x:x + cw], other), (w, h, content, window)
                        equal += 1
    print("live: %d files equal" % equal)
    assert equal == 2 * 2 * (2 * 6 * 3 + 6)


@pytest.mark.parametrize("sampling", ["grey", "4:4:4"])
def test_ragged_windows_keep_the_samples(pillow, sampling):
    """A window that ends inside the image off a block boundary cannot be Pillow's file (Pillow replicates the edge pixel
    where the source has real ones). Without subsampling Pillow's decode of it is the crop of Pillow's decode of the source,
    sample for sample. (Not for 4:2:0: fancy upsampling reads across the window's edge.)"""
    n = 0
    for w, h in W.SIZES:
        for content in W.CONTENTS:
            src = pillow(W.image(w, h, sampling, content), W.save_params(sampling))
            whole = pillow.decode(src)
            for x, y, cw, ch in W.ragged(w, h, 8, 8):
                for options in W.KINDS.values():
                    got = pillow.decode(Z.transform(src, (x, y, cw, ch), **options))
                    assert got.shape[:2] == (ch, cw) and (got == whole[y:y + ch, x:x + cw]).all(), (w, h, content, (x, y, cw, ch))
                    n += 1
    assert n == 2 * 2 * 6 * 3


def test_live_orientations_on_cell_images(pillow):
    """Orientations 2..8 with a crop, on the cell images of the orientation's own tests (a noisy image fails there: the
    FDCT's rounding is not mirror-symmetric): Pillow's file of the rectangle of Image.transpose of the (cut) pixels."""
    equal = 0
    for case in K.pin_cases():
        if (case["w"], case["h"]) not in ((48, 32), (64, 48), (35, 21), (17, 40)):
            continue
        src = K.pins()[0][case["name"]]
        hs, vs = K.FACTORS[case["sampling"]]
        for o in range(2, 9):
            for trim in (False, True):
                size = K.allowed(case, o, trim)
                if size is None:
                    continue
                tw, th, ths, tvs = Z.target_geometry(case["w"], case["h"], hs, vs, o, trim)
                turned = X.orient_pixels(K.cell_image(case)[:size[1], :size[0]], o)
                ux, uy = 8 * ths, 8 * tvs
                rects = {(ux, 0, tw - ux, th), (0, uy, tw, th - uy), (0, 0, ux, uy), (0, 0, tw, th), ((tw - 1) // ux * ux, (th - 1) // uy * uy, tw - (tw - 1) // ux * ux, th - (th - 1) // uy * uy)}
                for k, (x, y, w, h) in enumerate(sorted(r for r in rects if r[2] > 0 and r[3] > 0)):
                    options = list(W.KINDS.values())[(k + o) % 3]
                    assert Z.transform(src, (x, y, w, h), o, trim, **options) == pillow(turned[y:y + h, x:x + w], K.save_params(case), **options), (case["name"], o, trim, (x, y, w, h))
                    equal += 1
    print("live: %d oriented files equal" % equal)
    assert equal > 300


def test_pins_equal_the_restatement():
    """Every pinned file (Pillow's, tools/make_transcode_crop_pins.py) is what the restatement makes of the pinned source."""
    sources, want, _ = W.pins()
    orient_sources = K.pins()[0]
    n = 0
    for ci, case in enumerate(W.pin_cases()):
        for wi, (window, rect) in enumerate(W.windows(case["w"], case["h"], *W.imcu(case["sampling"])).items()):
            kind = W.pin_kind(ci, wi)
            assert Z.transform(sources[case["name"]], rect, **W.KINDS[kind]) == want[case["name"], window, kind], (case["name"], window)
            n += 1
    for name, o, trim, rect in W.oriented_pin_cases():
        kinds = [k for k in "ABC" if (name, o, trim, rect, k) in want]
        assert len(kinds) == 1
        assert Z.transform(orient_sources[name], rect, o, trim, **W.KINDS[kinds[0]]) == want[name, o, trim, rect, kinds[0]], (name, o, trim, rect)
        n += 1
    assert n == len(want) and n >= 48 + 40


def test_refusals_of_the_restatement():
    src = W.pins()[0]["80x64_420_photo"]
    for rect in ((8, 0, 16, 16), (0, 8, 16, 16)):
        with pytest.raises(Z.Unsupported):
            Z.transform(src, rect)
    for rect in ((0, 0, 81, 64), (64, 0, 17, 1), (0, 0, 0, 0), (0, 64, 1, 1)):
        with pytest.raises(Z.Invalid):
            Z.transform(src, rect)
    assert R.parse(Z.transform(src, (64, 48, 16, 16)))["w"] == 16
    assert Z.transform(src, (0, 0, 80, 64)) == R.transcode(src)  # whole iMCUs: no dummy block differs
