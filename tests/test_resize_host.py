"""Batched resize on the host (jpeggpu_ext_resize_*): the numpy restatement of Pillow's resampling against Pillow itself,
the library's weight tables against the restatement, argument checks and the scratch size. No GPU needed."""
import ctypes as C
import os

import numpy as np
import pytest

import jpeggpu_amd
from jpeggpu_amd import Status
from jpeggpu_amd import build as jbuild
from jpeggpu_amd.api import CropInfo, Img, ImgInfo, ResizeItem
from tests import pillow_resample_ref as R
from tests.conftest import GOLDEN

BILINEAR, BICUBIC = 0, 1


@pytest.fixture(scope="module")
def L():
    jbuild.build()
    return jpeggpu_amd.lib()


def pillow_cases():
    """(in_h, in_w, out_h, out_w) of every kind the issue names: up and down, 1-pixel inputs and outputs, ratios above 16,
    one direction unchanged; and seeded random sizes."""
    fixed = [(1, 1, 1, 1), (1, 1, 5, 7), (9, 1, 3, 1), (1, 40, 1, 3), (37, 53, 1, 1), (20, 30, 20, 7), (20, 30, 9, 30),
             (640, 480, 24, 20), (15, 700, 15, 31), (500, 17, 23, 17), (16, 16, 512, 512), (3, 4, 300, 2), (300, 300, 224, 224),
             (224, 224, 224, 224)]
    rng = np.random.default_rng(11)
    rand = [tuple(int(v) for v in (*rng.integers(1, 400, 2), *rng.integers(1, 300, 2))) for _ in range(60)]
    return fixed + rand


@pytest.mark.parametrize("filt", R.FILTERS)
def test_restatement_equals_pillow(filt):
    pytest.importorskip("PIL")
    rng = np.random.default_rng(3)
    for i, (ih, iw, oh, ow) in enumerate(pillow_cases()):
        a = rng.integers(0, 256, (ih, iw, 3), dtype=np.uint8)
        if i % 3 == 0:  # smooth content too: the clamps and the rounding see other sums
            a = np.clip(np.cumsum(np.cumsum(rng.integers(-9, 10, (ih, iw, 3)), 0), 1) + 128, 0, 255).astype(np.uint8)
        got, want = R.resize(a, ow, oh, filt), R.pillow_resize(a, ow, oh, filt)
        assert got.shape == want.shape == (oh, ow, 3)
        assert np.array_equal(got, want), (filt, ih, iw, oh, ow, int((got != want).sum()))
        g = a[:, :, 1]  # one channel: Pillow's "L" mode
        assert np.array_equal(R.resize(g, ow, oh, filt), R.pillow_resize(g, ow, oh, filt)), (filt, "L", ih, iw, oh, ow)


def table_pairs():
    rng = np.random.default_rng(5)
    pairs = [(i, o) for i in (1, 2, 3, 7, 8, 224, 225, 4032) for o in (1, 2, 3, 7, 224, 225, 256, 512)]
    pairs += [(int(i), int(o)) for i, o in zip(rng.integers(1, 5000, 300), rng.integers(1, 600, 300))]
    return pairs


@pytest.mark.parametrize("filt", R.FILTERS)
def test_library_tables_equal_the_restatement(L, filt):
    n = 0
    for i, o in table_pairs():
        first, count, w = jpeggpu_amd.resize_weights(i, o, filt)
        assert w.shape[1] == R.max_taps(i, o, filt)
        if i == o:  # the skipped direction: one tap of weight 1
            assert np.array_equal(first, np.arange(o)) and (count == 1).all()
            assert (w[:, 0] == 1 << 22).all() and (w[:, 1:] == 0).all()
            continue
        rf, rc, rw = R.weights(i, o, filt)
        assert np.array_equal(first, rf) and np.array_equal(count, rc), (i, o, filt)
        assert np.array_equal(w, rw), (i, o, filt)
        assert np.abs(w).max() < 1 << 23, (i, o, filt)  # the kernels multiply in 24 bits (v_mul_i32_i24)
        n += 1
    assert n > 300


def test_weights_arguments(L):
    f, c, w = (C.c_int * 8)(), (C.c_int * 8)(), (C.c_int * 64)()
    assert L.jpeggpu_ext_resize_weights(8, 4, BILINEAR, f, c, w, 5) == Status.SUCCESS  # 2 ceil(2) + 1
    assert L.jpeggpu_ext_resize_weights(8, 4, BILINEAR, f, c, w, 4) == Status.INVALID_ARGUMENT
    assert L.jpeggpu_ext_resize_weights(8, 4, BICUBIC, f, c, w, 8) == Status.INVALID_ARGUMENT  # needs 9
    assert L.jpeggpu_ext_resize_weights(8, 4, 2, f, c, w, 64) == Status.NOT_SUPPORTED
    assert L.jpeggpu_ext_resize_weights(0, 4, BILINEAR, f, c, w, 64) == Status.INVALID_ARGUMENT
    assert L.jpeggpu_ext_resize_weights(8, 0, BILINEAR, f, c, w, 64) == Status.INVALID_ARGUMENT
    assert L.jpeggpu_ext_resize_weights(8, 4, BILINEAR, None, c, w, 64) == Status.INVALID_ARGUMENT
    assert L.jpeggpu_ext_resize_weights(8, 4, BILINEAR, f, c, None, 64) == Status.INVALID_ARGUMENT


FAKE = 1 << 40  # a device address that is never dereferenced: every call below is refused before anything is enqueued


def item(sampling=((2, 2), (1, 1), (1, 1)), size=(64, 48), crop=None):
    """(ResizeItem, objects to keep) of a made-up decoded image of `size` pixels with fake plane addresses."""
    info, src = ImgInfo(), Img()
    n = len(sampling)
    info.num_components = n
    hmax, vmax = max(s[0] for s in sampling), max(s[1] for s in sampling)
    for c, (h, v) in enumerate(sampling):
        info.subsampling.x[c], info.subsampling.y[c] = h, v
        info.sizes_x[c] = -(-size[0] * h // hmax)
        info.sizes_y[c] = -(-size[1] * v // vmax)
        src.image[c], src.pitch[c] = FAKE + c * (1 << 20), info.sizes_x[c]
    it = ResizeItem()
    it.info, it.src = C.pointer(info), C.pointer(src)
    ci = None
    if crop is not None:
        ci = CropInfo()
        ci.x, ci.y, ci.width, ci.height = crop
        for c in range(n):
            ci.full_x[c], ci.full_y[c] = info.sizes_x[c], info.sizes_y[c]
        it.crop = C.pointer(ci)
    return it, (info, src, ci)


def arr(*its):
    a = (ResizeItem * len(its))()
    for i, (it, _) in enumerate(its):
        a[i] = it
    return a


def call(L, items, n=None, w=32, h=24, filt=BILINEAR, layout=0, dst=FAKE, scratch=FAKE, size=None):
    n = len(items) if n is None else n
    if size is None:
        size = L.jpeggpu_ext_resize_scratch_size(items, n, w, h, filt) if items is not None else 0
    return L.jpeggpu_ext_resize_to_rgb(items, n, w, h, filt, layout, dst, scratch, size, None)


def test_resize_arguments(L):
    good = arr(item(), item(((1, 1),)), item(crop=(3, 5, 20, 17)))
    assert L.jpeggpu_ext_resize_scratch_size(good, 3, 32, 24, BILINEAR) > 0
    assert call(L, None, n=1) == Status.INVALID_ARGUMENT
    assert call(L, good, n=0) == Status.INVALID_ARGUMENT
    assert call(L, good, w=0) == Status.INVALID_ARGUMENT
    assert call(L, good, h=-1) == Status.INVALID_ARGUMENT
    assert call(L, good, filt=2, size=1 << 30) == Status.NOT_SUPPORTED  # NEAREST, BOX, ... are not offered
    assert call(L, good, layout=2) == Status.INVALID_ARGUMENT
    assert call(L, good, dst=None) == Status.INVALID_ARGUMENT
    assert call(L, good, scratch=None) == Status.INVALID_ARGUMENT
    need = L.jpeggpu_ext_resize_scratch_size(good, 3, 32, 24, BILINEAR)
    assert call(L, good, size=need - 1) == Status.INVALID_ARGUMENT
    # items: 2 or 4 components, non-integral ratios -> NOT_SUPPORTED; broken descriptions -> INVALID_ARGUMENT
    for bad, want in ((item(((2, 1), (1, 1))), Status.NOT_SUPPORTED),
                      (item(((1, 1),) * 4), Status.NOT_SUPPORTED),
                      (item(((3, 1), (2, 1), (1, 1))), Status.NOT_SUPPORTED),
                      (item(crop=(0, 0, 0, 10)), Status.INVALID_ARGUMENT),
                      (item(crop=(-1, 0, 10, 10)), Status.INVALID_ARGUMENT)):
        a = arr(item(), bad)
        assert L.jpeggpu_ext_resize_scratch_size(a, 2, 32, 24, BILINEAR) == 0
        assert call(L, a, size=1 << 30) == want
    it, keep = item(crop=(3, 5, 20, 17))
    keep[2].origin_x[0] = 8  # the window no longer holds the rectangle's left halo
    assert call(L, arr((it, keep)), size=1 << 30) == Status.INVALID_ARGUMENT
    it, keep = item()
    it.src.contents.image[1] = None
    assert call(L, arr((it, keep)), size=1 << 30) == Status.INVALID_ARGUMENT
    it, keep = item()
    it.info = None
    assert call(L, arr((it, keep)), size=1 << 30) == Status.INVALID_ARGUMENT


@pytest.mark.parametrize("filt", (BILINEAR, BICUBIC))
def test_scratch_size_grows_with_the_batch(L, filt):
    rng = np.random.default_rng(8)
    its = []
    for _ in range(40):
        w, h = (int(v) for v in rng.integers(8, 3000, 2))
        samp = ((2, 2), (1, 1), (1, 1)) if rng.integers(0, 2) else ((1, 1),)
        crop = (0, 0, w, h) if rng.integers(0, 2) else None
        its.append(item(samp, (w, h), crop))
    a = arr(*its)
    sizes = [L.jpeggpu_ext_resize_scratch_size(a, n, 224, 224, filt) for n in range(1, 41)]
    assert all(s > 0 for s in sizes)
    assert all(b > a_ for a_, b in zip(sizes, sizes[1:]))


def test_pins_are_pillow(L):
    """tests/golden/resize_pins.npz holds Pillow's outputs for tools/make_resize_pins.py's inputs: the restatement
    applied to the pinned Pillow RGB gives them (arrays pinned in full; larger ones by SHA-256)."""
    import hashlib

    pins = np.load(os.path.join(GOLDEN, "resize_pins.npz"))
    lib_pins = np.load(os.path.join(GOLDEN, "libjpeg_pins.npz"))
    n = 0
    for key in pins.files:
        if not key.startswith(("out/", "out_sha256/")):
            continue
        kind, name, box, size, filt = key.split("/")
        rgbkey = "rgb/" + name
        if rgbkey not in lib_pins.files:
            continue  # the photo and files pinned by hash only: checked on the GPU
        x0, y0, x1, y1 = (int(v) for v in box.split(","))
        ow, oh = (int(v) for v in size.split("x"))
        got = R.resize(lib_pins[rgbkey][y0:y1, x0:x1], ow, oh, filt)
        if kind == "out":
            assert np.array_equal(got, pins[key]), key
        else:
            assert hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest() == str(pins[key]), key
        n += 1
    assert n >= 40
