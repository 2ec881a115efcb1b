"""Grey output on the host: jpeggpu_ext_set_luma_only at parse_header, and every refusal and scratch size of the grey output
calls -- each returned before anything is enqueued, so with made-up device addresses and without a device. No GPU needed."""
import ctypes as C

import pytest

import jpeggpu_amd
from jpeggpu_amd import Status
from jpeggpu_amd import build as jbuild
from jpeggpu_amd.api import ResizeItem, ResizeView, TensorSpec
from tests import color_ref, exif_ref, gray_ref
from tests.test_batch_rgb_host import FAKE, arr, item

GRAY, YCBCR, RGB, CMYK, YCCK = 1, 2, 3, 4, 5
BILINEAR, NHWC = 0, 0
FILES = gray_ref.files()


@pytest.fixture(scope="module")
def L():
    jbuild.build()
    return jpeggpu_amd.lib()


def parse(data, luma):
    dec = jpeggpu_amd.Decoder()
    try:
        dec.set_luma_only(luma)
        info = dec.parse_header(data)
        lay = dec.layout()
        scans = [(s.num_data_units, s.data_units_per_mcu, s.num_subsequences, s.off_symbols, s.off_du_table) for s in lay.scans[:lay.num_scans]]
        return (list(info.sizes_x), list(info.sizes_y), info.num_components, list(info.subsampling.x), list(info.subsampling.y),
                dec.get_buffer_size(), lay.num_scans, lay.transferred_bytes, lay.blob_bytes, scans)
    finally:
        dec.cleanup()


def test_set_luma_only_arguments(L):
    dec = jpeggpu_amd.Decoder()
    try:
        assert L.jpeggpu_ext_set_luma_only(None, 1) == Status.INVALID_ARGUMENT
        assert L.jpeggpu_ext_set_luma_only(dec._h, 2) == Status.INVALID_ARGUMENT
        assert L.jpeggpu_ext_set_luma_only(dec._h, -1) == Status.INVALID_ARGUMENT
        assert L.jpeggpu_ext_set_luma_only(dec._h, 1) == 0 and L.jpeggpu_ext_set_luma_only(dec._h, 0) == 0
    finally:
        dec.cleanup()


@pytest.mark.parametrize("name", ("s420", "s411", "gray", "rgb", "ni", "luma_small"))
def test_layout_and_buffer_size_are_unchanged(L, name):
    """set_luma_only(0) leaves parse_header's sizes, jpeggpu_ext_get_layout and the buffer size as they were -- and so does
    set_luma_only(1): only the IDCT stage differs."""
    plain = parse(FILES[name], False)
    assert parse(FILES[name], True) == plain
    dec = jpeggpu_amd.Decoder()
    try:
        info = dec.parse_header(FILES[name])
        assert (list(info.sizes_x), dec.get_buffer_size()) == (plain[0], plain[5])  # a decoder that was never told
    finally:
        dec.cleanup()


def test_models_without_a_grey_are_refused_at_parse_header(L):
    from tools import jpegsynth

    four = jpegsynth.encode(40, 24, ((1, 1),) * 4, seed=1)
    two = jpegsynth.encode(40, 24, ((1, 1),) * 2, seed=2)
    for data in (four, color_ref.splice(four, color_ref.app14_adobe(2)), exif_ref.gpu_files()["ycck"][0], two):
        dec = jpeggpu_amd.Decoder()
        try:
            dec.parse_header(data)  # taken without the setting
            dec.set_luma_only(True)
            with pytest.raises(jpeggpu_amd.JpegGpuError) as e:
                dec.parse_header(data)
            assert e.value.status == Status.NOT_SUPPORTED
            dec.set_luma_only(False)
            dec.parse_header(data)
        finally:
            dec.cleanup()


def one(L, it, o=1, color=None, dst=FAKE, pitch=None, crop=True):
    i, keep = it
    w, h = (i.crop.contents.width, i.crop.contents.height) if i.crop else (i.info.contents.sizes_x[0], i.info.contents.sizes_y[0])
    ow = h if o >= 5 else w
    return L.jpeggpu_ext_crop_to_gray_oriented(i.info, i.color if color is None else color, o, 0, i.crop if crop else None, i.src, dst,
                                               ow if pitch is None else pitch, None)


def test_single_image_refusals(L):
    good = item()
    assert one(L, good, o=0) == Status.INVALID_ARGUMENT and one(L, good, o=9) == Status.INVALID_ARGUMENT
    assert one(L, good, dst=None) == Status.INVALID_ARGUMENT
    assert one(L, good, pitch=63) == Status.INVALID_ARGUMENT
    assert one(L, good, o=6, pitch=47) == Status.INVALID_ARGUMENT
    assert one(L, good, color=GRAY) == Status.NOT_SUPPORTED       # a model that does not fit the component count
    assert one(L, good, color=0) == Status.NOT_SUPPORTED          # UNKNOWN
    four = item(sampling=((1, 1),) * 4, color=CMYK)
    assert one(L, four) == Status.NOT_SUPPORTED and one(L, four, color=YCCK) == Status.NOT_SUPPORTED
    assert one(L, item(sampling=((3, 1), (2, 1), (1, 1)))) == Status.NOT_SUPPORTED  # a non-integral ratio
    assert L.jpeggpu_ext_crop_to_gray_oriented(None, YCBCR, 1, 0, None, good[0].src, FAKE, 64, None) == Status.INVALID_ARGUMENT
    assert L.jpeggpu_ext_crop_to_gray_oriented(good[0].info, YCBCR, 1, 0, None, None, FAKE, 64, None) == Status.INVALID_ARGUMENT
    # a YCbCr source needs plane 0 alone; an RGB-coded one all three
    luma, keep = item()
    keep[1].image[1] = keep[1].image[2] = None
    no0, keep0 = item()
    keep0[1].image[0] = None
    assert one(L, (no0, keep0)) == Status.INVALID_ARGUMENT
    assert one(L, (luma, keep), color=RGB) == Status.INVALID_ARGUMENT
    # a window that does not hold the rectangle
    bad = item(crop=(8, 8, 16, 16))
    bad[1][2].full_x[0] = 4
    assert one(L, bad) == Status.INVALID_ARGUMENT


def test_batch_refusals_and_scratch(L):
    size = L.jpeggpu_ext_batch_gray_scratch_size
    assert size(0) == 0 and size(-1) == 0 and size(65536) == 0
    sizes = [size(n) for n in range(1, 41)]
    assert all(s > 0 for s in sizes) and all(b >= a for a, b in zip(sizes, sizes[1:]))
    call = lambda a, n, scratch=FAKE, ss=None: L.jpeggpu_ext_batch_to_gray(a, n, scratch, size(max(n, 1)) if ss is None else ss, None)
    g = lambda **kw: item(layout=1, **kw)  # (the CHW pitch of the RGB call: one byte per pixel)
    assert call(None, 1) == Status.INVALID_ARGUMENT
    assert call(arr(g()), 0) == Status.INVALID_ARGUMENT and call(arr(g()), 65536) == Status.INVALID_ARGUMENT
    assert call(arr(g()), 1, scratch=None) == Status.INVALID_ARGUMENT
    assert call(arr(g()), 1, ss=size(1) - 1) == Status.INVALID_ARGUMENT
    assert call(arr(g(), g(o=9)), 2) == Status.INVALID_ARGUMENT
    assert call(arr(g(), g(dst=None)), 2) == Status.INVALID_ARGUMENT
    assert call(arr(g(), g(pitch=63)), 2) == Status.INVALID_ARGUMENT
    assert call(arr(g(o=5, pitch=47)), 1) == Status.INVALID_ARGUMENT
    assert call(arr(g(), g(sampling=((1, 1),) * 4, color=CMYK)), 2) == Status.NOT_SUPPORTED
    assert call(arr(g(sampling=((1, 1),) * 4, color=YCCK)), 1) == Status.NOT_SUPPORTED
    assert call(arr(g(color=0)), 1) == Status.NOT_SUPPORTED


def resize_items(n, size=(64, 48)):
    its = [item(size=size) for _ in range(n)]
    a = (ResizeItem * n)()
    for i, (it, _) in enumerate(its):
        a[i].info, a[i].crop, a[i].src = it.info, it.crop, it.src
    return a, its


def test_resize_scratch_and_refusals(L):
    gsize, vsize = L.jpeggpu_ext_resize_view_to_gray_scratch_size, L.jpeggpu_ext_resize_view_scratch_size
    sizes = []
    for n in range(1, 12):
        a, keep = resize_items(n)
        v = (ResizeView * n)(*[ResizeView(32, 24, 0, 0, 0) for _ in range(n)])
        g, r = gsize(a, None, None, v, n, 32, 24, BILINEAR), vsize(a, None, None, v, n, 32, 24, BILINEAR)
        assert 0 < g < r, (n, g, r)                                  # below the RGB call's for the same items
        assert gsize(a, None, None, None, n, 32, 24, BILINEAR) == g  # views == NULL: whole rectangles to the output
        sizes.append(g)
    assert all(b >= a for a, b in zip(sizes, sizes[1:]))
    a, keep = resize_items(2, size=(640, 480))
    big_g = gsize(a, None, None, None, 2, 224, 224, BILINEAR)
    big_r = L.jpeggpu_ext_resize_scratch_size(a, 2, 224, 224, BILINEAR)
    assert 0 < big_g < big_r // 2, (big_g, big_r)  # one byte per pixel between the passes, against three
    assert gsize(a, None, None, None, 0, 32, 24, BILINEAR) == 0 and gsize(a, None, None, None, 2, 0, 24, BILINEAR) == 0
    assert gsize(a, None, None, None, 2, 32, 24, 7) == 0
    spec = TensorSpec()
    spec.type, spec.mean[0], spec.std[0] = 1, 0.5, 0.25
    spec.std[1] = spec.std[2] = 0.0  # never read: a grey call has one mean and one std
    call = lambda items=a, n=2, w=32, h=24, filt=BILINEAR, layout=NHWC, sp=C.byref(spec), dst=FAKE, scratch=FAKE, ss=1 << 30, colors=None, orients=None: \
        L.jpeggpu_ext_resize_view_to_gray_tensor(items, colors, orients, None, n, w, h, filt, layout, sp, dst, scratch, ss, None)
    assert call(sp=None) == Status.INVALID_ARGUMENT
    assert call(items=None) == Status.INVALID_ARGUMENT and call(n=0) == Status.INVALID_ARGUMENT and call(w=0) == Status.INVALID_ARGUMENT
    assert call(filt=7) == Status.NOT_SUPPORTED
    assert call(layout=2) == Status.INVALID_ARGUMENT
    assert call(dst=None) == Status.INVALID_ARGUMENT and call(scratch=None) == Status.INVALID_ARGUMENT
    assert call(dst=FAKE + 2) == Status.INVALID_ARGUMENT  # float elements on an odd half
    assert call(ss=gsize(a, None, None, None, 2, 32, 24, BILINEAR) - 1) == Status.INVALID_ARGUMENT
    assert call(orients=(C.c_int * 2)(1, 9)) == Status.INVALID_ARGUMENT
    assert call(colors=(C.c_int * 2)(YCBCR, CMYK)) == Status.NOT_SUPPORTED
    bad = TensorSpec()
    bad.type, bad.std[0] = 1, 0.0
    assert call(sp=C.byref(bad)) == Status.INVALID_ARGUMENT
    bad.type = 9
    assert call(sp=C.byref(bad)) == Status.INVALID_ARGUMENT


def test_python_arguments():
    with pytest.raises(ValueError):
        jpeggpu_amd.decode_resized([b""], 8, mode="YCbCr")
    with pytest.raises(ValueError):
        jpeggpu_amd.decode_center_cropped([b""], mode="LA")
