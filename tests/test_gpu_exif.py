"""EXIF orientation on the GPU (jpeggpu_ext_planes_to_rgbi_oriented, jpeggpu_ext_crop_to_rgbi_oriented,
jpeggpu_ext_resize_to_rgb_oriented, decode_to_rgb / decode_resized with exif_transpose): every result equals Pillow's pinned
ImageOps.exif_transpose output (tests/golden/exif_pins.npz) and the restatement -- the library's stored-order RGB put
through tests/exif_ref.apply, then tests/pillow_resample_ref; guard bytes around every output and between its rows."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

from tests import exif_ref
from tests import pillow_resample_ref as R
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

GUARD = 0xA5
PAD = 64


@pytest.fixture(scope="module")
def torch_cuda(gpu_lib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def files():
    return exif_ref.gpu_files()


@pytest.fixture(scope="module")
def pins():
    return np.load(os.path.join(GOLDEN, "exif_pins.npz"))


@pytest.fixture(scope="module")
def decoded(torch_cuda, files):
    """(name, d, stored crop or None) -> (planes, info, crop_info or None, color, replicate): decoded once, shared."""
    import jpeggpu_amd
    from jpeggpu_amd.api import _needs_replication

    cache = {}

    def get(name, d=1, crop=None):
        key = (name, d, crop)
        if key not in cache:
            kw = dict(idct="islow", scale=d, scale_mode="libjpeg", progressive=True, return_color=True)
            if crop is None:
                planes, info, color = jpeggpu_amd.decode_to_planes(files[name][0], **kw)
                ci = None
            else:
                planes, info, ci, color = jpeggpu_amd.decode_to_planes(files[name][0], crop=crop, **kw)
            cache[key] = (planes, info, ci, color, _needs_replication(info, d))
        return cache[key]

    return get


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def size_of(entry):
    from jpeggpu_amd.api import _frame_size

    planes, info, ci = entry[:3]
    return (ci.width, ci.height) if ci is not None else _frame_size(info)


def stored_rgb(entry):
    """The entry's RGB in stored order, by the calls that know no orientation: (h, w, 3) numpy."""
    import jpeggpu_amd

    planes, info, ci, color, rep = entry
    out = jpeggpu_amd.planes_to_rgb(planes, info, replicate=rep, color=color) if ci is None else jpeggpu_amd.crop_to_rgb(planes, info, ci, replicate=rep, color=color)
    return out.cpu().numpy()


def convert(torch, entry, o, extra_pitch=0, stream=None, expect=0):
    """jpeggpu_ext_planes_to_rgbi_oriented / jpeggpu_ext_crop_to_rgbi_oriented into a guarded buffer: the displayed image
    as (oh, ow, 3) numpy; the bytes around it and behind each row's 3 * ow must still be the guard."""
    import jpeggpu_amd
    from jpeggpu_amd.api import Img

    L = jpeggpu_amd.lib()
    planes, info, ci, color, rep = entry
    w, h = size_of(entry)
    ow, oh = (h, w) if o >= 5 else (w, h)
    pitch = 3 * ow + extra_pitch
    src = Img()
    for c, p in enumerate(planes):
        src.image[c], src.pitch[c] = p.data_ptr(), p.stride(0)
    buf = torch.full((oh * pitch + 2 * PAD,), GUARD, dtype=torch.uint8, device="cuda:0")
    handle = stream.cuda_stream if stream is not None else None
    torch.cuda.synchronize()
    if ci is None:
        st = L.jpeggpu_ext_planes_to_rgbi_oriented(C.byref(info), int(color), o, int(rep), C.byref(src), buf[PAD:].data_ptr(), pitch, w, h, handle)
    else:
        st = L.jpeggpu_ext_crop_to_rgbi_oriented(C.byref(info), int(color), o, int(rep), C.byref(ci), C.byref(src), buf[PAD:].data_ptr(), pitch, handle)
    assert st == expect, jpeggpu_amd.status_string(st)
    torch.cuda.synchronize()
    a = buf.cpu().numpy()
    assert (a[:PAD] == GUARD).all() and (a[PAD + oh * pitch:] == GUARD).all(), "a guard byte around the output was written"
    rows = a[PAD:PAD + oh * pitch].reshape(oh, pitch)
    if expect != 0:
        assert (rows == GUARD).all(), "dst was written by a refused call"
        return None
    assert (rows[:, 3 * ow:] == GUARD).all(), "a byte between two rows was written"
    return rows[:, :3 * ow].reshape(oh, ow, 3)


def assert_pin(pins, got, name, o, d):
    key = "%s/%d/%d" % (name, o, d)
    if "rgb/" + key in pins.files:
        assert np.array_equal(got, pins["rgb/" + key]), key
    else:
        assert sha(got) == str(pins["rgb_sha256/" + key]), key


def pinned(pins, name, d):
    return any(k in pins.files for k in ("rgb/%s/1/%d" % (name, d), "rgb_sha256/%s/1/%d" % (name, d)))


@pytest.mark.parametrize("d", exif_ref.SCALES)
def test_conversion_of_every_file_and_value(torch_cuda, files, pins, decoded, d):
    """All eight values on every file: Pillow's pin, and the stored-order RGB put through the table. At 1/8 the 4:2:2 file
    is libjpeg's replicate case (4:2:0 has no subsampling left there: its chroma gets the larger IDCT)."""
    n = 0
    for name in files:
        if not pinned(pins, name, d):
            continue  # draft() does not return this size at 1 / d
        entry = decoded(name, d)
        base = stored_rgb(entry)
        for o in range(1, 9):
            got = convert(torch_cuda, entry, o)
            assert np.array_equal(got, exif_ref.apply(base, o)), (name, o, d)
            assert_pin(pins, got, name, o, d)
            n += 1
    assert n >= 8 * (14 if d == 1 else 8)
    if d == 8:
        assert decoded("s422", 8)[4] and not decoded("s420", 8)[4]  # replication was asked for where libjpeg replicates


def test_larger_pitch_and_another_stream(torch_cuda, decoded):
    s = torch_cuda.cuda.Stream()
    for name in ("s420", "ycck", "wide", "tall", "t63x65", "t65x63", "col", "row"):
        entry = decoded(name)
        base = stored_rgb(entry)
        for o in range(1, 9):
            want = exif_ref.apply(base, o)
            for extra in (1, 7, 16):  # rows that do not start on a dword, and ones that do
                assert np.array_equal(convert(torch_cuda, entry, o, extra_pitch=extra), want), (name, o, extra)
            assert np.array_equal(convert(torch_cuda, entry, o, stream=s), want), (name, o, "stream")


def displayed_rects(ow, oh):
    """Each corner, odd origins, 1 x 1, a full row and a full column of the displayed image."""
    out = [(0, 0, min(5, ow), min(3, oh)), (max(ow - 7, 0), 0, min(7, ow), min(4, oh)), (0, max(oh - 5, 0), min(6, ow), min(5, oh)),
           (max(ow - 9, 0), max(oh - 3, 0), min(9, ow), min(3, oh)), (ow // 2 | 1 if ow > 2 else 0, oh // 2 | 1 if oh > 2 else 0, 1, 1),
           (0, oh // 3, ow, 1), (ow // 3, 0, 1, oh)]
    if ow > 12 and oh > 12:
        out.append((3, 5, ow - 8, oh - 11))
    return out


@pytest.mark.parametrize("name,d", (("s420", 1), ("s422", 1), ("s440", 1), ("ycck", 1), ("wide", 1), ("tall", 1), ("t65x63", 1), ("prog", 1),
                                    ("s420", 2), ("s422", 8)))
def test_crops_in_displayed_coordinates(torch_cuda, files, decoded, name, d):
    import jpeggpu_amd

    full = decoded(name, d)
    w, h = size_of(full)
    base = stored_rgb(full)
    for o in range(1, 9):
        shown = exif_ref.apply(base, o)
        ow, oh = jpeggpu_amd.orient_size(o, w, h)
        for rect in displayed_rects(ow, oh):
            stored = jpeggpu_amd.orient_rect(o, w, h, rect)
            entry = decoded(name, d, stored)
            assert size_of(entry) == stored[2:]
            got = convert(torch_cuda, entry, o, extra_pitch=(o % 3))
            x, y, rw, rh = rect
            assert np.array_equal(got, shown[y:y + rh, x:x + rw]), (name, d, o, rect)


def test_refused_arguments_write_nothing(torch_cuda, decoded):
    entry = decoded("s420")
    for o in (0, 9):
        convert(torch_cuda, entry, o if o else 0, expect=1)
    convert(torch_cuda, entry, 6, extra_pitch=-1, expect=1)  # 3 x the displayed width, less one
    convert(torch_cuda, entry, 2, extra_pitch=-1, expect=1)
    planes, info, ci, color, rep = entry
    convert(torch_cuda, (planes, info, ci, 4, rep), 6, expect=4)  # a model that does not fit: NOT_SUPPORTED, as the _cs call


def test_decode_to_rgb_with_exif_transpose(torch_cuda, files, pins):
    import jpeggpu_amd

    for name in ("s420", "gray", "ycck", "prog", "t63x65"):
        today = jpeggpu_amd.decode_to_rgb(files[name][0]).cpu().numpy()
        for o in range(1, 9):
            data = exif_ref.with_orientation(files[name][0], o)
            got = jpeggpu_amd.decode_to_rgb(data, exif_transpose=True).cpu().numpy()
            assert_pin(pins, got, name, o, 1)
            assert np.array_equal(jpeggpu_amd.decode_to_rgb(data).cpu().numpy(), today), (name, o, "the default ignores the tag, as it did")
    for o in range(1, 9):  # a scale, and a crop in displayed pixels at that scale
        data = exif_ref.with_orientation(files["s420"][0], o)
        got = jpeggpu_amd.decode_to_rgb(data, scale=2, exif_transpose=True).cpu().numpy()
        assert_pin(pins, got, "s420", o, 2)
        oh, ow = got.shape[:2]
        rect = (ow // 3, 1, ow // 2, oh - 3)
        part = jpeggpu_amd.decode_to_rgb(data, scale=2, crop=rect, exif_transpose=True).cpu().numpy()
        assert np.array_equal(part, got[rect[1]:rect[1] + rect[3], rect[0]:rect[0] + rect[2]]), o


# ------------------------------------------------------------------------------------------------
# resize
# ------------------------------------------------------------------------------------------------

def resize(torch, entries, orients, w, h, filt="bilinear", layout="NHWC", stream=None, expect=0, cs=False):
    """jpeggpu_ext_resize_to_rgb_oriented (`cs`: jpeggpu_ext_resize_to_rgb_cs, without orientations) into a guarded
    output: numpy NHWC / NCHW."""
    import jpeggpu_amd
    from jpeggpu_amd.api import FILTERS, LAYOUTS, _color_array, _resize_items

    L = jpeggpu_amd.lib()
    n = len(entries)
    items, _keep = _resize_items([e[0] for e in entries], [e[1] for e in entries], [e[2] for e in entries])
    colors = _color_array([e[3] for e in entries], n)
    os_ = _color_array(orients, n)
    if cs:
        need = L.jpeggpu_ext_resize_scratch_size_cs(items, colors, n, w, h, FILTERS[filt])
    else:
        need = L.jpeggpu_ext_resize_scratch_size_oriented(items, colors, os_, n, w, h, FILTERS[filt])
    assert (need > 0) == (expect == 0)
    scratch = torch.empty(max(need, 1), dtype=torch.uint8, device="cuda:0")
    size = n * h * w * 3
    buf = torch.full((size + 2 * PAD,), GUARD, dtype=torch.uint8, device="cuda:0")
    handle = stream.cuda_stream if stream is not None else None
    torch.cuda.synchronize()
    if cs:
        st = L.jpeggpu_ext_resize_to_rgb_cs(items, colors, n, w, h, FILTERS[filt], LAYOUTS[layout], buf[PAD:].data_ptr(), scratch.data_ptr(), need, handle)
    else:
        st = L.jpeggpu_ext_resize_to_rgb_oriented(items, colors, os_, n, w, h, FILTERS[filt], LAYOUTS[layout], buf[PAD:].data_ptr(),
                                                  scratch.data_ptr(), need, handle)
    assert st == expect, jpeggpu_amd.status_string(st)
    torch.cuda.synchronize()
    a = buf.cpu().numpy()
    assert (a[:PAD] == GUARD).all() and (a[PAD + size:] == GUARD).all(), "a guard byte around the output was written"
    out = a[PAD:PAD + size]
    if expect != 0:
        assert (out == GUARD).all(), "dst was written by a refused call"
        return None
    out = out.reshape((n, h, w, 3) if layout == "NHWC" else (n, 3, h, w))
    return out if layout == "NHWC" else out.transpose(0, 2, 3, 1)


def want_resized(entry, o, w, h, filt):
    return R.resize(np.ascontiguousarray(exif_ref.apply(stored_rgb(entry), o)), w, h, filt)


@pytest.mark.parametrize("layout", ("NHWC", "NCHW"))
@pytest.mark.parametrize("filt", exif_ref.FILTERS)
def test_resize_of_every_value(torch_cuda, pins, decoded, filt, layout):
    """53 x 37 and 300 x 20 to 24 x 16 and 16 x 24: both passes work, one axis up and the other down among them, so a
    wrong order of the passes shows (tests/test_exif_host.py asserts that it would)."""
    for name in exif_ref.RESIZE_FILES:
        entry = decoded(name)
        w0, h0 = size_of(entry)
        for o in range(1, 9):
            ow, oh = (h0, w0) if o >= 5 else (w0, h0)
            for w, h in exif_ref.RESIZE_SIZES:
                got = resize(torch_cuda, [entry], [o], w, h, filt, layout)[0]
                assert np.array_equal(got, pins["resize/%s/%d/0,0,%d,%d/%dx%d/%s" % (name, o, ow, oh, w, h, filt)]), (name, o, w, h, "the pin")
                assert np.array_equal(got, want_resized(entry, o, w, h, filt)), (name, o, w, h, "the restatement")


def test_resize_with_more_taps_than_fit_lds_and_partial_tiles(torch_cuda, decoded):
    """To 4 x 3 and 3 x 4: 75 input samples per output sample take the weights from the table, and the last tile of output
    columns is not full; to 300 x 300: every pass upscales, several tiles of columns."""
    for name in ("wide", "tall"):
        entry = decoded(name)
        for o in range(1, 9):
            for w, h in ((4, 3), (3, 4), (300, 300)):
                for filt in exif_ref.FILTERS:
                    got = resize(torch_cuda, [entry], [o], w, h, filt)[0]
                    assert np.array_equal(got, want_resized(entry, o, w, h, filt)), (name, o, w, h, filt)


@pytest.mark.parametrize("filt", exif_ref.FILTERS)
def test_one_call_of_all_values_and_three_models(torch_cuda, decoded, filt):
    import jpeggpu_amd

    names = ("s420", "gray", "ycck", "wide", "s422", "tall", "prog", "t65x63", "gray", "ycck", "odd")
    orients = (1, 2, 3, 4, 5, 6, 7, 8, 6, 7, 5)
    entries = []
    for name, o in zip(names, orients):
        full = decoded(name)
        if name in ("wide", "s422", "ycck"):  # some as crops given in displayed coordinates
            w, h = size_of(full)
            ow, oh = jpeggpu_amd.orient_size(o, w, h)
            entries.append(decoded(name, 1, jpeggpu_amd.orient_rect(o, w, h, (1, 3, ow - 4, oh - 5))))
        else:
            entries.append(full)
    assert len({int(e[3]) for e in entries}) == 3
    for layout in ("NHWC", "NCHW"):
        got = resize(torch_cuda, entries, orients, 24, 16, filt, layout)
        for i, (e, o) in enumerate(zip(entries, orients)):
            assert np.array_equal(got[i], want_resized(e, o, 24, 16, filt)), (i, names[i], o, layout)
    s = torch_cuda.cuda.Stream()
    assert np.array_equal(resize(torch_cuda, entries, orients, 24, 16, filt, stream=s), got)


def test_orientation_one_is_the_cs_call(torch_cuda, decoded):
    entries = [decoded(n) for n in ("s420", "gray", "ycck", "wide", "tall", "prog")] + [decoded("s420", 1, (3, 5, 40, 30))]
    for filt in exif_ref.FILTERS:
        for layout in ("NHWC", "NCHW"):
            a = resize(torch_cuda, entries, [1] * len(entries), 24, 16, filt, layout)
            b = resize(torch_cuda, entries, [1] * len(entries), 24, 16, filt, layout, cs=True)
            assert np.array_equal(a, b)


def test_refused_resize_calls(torch_cuda, decoded):
    entries = [decoded("s420"), decoded("gray")]
    resize(torch_cuda, entries, [1, 0], 8, 8, expect=1)
    resize(torch_cuda, entries, [9, 1], 8, 8, expect=1)


@pytest.mark.parametrize("filt", exif_ref.FILTERS)
def test_decode_resized_with_exif_transpose(torch_cuda, files, pins, filt):
    """An eight-image batch, one image per value, with seeded crops in displayed coordinates: Pillow's pins."""
    import jpeggpu_amd

    cases = exif_ref.batch_cases()
    datas = [exif_ref.with_orientation(files[name][0], o) for name, o, _ in cases]
    crops = [box for _, _, box in cases]
    got = jpeggpu_amd.decode_resized(datas, (16, 24), crops=crops, filt=filt, exif_transpose=True).cpu().numpy()
    assert got.shape == (8, 16, 24, 3)
    for i, (name, o, box) in enumerate(cases):
        assert np.array_equal(got[i], pins["resize/%s/%d/%s/24x16/%s" % (name, o, ",".join(map(str, box)), filt)]), (name, o, box)
    nchw = jpeggpu_amd.decode_resized(datas, (16, 24), crops=crops, filt=filt, layout="NCHW", exif_transpose=True).cpu().numpy()
    assert np.array_equal(nchw.transpose(0, 2, 3, 1), got)
    # without the flag the tag is ignored, as it was: the stored image's crops
    plain = jpeggpu_amd.decode_resized(datas, (16, 24), filt=filt).cpu().numpy()
    assert np.array_equal(plain, jpeggpu_amd.decode_resized([files[name][0] for name, _, _ in cases], (16, 24), filt=filt).cpu().numpy())
