"""Batched resize on the GPU (jpeggpu_ext_resize_to_rgb, decode_resized): every result equals the numpy restatement of
Pillow's resampling (tests/pillow_resample_ref.py) applied to the RGB of jpeggpu_ext_crop_to_rgbi_fancy /
jpeggpu_ext_planes_to_rgbi_fancy, and Pillow's own outputs where they are pinned (tests/golden/resize_pins.npz); guard
bytes around every output."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

from tests import cases
from tests import pillow_resample_ref as R
from tests.conftest import GOLDEN
from tools.crop_rate import random_resized_crop

pytestmark = pytest.mark.gpu

GUARD = 0xA5
PAD = 64


@pytest.fixture(scope="module")
def torch_cuda(gpu_lib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def matrix():
    return cases.matrix()


def components(data):
    import jpeggpu_amd

    dec = jpeggpu_amd.Decoder()
    try:
        return dec.parse_header(data).num_components
    finally:
        dec.cleanup()


def decode(data, crop=None, scale=1, method="islow"):
    """(planes, info, crop_info or None) of one decode."""
    import jpeggpu_amd

    if crop is None:
        planes, info = jpeggpu_amd.decode_to_planes(data, scale=scale, idct=method)
        return planes, info, None
    return jpeggpu_amd.decode_to_planes(data, scale=scale, idct=method, crop=crop)


def rgb(entry):
    """The item's RGB as jpeggpu_ext_crop_to_rgbi_fancy (or planes_to_rgbi_fancy, uncropped) gives it: (h, w, 3) numpy."""
    import jpeggpu_amd

    planes, info, ci = entry
    out = jpeggpu_amd.planes_to_rgb(planes, info) if ci is None else jpeggpu_amd.crop_to_rgb(planes, info, ci)
    return out.cpu().numpy()


def image_size(entry):
    planes, info, ci = entry
    if ci is not None:
        return ci.width, ci.height
    n = info.num_components
    hmax, vmax = max(info.subsampling.x[:n]), max(info.subsampling.y[:n])
    return (info.sizes_x[[c for c in range(n) if info.subsampling.x[c] == hmax][0]],
            info.sizes_y[[c for c in range(n) if info.subsampling.y[c] == vmax][0]])


def run(torch, entries, w, h, filt="bilinear", layout="NHWC", stream=None, expect=0):
    """jpeggpu_ext_resize_to_rgb of the entries into a guarded output; the result as numpy NHWC / NCHW."""
    import jpeggpu_amd
    from jpeggpu_amd.api import FILTERS, LAYOUTS, _resize_items

    L = jpeggpu_amd.lib()
    n = len(entries)
    items, _keep = _resize_items([e[0] for e in entries], [e[1] for e in entries], [e[2] for e in entries])
    need = L.jpeggpu_ext_resize_scratch_size(items, n, w, h, FILTERS[filt])
    scratch = torch.empty(max(need, 1), dtype=torch.uint8, device="cuda:0")
    size = n * h * w * 3
    buf = torch.full((size + 2 * PAD,), GUARD, dtype=torch.uint8, device="cuda:0")
    handle = stream.cuda_stream if stream is not None else None
    torch.cuda.synchronize()
    st = L.jpeggpu_ext_resize_to_rgb(items, n, w, h, FILTERS[filt], LAYOUTS[layout], buf[PAD:].data_ptr(), scratch.data_ptr(),
                                     need, handle)
    assert st == expect, jpeggpu_amd.status_string(st)
    torch.cuda.synchronize()
    a = buf.cpu().numpy()
    assert (a[:PAD] == GUARD).all() and (a[PAD + size:] == GUARD).all(), "a guard byte around the output was written"
    out = a[PAD:PAD + size]
    if expect != 0:
        assert (out == GUARD).all(), "dst was written by a refused call"
        return None
    return out.reshape((n, h, w, 3) if layout == "NHWC" else (n, 3, h, w))


def want(entry, w, h, filt):
    return R.resize(rgb(entry), w, h, filt)


def assert_items(got, entries, w, h, filt, layout, what):
    for i, e in enumerate(entries):
        g = got[i] if layout == "NHWC" else got[i].transpose(1, 2, 0)
        exp = want(e, w, h, filt)
        bad = np.argwhere(g != exp)
        assert len(bad) == 0, (what, i, filt, layout, len(bad), bad[:4].tolist())


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def test_matrix_files_equal_the_restatement(torch_cuda, matrix):
    n = 0
    for name, data in matrix.items():
        if components(data) not in (1, 3):
            continue
        full = decode(data)
        W, H = image_size(full)
        rect = (W // 5, H // 7, max(1, W // 2), max(1, H // 3))
        for entry in (full, decode(data, crop=rect)):
            iw, ih = image_size(entry)
            for w, h in ((max(1, iw // 3), max(1, ih // 4)), (iw + 13, ih + 7), (iw, max(1, ih // 2))):
                for filt in R.FILTERS:
                    got = run(torch_cuda, [entry], w, h, filt)
                    assert_items(got, [entry], w, h, filt, "NHWC", (name, iw, ih, w, h))
                    n += 1
    assert n >= 26 * 2 * 3 * 2


def test_pillow_pins(torch_cuda, photo_bytes):
    """Pillow's Image.open(f).convert("RGB").crop(box).resize(size, filter), pinned: decode (ISLOW, the box as the crop)
    followed by the resize gives exactly that."""
    pins = np.load(os.path.join(GOLDEN, "resize_pins.npz"))
    lib_pins = np.load(os.path.join(GOLDEN, "libjpeg_pins.npz"))
    groups = {}
    for key in pins.files:
        kind, name, box, size, filt = key.split("/")
        groups.setdefault((name, box), []).append((kind, size, filt, key))
    n = 0
    for (name, box), rows in groups.items():
        data = photo_bytes if name == "photo" else lib_pins["jpeg/" + name].tobytes()
        x0, y0, x1, y1 = (int(v) for v in box.split(","))
        full = decode(data)
        whole = (x0, y0) == (0, 0) and (x1, y1) == image_size(full)
        entry = full if whole else decode(data, crop=(x0, y0, x1 - x0, y1 - y0))
        for kind, size, filt, key in rows:
            w, h = (int(v) for v in size.split("x"))
            got = run(torch_cuda, [entry], w, h, filt)[0]
            if kind == "out":
                assert np.array_equal(got, pins[key]), key
            else:
                assert sha(got) == str(pins[key]), key
            n += 1
    assert n == len(pins.files) >= 400


def test_two_and_four_components_are_not_supported(torch_cuda, matrix):
    for name in ("two_comp", "four_comp_opt", "four_comp_444"):
        planes, info = __import__("jpeggpu_amd").decode_to_planes(matrix[name])
        run(torch_cuda, [decode(matrix["ss_2x2"]), (planes, info, None)], 32, 24, expect=4)


def mixed_entries(matrix):
    """Grey and colour, every sampling layout of the matrix (h1v2 among them), cropped and whole, scale 1/2 and the
    reference IDCT; for a 120 x 90 output: down- and up-scaling, and one item whose width is unchanged."""
    e = []
    for name in ("gray", "gray_hdr_2x2", "ss_1x1", "ss_2x1", "ss_2x2", "ss_1x2", "ss_4x1", "odd_partial_mcu"):
        e.append(decode(matrix[name]))
    for name, rect in (("ss_1x2", (13, 9, 57, 41)), ("ss_2x1", (10, 5, 120, 70)), ("ss_4x1", (3, 3, 150, 140)),
                       ("gray", (1, 2, 30, 20)), ("dri_7", (31, 17, 150, 100)), ("odd_17x9", (1, 1, 15, 7))):
        e.append(decode(matrix[name], crop=rect))
    e.append(decode(matrix["ss_2x2"], scale=2))
    e.append(decode(matrix["ss_2x1"], scale=2, crop=(5, 3, 60, 40)))
    e.append(decode(matrix["ss_2x2"], method="reference"))
    e.append(decode(matrix["cfg2_small"], method="reference", crop=(7, 9, 130, 90)))
    return e


@pytest.mark.parametrize("layout", ("NHWC", "NCHW"))
@pytest.mark.parametrize("filt", R.FILTERS)
def test_mixed_batch(torch_cuda, matrix, layout, filt):
    entries = mixed_entries(matrix)
    assert (120, 70) in [image_size(e) for e in entries]  # the width-unchanged item
    got = run(torch_cuda, entries, 120, 90, filt, layout)
    assert_items(got, entries, 120, 90, filt, layout, "mixed")


def test_layouts_agree(torch_cuda, matrix):
    entries = mixed_entries(matrix)
    a = run(torch_cuda, entries, 67, 45, "bicubic", "NHWC")
    b = run(torch_cuda, entries, 67, 45, "bicubic", "NCHW")
    assert np.array_equal(a, b.transpose(0, 2, 3, 1))


def test_random_resized_crop_batch(torch_cuda):
    """64 configs[2] images (4032 x 3024 4:2:0) with seeded RandomResizedCrop rectangles, to 224 x 224 through
    decode_resized (one batch decode + one resize call), against the per-image route."""
    import jpeggpu_amd
    from tools import jpegsynth

    cfg = [jpegsynth.config(2, seed=100 + s) for s in range(8)]
    datas = [cfg[i % 8] for i in range(64)]
    rng = np.random.default_rng(2024)
    rects = [random_resized_crop(rng, 4032, 3024) for _ in range(64)]
    got = jpeggpu_amd.decode_resized(datas, 224, crops=rects).cpu().numpy()
    assert got.shape == (64, 224, 224, 3)
    for i in range(64):
        exp = want(decode(datas[i], crop=rects[i]), 224, 224, "bilinear")
        assert np.array_equal(got[i], exp), (i, rects[i], int((got[i] != exp).sum()))


def test_one_pixel_output_and_a_large_upscale(torch_cuda, matrix, photo_bytes):
    photo = decode(photo_bytes, crop=(1000, 700, 1500, 1100))
    small = decode(matrix["ss_2x2"], crop=(40, 30, 16, 16))
    for filt in R.FILTERS:
        got = run(torch_cuda, [photo, decode(matrix["gray"])], 1, 1, filt)
        assert_items(got, [photo, decode(matrix["gray"])], 1, 1, filt, "NHWC", "1x1")
        got = run(torch_cuda, [small], 512, 512, filt, "NCHW")
        assert_items(got, [small], 512, 512, filt, "NCHW", "16 -> 512")


def test_non_default_stream(torch_cuda, matrix):
    import jpeggpu_amd

    entries = mixed_entries(matrix)
    ref = run(torch_cuda, entries, 96, 64, "bilinear")
    s = torch_cuda.cuda.Stream()
    assert np.array_equal(run(torch_cuda, entries, 96, 64, "bilinear", stream=s), ref)
    with torch_cuda.cuda.stream(s):
        out = jpeggpu_amd.resize_to_rgb([e[0] for e in entries], [e[1] for e in entries], (64, 96),
                                        [e[2] for e in entries], "bilinear")
    s.synchronize()
    assert np.array_equal(out.cpu().numpy(), ref)


@pytest.mark.parametrize("layout", ("NHWC", "NCHW"))
def test_decode_resized_equals_the_per_image_route(torch_cuda, matrix, layout):
    import jpeggpu_amd

    names = ["gray", "ss_1x1", "ss_2x1", "ss_2x2", "ss_1x2", "ss_4x1", "dri_7", "ni_420", "q100_noisy", "cfg2_small"]
    datas = [matrix[n] for n in names]
    crops = [None, (5, 5, 100, 80), None, (33, 21, 77, 99), (0, 0, 200, 152), None, (100, 50, 140, 118), (1, 1, 10, 10),
             None, (10, 10, 64, 64)]
    for filt in R.FILTERS:
        got = jpeggpu_amd.decode_resized(datas, (70, 90), crops=crops, filt=filt, layout=layout).cpu().numpy()
        assert got.shape == ((10, 70, 90, 3) if layout == "NHWC" else (10, 3, 70, 90))
        entries = [decode(d, crop=c) for d, c in zip(datas, crops)]
        assert_items(got, entries, 90, 70, filt, layout, "decode_resized")
