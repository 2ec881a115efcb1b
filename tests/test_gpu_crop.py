"""Cropped decoding on the GPU (jpeggpu_ext_set_crop, jpeggpu_ext_crop_to_rgbi_fancy): the window planes equal the
uncropped planes sliced, the rectangle's RGB equals the full image's, with guard bytes around every window plane and
every RGB output; skipped restart segments are really not decoded; batches, the device scan and lone decodes."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

from tests import cases, libjpeg_ref
from tests.conftest import GOLDEN
from tests.test_crop_host import rectangles, restart_interval
from tests.test_gpu_scaled import GUARD, Guarded, _tmp

pytestmark = pytest.mark.gpu

SCALES = (1, 2, 4, 8)


@pytest.fixture(scope="module")
def torch_cuda(gpu_lib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def matrix():
    return cases.matrix()


@pytest.fixture(scope="module")
def pins():
    return np.load(os.path.join(GOLDEN, "libjpeg_pins.npz"))


def rgb_of(torch, g, info, ci):
    """jpeggpu_ext_crop_to_rgbi_fancy of the guarded window planes into a guarded output; (h, w, 3) numpy."""
    import jpeggpu_amd
    from jpeggpu_amd.api import Img

    w, h = ci.width, ci.height
    buf = torch.full((h + 2, 3 * w + 24), GUARD, dtype=torch.uint8, device="cuda:0")
    src = Img()
    for c in range(info.num_components):
        src.image[c], src.pitch[c] = g.ptrs[c], g.pitches[c]
    st = jpeggpu_amd.lib().jpeggpu_ext_crop_to_rgbi_fancy(C.byref(info), C.byref(ci), C.byref(src), buf[1:, 8:].data_ptr(), buf.stride(0), None)
    assert st == 0, jpeggpu_amd.status_string(st)
    torch.cuda.synchronize()
    a = buf.cpu().numpy()
    out = a[1:1 + h, 8:8 + 3 * w].copy()
    a[1:1 + h, 8:8 + 3 * w] = GUARD
    assert (a == GUARD).all(), "a guard byte around the RGB output was written"
    return out.reshape(h, w, 3)


def decode(torch, data, scale=1, method="reference", crop=None, device_scan=False, subseq_bytes=None, rgb=False):
    """One lone decode (jpeggpu_decoder_decode) into guarded planes: (planes, info, crop_info[, rgb])."""
    import jpeggpu_amd

    dec = jpeggpu_amd.Decoder(subseq_bytes)
    try:
        dec.set_scale(scale)
        dec.set_idct(method)
        dec.set_device_scan(device_scan)
        if crop is not None:
            dec.set_crop(*crop)
        info = dec.parse_header(data)
        ci = dec.crop_info()
        n = dec.get_buffer_size()
        tmp, base = _tmp(torch, n)
        g = Guarded(torch, info)
        dec.transfer(base, n, 0)
        dec.decode(g.ptrs, g.pitches, base, n, 0)
        torch.cuda.synchronize()
        if device_scan:
            assert dec.device_status(base, 0) == jpeggpu_amd.Status.SUCCESS
        out = rgb_of(torch, g, info, ci) if rgb else None
        return g.planes(), info, ci, out
    finally:
        dec.cleanup()


def window_of(full_planes, info, ci):
    return [full_planes[c][ci.origin_y[c]:ci.origin_y[c] + info.sizes_y[c], ci.origin_x[c]:ci.origin_x[c] + info.sizes_x[c]]
            for c in range(info.num_components)]


def assert_window(planes, full_planes, info, ci, what):
    want = window_of(full_planes, info, ci)
    for c in range(info.num_components):
        assert planes[c].shape == want[c].shape, (what, c, planes[c].shape, want[c].shape)
        bad = np.argwhere(planes[c] != want[c])
        assert len(bad) == 0, (what, c, len(bad), bad[:4].tolist())


def full_rgb(torch, data, scale=1, method="islow"):
    import jpeggpu_amd

    planes, info = jpeggpu_amd.decode_to_planes(data, scale=scale, idct=method)
    rgb = jpeggpu_amd.planes_to_rgb(planes, info).cpu().numpy()
    return rgb


def kinds():
    return [(1, "reference"), (1, "islow"), (2, "reference"), (4, "reference"), (8, "reference")]


def test_matrix_crop_planes_equal_the_uncropped_planes_sliced(torch_cuda, matrix):
    n = 0
    for name, data in matrix.items():
        for scale, method in kinds():
            full, _, full_ci, _ = decode(torch_cuda, data, scale, method)
            for rect in rectangles(full_ci.width, full_ci.height):
                planes, info, ci, _ = decode(torch_cuda, data, scale, method, crop=rect)
                assert_window(planes, full, info, ci, (name, scale, method, rect))
                n += 1
    assert n > 1000


def _rgb_files(matrix):
    """The files of one or three components (jpeggpu_ext_crop_to_rgbi_fancy refuses two and four)."""
    import jpeggpu_amd

    out = []
    for name, data in matrix.items():
        dec = jpeggpu_amd.Decoder()
        try:
            if dec.parse_header(data).num_components in (1, 3):
                out.append(name)
        finally:
            dec.cleanup()
    assert len(out) > 20
    return out


def test_crop_rgb_equals_the_full_fancy_rgb_sliced(torch_cuda, matrix):
    for name in _rgb_files(matrix):
        data = matrix[name]
        for scale, method in ((1, "islow"), (1, "reference"), (2, "islow"), (8, "islow")):
            want = full_rgb(torch_cuda, data, scale, method)
            for rect in rectangles(want.shape[1], want.shape[0]):
                x, y, w, h = rect
                _, _, _, got = decode(torch_cuda, data, scale, method, crop=rect, rgb=True)
                assert np.array_equal(got, want[y:y + h, x:x + w]), (name, scale, method, rect)


def test_crop_rgb_equals_pillow_pins(torch_cuda, pins):
    import jpeggpu_amd

    n = 0
    for name, _, array, _ in libjpeg_ref.pinned_arrays(pins, "rgb"):
        if array is None:
            continue
        data = libjpeg_ref.pinned_jpeg(pins, name)
        for x, y, w, h in rectangles(array.shape[1], array.shape[0]):
            got = jpeggpu_amd.decode_to_rgb(data, crop=(x, y, w, h)).cpu().numpy()
            assert np.array_equal(got, array[y:y + h, x:x + w]), (name, (x, y, w, h))
            n += 1
    assert n > 0


def test_photo_crops_equal_the_full_decode(torch_cuda, photo_bytes):
    import jpeggpu_amd

    full = jpeggpu_amd.decode_to_rgb(photo_bytes).cpu().numpy()
    H, W = full.shape[:2]
    for x, y, w, h in (((W - 224) // 2, (H - 224) // 2, 224, 224), (W - 301, H - 177, 301, 177)):
        got = jpeggpu_amd.decode_to_rgb(photo_bytes, crop=(x, y, w, h)).cpu().numpy()
        assert np.array_equal(got, full[y:y + h, x:x + w]), (x, y, w, h)
    for scale in (1, 2, 4):
        planes, info, ci, _ = decode(torch_cuda, photo_bytes, scale, "islow", crop=(W // scale // 3, H // scale // 2, 224 // scale, 224 // scale))
        fp = decode(torch_cuda, photo_bytes, scale, "islow")[0]
        assert_window(planes, fp, info, ci, ("photo", scale))


def _segments(data):
    """[(begin, end)] file offsets of the entropy-coded bytes of each restart segment of a one-scan file."""
    sos = data.index(b"\xff\xda")
    i = sos + 2 + (data[sos + 2] << 8 | data[sos + 3])
    begin, out = i, []
    while i < len(data) - 1:
        if data[i] == 0xFF and data[i + 1] != 0x00:
            out.append((begin, i))
            if not 0xD0 <= data[i + 1] <= 0xD7:
                break
            begin = i + 2
            i += 2
            continue
        i += 1
    return out


def _corrupt(data, begin, end):
    """Flip bits of bytes in [begin, end) without making (or breaking) a marker or a stuffed zero."""
    b = bytearray(data)
    changed = 0
    for i in range(begin + 1, end - 1, 3):
        if b[i] in (0xFF, 0x00) or b[i - 1] == 0xFF:
            continue
        v = b[i] ^ 0x5A
        if v == 0xFF:
            continue
        b[i] = v
        changed += 1
    assert changed > 0
    return bytes(b)


@pytest.mark.parametrize("name", ["dri_row", "dri_7", "multi_seq_dri"])
def test_skipped_segments_are_not_decoded(torch_cuda, matrix, name):
    data = matrix[name]
    segs = _segments(data)
    assert len(segs) > 4 and restart_interval(data) > 0
    full, _, ci, _ = decode(torch_cuda, data)
    band = (0, ci.height - ci.height // 4, ci.width, ci.height // 4)  # the bottom quarter: segment 0 is far outside it
    bad = _corrupt(data, *segs[0])
    clean_crop, _, _, _ = decode(torch_cuda, data, crop=band)
    bad_crop, _, _, _ = decode(torch_cuda, bad, crop=band)
    for c in range(len(clean_crop)):
        assert np.array_equal(bad_crop[c], clean_crop[c]), (name, c)
    bad_full, _, _, _ = decode(torch_cuda, bad)
    assert any(not np.array_equal(bad_full[c], full[c]) for c in range(len(full))), name


def _batch_decode(torch, items, hint):
    """items: [(bytes, scale, method, crop or None, device_scan)] through one jpeggpu_ext_decode_batch call."""
    import jpeggpu_amd

    keep, entries, total = [], [], 0
    for data, d, method, crop, dscan in items:
        dec = jpeggpu_amd.Decoder()
        dec.set_batch_hint(hint)
        dec.set_scale(d)
        dec.set_idct(method)
        dec.set_device_scan(dscan)
        if crop is not None:
            dec.set_crop(*crop)
        info = dec.parse_header(data)
        ci = dec.crop_info()
        n = dec.get_buffer_size()
        tmp, base = _tmp(torch, n)
        g = Guarded(torch, info)
        dec.transfer(base, n, 0)
        total += dec.layout().num_scans
        keep.append((dec, tmp, g, base, info, ci))
        entries.append((dec, g.ptrs, g.pitches, base, n))
    batch = jpeggpu_amd.Batch(total)
    scratch = torch.empty(batch.scratch_size, dtype=torch.uint8, device="cuda:0")
    batch.set_items(entries)
    batch.decode(scratch.data_ptr(), 0)
    torch.cuda.synchronize()
    out = []
    for dec, _tmp_, g, base, info, ci in keep:
        assert dec.device_status(base, 0) == jpeggpu_amd.Status.SUCCESS
        out.append((g.planes(), info, ci))
        dec.cleanup()
    batch.destroy()
    return out


def test_batch_mixes_cropped_uncropped_scaled_and_islow(torch_cuda, matrix):
    import jpeggpu_amd

    names = ["multi_seq_dri", "ni_420_dri", "four_comp_opt", "gray", "odd_1x1px", "cfg4_small", "dri_1", "odd_partial_mcu",
             "ss_4x1", "q16_tables", "dense_escapes", "ni_big_last", "dri_row", "dri_nondiv"]
    pattern = [(1, "islow", True), (1, "reference", False), (2, "reference", True), (1, "reference", True), (8, "reference", True),
               (1, "islow", False), (4, "reference", True)]
    full = {}
    items = []
    for k, name in enumerate(names + names[::-1]):
        d, method, cropped = pattern[k % len(pattern)]
        if (name, d, method) not in full:
            full[(name, d, method)] = decode(torch_cuda, matrix[name], d, method)
        ci = full[(name, d, method)][2]
        rect = rectangles(ci.width, ci.height)[k % len(rectangles(ci.width, ci.height))] if cropped else None
        items.append((matrix[name], d, method, rect, k % 3 == 1))
    keys = [(name, *pattern[k % len(pattern)][:2]) for k, name in enumerate(names + names[::-1])]
    for hint in (0, 64):
        for (data, d, method, rect, dscan), (planes, info, ci), key in zip(items, _batch_decode(torch_cuda, items, hint), keys):
            assert_window(planes, full[key][0], info, ci, (key, rect, dscan, hint))
    # a batch of one cropped item: decoded as jpeggpu_decoder_decode decodes it
    ref = decode(torch_cuda, matrix["multi_seq_dri"])[0]
    for rect in ((0, 0, 1, 1), (100, 200, 300, 150)):
        (planes, info, ci), = _batch_decode(torch_cuda, [(matrix["multi_seq_dri"], 1, "reference", rect, False)], 0)
        assert_window(planes, ref, info, ci, rect)
    assert jpeggpu_amd.fused_tail_timeouts() == 0


def test_full_batch_of_64_random_resized_crops(torch_cuda):
    """BASELINE.json configs[2] (64 x 12 MP 4:2:0) in one call, each item a seeded RandomResizedCrop-style rectangle (half
    of them ISLOW): the windows against the lone uncropped decodes, and no fused-tail writer timed out."""
    import jpeggpu_amd
    from tools import crop_rate, jpegsynth

    datas = [jpegsynth.config(2, seed=100 + s) for s in range(4)]
    rng = np.random.default_rng(7)
    items, keys = [], []
    full = {}
    for i in range(64):
        method = "islow" if i % 2 else "reference"
        if (i % 4, method) not in full:
            full[(i % 4, method)] = decode(torch_cuda, datas[i % 4], 1, method)
        ci = full[(i % 4, method)][2]
        items.append((datas[i % 4], 1, method, crop_rate.random_resized_crop(rng, ci.width, ci.height), False))
        keys.append((i % 4, method))
    got = _batch_decode(torch_cuda, items, 64)
    for (planes, info, ci), key, it in zip(got, keys, items):
        assert_window(planes, full[key][0], info, ci, (key, it[3]))
    assert jpeggpu_amd.fused_tail_timeouts() == 0


@pytest.mark.parametrize("name", ["dri_row", "multi_seq_nodri", "ni_big_last", "ni_big_last_dri", "cfg2_small"])
def test_device_scan_with_a_crop(torch_cuda, matrix, name):
    data = matrix[name]
    full, _, ci, _ = decode(torch_cuda, data, device_scan=True)
    for rect in rectangles(ci.width, ci.height):
        for scale, method in ((1, "reference"), (1, "islow")):
            planes, info, cci, _ = decode(torch_cuda, data, scale, method, crop=rect, device_scan=True)
            ref = full if method == "reference" else decode(torch_cuda, data, 1, "islow")[0]
            assert_window(planes, ref, info, cci, (name, rect, method))


def test_device_scan_failure_with_a_crop_leaves_the_planes(torch_cuda):
    """A truncated scan found on the device (ip.num_du = 0): the cropped decode writes nothing and reports the status."""
    import jpeggpu_amd

    data = cases.matrix()["dri_row"]
    cut = data[:len(data) * 2 // 3]  # no terminating marker
    dec = jpeggpu_amd.Decoder()
    try:
        dec.set_device_scan(True)
        dec.set_crop(10, 10, 100, 60)
        info = dec.parse_header(cut)
        n = dec.get_buffer_size()
        tmp, base = _tmp(torch_cuda, n)
        g = Guarded(torch_cuda, info)
        for buf in g.bufs:
            buf.fill_(GUARD)
        dec.transfer(base, n, 0)
        dec.decode(g.ptrs, g.pitches, base, n, 0)
        torch_cuda.cuda.synchronize()
        assert dec.device_status(base, 0) != jpeggpu_amd.Status.SUCCESS
        for p in g.planes():
            assert (p == GUARD).all()
    finally:
        dec.cleanup()


def test_lone_decode_of_the_photo_with_a_crop(torch_cuda, photo_bytes):
    """jpeggpu_decoder_decode of a cropped 12 MP photo (multi-hypothesis speculation on its restart segments) at two
    subsequence sizes, and the cropped buffer is smaller."""
    import jpeggpu_amd

    full, _, ci, _ = decode(torch_cuda, photo_bytes)
    for sb in (None, 32, 256):
        for rect in ((ci.width // 2 - 112, ci.height // 2 - 112, 224, 224), (0, ci.height // 4, ci.width, ci.height // 2)):
            planes, info, cci, _ = decode(torch_cuda, photo_bytes, crop=rect, subseq_bytes=sb)
            assert_window(planes, full, info, cci, (sb, rect))
    digest = hashlib.sha256(full[0].tobytes()).hexdigest()
    assert digest == hashlib.sha256(jpeggpu_amd.decode_to_planes(photo_bytes)[0][0].cpu().numpy().tobytes()).hexdigest()
