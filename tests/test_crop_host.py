"""Cropped decoding on the host (jpeggpu_ext_set_crop): argument checks, the windows parse_header reports, and the restart
segments it keeps. No GPU needed."""
import pytest

import jpeggpu_amd
from jpeggpu_amd import JpegGpuError, Status
from jpeggpu_amd import build as jbuild
from tests import cases

SCALES = (1, 2, 4, 8)


@pytest.fixture(scope="module")
def L():
    jbuild.build()
    return jpeggpu_amd.lib()


@pytest.fixture(scope="module")
def matrix():
    return cases.matrix()


def parse(data, scale=1, crop=None, shard=None, device_scan=False):
    """(info, crop_info, layout, buffer size) of one parse_header."""
    dec = jpeggpu_amd.Decoder()
    try:
        if scale != 1:
            dec.set_scale(scale)
        if crop is not None:
            dec.set_crop(*crop)
        if shard is not None:
            dec.set_segment_shard(*shard)
        if device_scan:
            dec.set_device_scan(True)
        info = dec.parse_header(data)
        return info, dec.crop_info(), dec.layout(), dec.get_buffer_size()
    finally:
        dec.cleanup()


def image_size(info):
    """Width and height of the image at the scale: the plane of a component with the largest factor has its extent."""
    n = info.num_components
    hmax, vmax = max(info.subsampling.x[:n]), max(info.subsampling.y[:n])
    w = info.sizes_x[[c for c in range(n) if info.subsampling.x[c] == hmax][0]]
    h = info.sizes_y[[c for c in range(n) if info.subsampling.y[c] == vmax][0]]
    return w, h


def expected_window(full, scale, rect):
    """The windows of jpeggpu_ext.h restated: {origin_x, origin_y, size_x, size_y} per component, and the frame MCU range."""
    x, y, w, h = rect
    n = full.num_components
    hs, vs = list(full.subsampling.x[:n]), list(full.subsampling.y[:n])
    hmax, vmax = max(hs), max(vs)
    if n == 1:  # a single component's factors are ignored
        hs, vs, hmax, vmax = [1], [1], 1, 1
    blk = 8 // scale
    lo_x = [max(x * hs[c] // hmax - 1, 0) for c in range(n)]
    hi_x = [min((x + w - 1) * hs[c] // hmax + 1, full.sizes_x[c] - 1) for c in range(n)]
    lo_y = [max(y * vs[c] // vmax - 1, 0) for c in range(n)]
    hi_y = [min((y + h - 1) * vs[c] // vmax + 1, full.sizes_y[c] - 1) for c in range(n)]
    mx0 = min(lo_x[c] // (blk * hs[c]) for c in range(n))
    mx1 = max(hi_x[c] // (blk * hs[c]) + 1 for c in range(n))
    my0 = min(lo_y[c] // (blk * vs[c]) for c in range(n))
    my1 = max(hi_y[c] // (blk * vs[c]) + 1 for c in range(n))
    win = []
    for c in range(n):
        ox, oy = mx0 * blk * hs[c], my0 * blk * vs[c]
        win.append((ox, oy, hi_x[c] + 1 - ox, hi_y[c] + 1 - oy))
    return win, (mx0, my0, mx1, my1)


def rectangles(width, height):
    """1x1 in each corner, the whole image, odd offsets, full-width bands and full-height strips."""
    out = {(0, 0, 1, 1), (width - 1, 0, 1, 1), (0, height - 1, 1, 1), (width - 1, height - 1, 1, 1), (0, 0, width, height)}
    out.add((min(3, width - 1), min(5, height - 1), max(1, min(width - 3, width // 2 + 1)), max(1, min(height - 5, height // 3 + 1))))
    out.add((width // 3 | 1 if width > 2 else 0, height // 4 | 1 if height > 2 else 0, max(1, width // 5), max(1, height // 7)))
    out.add((0, height // 3, width, max(1, height // 3)))
    out.add((0, height - max(1, height // 5), width, max(1, height // 5)))
    out.add((width // 2, 0, max(1, width // 4), height))
    out.add((width - 1, 0, 1, height))
    return sorted(r for r in out if r[0] + r[2] <= width and r[1] + r[3] <= height)


def restart_interval(data):
    """Ri of the DRI segment in front of the first scan (0: none), walking the marker segments."""
    i, ri = 2, 0
    while data[i + 1] != 0xDA:
        assert data[i] == 0xFF
        if data[i + 1] == 0xDD:
            ri = data[i + 4] << 8 | data[i + 5]
        i += 2 + (data[i + 2] << 8 | data[i + 3])
    return ri


def test_set_crop_arguments(L, matrix):
    dec = jpeggpu_amd.Decoder()
    try:
        for bad in ((-1, 0, 4, 4), (0, -1, 4, 4), (0, 0, -4, 4), (0, 0, 4, -4), (0, 0, 0, 4), (0, 0, 4, 0)):
            with pytest.raises(JpegGpuError) as e:
                dec.set_crop(*bad)
            assert e.value.status == Status.INVALID_ARGUMENT, bad
        assert L.jpeggpu_ext_set_crop(None, 0, 0, 1, 1) == Status.INVALID_ARGUMENT
        assert L.jpeggpu_ext_get_crop(dec._h, None) == Status.INVALID_ARGUMENT
        with pytest.raises(JpegGpuError) as e:  # nothing parsed yet
            dec.crop_info()
        assert e.value.status == Status.INVALID_ARGUMENT
        dec.set_crop(0, 0, 0, 0)  # clears: fine
    finally:
        dec.cleanup()


def test_crop_takes_effect_at_the_next_parse(L, matrix):
    data = matrix["ss_2x2"]  # 200 x 152
    dec = jpeggpu_amd.Decoder()
    try:
        full = dec.parse_header(data)
        dec.set_crop(50, 40, 30, 20)
        ci = dec.crop_info()  # the parsed image is still uncropped
        assert (ci.x, ci.y, ci.width, ci.height) == (0, 0, 200, 152)
        info = dec.parse_header(data)
        ci = dec.crop_info()
        assert (ci.x, ci.y, ci.width, ci.height) == (50, 40, 30, 20)
        assert info.sizes_x[0] < full.sizes_x[0] and info.sizes_y[0] < full.sizes_y[0]
        dec.set_scale(2)  # the rectangle is in pixels of the image at the scale: 100 x 76
        with pytest.raises(JpegGpuError) as e:
            dec.set_crop(80, 0, 30, 10)
            dec.parse_header(data)
        assert e.value.status == Status.INVALID_ARGUMENT
        dec.set_crop(70, 0, 30, 76)
        dec.parse_header(data)
        dec.set_crop(0, 0, 0, 0)
        info = dec.parse_header(data)
        assert [info.sizes_x[c] for c in range(3)] == [100, 50, 50]
    finally:
        dec.cleanup()


@pytest.mark.parametrize("rect", [(0, 0, 201, 1), (0, 0, 1, 153), (200, 0, 1, 1), (0, 152, 1, 1), (150, 100, 51, 10)])
def test_rectangle_outside_the_image(L, matrix, rect):
    with pytest.raises(JpegGpuError) as e:
        parse(matrix["ss_2x2"], crop=rect)
    assert e.value.status == Status.INVALID_ARGUMENT


def test_windows_match_the_formula(L, matrix):
    checked = 0
    for name, data in matrix.items():
        for scale in SCALES:
            full, full_ci, _, _ = parse(data, scale)
            n = full.num_components
            width, height = full_ci.width, full_ci.height
            if n != 2 and n != 4:
                assert (width, height) == image_size(full), name
            for rect in rectangles(width, height):
                info, ci, _, _ = parse(data, scale, crop=rect)
                win, _ = expected_window(full, scale, rect)
                assert (ci.x, ci.y, ci.width, ci.height) == rect
                for c in range(n):
                    got = (ci.origin_x[c], ci.origin_y[c], info.sizes_x[c], info.sizes_y[c])
                    assert got == win[c], (name, scale, rect, c, got, win[c])
                    assert (ci.full_x[c], ci.full_y[c]) == (full.sizes_x[c], full.sizes_y[c])
                    assert info.subsampling.x[c] == full.subsampling.x[c] and info.subsampling.y[c] == full.subsampling.y[c]
                if rect == (0, 0, width, height):  # the whole image: the windows are the planes
                    assert [info.sizes_x[c] for c in range(n)] == [full.sizes_x[c] for c in range(n)], (name, scale)
                    assert [info.sizes_y[c] for c in range(n)] == [full.sizes_y[c] for c in range(n)], (name, scale)
                checked += 1
    assert checked > 1000


def band_segments(data, full, lay_full, rect):
    """Restart segments [a, b) that hold the frame MCUs of the band's windows."""
    ri = restart_interval(data)
    _, (mx0, my0, mx1, my1) = expected_window(full, 1, rect)
    sl = lay_full.scans[0]
    mcus = sl.num_data_units // sl.data_units_per_mcu
    mcus_x = -(-image_size(full)[0] // (8 * max(full.subsampling.x[:full.num_components])))
    assert mcus % mcus_x == 0
    m0, m1 = my0 * mcus_x + mx0, (my1 - 1) * mcus_x + mx1 - 1
    return m0 // ri, m1 // ri + 1, ri, mcus


@pytest.mark.parametrize("name", ["dri_row", "dri_7", "dri_nondiv", "multi_seq_dri", "photo"])
def test_band_crop_keeps_its_segments(L, matrix, photo_bytes, name):
    data = photo_bytes if name == "photo" else matrix[name]
    full, ci, lay_full, size_full = parse(data)
    width, height = ci.width, ci.height
    for rect in ((0, height // 2 - height // 10, width, height // 5), (width // 3, height // 3, width // 3, 1 + height // 9)):
        info, _, lay, size = parse(data, crop=rect)
        a, b, ri, mcus = band_segments(data, full, lay_full, rect)
        sl, slf = lay.scans[0], lay_full.scans[0]
        assert slf.num_segments == -(-mcus // ri)
        assert sl.num_segments == b - a, (name, rect)
        assert sl.num_data_units == (min(b * ri, mcus) - a * ri) * sl.data_units_per_mcu
        assert sl.num_subsequences < slf.num_subsequences
        assert lay.transferred_bytes < lay_full.transferred_bytes
        assert size <= size_full
    if name == "photo":  # a centre 224 x 224 crop of the 12 MP photo copies a small part of its entropy-coded bytes
        _, _, lay, _ = parse(data, crop=((width - 224) // 2, (height - 224) // 2, 224, 224))
        assert lay.transferred_bytes < 0.15 * lay_full.transferred_bytes


@pytest.mark.parametrize("name", ["multi_seq_nodri", "ni_444", "ni_420", "ni_420_dri", "ni_big_last_dri"])
def test_no_segment_skipping_without_restarts_or_with_several_scans(L, matrix, name):
    data = matrix[name]
    full, ci, lay_full, size_full = parse(data)
    rect = (ci.width // 4, ci.height // 4, ci.width // 3, ci.height // 5)
    _, _, lay, size = parse(data, crop=rect)
    assert lay.transferred_bytes == lay_full.transferred_bytes and size == size_full
    for i in range(lay.num_scans):
        assert lay.scans[i].num_segments == lay_full.scans[i].num_segments
        assert lay.scans[i].num_subsequences == lay_full.scans[i].num_subsequences
        assert lay.scans[i].num_data_units == lay_full.scans[i].num_data_units


def test_device_scan_keeps_the_whole_scan(L, photo_bytes):
    full, ci, lay_full, _ = parse(photo_bytes, device_scan=True)
    _, _, lay, _ = parse(photo_bytes, crop=(100, 100, 224, 224), device_scan=True)
    assert lay.scans[0].device_scan == 1
    assert lay.transferred_bytes == lay_full.transferred_bytes


def test_shard_and_crop_do_not_go_together(L, matrix):
    with pytest.raises(JpegGpuError) as e:
        parse(matrix["dri_row"], crop=(0, 0, 16, 16), shard=(0, 2))
    assert e.value.status == Status.NOT_SUPPORTED
    parse(matrix["dri_row"], crop=(0, 0, 16, 16), shard=(0, 1))  # world 1: no shard


def test_shard_still_cuts_as_before(L, matrix):
    data = matrix["dri_row"]
    _, _, lay_full, _ = parse(data)
    n = lay_full.scans[0].num_segments
    total = 0
    for rank in range(3):
        _, _, lay, _ = parse(data, shard=(rank, 3))
        assert lay.scans[0].num_segments == n * (rank + 1) // 3 - n * rank // 3
        total += lay.scans[0].num_data_units
    assert total == lay_full.scans[0].num_data_units


def test_crop_kernels_use_no_scratch(L):
    meta = jbuild.kernel_metadata(jbuild.device_assembly(source="jg_idct.hip"))
    crop = {k: v for k, v in meta.items() if "CropJobs" in k}
    # the cropped colour conversion: the windowed instantiation of fancy_rgbi_kernel (jg_output.hip)
    crop.update({k: v for k, v in jbuild.kernel_metadata(jbuild.device_assembly(source="jg_output.hip")).items() if "fancy_rgbi_kernelILb1E" in k})
    assert sum("fancy_rgbi_kernelILb1E" in k for k in crop) == 1
    assert sum("idct_kernel" in k for k in crop) >= 9 and sum("idct_scaled_kernel" in k for k in crop) >= 12, sorted(crop)
    for k, v in crop.items():
        assert v.get("private_seg_size", 1) == 0 and v.get("uses_dynamic_stack", 0) == 0, (k, v)
        assert v["num_vgpr"] <= (256 if "idct_scaled_kernel" in k else 128), (k, v)  # the bounds of the uncropped ones
