"""Colour-model detection on the host (jpeggpu_ext_get_color_space, Decoder.color_space): every row of libjpeg's precedence
table -- JFIF and Adobe segments, component ids, component counts -- on synthetic files with the segments spliced in and the
ids patched (tests/color_ref.py), and the photo. No GPU needed."""
import ctypes as C

import pytest

import jpeggpu_amd
from jpeggpu_amd import ColorSpace, JpegGpuError, Status
from jpeggpu_amd import build as jbuild
from tests import color_ref
from tests.color_ref import IDS_RGB, app0_jfif, app14_adobe, patch_ids, splice


@pytest.fixture(scope="module")
def L():
    jbuild.build()
    return jpeggpu_amd.lib()


@pytest.fixture(scope="module")
def base():
    from tools import jpegsynth

    return {n: jpegsynth.encode(40, 24, ((2, 2),) + ((1, 1),) * (n - 1) if n > 1 else ((1, 1),), seed=50 + n) for n in (1, 2, 3, 4)}


def color_of(data, **kw):
    dec = jpeggpu_amd.Decoder()
    try:
        if kw.get("device_scan"):
            dec.set_device_scan(True)
        dec.parse_header(data)
        return dec.color_space()
    finally:
        dec.cleanup()


def test_enum_values_are_the_headers():
    assert [int(c) for c in ColorSpace] == [0, 1, 2, 3, 4, 5]
    assert [c.name for c in ColorSpace] == list(color_ref.NAMES)


def test_precedence_table(L, base):
    three, four = base[3], base[4]
    rows = [
        ("plain ids 1, 2, 3", three, ColorSpace.YCBCR),
        ("JFIF", splice(three, app0_jfif()), ColorSpace.YCBCR),
        ("Adobe 0", splice(three, app14_adobe(0)), ColorSpace.RGB),
        ("Adobe 1", splice(three, app14_adobe(1)), ColorSpace.YCBCR),
        ("Adobe 2", splice(three, app14_adobe(2)), ColorSpace.YCBCR),
        ("JFIF + Adobe 0", splice(three, app0_jfif(), app14_adobe(0)), ColorSpace.YCBCR),
        ("Adobe 0 + JFIF", splice(three, app14_adobe(0), app0_jfif()), ColorSpace.YCBCR),
        ("ids RGB", patch_ids(three, IDS_RGB), ColorSpace.RGB),
        ("ids RGB + JFIF", splice(patch_ids(three, IDS_RGB), app0_jfif()), ColorSpace.YCBCR),
        ("ids RGB + Adobe 1", splice(patch_ids(three, IDS_RGB), app14_adobe(1)), ColorSpace.YCBCR),
        ("ids in another order", patch_ids(three, (71, 82, 66)), ColorSpace.YCBCR),
        ("4 components", four, ColorSpace.CMYK),
        ("4 components + Adobe 0", splice(four, app14_adobe(0)), ColorSpace.CMYK),
        ("4 components + Adobe 1", splice(four, app14_adobe(1)), ColorSpace.YCCK),
        ("4 components + Adobe 2", splice(four, app14_adobe(2)), ColorSpace.YCCK),
        ("4 components + JFIF + Adobe 2", splice(four, app0_jfif(), app14_adobe(2)), ColorSpace.YCCK),
        ("Adobe of length 13 is ignored", splice(three, app14_adobe(0, length=13)), ColorSpace.YCBCR),
        ("Adobe of length 13 is ignored, 4 components", splice(four, app14_adobe(2, length=13)), ColorSpace.CMYK),
        ("JFIF of length 15 is ignored", splice(three, app0_jfif(length=15), app14_adobe(0)), ColorSpace.RGB),
        ("1 component", base[1], ColorSpace.GRAY),
        ("1 component + Adobe 0", splice(base[1], app14_adobe(0)), ColorSpace.GRAY),
        ("2 components", base[2], ColorSpace.UNKNOWN),
    ]
    for what, data, want in rows:
        assert color_of(data) == want, what
        assert color_of(data, device_scan=True) == want, (what, "device scan")
        assert int(want) == color_ref.model_of_file(data), (what, "the restatement")


def test_the_photo_is_ycbcr(L, photo_bytes):
    assert color_of(photo_bytes) == ColorSpace.YCBCR


def test_case_list_models(L):
    for name, (data, model) in color_ref.cases().items():
        assert int(color_of(data)) == model, name


def test_segments_change_nothing_else(L, base):
    """The planes' geometry and the decode's layout do not depend on the segments or the ids."""
    def parse(data):
        dec = jpeggpu_amd.Decoder()
        try:
            info = dec.parse_header(data)
            lay = dec.layout()
            return ([info.sizes_x[c] for c in range(4)], [info.sizes_y[c] for c in range(4)], info.num_components,
                    list(info.subsampling.x), list(info.subsampling.y), lay.num_scans, lay.scans[0].num_subsequences, dec.get_buffer_size())
        finally:
            dec.cleanup()

    for n in (3, 4):
        want = parse(base[n])
        assert parse(splice(base[n], app0_jfif(), app14_adobe(2))) == want
    assert parse(patch_ids(base[3], IDS_RGB)) == parse(base[3])


def test_a_truncated_app_segment_is_refused_as_before(L, base):
    """An APPn segment that runs past the end of the file: the status every other skipped segment gets."""
    data = base[3][:2] + b"\xff\xee\x40\x00Adobe"
    with pytest.raises(JpegGpuError) as e:
        color_of(data)
    assert e.value.status == Status.INCOMPLETE_BITSTREAM
    with pytest.raises(JpegGpuError) as e:
        color_of(base[3][:2] + b"\xff\xee\x00\x01" + base[3][2:])
    assert e.value.status == Status.INVALID_JPEG


def test_arguments(L, base):
    dec = jpeggpu_amd.Decoder()
    try:
        cs = C.c_int(77)
        assert L.jpeggpu_ext_get_color_space(dec._h, C.byref(cs)) == Status.INVALID_ARGUMENT  # nothing parsed yet
        assert L.jpeggpu_ext_get_color_space(None, C.byref(cs)) == Status.INVALID_ARGUMENT
        dec.parse_header(base[3])
        assert L.jpeggpu_ext_get_color_space(dec._h, None) == Status.INVALID_ARGUMENT
        assert cs.value == 77
        assert dec.color_space() == ColorSpace.YCBCR
        # the last parsed image's
        dec.parse_header(splice(base[4], app14_adobe(2)))
        assert dec.color_space() == ColorSpace.YCCK
        dec.parse_header(base[3])
        assert dec.color_space() == ColorSpace.YCBCR
    finally:
        dec.cleanup()


def test_color_kernels_use_no_scratch(L):
    """The all-model instantiations (jg_output.hip) under the bounds of the grey / YCbCr ones, which keep their names."""
    meta = jbuild.kernel_metadata(jbuild.device_assembly(source="jg_output.hip"))
    color = {k: v for k, v in meta.items() if "fancy_color_kernel" in k or "resize_h_color_kernel" in k}
    assert sum("fancy_color_kernelILb0E" in k for k in color) == 1 and sum("fancy_color_kernelILb1E" in k for k in color) == 1
    assert sum("resize_h_color_kernel" in k for k in color) == 1 and len(color) == 3, sorted(meta)
    for k, v in color.items():
        assert v.get("private_seg_size", 1) == 0 and v.get("uses_dynamic_stack", 0) == 0, (k, v)
        assert v["num_vgpr"] <= 128, (k, v)
