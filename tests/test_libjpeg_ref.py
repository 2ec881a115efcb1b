"""libjpeg-compatible full-size decoding without a GPU: the numpy restatement of jpeg_idct_islow, fancy upsampling and
the integer colour conversion (tests/libjpeg_ref.py) against Pillow's pinned and live output, the 32-bit bound of the
kernel's pass 1, the host side of jpeggpu_ext_set_idct and the new kernels' generated code."""
import hashlib
import itertools
import os

import numpy as np
import pytest

import jpeggpu_amd
from jpeggpu_amd import Status
from jpeggpu_amd import build as jbuild
from oracle import oracle
from tests import cases, libjpeg_ref
from tests.conftest import GOLDEN


@pytest.fixture(scope="module")
def L():
    jbuild.build()
    return jpeggpu_amd.lib()


@pytest.fixture(scope="module")
def pins():
    return np.load(os.path.join(GOLDEN, "libjpeg_pins.npz"))


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def test_restatement_equals_pinned_pillow_planes(pins):
    checked = 0
    for name, c, array, sha in libjpeg_ref.pinned_arrays(pins, "planes"):
        mine = libjpeg_ref.islow_planes(libjpeg_ref.pinned_jpeg(pins, name))[c]
        assert libjpeg_ref.matches_pin(mine, array, sha), (name, c)
        checked += 1
    assert checked >= 30  # 4:4:4 and grayscale files of the matrix and Pillow-encoded ones


def test_restatement_equals_pinned_pillow_rgb(pins):
    checked = 0
    for name, _, array, sha in libjpeg_ref.pinned_arrays(pins, "rgb"):
        mine = libjpeg_ref.libjpeg_rgb(libjpeg_ref.pinned_jpeg(pins, name))
        assert libjpeg_ref.matches_pin(mine, array, sha), name
        checked += 1
    assert checked >= 47  # 26 matrix files, 21 Pillow-encoded ones


def test_restatement_equals_pinned_photo_rgb(pins, photo_bytes):
    assert _sha(libjpeg_ref.libjpeg_rgb(photo_bytes)) == str(pins["photo_rgb_sha256"])


def test_restatement_equals_live_pillow():
    pytest.importorskip("PIL")
    n = 0
    for name, data in cases.matrix().items():
        if name == "dense_escapes":
            continue  # libjpeg-turbo's SIMD ISLOW differs from jidctint.c there (tools/make_libjpeg_pins.py)
        dec = oracle.decode(data)
        if dec.ncomp not in (1, 3):
            continue
        mine, pil = libjpeg_ref.libjpeg_rgb_of(dec), libjpeg_ref.pillow_rgb(data)
        assert mine.shape == pil.shape and np.array_equal(mine, pil), name
        n += 1
    assert n >= 26


def test_restatement_differs_from_the_reference_idct_on_the_photo(photo_bytes):
    dec = oracle.decode(photo_bytes)
    mine = libjpeg_ref.islow_planes_of(dec)
    differ = sum(int((a != b).sum()) for a, b in zip(mine, dec.planes))
    assert differ > 1_000_000, differ  # about 19 % of the luma samples alone
    assert all(int(np.abs(a.astype(int) - b.astype(int)).max()) <= 8 for a, b in zip(mine, dec.planes))


def test_pass1_bound_holds_on_every_sign_pattern():
    """jg_idct.hip, kIslowPass1Max: with every input of a column within +-32,767 each pass-1 output, plus DESCALE's
    2^10, fits an int -- on every sign pattern at the limit, which is where each output's magnitude is largest."""
    signs = np.array(list(itertools.product((-1, 1), repeat=8)), np.int64).T  # [8, 256]
    out = libjpeg_ref.islow_1d([signs[k] * 32767 for k in range(8)])
    worst = max(int(np.abs(o).max()) for o in out)
    assert worst == 61214 * 32767
    assert worst + (1 << 10) < 2**31
    # and the bound is tight: one more in magnitude and some output leaves the int range
    out = libjpeg_ref.islow_1d([signs[k] * 35083 for k in range(8)])
    assert max(int(np.abs(o).max()) for o in out) + (1 << 10) >= 2**31


def test_range_limit_and_colour_conversion_corners():
    y = np.array([[0, 255, 128, 16]], np.uint8)
    rgb = libjpeg_ref.ycc_to_rgb(y, np.array([[255, 0, 128, 128]], np.uint8), np.array([[255, 0, 128, 240]], np.uint8))
    assert rgb[0, 0].tolist() == [178, 0, 225]  # clamped below and above
    assert rgb[0, 2].tolist() == [128, 128, 128]  # neutral chroma
    assert rgb[0, 3].tolist() == [16 + ((91881 * 112 + 32768) >> 16), max(0, 16 + ((-46802 * 112 + 32768) >> 16)), 16]


def test_fancy_upsampling_edges():
    s = np.array([[10, 20, 40], [50, 90, 130]], np.uint8)
    # h2v1: the first and last output columns are the edge samples
    out = libjpeg_ref.upsample_fancy(s, 2, 1, 6, 2)
    assert out[0].tolist() == [10, (3 * 10 + 20 + 2) >> 2, (3 * 20 + 10 + 1) >> 2, (3 * 20 + 40 + 2) >> 2, (3 * 40 + 20 + 1) >> 2, 40]
    # 2 samples wide or fewer: replication
    assert libjpeg_ref.upsample_fancy(s[:, :2], 2, 1, 4, 2)[0].tolist() == [10, 10, 20, 20]
    assert libjpeg_ref.upsample_fancy(s[:, :2], 2, 2, 4, 4)[:, 0].tolist() == [10, 10, 50, 50]
    # h1v2: biases 1 above, 2 below; the row above the first is the first
    out = libjpeg_ref.upsample_fancy(s, 1, 2, 3, 4)
    assert out[:, 0].tolist() == [10, (3 * 10 + 50 + 2) >> 2, (3 * 50 + 10 + 1) >> 2, 50]


def test_set_idct_validates_its_argument(L):
    import ctypes as C

    dec = jpeggpu_amd.Decoder()
    try:
        for bad in (-1, 2, 3, 255):
            assert L.jpeggpu_ext_set_idct(dec._h, bad) == int(Status.INVALID_ARGUMENT)
        assert L.jpeggpu_ext_set_idct(C.c_void_p(), 1) == int(Status.INVALID_ARGUMENT)
        for good in ("reference", "islow"):
            dec.set_idct(good)
        with pytest.raises(ValueError):
            dec.set_idct("ifast")
    finally:
        dec.cleanup()


def test_parse_header_does_not_depend_on_the_method(L):
    for name in ("ss_2x2", "ss_1x1", "dri_7", "odd_17x9", "ni_420_dri", "gray", "four_comp_opt"):
        data = cases.matrix()[name]
        got = []
        for method in ("reference", "islow", "reference"):
            dec = jpeggpu_amd.Decoder()
            try:
                dec.set_idct(method)
                info = dec.parse_header(data)
                lay = dec.layout()
                got.append(([(info.sizes_x[c], info.sizes_y[c], info.subsampling.x[c], info.subsampling.y[c]) for c in range(info.num_components)],
                            dec.get_buffer_size(), lay.subsequence_bytes, lay.transferred_bytes, lay.blob_bytes))
            finally:
                dec.cleanup()
        assert got[0] == got[1] == got[2], name


def test_new_kernels_use_no_scratch():
    meta = jbuild.kernel_metadata(jbuild.device_assembly(source="jg_idct.hip"))  # the IDCT stage has its own file
    output = jbuild.kernel_metadata(jbuild.device_assembly(source="jg_output.hip"))  # and so have the colour kernels
    # an instantiation in both files would be in the code object twice: the entropy pass's file holds no IDCT kernel
    entropy = jbuild.device_assembly()
    assert not set(jbuild.kernel_metadata(entropy)) & set(meta) and not any("idct_" in ln for ln in entropy)
    islow = {k: v for k, v in meta.items() if "idct_kernel" in k and "IslowJobs" in k}
    fancy = {k: v for k, v in output.items() if "fancy_rgbi_kernel" in k}
    resize = {k: v for k, v in output.items() if "resize_h_kernel" in k or "resize_v_kernel" in k}
    assert len(islow) >= 5, sorted(meta)  # four job sources and the mixed batch's view
    # fancy_rgbi_kernel<false>: the whole image; <true>: a rectangle read from the planes' windows
    assert len(fancy) == 2 and sum("fancy_rgbi_kernelILb0E" in k for k in fancy) == 1 and sum("fancy_rgbi_kernelILb1E" in k for k in fancy) == 1, sorted(output)
    assert sum("resize_h_kernel" in k for k in resize) == 1 and sum("resize_v_kernel" in k for k in resize) == 1, sorted(output)
    for k, v in {**islow, **fancy, **resize}.items():
        assert v.get("private_seg_size", 1) == 0 and v.get("uses_dynamic_stack", 0) == 0, (k, v)
        assert v["num_vgpr"] <= 128, (k, v)
