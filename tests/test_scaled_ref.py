"""Scaled decoding without a GPU: the numpy restatement of libjpeg-turbo's reduced IDCTs (tests/scaled_ref.py) against
Pillow's pinned and live output, the host side of jpeggpu_ext_set_scale, and the new kernels' generated code."""
import os

import numpy as np
import pytest

import jpeggpu_amd
from jpeggpu_amd import Status
from jpeggpu_amd import build as jbuild
from oracle import oracle
from tests import cases, scaled_ref
from tests.conftest import GOLDEN


@pytest.fixture(scope="module")
def L():
    jbuild.build()
    return jpeggpu_amd.lib()


def test_restatement_equals_pinned_pillow_planes():
    z = np.load(os.path.join(GOLDEN, "scaled_pins.npz"))
    checked = 0
    for key in z.files:
        if not key.startswith("planes/"):
            continue
        _, name, d, c = key.split("/")
        mine = scaled_ref.scaled_planes(z["jpeg/" + name].tobytes(), int(d))[int(c)]
        assert mine.shape == z[key].shape and np.array_equal(mine, z[key]), key
        checked += 1
    assert checked >= 60


def _is_444_or_gray(dec):
    return dec.ncomp == 1 or (dec.ncomp == 3 and set(dec.hs) == {1} and set(dec.vs) == {1})


def test_restatement_equals_live_pillow_draft():
    pytest.importorskip("PIL")
    n = 0
    for name, data in cases.matrix().items():
        dec = oracle.decode(data)
        if not _is_444_or_gray(dec):
            continue
        for d in (2, 4, 8):
            if (name, d) == ("dense_escapes", 2):
                continue  # libjpeg-turbo's SIMD 4x4 differs from jidctred.c there (tools/make_scaled_pins.py)
            mine, pil = scaled_ref.scaled_planes_of(dec, d), scaled_ref.pillow_draft(data, d)
            assert len(mine) == len(pil), name
            for c, (a, b) in enumerate(zip(mine, pil)):
                assert a.shape == b.shape and np.array_equal(a, b), (name, d, c)
            n += 1
    assert n >= 15


def test_range_limit_wraps_like_libjpeg():
    # the post-IDCT part of libjpeg's sample_range_limit table (jdmaster.c, prepare_range_limit_table), 8-bit samples:
    # 128..255 for 0..127, 255 up to 511, 0 from 512 (the "wrapped" negatives) to 895, then 0..127 again
    table = np.concatenate([np.arange(128, 256), np.full(384, 255), np.zeros(384), np.arange(0, 128)]).astype(np.uint8)
    x = np.arange(-3000, 3000)
    assert np.array_equal(scaled_ref.range_limit(x), table[x & 1023])
    assert list(scaled_ref.range_limit([-129, -128, 127, 128, 600, -600])) == [0, 0, 255, 255, 0, 255]


def test_set_scale_rejects_other_denominators(L):
    dec = jpeggpu_amd.Decoder()
    try:
        for bad in (0, 3, 16, -2, 5):
            with pytest.raises(jpeggpu_amd.JpegGpuError) as e:
                dec.set_scale(bad)
            assert e.value.status == Status.INVALID_ARGUMENT
        for good in (1, 2, 4, 8):
            dec.set_scale(good)
    finally:
        dec.cleanup()


def test_parse_header_reports_scaled_sizes(L):
    for name, data in cases.matrix().items():
        ref = oracle.decode(data)
        hmax, vmax = max(ref.hs), max(ref.vs)
        dec = jpeggpu_amd.Decoder()
        try:
            base = dec.parse_header(data)
            sizes = {}
            for d in (2, 4, 8, 1):
                dec.set_scale(d)
                info = dec.parse_header(data)
                sizes[d] = [(info.sizes_x[c], info.sizes_y[c]) for c in range(info.num_components)]
                for c in range(ref.ncomp):
                    want_x = -(-ref.width * ref.hs[c] // (hmax * d))
                    want_y = -(-ref.height * ref.vs[c] // (vmax * d))
                    assert (info.sizes_x[c], info.sizes_y[c]) == (want_x, want_y), (name, d, c)
                    assert [info.subsampling.x[c], info.subsampling.y[c]] == [base.subsampling.x[c], base.subsampling.y[c]]
            # scale 1 reports what an unscaled decoder reports
            assert sizes[1] == [(base.sizes_x[c], base.sizes_y[c]) for c in range(base.num_components)], name
        finally:
            dec.cleanup()


def test_scale_takes_effect_at_the_next_parse_and_leaves_the_plan_alone(L):
    data = cases.matrix()["dri_7"]
    dec = jpeggpu_amd.Decoder()
    try:
        info = dec.parse_header(data)
        n1 = dec.get_buffer_size()
        lay1 = dec.layout()
        dec.set_scale(8)
        assert dec.get_buffer_size() == n1
        assert info.sizes_x[0] == dec.parse_header(data).sizes_x[0] * 8
        lay8 = dec.layout()
        assert dec.get_buffer_size() == n1  # d_tmp does not depend on the scale
        assert (lay8.subsequence_bytes, lay8.transferred_bytes, lay8.blob_bytes) == (lay1.subsequence_bytes, lay1.transferred_bytes, lay1.blob_bytes)
    finally:
        dec.cleanup()


def test_shard_rows_scale_with_the_plane(L):
    from tools import jpegsynth

    data = jpegsynth.encode(333, 251, cases.S420, restart_interval=21, seed=78)  # MCU rows of 21 MCUs, 16 luma rows each
    for world in (2, 3):
        for d in (1, 2, 4, 8):
            covered = {0: 0, 1: 0, 2: 0}
            for rank in range(world):
                dec = jpeggpu_amd.Decoder()
                try:
                    dec.set_scale(d)
                    dec.set_segment_shard(rank, world)
                    info = dec.parse_header(data)
                    for c in range(3):
                        a, n = dec.shard_rows(c)
                        v = 2 if c == 0 else 1
                        assert a == covered[c], (world, d, rank, c)
                        assert a % (8 * v // d) == 0, (world, d, rank, c)  # whole MCU rows of the scaled plane
                        covered[c] = a + n
                finally:
                    dec.cleanup()
            for c in range(3):
                assert covered[c] == info.sizes_y[c], (world, d, c)


def test_scaled_kernels_use_no_scratch():
    meta = jbuild.kernel_metadata(jbuild.device_assembly(source="jg_idct.hip"))
    scaled = {k: v for k, v in meta.items() if "idct_scaled_kernel" in k}
    assert len(scaled) >= 12, sorted(meta)  # three scales x four job sources
    for k, v in scaled.items():
        assert v.get("private_seg_size", 1) == 0 and v.get("uses_dynamic_stack", 0) == 0, (k, v)
        assert v["num_vgpr"] <= 256, (k, v)
