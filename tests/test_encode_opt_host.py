"""The host half of encoding with optimised Huffman tables: the `optimize` field of struct jpeggpu_ext_encode_item, what
jpeggpu_ext_encode_header, _bound and _scratch_size make of it, and that items without it plan to the byte as they did. No
GPU needed."""
import ctypes as C

import pytest

import jpeggpu_amd
from jpeggpu_amd import Status
from jpeggpu_amd import build as jbuild
from jpeggpu_amd.api import EncodeItem, encode_item
from tests import encode_cases as K
from tests import encode_opt_ref as R

CASES = K.cases()
MAX_BLOCK_BITS_OPTIMIZED = 16 + 11 + 63 * 26
ITEM_BYTES, TABLES_BYTES = 392, 4 * (2 * 16 + 2 * 256)  # sizeof(jg::enc::Item), sizeof(jg::enc::Tables)


@pytest.fixture(scope="module")
def L():
    jbuild.build()
    return jpeggpu_amd.lib()


def _args(c):
    return c["w"], c["h"], 1 if c["grey"] else 3, c["quality"], c["subsampling"], c["restart_interval"]


def _everything():
    return CASES + [c for c, _ in R.edge_cases()]


def test_struct_layout_is_unchanged():
    assert C.sizeof(EncodeItem) == 80
    assert EncodeItem.out.offset == 64 and EncodeItem.capacity.offset == 72 and EncodeItem.restart_interval.offset == 56
    assert EncodeItem.optimize.offset == 60 and EncodeItem.optimize.size == 4
    assert EncodeItem().optimize == 0 and encode_item(8, 8).optimize == 0, "a zero-initialised item asks for the standard tables"
    assert encode_item(8, 8, optimize=True).optimize == 1


def test_other_values_of_optimize_are_refused(L):
    for v in (2, -1, 256):
        it = encode_item(16, 16)
        it.optimize = v
        size = C.c_size_t(0)
        assert L.jpeggpu_ext_encode_header(C.byref(it), None, C.byref(size)) == Status.INVALID_ARGUMENT
        assert L.jpeggpu_ext_encode_bound(C.byref(it)) == 0
        assert L.jpeggpu_ext_encode_scratch_size((EncodeItem * 1)(it), 1) == 0
        it.data, it.out, it.capacity = 256, 512, 64
        it.row_pitch, it.pixel_stride, it.channel_stride = 48, 3, 1
        assert L.jpeggpu_ext_encode_batch((EncodeItem * 1)(it), 1, 256, 1 << 30, 256, 256, None) == Status.INVALID_ARGUMENT


def test_header_of_an_optimised_item_is_not_supported(L):
    for c in _everything()[::7]:
        plain = jpeggpu_amd.encode_header(*_args(c))
        it = encode_item(*_args(c), optimize=True)
        size = C.c_size_t(0)
        assert L.jpeggpu_ext_encode_header(C.byref(it), None, C.byref(size)) == Status.NOT_SUPPORTED
        assert size.value == len(plain), "the standard header's length: no optimised header is longer"
        buf = C.create_string_buffer(b"\xa5" * 1024, 1024)
        size = C.c_size_t(1024)
        assert L.jpeggpu_ext_encode_header(C.byref(it), buf, C.byref(size)) == Status.NOT_SUPPORTED and buf.raw == b"\xa5" * 1024
        with pytest.raises(jpeggpu_amd.JpegGpuError) as e:
            jpeggpu_amd.encode_header(*_args(c), optimize=True)
        assert e.value.status == Status.NOT_SUPPORTED


def _stream_bound(c, bits):
    n = K.counts(c)
    return -(-n["blocks"] * bits // 8) + n["segments"]


def _header_len(data):
    """SOI up to the end of the scan header, by walking the marker segments."""
    at = 2
    while True:
        assert data[at] == 0xFF
        end = at + 2 + int.from_bytes(data[at + 2:at + 4], "big")
        if data[at + 1] == 0xDA:
            return end
        at = end


def test_bound_of_optimised_items(L):
    """1665 bits a block, the standard header's length; at least every pinned optimised file, whose header is no longer."""
    pins = R.pins()[0]
    for c in _everything():
        header = jpeggpu_amd.encode_header(*_args(c))
        bound = jpeggpu_amd.encode_bound(*_args(c), optimize=True)
        assert bound == len(header) + 2 * _stream_bound(c, MAX_BLOCK_BITS_OPTIMIZED) + 2 * (K.counts(c)["segments"] - 1) + 2, c["name"]
        assert bound >= pins[c["name"]]["length"], c["name"]
        data = pins[c["name"]]["data"]
        if data is not None:
            assert _header_len(data) <= len(header), c["name"]


def _plan_total(items, flags):
    """jg_encode_plan.cpp's make_plan restated for items without optimised tables: every part starts on a multiple of 256."""
    assert not any(flags)
    off = 0

    def take(n):
        nonlocal off
        off = -(-(off + n) // 256) * 256

    take(TABLES_BYTES)
    take(ITEM_BYTES * (len(items) + 1))
    take(sum(-(-len(jpeggpu_amd.encode_header(*_args(c))) // 16) * 16 for c in items))
    tiles, chunks = K.starts(items, "tiles")[-1], K.starts(items, "chunks")[-1]
    take(tiles * K.TILE_BLOCKS * 4)
    take(tiles * 12)
    take(tiles * 12)
    take(chunks * 12)
    take(chunks * 12)
    for c in items:
        n = K.counts(c)
        take(n["blocks"] * 128)
        take(n["chunks"] * K.CHUNK_BYTES)
        take(n["chunks"] * K.CHUNK_BYTES // 8)
    return off + 256


def test_items_without_the_flag_plan_as_before(L):
    """Bound and scratch size of calls without the flag, to the byte: the restated counts of encode_cases.counts."""
    for c in CASES:
        header = jpeggpu_amd.encode_header(*_args(c))
        n = K.counts(c)
        assert jpeggpu_amd.encode_bound(*_args(c)) == len(header) + 2 * n["stream_bound"] + 2 * (n["segments"] - 1) + 2, c["name"]
    calls = [[c] for c in CASES[::9]] + [CASES[:40], CASES[40:47], K.many_call()[:300], K.grid_call()["items"]]
    for items in calls:
        arr = (EncodeItem * len(items))(*[encode_item(*_args(c)) for c in items])
        assert L.jpeggpu_ext_encode_scratch_size(arr, len(items)) == _plan_total(items, [0] * len(items)), items[0]["name"]


def test_scratch_size_with_the_flag_is_at_least_the_size_without(L):
    for items in ([c] for c in _everything()[::5]):
        plain = (EncodeItem * 1)(encode_item(*_args(items[0])))
        opt = (EncodeItem * 1)(encode_item(*_args(items[0]), optimize=True))
        a, b = L.jpeggpu_ext_encode_scratch_size(plain, 1), L.jpeggpu_ext_encode_scratch_size(opt, 1)
        # on top: five bits a block of stream, perhaps one chunk more for them with its start bits, and the item's tables and state
        assert 0 < a <= b < a + 20480 + K.counts(items[0])["blocks"], items[0]["name"]
    items = CASES[:16]
    mixed = (EncodeItem * 16)(*[encode_item(*_args(c), optimize=i % 2 == 0) for i, c in enumerate(items)])
    plain = (EncodeItem * 16)(*[encode_item(*_args(c)) for c in items])
    assert L.jpeggpu_ext_encode_scratch_size(mixed, 16) > L.jpeggpu_ext_encode_scratch_size(plain, 16)


def test_tables_from_counts_refuses_null_arguments(L):
    f = L.jpeggpu_ext_encode_tables_from_counts
    assert f(None, 1, 256, 256, None) == Status.INVALID_ARGUMENT
    assert f(256, 0, 256, 256, None) == Status.INVALID_ARGUMENT
    assert f(256, 1, None, 256, None) == Status.INVALID_ARGUMENT
    assert f(256, 1, 256, None, None) == Status.INVALID_ARGUMENT
