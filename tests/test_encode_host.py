"""The encoder's host half (jpeggpu_ext_encode_header, _bound, _scratch_size and the argument checks of _batch) against
Pillow's pinned files and the restatement. No GPU needed."""
import ctypes as C

import pytest

import jpeggpu_amd
from jpeggpu_amd import Status
from jpeggpu_amd import build as jbuild
from jpeggpu_amd.api import EncodeItem, encode_item
from tests import encode_cases as K
from tests import encode_ref as E

CASES = K.cases()


@pytest.fixture(scope="module")
def L():
    jbuild.build()
    return jpeggpu_amd.lib()


def _args(c):
    return c["w"], c["h"], 1 if c["grey"] else 3, c["quality"], c["subsampling"], c["restart_interval"]


def test_header_equals_every_pinned_file(L):
    """Every case: all qualities on one geometry (qsweep_*), every geometry at quality 75 (geometry_*), and the rest."""
    pins = K.pins()[0]
    seen_q, seen_geometry = set(), 0
    for c in CASES:
        header = jpeggpu_amd.encode_header(*_args(c))
        hs, vs = E.SUBSAMPLINGS[c["subsampling"]]
        assert header == E.header(c["w"], c["h"], 1 if c["grey"] else 3, hs, vs, c["quality"], c["restart_interval"]), c["name"]
        assert header[-3:] == b"\x00\x3f\x00" and header[:2] == b"\xff\xd8"
        data = pins[c["name"]]["data"]
        if data is not None:  # (a file pinned by hash is the restatement's, tests/test_encode_ref.py: its header was compared above)
            assert data[:len(header)] == header, c["name"]
            seen_q.add(c["quality"]) if c["name"].startswith("qsweep") else None
            seen_geometry += c["name"].startswith("geometry")
    assert seen_q == set(range(1, 101)) and seen_geometry == 2 * len(K.SIZES)


def test_header_length_query_and_room(L):
    it = encode_item(53, 37, 3, 75, "4:2:0", 3)
    size = C.c_size_t(0)
    assert L.jpeggpu_ext_encode_header(C.byref(it), None, C.byref(size)) == Status.SUCCESS
    n = size.value
    assert n == len(jpeggpu_amd.encode_header(53, 37, 3, 75, "4:2:0", 3))
    buf = C.create_string_buffer(n + 8)
    buf.raw = b"\xa5" * (n + 8)
    size = C.c_size_t(n - 1)
    assert L.jpeggpu_ext_encode_header(C.byref(it), buf, C.byref(size)) == Status.INVALID_ARGUMENT and size.value == n
    assert buf.raw == b"\xa5" * (n + 8), "nothing is written into a buffer that is too small"
    size = C.c_size_t(n)
    assert L.jpeggpu_ext_encode_header(C.byref(it), buf, C.byref(size)) == Status.SUCCESS
    assert buf.raw[n:] == b"\xa5" * 8


def test_bound_covers_every_pinned_file(L):
    pins = K.pins()[0]
    for c in CASES:
        assert jpeggpu_amd.encode_bound(*_args(c)) >= pins[c["name"]]["length"], c["name"]


def test_header_and_bound_of_every_new_case(L):
    """The sweep, the edge cases and the items of the big calls (tests/golden/encode_sweep_pins.npz holds lengths and hashes
    only): the header is the restatement's, the bound covers the pinned length, and the bound is what encode_cases.counts
    restates -- the tile and chunk counts the structure tests of tests/test_encode_ref.py rest on."""
    pins = K.sweep_pins()[0]
    for c in K.new_cases():
        header = jpeggpu_amd.encode_header(*_args(c))
        hs, vs = E.SUBSAMPLINGS[c["subsampling"]]
        assert header == E.header(c["w"], c["h"], 1 if c["grey"] else 3, hs, vs, c["quality"], c["restart_interval"]), c["name"]
        bound = jpeggpu_amd.encode_bound(*_args(c))
        assert bound >= pins[c["name"]]["length"], c["name"]
        n = K.counts(c)
        assert bound == len(header) + 2 * n["stream_bound"] + 2 * (n["segments"] - 1) + 2, c["name"]


def test_scratch_size_follows_the_restated_counts(L):
    """jpeggpu_ext_encode_scratch_size of the big calls holds at least what the restated tiles and chunks need: the
    coefficients, the stream and the start bits of every item, and the per-tile and per-chunk arrays."""
    for items in (K.many_call(), K.grid_call()["items"]):
        arr = (EncodeItem * len(items))(*[encode_item(*_args(c)) for c in items])
        need = L.jpeggpu_ext_encode_scratch_size(arr, len(items))
        tiles, chunks = K.starts(items, "tiles")[-1], K.starts(items, "chunks")[-1]
        least = sum(K.counts(c)["blocks"] * 128 + K.counts(c)["chunks"] * (K.CHUNK_BYTES + K.CHUNK_BYTES // 8) for c in items)
        least += tiles * (K.TILE_BLOCKS * 4 + 24) + chunks * 24
        assert least < need < least + 2048 * len(items) + 8192, "and no more than the descriptors, headers and alignment on top"


@pytest.mark.parametrize("w,h,ch,sub,ri", [(1, 1, 1, "4:4:4", 0), (8, 8, 3, "4:2:0", 0), (53, 37, 3, "4:2:0", 1), (53, 37, 3, "4:2:2", 3), (19, 3, 3, "4:4:4", 11),
                                            (40, 24, 1, "4:2:0", 1), (200, 64, 3, "4:2:0", 0)])
def test_bound_covers_the_worst_stream(L, w, h, ch, sub, ri):
    """Crafted coefficients, every one at the longest code of its table: the stream no image can exceed, up to stuffing --
    and the bound also pays for a stuffed byte behind every byte."""
    hs, vs = E.SUBSAMPLINGS[sub]
    worst = E.worst_case_stream(w, h, ch, hs, vs, ri)
    bound = jpeggpu_amd.encode_bound(w, h, ch, 75, sub, ri)
    header = len(jpeggpu_amd.encode_header(w, h, ch, 75, sub, ri))
    assert bound >= len(worst)
    assert bound >= header + 2 * (len(worst) - header - 2) + 2 - 2 * worst.count(b"\xff\x00"), "room for every data byte to be stuffed"
    _, _, mx, my, per_mcu = E.geometry(w, h, ch, hs, vs)
    assert bound <= header + 2 * (mx * my * per_mcu * 208 + 2 * mx * my) + 4, "and not absurdly more: 1660 bits a block"


BAD = [dict(quality=0), dict(quality=101), dict(channels=2), dict(channels=4), dict(channels=0), dict(subsampling=3), dict(subsampling=-1), dict(width=0),
       dict(width=65536), dict(height=0), dict(height=65536), dict(restart_interval=-1), dict(restart_interval=65536)]


@pytest.mark.parametrize("bad", BAD, ids=[next(iter(b)) + "=" + str(next(iter(b.values()))) for b in BAD])
def test_bad_items_are_refused_everywhere(L, bad):
    it = encode_item(16, 16)
    it.data, it.out, it.capacity = 256, 512, 64  # never dereferenced: the checks come first
    it.row_pitch, it.pixel_stride, it.channel_stride = 48, 3, 1
    setattr(it, next(iter(bad)), next(iter(bad.values())))
    size = C.c_size_t(0)
    assert L.jpeggpu_ext_encode_header(C.byref(it), None, C.byref(size)) == Status.INVALID_ARGUMENT
    assert L.jpeggpu_ext_encode_bound(C.byref(it)) == 0
    items = (EncodeItem * 2)(encode_item(8, 8), it)
    assert L.jpeggpu_ext_encode_scratch_size(items, 2) == 0
    items[0].data, items[0].out, items[0].capacity = 256, 512, 64
    assert L.jpeggpu_ext_encode_batch(items, 2, 256, 1 << 30, 256, 256, None) == Status.INVALID_ARGUMENT


def test_null_pointers_and_counts_are_refused(L):
    ok = encode_item(16, 16)
    ok.data, ok.out, ok.capacity = 256, 512, 64
    items = (EncodeItem * 1)(ok)
    need = L.jpeggpu_ext_encode_scratch_size(items, 1)
    assert need > 0 and L.jpeggpu_ext_encode_scratch_size(items, 0) == 0 and L.jpeggpu_ext_encode_scratch_size(None, 1) == 0
    call = lambda it=items, n=1, scratch=256, size=need, sizes=256, status=256: L.jpeggpu_ext_encode_batch(it, n, scratch, size, sizes, status, None)  # noqa: E731
    assert call(it=None) == Status.INVALID_ARGUMENT
    assert call(n=0) == Status.INVALID_ARGUMENT
    assert call(scratch=None) == Status.INVALID_ARGUMENT
    assert call(sizes=None) == Status.INVALID_ARGUMENT
    assert call(status=None) == Status.INVALID_ARGUMENT
    assert call(size=need - 257) == Status.INVALID_ARGUMENT, "scratch too small"
    for field in ("data", "out"):
        bad = encode_item(16, 16)
        bad.data, bad.out, bad.capacity = 256, 512, 64
        setattr(bad, field, None)
        assert call(it=(EncodeItem * 1)(bad)) == Status.INVALID_ARGUMENT, field
    assert L.jpeggpu_ext_encode_header(None, None, C.byref(C.c_size_t(0))) == Status.INVALID_ARGUMENT
    assert L.jpeggpu_ext_encode_header(C.byref(ok), None, None) == Status.INVALID_ARGUMENT
    assert L.jpeggpu_ext_encode_bound(None) == 0


def test_scratch_size_grows_with_the_call(L):
    a, b = encode_item(640, 427), encode_item(33, 17, 1)
    one = L.jpeggpu_ext_encode_scratch_size((EncodeItem * 1)(a), 1)
    two = L.jpeggpu_ext_encode_scratch_size((EncodeItem * 2)(a, b), 2)
    assert 0 < one < two
    huge = encode_item(65535, 65535, 1)  # beyond the kernels' 32-bit bit offsets: refused, not wrapped
    assert L.jpeggpu_ext_encode_scratch_size((EncodeItem * 1)(huge), 1) == 0
    assert L.jpeggpu_ext_encode_bound(C.byref(huge)) > 2 ** 32, "the bound itself is host arithmetic in 64 bits"
