"""The host half of DCT-domain access (jpeggpu_ext_get_coefficient_info, the jpeggpu_ext_read_coefficients_ and
jpeggpu_ext_write_coefficients_ calls): the structs against their ctypes mirrors, the real grids, factors and tables of
every layout, jpeggpu_ext_write_coefficients_header and _bound against the reference's files, every refusal with its status
-- all made before anything is enqueued --, and scratch sizes that never shrink with n. No GPU needed."""
import ctypes as C

import numpy as np
import pytest

import jpeggpu_amd
from jpeggpu_amd import ColorSpace, Status, api
from jpeggpu_amd import build as jbuild
from tests import coefficients_ref as K
from tools import jpegsynth

FAKE = 4096  # a device address that is never followed: every call here is refused first, or is host only


@pytest.fixture(scope="module")
def L():
    jbuild.build()
    lib = jpeggpu_amd.lib()
    assert hasattr(lib, "jpeggpu_ext_read_coefficients_batch"), "the library lacks jpeggpu_ext_read_coefficients_batch"
    assert hasattr(lib, "jpeggpu_ext_write_coefficients_batch"), "the library lacks jpeggpu_ext_write_coefficients_batch"
    return lib


def parsed(data, setup=None):
    dec = jpeggpu_amd.Decoder()
    dec.set_progressive(True)
    if setup:
        setup(dec)
    dec.parse_header(data)
    return dec


def item_of(co, **options):
    """The write item of a reference Coef, its tensors at a fake aligned address."""
    it = api.CoefficientItem()
    it.width, it.height, it.components, it.color_space = co.w, co.h, len(co.coef), co.color
    for c in range(len(co.coef)):
        it.h[c], it.v[c] = co.sampling[c]
        it.coef[c] = FAKE
        for k in range(64):
            it.qtable[c][k] = int(co.qtables[c][k])
    it.optimize, it.progressive, it.restart_interval = int(options.get("optimize", 0)), int(options.get("progressive", 0)), options.get("restart_interval", 0)
    return it


def header(L, it):
    size = C.c_size_t(2048)
    buf = C.create_string_buffer(2048)
    st = L.jpeggpu_ext_write_coefficients_header(C.byref(it), buf, C.byref(size))
    return st, buf.raw[:size.value] if st == 0 else size.value


def test_struct_sizes(L):
    """The sizes jg_coefficients.cpp asserts of the C structs."""
    assert C.sizeof(api.CoefficientInfo) == 612 and api.CoefficientInfo.qtable.offset == 100
    assert C.sizeof(api.CoefficientSpec) == 8 and C.sizeof(api.CoefficientReadItem) == 48
    assert C.sizeof(api.CoefficientItem) == 624 and api.CoefficientItem.coef.offset == 560 and api.CoefficientItem.out.offset == 608


@pytest.mark.parametrize("name", ["grey_1x1", "17x9_420", "17x9_422", "17x9_444", "17x9_440", "17x9_411", "cmyk", "q16", "two_comp", "prog_of_ni_420"])
def test_coefficient_info(L, name):
    data = K.sources()[name]
    ref = K.read(data)
    ci = parsed(data).coefficient_info()
    n = len(ref.coef)
    assert (ci.width, ci.height, ci.num_components, ci.color_space, ci.progressive) == (ref.w, ref.h, n, ref.color, int(ref.progressive))
    assert [(ci.blocks_y[c], ci.blocks_x[c]) for c in range(n)] == [g.shape[:2] for g in ref.coef]
    assert [(ci.h[c], ci.v[c]) for c in range(n)] == ref.sampling
    for c in range(n):
        assert np.array_equal(np.ctypeslib.as_array(ci.qtable[c]), ref.qtables[c])
        assert ci.table16[c] == int(ref.qtables[c].max() > 255)
    for c in range(n, 4):
        assert (ci.blocks_x[c], ci.blocks_y[c], ci.h[c], ci.table16[c]) == (0, 0, 0, 0) and not any(ci.qtable[c])


def test_info_of_the_named_layouts(L):
    """The numbers themselves, not only their agreement with the reference: libjpeg's width_in_blocks x height_in_blocks."""
    S = K.sources()
    grid = lambda name: [(ci.blocks_x[c], ci.blocks_y[c]) for ci in [parsed(S[name]).coefficient_info()] for c in range(ci.num_components)]
    assert grid("grey_1x1") == [(1, 1)]
    assert grid("17x9_420") == [(3, 2), (2, 1), (2, 1)] and grid("17x9_422") == [(3, 2), (2, 2), (2, 2)]
    assert grid("17x9_444") == [(3, 2)] * 3 and grid("17x9_440") == [(3, 2), (3, 1), (3, 1)] and grid("17x9_411") == [(3, 2), (1, 2), (1, 2)]
    assert grid("cmyk") == [(5, 3)] * 4
    ci = parsed(S["q16"]).coefficient_info()
    assert ci.table16[0] == 1 and max(ci.qtable[0]) > 255
    assert parsed(S["cmyk"]).coefficient_info().color_space == ColorSpace.CMYK
    assert jpeggpu_amd.coefficient_grid(17, 9, [(2, 2), (1, 1), (1, 1)]) == [(2, 3), (1, 2), (1, 2)]
    assert jpeggpu_amd.coefficient_grid(17, 9, [(2, 2)]) == [(2, 3)]  # one component: its factors change nothing
    dec = jpeggpu_amd.Decoder()
    assert L.jpeggpu_ext_get_coefficient_info(dec._h, C.byref(api.CoefficientInfo())) == Status.INVALID_ARGUMENT  # not parsed
    assert L.jpeggpu_ext_get_coefficient_info(None, C.byref(api.CoefficientInfo())) == Status.INVALID_ARGUMENT


@pytest.mark.parametrize("name", sorted(K.sources()))
def test_header_and_bound_against_the_reference(L, name):
    co = K.read(K.sources()[name])
    for options in (dict(), dict(restart_interval=3), dict(optimize=True), dict(progressive=True, restart_interval=2)):
        want = K.write(co, **options)
        it = item_of(co, **options)
        st, head = header(L, it)
        if options.get("optimize") or options.get("progressive"):
            assert st == Status.NOT_SUPPORTED and head > 100  # its tables depend on the coefficients: only a size is reported
        else:
            assert st == Status.SUCCESS and len(head) > 100 and want.startswith(head) and b"\xff\xda" in head[-16:]
        assert L.jpeggpu_ext_write_coefficients_bound(C.byref(it)) >= len(want), options


def test_pillows_headers(L):
    """The encoder's own layouts get the encoder's header: the first bytes of Pillow's file."""
    for name, f in K.pins()[0].items():
        st, head = header(L, item_of(K.read(f["A"])))
        assert st == Status.SUCCESS and f["A"][:len(head)] == head, name
        for kind, options in K.KINDS.items():
            assert L.jpeggpu_ext_write_coefficients_bound(C.byref(item_of(K.read(f["A"]), **options))) >= len(f[kind])


def refused(L, it, want):
    """Every call makes the same of the item, before a pointer is followed or anything is enqueued."""
    size = C.c_size_t(0)
    assert L.jpeggpu_ext_write_coefficients_header(C.byref(it), None, C.byref(size)) == want
    assert L.jpeggpu_ext_write_coefficients_bound(C.byref(it)) == 0
    arr = (api.CoefficientItem * 1)(it)
    assert L.jpeggpu_ext_write_coefficients_scratch_size(arr, 1) == 0
    assert L.jpeggpu_ext_write_coefficients_batch(arr, 1, FAKE, 1 << 30, FAKE, FAKE, None) == want


def test_write_refusals(L):
    co = K.read(K.sources()["17x9_420"])
    base = lambda: item_of(co)

    def changed(**fields):
        it = base()
        for k, v in fields.items():
            setattr(it, k, v)
        return it

    for fields in (dict(width=0), dict(width=65536), dict(height=0), dict(components=0), dict(components=5), dict(restart_interval=-1),
                   dict(restart_interval=65536), dict(optimize=2), dict(progressive=-1), dict(color_space=6), dict(color_space=-1),
                   dict(color_space=int(ColorSpace.GRAY)), dict(color_space=int(ColorSpace.CMYK)), dict(capacity=1)):
        refused(L, changed(**fields), Status.INVALID_ARGUMENT)
    for c, h, v in ((0, 0, 1), (0, 5, 1), (1, 1, 0), (2, 1, 5)):  # a factor outside 1..4
        it = base()
        it.h[c], it.v[c] = h, v
        refused(L, it, Status.INVALID_ARGUMENT)
    it = base()  # an MCU of more than 10 blocks: 2 x 2 + 2 x 2 + 2 x 2
    for c in range(3):
        it.h[c], it.v[c] = 2, 2
    refused(L, it, Status.INVALID_ARGUMENT)
    it = base()  # 3 x 3 + 1 + 1 = 11
    it.h[0], it.v[0] = 3, 3
    refused(L, it, Status.INVALID_ARGUMENT)
    it = base()
    it.qtable[1][63] = 0  # a zero table entry
    refused(L, it, Status.INVALID_ARGUMENT)
    # a tensor that is missing or misaligned is the batch call's to refuse: the host calls do not read `coef`
    for address in (0, FAKE + 2, FAKE + 8):
        it = base()
        it.coef[2] = address
        assert header(L, it)[0] == Status.SUCCESS
        arr = (api.CoefficientItem * 1)(it)
        assert L.jpeggpu_ext_write_coefficients_batch(arr, 1, FAKE, 1 << 30, FAKE, FAKE, None) == Status.INVALID_ARGUMENT
    ok = (api.CoefficientItem * 1)(base())
    assert L.jpeggpu_ext_write_coefficients_batch(ok, 0, FAKE, 1 << 30, FAKE, FAKE, None) == Status.INVALID_ARGUMENT
    assert L.jpeggpu_ext_write_coefficients_batch(None, 1, FAKE, 1 << 30, FAKE, FAKE, None) == Status.INVALID_ARGUMENT
    assert L.jpeggpu_ext_write_coefficients_batch(ok, 1, None, 1 << 30, FAKE, FAKE, None) == Status.INVALID_ARGUMENT
    assert L.jpeggpu_ext_write_coefficients_batch(ok, 1, FAKE, 1 << 30, None, FAKE, None) == Status.INVALID_ARGUMENT
    assert L.jpeggpu_ext_write_coefficients_batch(ok, 1, FAKE, 16, FAKE, FAKE, None) == Status.INVALID_ARGUMENT  # a scratch too small
    assert L.jpeggpu_ext_write_coefficients_header(None, None, C.byref(C.c_size_t(0))) == Status.INVALID_ARGUMENT


def test_python_refuses_tensors_that_do_not_fit():
    """Shape, dtype and contiguity are the wrapper's to check (the C item has only a pointer): on CPU tensors, before the
    library is asked anything."""
    torch = pytest.importorskip("torch")
    co = K.read(K.sources()["17x9_420"])
    one = jpeggpu_amd.Coefficients([torch.zeros(g.shape[:2] + (8, 8), dtype=torch.int16) for g in co.coef], [q.reshape(8, 8) for q in co.qtables], co.w, co.h,
                                   co.sampling, co.color)
    with pytest.raises(jpeggpu_amd.JpegGpuError) as e:  # not on the device
        jpeggpu_amd.write_coefficients([one])
    assert e.value.status == Status.INVALID_ARGUMENT
    with pytest.raises(ValueError):
        jpeggpu_amd.write_coefficients([jpeggpu_amd.Coefficients(one.coefficients[:2], one.qtables, co.w, co.h, co.sampling, co.color)])


def read_item(dec, tmp=FAKE, dst=FAKE):
    it = api.CoefficientReadItem()
    it.decoder, it.d_tmp = dec._h, tmp
    for c in range(4):
        it.dst[c] = dst
    return (api.CoefficientReadItem * 1)(it)


def read_status(L, items, n=1, type_=0, dequantize=0, scratch=FAKE, size=1 << 20):
    spec = api.CoefficientSpec(type_, dequantize)
    return L.jpeggpu_ext_read_coefficients_batch(items, n, C.byref(spec), scratch, size, None)


def test_read_refusals(L):
    S = K.sources()
    dec = parsed(S["17x9_420"])
    ok = read_item(dec)
    assert read_status(L, ok, dequantize=1) == Status.INVALID_ARGUMENT  # dequantised int16: a 16-bit table overflows it
    assert read_status(L, ok, type_=3) == Status.INVALID_ARGUMENT and read_status(L, ok, type_=-1) == Status.INVALID_ARGUMENT
    assert read_status(L, ok, type_=1, dequantize=2) == Status.INVALID_ARGUMENT
    assert read_status(L, ok, n=0) == Status.INVALID_ARGUMENT and read_status(L, ok, n=65536) == Status.INVALID_ARGUMENT
    assert read_status(L, None) == Status.INVALID_ARGUMENT and read_status(L, ok, scratch=None) == Status.INVALID_ARGUMENT
    assert L.jpeggpu_ext_read_coefficients_batch(ok, 1, None, FAKE, 1 << 20, None) == Status.INVALID_ARGUMENT
    assert read_status(L, ok, size=64) == Status.INVALID_ARGUMENT  # a scratch too small
    assert read_status(L, read_item(dec, tmp=0)) == Status.INVALID_ARGUMENT
    assert read_status(L, read_item(dec, tmp=FAKE + 128)) == Status.INVALID_ARGUMENT  # d_tmp is aligned to 256 bytes
    assert read_status(L, read_item(dec, dst=0)) == Status.INVALID_ARGUMENT
    assert read_status(L, read_item(dec, dst=FAKE + 8), type_=1) == Status.INVALID_ARGUMENT  # a tensor is aligned to 16 bytes
    assert read_status(L, read_item(jpeggpu_amd.Decoder())) == Status.INVALID_ARGUMENT  # not parsed
    none = read_item(dec)
    none[0].decoder = None
    assert read_status(L, none) == Status.INVALID_ARGUMENT
    # what a transcode refuses too: a scale, a segment shard -- and a decode window, since windowed reading is not offered
    assert read_status(L, read_item(parsed(S["264x200_420"], lambda d: d.set_scale(2)))) == Status.NOT_SUPPORTED
    rows = jpegsynth.encode(40, 24, K.LAYOUTS["420"], restart_interval=3, seed=548)  # a restart interval of one MCU row: what a shard asks for
    assert read_status(L, read_item(parsed(rows, lambda d: d.set_segment_shard(0, 2)))) == Status.NOT_SUPPORTED
    assert read_status(L, read_item(parsed(S["264x200_420"], lambda d: d.set_crop(16, 16, 64, 64)))) == Status.NOT_SUPPORTED
    assert read_status(L, read_item(parsed(S["prog_of_ni_420"], lambda d: d.set_crop(16, 16, 32, 32)))) == Status.NOT_SUPPORTED


def test_scratch_sizes_never_shrink(L):
    assert L.jpeggpu_ext_read_coefficients_scratch_size(0) == 0 and L.jpeggpu_ext_read_coefficients_scratch_size(65536) == 0
    sizes = [L.jpeggpu_ext_read_coefficients_scratch_size(n) for n in (1, 2, 3, 64, 65535)]
    assert sizes[0] > 0 and sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    S = K.sources()
    names = ["grey_1x1", "17x9_411", "cmyk", "264x200_420", "q16"]
    kinds = [dict(), dict(optimize=True), dict(progressive=True), dict(restart_interval=1), dict(optimize=True)]
    items = (api.CoefficientItem * len(names))(*[item_of(K.read(S[n]), **k) for n, k in zip(names, kinds)])
    sizes = [L.jpeggpu_ext_write_coefficients_scratch_size(items, n) for n in range(1, len(names) + 1)]
    assert sizes[0] > 0 and sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    assert L.jpeggpu_ext_write_coefficients_scratch_size(items, 0) == 0


def test_write_is_a_transcode_of_the_same_frame(L):
    """The header and the scratch of a write item are those of the transcode item of a source with the same frame: what lies
    behind the first launch is the same call."""
    from tests.test_transcode_host import Source

    for name in ("17x9_420", "cmyk", "q16", "two_comp", "17x9_411"):
        data = K.sources()[name]
        co = K.read(data)
        for options in (dict(), dict(optimize=True), dict(progressive=True)):
            with Source(data, lambda d: d.set_transcode_frame(1), restart_interval=3, **options) as src:
                it = item_of(co, restart_interval=3, **options)
                size = C.c_size_t(2048)
                buf = C.create_string_buffer(2048)
                st = L.jpeggpu_ext_transcode_header(C.byref(src.item), buf, C.byref(size))
                assert (st, buf.raw[:size.value] if st == 0 else size.value) == header(L, it)
                assert L.jpeggpu_ext_transcode_bound(C.byref(src.item)) == L.jpeggpu_ext_write_coefficients_bound(C.byref(it))
                assert (L.jpeggpu_ext_transcode_scratch_size((api.TranscodeItem * 1)(src.item), 1)
                        == L.jpeggpu_ext_write_coefficients_scratch_size((api.CoefficientItem * 1)(it), 1))
