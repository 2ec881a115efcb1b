"""The host half of the lossless transcode: jpeggpu_ext_transcode_header against the headers of Pillow's pinned files,
jpeggpu_ext_transcode_bound against their sizes, and everything the calls refuse before anything is enqueued. No GPU needed."""
import ctypes as C

import pytest

import jpeggpu_amd
from jpeggpu_amd import Status, api
from jpeggpu_amd import build as jbuild
from tests import cases, color_ref
from tests import transcode_cases as T

CASES = T.cases()


@pytest.fixture(scope="module")
def L():
    jbuild.build()
    return jpeggpu_amd.lib()


class Source:
    """A parsed file and a transcode item for it (no device memory: the host calls do not look at d_tmp)."""

    def __init__(self, data, setup=None, **options):
        self.dec = jpeggpu_amd.Decoder()
        self.dec.set_progressive(True)
        if setup:
            setup(self.dec)
        self.info = self.dec.parse_header(data)
        it = self.item = api.TranscodeItem()
        it.decoder = self.dec._h
        it.optimize, it.progressive = int(options.get("optimize", 0)), int(options.get("progressive", 0))
        it.restart_interval = options.get("restart_interval", -1)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.dec.cleanup()

    def header(self, L):
        size = C.c_size_t(1024)
        buf = C.create_string_buffer(1024)
        st = L.jpeggpu_ext_transcode_header(C.byref(self.item), buf, C.byref(size))
        return st, buf.raw[:size.value]

    def status(self, L):
        """What every call makes of the item: the header's status, and that the bound, the scratch size and the batch call agree."""
        st, _ = self.header(L)
        arr = (api.TranscodeItem * 1)(self.item)
        if st not in (Status.SUCCESS, Status.NOT_SUPPORTED) or (st == Status.NOT_SUPPORTED and not (self.item.optimize or self.item.progressive)):
            assert L.jpeggpu_ext_transcode_bound(C.byref(self.item)) == 0
            assert L.jpeggpu_ext_transcode_scratch_size(arr, 1) == 0
            arr[0].d_tmp = 256  # (refused before a pointer is followed or anything is enqueued)
            assert L.jpeggpu_ext_transcode_batch(arr, 1, 256, 1 << 30, 256, 256, None) == st
        return st


def file_header(data):
    """SOI up to the end of the first scan header."""
    sos = data.index(b"\xff\xda")
    return data[:sos + 2 + (data[sos + 2] << 8 | data[sos + 3])]


def test_struct_layout():
    assert C.sizeof(api.TranscodeItem) == 48
    assert api.TranscodeItem.d_tmp.offset == 8 and api.TranscodeItem.restart_interval.offset == 24 and api.TranscodeItem.out.offset == 32


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_header_and_bound_against_the_pins(L, case):
    files = T.pins()[0][case["name"]]
    for kind in "ABC":  # whatever the source, the plain header is A's: the source's tables, its sampling byte, its restart interval
        with Source(files[kind]) as s:
            st, head = s.header(L)
            assert st == Status.SUCCESS and head == file_header(files["A"]), kind
            assert L.jpeggpu_ext_transcode_bound(C.byref(s.item)) >= len(files["A"])
            size = C.c_size_t(0)
            assert L.jpeggpu_ext_transcode_header(C.byref(s.item), None, C.byref(size)) == Status.SUCCESS and size.value == len(head)
            small = C.c_size_t(len(head) - 1)
            assert L.jpeggpu_ext_transcode_header(C.byref(s.item), C.create_string_buffer(1024), C.byref(small)) == Status.INVALID_ARGUMENT
        for options, want in ((dict(optimize=True), "B"), (dict(progressive=True), "C")):
            with Source(files[kind], **options) as s:
                st, _ = s.header(L)
                assert st == Status.NOT_SUPPORTED  # as jpeggpu_ext_encode_header: these headers hold tables made from the coefficients
                assert L.jpeggpu_ext_transcode_bound(C.byref(s.item)) >= len(files[want])
                assert L.jpeggpu_ext_transcode_scratch_size((api.TranscodeItem * 1)(s.item), 1) > 0
    if case["restart_to"] is not None:
        with Source(files["A"], restart_interval=case["restart_to"]) as s:
            st, head = s.header(L)
            assert st == Status.SUCCESS and head == file_header(files["R"])
            assert L.jpeggpu_ext_transcode_bound(C.byref(s.item)) >= len(files["R"])


def _colour_pin():
    return T.pins()[0]["17x13_420_q75_r0_noise"]["A"]


def test_unsupported_sources(L):
    sweep, matrix, colour = cases.sampling_sweep(), cases.matrix(), color_ref.cases()
    refused = {
        "4:4:0": sweep["y1x2_a"], "4:1:1": sweep["y4x1_a"], "4:1:1 in its own scans": sweep["y4x2_ni"], "chroma 2x1": sweep["y2x2_c2x1_a"],
        "CMYK": next(d for d, m in colour.values() if m == color_ref.CMYK),
        "YCCK": next(d for d, m in colour.values() if m == color_ref.YCCK), "RGB-coded": next(d for d, m in colour.values() if m == color_ref.RGB),
        "two components": matrix["two_comp"], "four components": matrix["four_comp_444"], "Pq = 1": matrix["q16_tables"],
    }
    for name, data in refused.items():
        for options in (dict(), dict(optimize=True), dict(progressive=True)):
            with Source(data, **options) as s:
                assert s.status(L) == Status.NOT_SUPPORTED, (name, options)
    # the control: the same kinds of file in a layout the writer has
    for name in ("ss_1x1", "ss_2x1", "ss_2x2", "gray", "gray_hdr_2x2", "ni_420", "dri_7"):
        with Source(matrix[name]) as s:
            assert s.status(L) == Status.SUCCESS, name


def test_cb_and_cr_on_different_tables(L):
    data = bytearray(_colour_pin())
    segs = color_ref.segments_of(bytes(data))
    sof = next(off for m, off, n in segs if m == 0xC0)
    dqt = next(off for m, off, n in segs if m == 0xDB)
    third = bytes(data[dqt - 2:dqt + 67])  # a copy of table 0 as table 2, and Cr on it
    third = third[:4] + b"\x02" + third[5:]
    data[sof + 8 + 3 * 2 + 2] = 2
    data = bytes(data[:dqt - 2]) + third + bytes(data[dqt - 2:])
    with Source(data) as s:
        assert s.info.num_components == 3
        assert s.status(L) == Status.NOT_SUPPORTED


def test_decoders_with_a_window_a_scale_or_a_shard(L):
    big = T.pins()[0]["136x120_420_q75_r0_smooth"]
    with Source(big["A"], setup=lambda d: d.set_crop(16, 16, 64, 48)) as s:
        assert s.status(L) == Status.NOT_SUPPORTED
    with Source(big["A"], setup=lambda d: d.set_scale(2)) as s:
        assert s.status(L) == Status.NOT_SUPPORTED
    with Source(cases.matrix()["dri_row"], setup=lambda d: d.set_segment_shard(0, 2)) as s:
        assert s.status(L) == Status.NOT_SUPPORTED
    with Source(big["A"]) as s:
        assert s.status(L) == Status.SUCCESS


def test_large_sources_on_the_host(L):
    """What tests/test_gpu_transcode_scale.py takes the large sources for: baseline sources whose symbol stream has several
    tiles of 64 subsequences (jg_defs.h: kSymTileSubseq), whatever the batch hint; bounds that cover the expected files."""
    files = T.large()
    for name, tiles in (("photo_twin", 8), ("photo_rst_twin", 2), ("camera", 64)):
        for hint in (1, 7, 12):
            with Source(files[name], setup=lambda d: d.set_batch_hint(hint)) as s:
                lay = s.dec.layout()
                assert lay.num_scans == 1 and lay.scans[0].num_subsequences > 64 * tiles, (name, hint, lay.scans[0].num_subsequences)
                assert lay.scans[0].num_data_units == T.blocks_of(s.info.sizes_x[0], s.info.sizes_y[0], "4:2:0")[0]
    pins = T.large_pins()[0]
    for source, label, options, expected in T.LARGE_PAIRS:
        with Source(files[source], **options) as s:
            assert s.status(L) == (Status.NOT_SUPPORTED if options.get("optimize") or options.get("progressive") else Status.SUCCESS)
            size = len(files[expected]) if expected is not None else pins["%s/%s" % (source, label)]["size"]
            assert L.jpeggpu_ext_transcode_bound(C.byref(s.item)) >= size, (source, label)


def test_crafted_and_limit_sources_on_the_host(L):
    """The four-component file is refused here, before anything is enqueued; a source at or past a coding limit is not: what
    its coefficients are is known on the device only."""
    crafted = T.crafted_progressive()
    for name, (prog, _) in crafted.items():
        with Source(prog) as s:
            assert s.status(L) == (Status.NOT_SUPPORTED if name == T.CRAFTED_REFUSED else Status.SUCCESS), name
    for src in T.limit_sources():
        for r in src["codable"]:
            with Source(src["data"], restart_interval=r) as s:
                assert s.status(L) == Status.SUCCESS, src["name"]


def test_invalid_arguments(L):
    a = _colour_pin()
    for r in (-2, 65536, 1 << 20):
        with Source(a, restart_interval=r) as s:
            assert s.status(L) == Status.INVALID_ARGUMENT
    for r in (-1, 0, 65535):
        with Source(a, restart_interval=r) as s:
            assert s.status(L) == Status.SUCCESS
    for field in ("optimize", "progressive"):
        with Source(a) as s:
            setattr(s.item, field, 2)
            assert s.status(L) == Status.INVALID_ARGUMENT
    with Source(a) as s:  # a NULL out with a capacity
        s.item.capacity = 16
        assert s.status(L) == Status.INVALID_ARGUMENT
    dec = jpeggpu_amd.Decoder()  # a decoder that has parsed nothing
    it = api.TranscodeItem()
    it.decoder, it.restart_interval = dec._h, -1
    size = C.c_size_t(0)
    assert L.jpeggpu_ext_transcode_header(C.byref(it), None, C.byref(size)) == Status.INVALID_ARGUMENT
    dec.cleanup()
    it.decoder = None
    assert L.jpeggpu_ext_transcode_header(C.byref(it), None, C.byref(size)) == Status.INVALID_ARGUMENT
    assert L.jpeggpu_ext_transcode_bound(None) == 0
    assert L.jpeggpu_ext_transcode_scratch_size(None, 1) == 0
    with Source(a) as s:
        arr = (api.TranscodeItem * 1)(s.item)
        arr[0].d_tmp = 256
        assert L.jpeggpu_ext_transcode_scratch_size(arr, 0) == 0
        for args in ((arr, 0, 256, 1 << 30, 256, 256), (arr, 1, None, 1 << 30, 256, 256), (arr, 1, 256, 1 << 30, None, 256), (arr, 1, 256, 1 << 30, 256, None),
                     (None, 1, 256, 1 << 30, 256, 256), (arr, 1, 256, 16, 256, 256)):
            assert L.jpeggpu_ext_transcode_batch(*args, None) == Status.INVALID_ARGUMENT, args[1:]
        arr[0].d_tmp = 260  # not 256-aligned
        assert L.jpeggpu_ext_transcode_batch(arr, 1, 256, 1 << 30, 256, 256, None) == Status.INVALID_ARGUMENT
        arr[0].d_tmp = None
        assert L.jpeggpu_ext_transcode_batch(arr, 1, 256, 1 << 30, 256, 256, None) == Status.INVALID_ARGUMENT


def test_symbols_an_older_library_lacks(monkeypatch):
    class Older:
        pass

    monkeypatch.setattr(api, "lib", lambda: Older())
    batch = object.__new__(jpeggpu_amd.Batch)
    batch._h = None
    with pytest.raises(RuntimeError, match="jpeggpu_ext_batch_set_coefficients_only"):
        batch.set_coefficients_only(True)
    with pytest.raises(RuntimeError, match="jpeggpu_ext_transcode_batch"):
        jpeggpu_amd.transcode_jpeg([_colour_pin()])


def test_an_item_at_the_encoders_size_limits(L):
    """A frame header of 65535 x 65535 over a grey pin's scan (the host calls never look at the data): the item's stream
    bound passes 2^32 bits, which the encoder's plan refuses. The bound itself is the encoder's for that geometry."""
    data = bytearray(T.pins()[0]["136x120_grey_q75_r0_smooth"]["A"])  # (no restart markers that would have to match the geometry)
    sof = next(off for m, off, n in color_ref.segments_of(bytes(data)) if m == 0xC0)
    data[sof + 3:sof + 7] = b"\xff\xff\xff\xff"
    data = bytes(data)
    for options in (dict(), dict(optimize=True), dict(progressive=True)):
        with Source(data, **options) as s:
            arr = (api.TranscodeItem * 1)(s.item)
            assert L.jpeggpu_ext_transcode_scratch_size(arr, 1) == 0
            arr[0].d_tmp = 256
            assert L.jpeggpu_ext_transcode_batch(arr, 1, 256, 1 << 40, 256, 256, None) == Status.NOT_SUPPORTED
            same = api.encode_item(65535, 65535, 1, 75, "4:2:0", 0, **options)  # (a grey frame: the subsampling is only the sampling byte)
            assert L.jpeggpu_ext_transcode_bound(C.byref(s.item)) == L.jpeggpu_ext_encode_bound(C.byref(same)) > 0
            assert L.jpeggpu_ext_encode_scratch_size((api.EncodeItem * 1)(same), 1) == 0
