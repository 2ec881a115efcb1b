"""The host half of the transcode that keeps its source's frame (jpeggpu_ext_set_transcode_frame): the setter, what the mode
accepts and still refuses, jpeggpu_ext_transcode_header against the restatement's header, the bound and the scratch size
against its files, and the edge and crop rules on the iMCU of general layouts. No GPU needed."""
import ctypes as C

import pytest

import jpeggpu_amd
from jpeggpu_amd import Status, api
from jpeggpu_amd import build as jbuild
from tests import cases, color_ref
from tests import transcode_cases as T
from tests import transcode_frame_cases as K
from tests import transcode_frame_ref as F
from tests import transcode_orient_ref as X
from tests.test_transcode_host import Source as Base

ENCODER, SOURCE = 0, 1


@pytest.fixture(scope="module")
def L():
    jbuild.build()
    lib = jpeggpu_amd.lib()
    assert hasattr(lib, "jpeggpu_ext_set_transcode_frame"), "the library lacks jpeggpu_ext_set_transcode_frame"
    return lib


class Source(Base):
    def header(self, L):
        size = C.c_size_t(2048)
        buf = C.create_string_buffer(2048)
        st = L.jpeggpu_ext_transcode_header(C.byref(self.item), buf, C.byref(size))
        return st, buf.raw[:size.value]


def keeping(o=1, trim=False, crop=None, frame=SOURCE):
    def setup(dec):
        dec.set_transcode_frame(frame)
        dec.set_transcode_orientation(o, trim)
        if crop:
            dec.set_transcode_crop(*crop)
    return setup


def refused_by_default():
    sweep, matrix, colour = cases.sampling_sweep(), cases.matrix(), color_ref.cases()
    return {
        "4:4:0": sweep["y1x2_a"], "4:1:1": sweep["y4x1_a"], "4:1:1 in its own scans": sweep["y4x2_ni"], "chroma 2x1": sweep["y2x2_c2x1_a"],
        "CMYK": next(d for d, m in colour.values() if m == color_ref.CMYK),
        "YCCK": next(d for d, m in colour.values() if m == color_ref.YCCK), "RGB-coded": next(d for d, m in colour.values() if m == color_ref.RGB),
        "two components": matrix["two_comp"], "four components": matrix["four_comp_444"], "Pq = 1": matrix["q16_tables"],
    }


def _sos_end(data):
    at = 2
    while True:
        end = at + 2 + int.from_bytes(data[at + 2:at + 4], "big")
        if data[at + 1] == 0xDA:
            return end
        at = end


def _entropy_bytes(data):
    """What is not a marker segment: the entropy-coded bytes of every scan, restart markers and EOI."""
    out, at = bytearray(), 2
    while at < len(data):
        if data[at] == 0xFF and data[at + 1] not in (0x00, 0xFF, 0xD9) and not 0xD0 <= data[at + 1] <= 0xD7:
            at += 2 + int.from_bytes(data[at + 2:at + 4], "big")
        else:
            out.append(data[at])
            at += 1
    return bytes(out)


def test_the_setter(L):
    dec = jpeggpu_amd.Decoder()
    try:
        assert L.jpeggpu_ext_set_transcode_frame(None, 0) == Status.INVALID_ARGUMENT
        data = cases.sampling_sweep()["y1x2_a"]
        dec.set_progressive(True)
        dec.parse_header(data)
        it = api.TranscodeItem()
        it.decoder, it.restart_interval = dec._h, -1
        size = C.c_size_t(0)
        status = lambda: L.jpeggpu_ext_transcode_header(C.byref(it), None, C.byref(size))  # noqa: E731
        assert status() == Status.NOT_SUPPORTED, "the default is ENCODER"
        assert L.jpeggpu_ext_set_transcode_frame(dec._h, SOURCE) == Status.SUCCESS and status() == Status.SUCCESS
        for bad in (2, -1, 256):
            assert L.jpeggpu_ext_set_transcode_frame(dec._h, bad) == Status.INVALID_ARGUMENT
            assert status() == Status.SUCCESS, "a refused value leaves the setting"
        dec.parse_header(data)
        assert status() == Status.SUCCESS, "held until it is set again"
        assert L.jpeggpu_ext_set_transcode_frame(dec._h, ENCODER) == Status.SUCCESS and status() == Status.NOT_SUPPORTED
        for bad in (2, -1):
            assert L.jpeggpu_ext_set_transcode_frame(dec._h, bad) == Status.INVALID_ARGUMENT
            assert status() == Status.NOT_SUPPORTED
    finally:
        dec.cleanup()


def test_sources_the_default_refuses(L):
    for name, data in refused_by_default().items():
        for options in (dict(), dict(optimize=True)):
            with Source(data, **options) as s:
                assert s.status(L) == Status.NOT_SUPPORTED, (name, options)
            with Source(data, keeping(), **options) as s:
                st, head = s.header(L)
                assert st == (Status.NOT_SUPPORTED if options else Status.SUCCESS), (name, options)  # (an optimised header: its length only)
                arr = (api.TranscodeItem * 1)(s.item)
                assert L.jpeggpu_ext_transcode_bound(C.byref(s.item)) > 0 and L.jpeggpu_ext_transcode_scratch_size(arr, 1) > 0, (name, options)
        with Source(data, keeping(), progressive=True) as s:  # (a progressive header: the bound of its marker segments only)
            want = F.transcode(data, progressive=True)
            size = C.c_size_t(0)
            assert L.jpeggpu_ext_transcode_header(C.byref(s.item), None, C.byref(size)) == Status.NOT_SUPPORTED, name
            markers = len(want) - len(_entropy_bytes(want))
            assert size.value >= markers, (name, size.value, markers)
            arr = (api.TranscodeItem * 1)(s.item)
            assert L.jpeggpu_ext_transcode_bound(C.byref(s.item)) >= len(want) and L.jpeggpu_ext_transcode_scratch_size(arr, 1) > 0, name


def test_header_bound_and_scratch_against_the_restatement(L):
    sources = dict(refused_by_default())
    sources.update({k[2:-2]: v for k, v in K.pins().items() if k.startswith("S_") and k.endswith("-A")})
    for name, data in sources.items():
        for r in (None, 0, 2):
            with Source(data, keeping(), restart_interval=-1 if r is None else r) as s:
                want = F.transcode(data, restart_interval=r)
                st, head = s.header(L)
                assert st == Status.SUCCESS and head == want[:_sos_end(want)], (name, r)
                assert L.jpeggpu_ext_transcode_bound(C.byref(s.item)) >= len(want), (name, r)
            with Source(data, keeping(), restart_interval=-1 if r is None else r, optimize=True) as s:
                want = F.transcode(data, restart_interval=r, optimize=True)
                size = C.c_size_t(0)
                assert L.jpeggpu_ext_transcode_header(C.byref(s.item), None, C.byref(size)) == Status.NOT_SUPPORTED
                assert size.value >= _sos_end(want), (name, r)
                assert L.jpeggpu_ext_transcode_bound(C.byref(s.item)) >= len(want), (name, r)
                plain = (api.TranscodeItem * 1)(s.item)
                plain[0].optimize = 0
                assert L.jpeggpu_ext_transcode_scratch_size((api.TranscodeItem * 1)(s.item), 1) >= L.jpeggpu_ext_transcode_scratch_size(plain, 1) > 0


def test_files_in_the_encoders_range_keep_their_header(L):
    for case in T.cases()[::5]:
        data = T.pins()[0][case["name"]]["A"]
        with Source(data) as a, Source(data, keeping()) as b:
            assert a.header(L) == b.header(L) and a.header(L)[0] == Status.SUCCESS, case["name"]
            assert L.jpeggpu_ext_transcode_bound(C.byref(a.item)) == L.jpeggpu_ext_transcode_bound(C.byref(b.item))
            assert L.jpeggpu_ext_transcode_scratch_size((api.TranscodeItem * 1)(a.item), 1) == L.jpeggpu_ext_transcode_scratch_size((api.TranscodeItem * 1)(b.item), 1)
        for options in (dict(optimize=True), dict(progressive=True)):
            with Source(data, keeping(), **options) as b:
                assert b.status(L) == Status.NOT_SUPPORTED and L.jpeggpu_ext_transcode_bound(C.byref(b.item)) > 0


def test_a_file_the_default_takes_under_other_table_numbers(L):
    """Grey on table 2 and YCbCr on tables 2 / 3 / 3: the default writes them as 0 and 0 / 1 / 1, and so does this mode."""
    files = [T.pins()[0][c["name"]]["A"] for c in T.cases()]
    picked = [next(f for f in files if len(F.parse(f)["comps"]) == n) for n in (1, 3)]
    for data in picked:
        data = K.renumbered(data, 2)
        assert [c["q"] for c in F.parse(data)["comps"]] in ([2], [2, 3, 3])
        for options in (dict(), dict(optimize=True), dict(progressive=True)):
            with Source(data, **options) as a, Source(data, keeping(), **options) as b:
                assert a.header(L) == b.header(L) and a.header(L)[0] == (Status.NOT_SUPPORTED if options else Status.SUCCESS)
                assert L.jpeggpu_ext_transcode_bound(C.byref(a.item)) == L.jpeggpu_ext_transcode_bound(C.byref(b.item)) > 0
        with Source(data, keeping()) as b:
            assert [c["q"] for c in F.parse(b.header(L)[1])["comps"]] in ([0], [0, 1, 1])


def _sof(head):
    info = F.parse(head)
    return info["w"], info["h"], [c["sampling"] for c in info["comps"]]


def test_422_takes_every_orientation(L):
    from tests.test_transcode_orient_host import _file
    data = _file(32, 48, "4:2:2")
    for o in range(5, 9):
        with Source(data, keeping(o, frame=ENCODER)) as s:
            assert s.status(L) == Status.NOT_SUPPORTED, o
        with Source(data, keeping(o)) as s:
            st, head = s.header(L)
            assert st == Status.SUCCESS and _sof(head) == (48, 32, [0x12, 0x11, 0x11]), o
            assert head == F.transcode(data, orientation=o)[:len(head)], o
    for o in range(1, 5):
        with Source(data, keeping(o)) as s, Source(data, keeping(o, frame=ENCODER)) as e:
            assert s.header(L) == e.header(L) and _sof(s.header(L)[1]) == (32, 48, [0x21, 0x11, 0x11]), o


@pytest.mark.parametrize("layout,ux,uy", [("y4x1", 32, 8), ("y1x2", 8, 16)])
def test_edge_trim_and_crop_rules_use_the_imcu(L, layout, ux, uy):
    from tools import jpegsynth
    samp = cases.SWEEP_LAYOUTS[layout]
    for o in range(1, 9):
        tux, tuy = (uy, ux) if o >= 5 else (ux, uy)
        for w, h, axis in ((2 * ux, 3 * uy, None), (2 * ux + 8 if ux > 8 else 2 * ux + 3, 3 * uy, "x"), (2 * ux, 3 * uy + 8 if uy > 8 else 3 * uy + 5, "y"),
                           (ux - 1, 3 * uy, "x small"), (2 * ux, uy - 1, "y small")):
            data = jpegsynth.encode(w, h, samp, seed=7)
            refused = axis is not None and o in (X.STORED_X if axis[0] == "x" else X.STORED_Y)
            what = (layout, o, w, h)
            with Source(data, keeping(o)) as s:
                assert s.status(L) == (Status.NOT_SUPPORTED if refused else Status.SUCCESS), what
            with Source(data, keeping(o, True)) as s:
                small = refused and axis.endswith("small")
                assert s.status(L) == (Status.NOT_SUPPORTED if small else Status.SUCCESS), what
                if not small:
                    cut = (w - w % ux if refused and axis == "x" else w, h - h % uy if refused and axis == "y" else h)
                    tw, th, bytes_ = _sof(s.header(L)[1])
                    assert (tw, th) == (cut[::-1] if o >= 5 else cut), what
                    assert bytes_ == [(v << 4 | h_) if o >= 5 else (h_ << 4 | v) for h_, v in samp], what
        # the crop's origin: a multiple of the TARGET's iMCU
        data = jpegsynth.encode(3 * ux, 3 * uy, samp, seed=8)
        for (x, y), st in (((tux, tuy), Status.SUCCESS), ((0, 2 * tuy), Status.SUCCESS), ((8, 0) if tux > 8 else (4, 0), Status.NOT_SUPPORTED),
                           ((0, 8) if tuy > 8 else (0, 4), Status.NOT_SUPPORTED), ((tux // 2, tuy), Status.NOT_SUPPORTED)):
            with Source(data, keeping(o, crop=(x, y, 9, 7))) as s:
                assert s.status(L) == st, (layout, o, x, y)
                if st == Status.SUCCESS:
                    assert _sof(s.header(L)[1])[:2] == (9, 7)
        tw, th = (3 * uy, 3 * ux) if o >= 5 else (3 * ux, 3 * uy)
        with Source(data, keeping(o, crop=(tux, tuy, tw - tux + 1, 5))) as s:
            assert s.status(L) == Status.INVALID_ARGUMENT, (layout, o)


def test_scale_shard_and_a_lone_window_stay_refused(L):
    sweep = cases.sampling_sweep()
    both = lambda f: lambda d: (d.set_transcode_frame(SOURCE), f(d))  # noqa: E731
    with Source(sweep["y4x2_a"], both(lambda d: d.set_crop(0, 0, 32, 16))) as s:
        assert s.status(L) == Status.NOT_SUPPORTED
    with Source(sweep["y4x2_a"], both(lambda d: d.set_scale(2))) as s:
        assert s.status(L) == Status.NOT_SUPPORTED
    with Source(cases.matrix()["dri_row"], both(lambda d: d.set_segment_shard(0, 2))) as s:
        assert s.status(L) == Status.NOT_SUPPORTED
    with Source(sweep["y4x2_a"], keeping()) as s:
        assert s.status(L) == Status.SUCCESS


def test_python_arguments():
    with pytest.raises(ValueError, match="frame"):
        api._transcode_frames(2, "jpegtran")
    with pytest.raises(ValueError):
        api._transcode_frames(2, ["source"])
    assert api._transcode_frames(2, "source") == ["source", "source"] and api._transcode_frames(2, ["encoder", "source"]) == ["encoder", "source"]


def test_a_library_without_the_symbol(monkeypatch):
    class Old:
        def __getattr__(self, name):
            if name == "jpeggpu_ext_set_transcode_frame":
                raise AttributeError(name)
            return getattr(jpeggpu_amd.lib(), name)

    jbuild.build()
    real = jpeggpu_amd.lib()
    monkeypatch.setattr(api, "lib", lambda: Old())
    dec = jpeggpu_amd.Decoder.__new__(jpeggpu_amd.Decoder)
    dec._h = None
    with pytest.raises(RuntimeError, match="jpeggpu_ext_set_transcode_frame"):
        dec.set_transcode_frame(1)
    assert real is not None
