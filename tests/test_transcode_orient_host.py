"""The host half of the oriented transcode (jpeggpu_ext_set_transcode_orientation): the setter's argument checks, header,
bound and scratch size of an oriented item against the reference's file and the encoder's arithmetic on the TARGET's
geometry, every refusal, and orientation 1 against an untouched decoder. No GPU needed."""
import ctypes as C

import numpy as np
import pytest

import jpeggpu_amd
from jpeggpu_amd import Status, api
from tests import encode_ref as E
from tests import transcode_orient_cases as K
from tests import transcode_orient_ref as X
from tests import transcode_ref as R
from tests.test_transcode_host import L, Source, file_header  # noqa: F401 (L is a fixture)

SUBSAMPLING_OF = {0x11: "4:4:4", 0x21: "4:2:2", 0x22: "4:2:0", 0x12: "4:4:4"}  # (a grey frame's byte: only the header shows it)


def oriented(o, trim=False):
    return lambda dec: dec.set_transcode_orientation(o, trim)


def test_setter_arguments(L):
    dec = jpeggpu_amd.Decoder()
    f = L.jpeggpu_ext_set_transcode_orientation
    assert f(None, 1, 0) == Status.INVALID_ARGUMENT
    for o in (0, 9, -1, 1 << 20):
        assert f(dec._h, o, 0) == Status.INVALID_ARGUMENT
    for t in (2, -1):
        assert f(dec._h, 3, t) == Status.INVALID_ARGUMENT
    for o in range(1, 9):
        for t in (0, 1):
            assert f(dec._h, o, t) == Status.SUCCESS  # (any time after creation: nothing has been parsed)
    dec.cleanup()


def test_a_refused_value_leaves_the_setting(L):
    src = K.pins()[0]["48x32_420_q100"]
    with Source(src, oriented(6)) as s:
        want = s.header(L)
        assert L.jpeggpu_ext_set_transcode_orientation(s.dec._h, 9, 0) == Status.INVALID_ARGUMENT
        assert L.jpeggpu_ext_set_transcode_orientation(s.dec._h, 2, 2) == Status.INVALID_ARGUMENT
        assert s.header(L) == want and want[1] == file_header(X.transform(src, 6))
        s.dec.set_transcode_orientation(1)  # it holds until it is set again, and is read when the calls run
        assert s.header(L)[1] == file_header(src)


def _sources():
    """Pinned cell images, and noise files with Annex K's (asymmetric) tables, restart intervals and a grey 0x21 byte."""
    out = {name: data for name, data in K.pins()[0].items() if name.split("_")[0] in ("35x21", "17x40", "5x3")}
    rng = np.random.default_rng(20261104)
    for k, (w, h, sampling, grey) in enumerate([(48, 32, "4:2:0", False), (35, 21, "4:4:4", False), (17, 40, "4:2:0", False), (40, 17, "4:2:2", False),
                                                 (35, 21, "4:2:2", True), (16, 24, "4:2:0", True)]):
        img = rng.integers(0, 256, (h, w) if grey else (h, w, 3), dtype=np.uint8)
        out["noise_%dx%d_%s_%s" % (w, h, sampling, "grey" if grey else "colour")] = E.encode(img, 40 + 10 * k, sampling, k % 3)
    return out


def test_header_bound_and_scratch_follow_the_target(L):
    n = 0
    for name, src in _sources().items():
        info = R._checked(src)
        case = dict(w=info["w"], h=info["h"], sampling="grey" if len(info["comps"]) == 1 else info["subsampling"])
        for o in range(1, 9):
            for trim in (False, True):
                if K.allowed(case, o, trim) is None:
                    continue
                ref = X.transform(src, o, trim)
                head = R.parse(ref)
                with Source(src, oriented(o, trim)) as s, Source(ref) as plain:
                    assert s.header(L) == (Status.SUCCESS, file_header(ref)), (name, o, trim)
                    for options in (dict(), dict(optimize=True), dict(progressive=True), dict(restart_interval=3)):
                        s.item.optimize = plain.item.optimize = int(options.get("optimize", 0))
                        s.item.progressive = plain.item.progressive = int(options.get("progressive", 0))
                        s.item.restart_interval = plain.item.restart_interval = options.get("restart_interval", -1)
                        r = options.get("restart_interval", info["restart"])
                        same = api.encode_item(head["w"], head["h"], len(head["comps"]), 75, SUBSAMPLING_OF[head["comps"][0]["sampling"]], r,
                                               optimize=bool(s.item.optimize), progressive=bool(s.item.progressive))
                        bound = L.jpeggpu_ext_transcode_bound(C.byref(s.item))
                        assert bound == L.jpeggpu_ext_encode_bound(C.byref(same)) > 0, (name, o, trim, options)
                        assert bound >= len(ref) or options
                        size = L.jpeggpu_ext_transcode_scratch_size((api.TranscodeItem * 1)(s.item), 1)
                        assert size == L.jpeggpu_ext_transcode_scratch_size((api.TranscodeItem * 1)(plain.item), 1) > 0, (name, o, trim, options)
                        n += 1
    assert n > 500


def test_orientation_one_is_an_untouched_decoder(L):
    for name, src in _sources().items():
        with Source(src) as a, Source(src, oriented(1)) as b, Source(src, oriented(1, True)) as c:
            want = a.header(L)
            assert want[0] == Status.SUCCESS and want[1] == file_header(R.transcode(src))
            for s in (b, c):
                assert s.header(L) == want, name
                assert L.jpeggpu_ext_transcode_bound(C.byref(s.item)) == L.jpeggpu_ext_transcode_bound(C.byref(a.item))
                assert L.jpeggpu_ext_transcode_scratch_size((api.TranscodeItem * 1)(s.item), 1) == L.jpeggpu_ext_transcode_scratch_size((api.TranscodeItem * 1)(a.item), 1)


def _file(w, h, sampling, grey=False):
    img = np.full((h, w) if grey else (h, w, 3), 90, np.uint8)
    return E.encode(img, 75, sampling, 0)


def test_refusals(L):
    """Every call refuses, before anything is enqueued: 4:2:2 with 5..8, each imperfect axis of each orientation, an axis
    below one iMCU with trim. The same sizes made perfect are accepted."""
    for o in range(5, 9):
        for trim in (False, True):
            with Source(_file(32, 32, "4:2:2"), oriented(o, trim)) as s:
                assert s.status(L) == Status.NOT_SUPPORTED, o
    for o in range(1, 5):
        with Source(_file(32, 32, "4:2:2"), oriented(o)) as s:
            assert s.status(L) == Status.SUCCESS, o
    for sampling, grey, (ux, uy) in (("4:4:4", False, (8, 8)), ("4:2:0", False, (16, 16)), ("4:2:2", False, (16, 8)), ("4:2:0", True, (8, 8)), ("4:2:2", True, (8, 8))):
        for o in range(1, 9):
            if sampling == "4:2:2" and not grey and o >= 5:
                continue
            for w, h, axis in ((3 * ux, 2 * uy, None), (3 * ux - 8 if ux > 8 else 3 * ux - 3, 2 * uy, "x"), (3 * ux, 2 * uy + 5, "y"), (ux - 1, 2 * uy, "x small"),
                               (3 * ux, uy - 1, "y small")):
                refused = axis is not None and o in (X.STORED_X if axis[0] == "x" else X.STORED_Y)
                what = (sampling, grey, o, w, h)
                src = _file(w, h, sampling, grey)
                with Source(src, oriented(o)) as s:
                    assert s.status(L) == (Status.NOT_SUPPORTED if refused else Status.SUCCESS), what
                with Source(src, oriented(o, True)) as s:
                    small = refused and axis.endswith("small")
                    assert s.status(L) == (Status.NOT_SUPPORTED if small else Status.SUCCESS), what
                    if refused and not small:
                        head = R.parse(s.header(L)[1])
                        cut = (w - w % ux, h) if axis == "x" else (w, h - h % uy)
                        assert (head["w"], head["h"]) == (cut[::-1] if o >= 5 else cut), what
    with Source(_file(17, 40, "4:2:0"), oriented(5)) as s:  # orientation 5 never needs either
        assert s.status(L) == Status.SUCCESS
    with Source(_file(5, 3, "4:4:4"), oriented(5)) as s:
        assert s.status(L) == Status.SUCCESS


def test_python_arguments_before_any_device_work(monkeypatch):
    class Bd:
        decoders = [None, None]
        orientations = [6, 1]

    with pytest.raises(ValueError, match="item 0"):
        api._transcode_orientations(Bd, 6, True, False)
    with pytest.raises(ValueError, match="item 1"):
        api._transcode_orientations(Bd, [None, 3], [True, True], False)
    with pytest.raises(ValueError, match="1..8"):
        api._transcode_orientations(Bd, 9, False, False)
    with pytest.raises(ValueError):
        api._transcode_orientations(Bd, [1, 2, 3], False, False)
    assert api._transcode_orientations(Bd, [None, 3], [True, False], [False, True]) == [(6, False), (3, True)]
    assert api._transcode_orientations(Bd, None, False, False) == [(1, False), (1, False)]
    assert api._transcode_orientations(Bd, None, True, True) == [(6, True), (1, True)]
