"""The host half of the cropped transcode (jpeggpu_ext_set_transcode_crop): the setter's argument checks, header, bound and
scratch size of a cropped item against the restatement's file and the encoder's arithmetic on the rectangle's size, every
refusal with its status, the rule that lets a decode window (jpeggpu_ext_set_crop) stand under a transcode crop on both
sides of its boundary, and (0, 0, 0, 0) against an untouched decoder. No GPU needed."""
import ctypes as C

import numpy as np
import pytest

import jpeggpu_amd
from jpeggpu_amd import Status, api
from tests import encode_ref as E
from tests import transcode_crop_cases as W
from tests import transcode_crop_ref as Z
from tests import transcode_orient_cases as K
from tests import transcode_ref as R
from tests.test_transcode_host import L, Source, file_header  # noqa: F401 (L is a fixture)
from tests.test_transcode_orient_host import SUBSAMPLING_OF, _sources


def setup(rect=None, o=1, trim=False, window=None, scale=None, shard=None):
    """What a Source does to its decoder before it parses: the transcode's crop and orientation, the decode's window."""
    def f(dec):
        dec.set_transcode_orientation(o, trim)
        if rect is not None:
            dec.set_transcode_crop(*rect)
        if window is not None:
            dec.set_crop(*window)
        if scale is not None:
            dec.set_scale(scale)
        if shard is not None:
            dec.set_segment_shard(*shard)
    return f


def test_setter_arguments(L):
    dec = jpeggpu_amd.Decoder()
    f = L.jpeggpu_ext_set_transcode_crop
    assert f(None, 0, 0, 8, 8) == Status.INVALID_ARGUMENT
    for bad in ((-8, 0, 8, 8), (0, -8, 8, 8), (0, 0, -8, 8), (0, 0, 8, -8), (0, 0, 0, 8), (0, 0, 8, 0), (8, 0, 0, 0), (0, 8, 0, 0), (-1, -1, -1, -1)):
        assert f(dec._h, *bad) == Status.INVALID_ARGUMENT, bad
    for good in ((0, 0, 0, 0), (0, 0, 1, 1), (16, 32, 5, 7), (3, 5, 1, 1), (1 << 20, 0, 8, 8)):  # (what the image allows is the calls' to say)
        assert f(dec._h, *good) == Status.SUCCESS, good
    dec.cleanup()


def test_a_refused_value_leaves_the_setting(L):
    src = W.pins()[0]["80x64_420_photo"]
    with Source(src, setup((16, 16, 32, 32))) as s:
        want = s.header(L)
        assert want == (Status.SUCCESS, file_header(Z.transform(src, (16, 16, 32, 32))))
        assert L.jpeggpu_ext_set_transcode_crop(s.dec._h, 0, 0, 16, 0) == Status.INVALID_ARGUMENT
        assert L.jpeggpu_ext_set_transcode_crop(s.dec._h, -16, 0, 16, 16) == Status.INVALID_ARGUMENT
        assert s.header(L) == want
        s.dec.set_transcode_crop(0, 0, 0, 0)  # it holds until it is set again, and is read when the calls run
        assert s.header(L) == (Status.SUCCESS, file_header(src))


def _rects(tw, th, ux, uy):
    """Rectangles of a tw x th target with an iMCU of ux x uy: whole iMCUs, to the edges, ragged inside, one pixel, all."""
    out = [(0, 0, tw, th), (0, 0, 1, 1), ((tw - 1) // ux * ux, (th - 1) // uy * uy, 1, 1), (0, 0, min(tw, ux + 3), min(th, uy + 5))]
    if tw > ux:
        out += [(ux, 0, tw - ux, th), (ux, 0, min(ux, tw - ux), min(uy, th))]
    if th > uy:
        out += [(0, uy, tw, th - uy), (0, uy, min(tw, 9), th - uy)]
    return out


def test_header_bound_and_scratch_follow_the_rectangle(L):
    """SOF size, tables and sampling byte (transposed and exchanged under 5..8), the restart interval: the restatement's
    header. Bound and scratch size: the encoder's on the rectangle's size."""
    n = 0
    for name, src in _sources().items():
        info = R._checked(src)
        case = dict(w=info["w"], h=info["h"], sampling="grey" if len(info["comps"]) == 1 else info["subsampling"])
        for o in range(1, 9):
            for trim in (False, True):
                if K.allowed(case, o, trim) is None:
                    continue
                tw, th, ths, tvs = Z.target_geometry(info["w"], info["h"], info["hs"], info["vs"], o, trim)
                for rect in _rects(tw, th, 8 * ths, 8 * tvs):
                    ref = Z.transform(src, rect, o, trim)
                    head = R.parse(ref)
                    assert (head["w"], head["h"]) == rect[2:]
                    with Source(src, setup(rect, o, trim)) as s, Source(ref) as plain:
                        assert s.header(L) == (Status.SUCCESS, file_header(ref)), (name, o, trim, rect)
                        for options in (dict(), dict(optimize=True), dict(progressive=True), dict(restart_interval=3)):
                            s.item.optimize = plain.item.optimize = int(options.get("optimize", 0))
                            s.item.progressive = plain.item.progressive = int(options.get("progressive", 0))
                            s.item.restart_interval = plain.item.restart_interval = options.get("restart_interval", -1)
                            r = options.get("restart_interval", info["restart"])
                            same = api.encode_item(rect[2], rect[3], len(head["comps"]), 75, SUBSAMPLING_OF[head["comps"][0]["sampling"]], r,
                                                   optimize=bool(s.item.optimize), progressive=bool(s.item.progressive))
                            bound = L.jpeggpu_ext_transcode_bound(C.byref(s.item))
                            assert bound == L.jpeggpu_ext_encode_bound(C.byref(same)) > 0, (name, o, trim, rect, options)
                            size = L.jpeggpu_ext_transcode_scratch_size((api.TranscodeItem * 1)(s.item), 1)
                            assert size == L.jpeggpu_ext_transcode_scratch_size((api.TranscodeItem * 1)(plain.item), 1) > 0, (name, o, trim, rect, options)
                            n += 1
    assert n > 1500


def test_no_crop_is_an_untouched_decoder(L):
    for name, src in _sources().items():
        with Source(src) as a, Source(src, setup((0, 0, 0, 0))) as b:
            want = a.header(L)
            assert want[0] == Status.SUCCESS and b.header(L) == want, name
            assert L.jpeggpu_ext_transcode_bound(C.byref(b.item)) == L.jpeggpu_ext_transcode_bound(C.byref(a.item))
            assert L.jpeggpu_ext_transcode_scratch_size((api.TranscodeItem * 1)(b.item), 1) == L.jpeggpu_ext_transcode_scratch_size((api.TranscodeItem * 1)(a.item), 1)


def _file(w, h, sampling, grey=False, restart=0):
    rng = np.random.default_rng([w, h, restart])
    img = rng.integers(60, 200, (h, w) if grey else (h, w, 3), dtype=np.uint8)
    return E.encode(img, 75, sampling, restart)


def test_refusals(L):
    """Before anything is enqueued, from all four calls: a rectangle that leaves the uncropped target (INVALID_ARGUMENT), an
    origin off the target's iMCU (NOT_SUPPORTED), under every layout and with the factors exchanged for 5..8; the
    orientation's own refusals stay on the whole source."""
    for sampling, grey, (ux, uy) in (("4:4:4", False, (8, 8)), ("4:2:0", False, (16, 16)), ("4:2:2", False, (16, 8)), ("4:2:0", True, (8, 8))):
        src = _file(48, 32, sampling, grey)
        for o in range(1, 9):
            if sampling == "4:2:2" and o >= 5:
                with Source(src, setup((0, 0, 8, 8), o)) as s:
                    assert s.status(L) == Status.NOT_SUPPORTED
                continue
            tw, th, tux, tuy = (32, 48, uy, ux) if o >= 5 else (48, 32, ux, uy)
            cases = [((0, 0, tw, th), Status.SUCCESS), ((tux, tuy, tw - tux, th - tuy), Status.SUCCESS), ((tux, tuy, 1, 1), Status.SUCCESS),
                     ((0, 0, tw + 1, th), Status.INVALID_ARGUMENT), ((0, 0, tw, th + 1), Status.INVALID_ARGUMENT), ((tux, 0, tw - tux + 1, 8), Status.INVALID_ARGUMENT),
                     ((0, tuy, 8, th - tuy + 1), Status.INVALID_ARGUMENT), ((2 * tw, 0, 8, 8), Status.INVALID_ARGUMENT),
                     ((tux - 1, 0, 8, 8), Status.NOT_SUPPORTED), ((0, tuy + 1, 8, 8), Status.NOT_SUPPORTED), ((tux // 2, 0, 8, 8), Status.NOT_SUPPORTED),
                     ((0, tuy // 2, 8, 8), Status.NOT_SUPPORTED)]
            if tux != tuy:  # 4:2:2: 8 is an iMCU down and half of one across
                cases += [((8, 8, 8, 8), Status.NOT_SUPPORTED), ((16, 8, 8, 8), Status.SUCCESS)]
            for rect, want in cases:
                with Source(src, setup(rect, o)) as s:
                    assert s.status(L) == want, (sampling, grey, o, rect)
    # the edge rules look at the whole source, whatever the rectangle
    src = _file(45, 32, "4:2:0")
    with Source(src, setup((0, 0, 16, 16), 2)) as s:
        assert s.status(L) == Status.NOT_SUPPORTED
    with Source(src, setup((0, 0, 16, 16), 2, True)) as s:
        assert s.status(L) == Status.SUCCESS
    with Source(src, setup((16, 0, 17, 16), 2, True)) as s:  # the uncropped target is 32 wide once trimmed
        assert s.status(L) == Status.INVALID_ARGUMENT
    with Source(src, setup((32, 0, 13, 16), 1)) as s:
        assert s.status(L) == Status.SUCCESS


def test_scale_shard_and_a_window_alone_stay_refused(L):
    src = _file(80, 64, "4:2:0", restart=5)
    with Source(src, setup(window=(16, 16, 32, 16))) as s:  # a decode window without a transcode crop
        assert s.status(L) == Status.NOT_SUPPORTED
    with Source(src, setup((0, 0, 32, 32), scale=2)) as s:
        assert s.status(L) == Status.NOT_SUPPORTED
    with Source(src, setup((0, 0, 32, 32), shard=(0, 2))) as s:
        assert s.status(L) == Status.NOT_SUPPORTED
    with Source(src, setup((0, 0, 32, 32))) as s:
        assert s.status(L) == Status.SUCCESS


def _window_mcus(s, hs, vs):
    """[mx0, mx1) x [my0, my1): the frame MCUs of the decoder's window, from where luma's window lies in its plane."""
    ci = s.dec.crop_info()
    x0, y0 = ci.origin_x[0], ci.origin_y[0]
    return x0 // (8 * hs), -(-(x0 + s.info.sizes_x[0]) // (8 * hs)), y0 // (8 * vs), -(-(y0 + s.info.sizes_y[0]) // (8 * vs))


@pytest.mark.parametrize("kind", ["rows", "three", "none", "grey", "progressive", "own_scans"])
def test_the_decode_window_must_hold_what_is_read(L, kind):
    """The window's MCUs against the rectangle's on both sides of every edge: a rectangle that fills the window exactly is
    taken, one that reads one block more on any side is JPEGGPU_NOT_SUPPORTED -- for a single scan with restart intervals of
    one MCU row and of 3 MCUs (the kept segments), one without markers, a grey one, a progressive and a multi-scan file."""
    grey = kind == "grey"
    sampling = "grey" if grey else "4:2:0"
    hs, vs = (1, 1) if grey else (2, 2)
    ux, uy = 8 * hs, 8 * vs
    w, h = (10 * ux, 8 * uy)
    if kind in ("progressive", "own_scans"):
        src = W.source_of_kind(kind, sampling, w, h, "photo", 1, 0)
    else:
        src = _file(w, h, "4:4:4" if grey else sampling, grey, dict(rows=10, three=3, none=0, grey=10)[kind])
    n = 0
    for window in ((3 * ux, 2 * uy, 3 * ux, 2 * uy), (0, 5 * uy, 4 * ux, 3 * uy), (6 * ux + 3, uy + 5, 10, 9), (0, 0, w, h)):
        with Source(src, setup((0, 0, 8, 8), window=window)) as s:
            mx0, mx1, my0, my1 = _window_mcus(s, hs, vs)
        assert mx0 * ux <= window[0] and window[0] + window[2] <= mx1 * ux and my0 * uy <= window[1] and window[1] + window[3] <= my1 * uy
        fill = (mx0 * ux, my0 * uy, min(mx1 * ux, w) - mx0 * ux, min(my1 * uy, h) - my0 * uy)
        cases = [(fill, True), (window if window[0] % ux == 0 and window[1] % uy == 0 else fill, True), ((fill[0], fill[1], 1, 1), True)]
        if mx0 > 0:
            cases.append(((fill[0] - ux, fill[1], fill[2], fill[3]), False))
        if my0 > 0:
            cases.append(((fill[0], fill[1] - uy, fill[2], fill[3]), False))
        if mx1 * ux < w:
            cases.append(((fill[0], fill[1], fill[2] + 1, fill[3]), False))
        if my1 * uy < h:
            cases.append(((fill[0], fill[1], fill[2], fill[3] + 1), False))
        for rect, ok in cases:
            with Source(src, setup(rect, window=window)) as s:
                assert s.status(L) == (Status.SUCCESS if ok else Status.NOT_SUPPORTED), (kind, window, rect)
                if ok:
                    assert s.header(L)[1] == file_header(Z.transform(src, rect))
            n += 1
    assert n >= 4 * 3 + 6
    # under an orientation the rectangle is in displayed pixels: its source blocks are what the window must hold
    if not grey:
        window = (6 * ux, uy, 3 * ux, 2 * uy)
        for o in range(2, 9):
            tw, th, _, _ = Z.target_geometry(w, h, hs, vs, o)
            with Source(src, setup((0, 0, 8, 8), o, window=window)) as s:
                mx0, mx1, my0, my1 = _window_mcus(s, hs, vs)
            stored = (mx0 * ux, my0 * uy, (mx1 - mx0) * ux, (my1 - my0) * uy)
            shown = next(r for r in ((x, y, cw, ch) for x in range(0, tw, ux) for y in range(0, th, uy) for cw, ch in (stored[2:], stored[:1:-1]))
                         if r[0] + r[2] <= tw and r[1] + r[3] <= th and Z.source_rect(r, tw, th, o) == stored)
            with Source(src, setup(shown, o, window=window)) as s:
                assert s.status(L) == Status.SUCCESS, (kind, o)
            with Source(src, setup((0, 0) + shown[2:], o, window=window)) as s:
                assert s.status(L) == (Status.SUCCESS if shown[:2] == (0, 0) else Status.NOT_SUPPORTED), (kind, o)


def test_python_arguments_before_any_device_work():
    assert api._transcode_crops(3, None) == [None] * 3
    assert api._transcode_crops(2, (16, 0, 8, 8)) == [(16, 0, 8, 8)] * 2
    assert api._transcode_crops(2, [None, (16, 0, 8, 8)]) == [None, (16, 0, 8, 8)]
    assert api._transcode_crops(4, [(0, 0, 8, 8)] * 4) == [(0, 0, 8, 8)] * 4
    with pytest.raises(ValueError):
        api._transcode_crops(3, [None, (16, 0, 8, 8)])
    with pytest.raises(ValueError, match="crops.1"):
        api._transcode_crops(2, [None, (16, 0, 8)])
    assert api._expanded((17, 9, 10, 10), 2, 2) == Z.expanded((17, 9, 10, 10), 2, 2)
