#!/usr/bin/env python3
"""Writes tests/golden/encode_plan_pins.npz: what the encoder's host exports of the loaded library say for a listed sweep --
per case the status of the header call, the header's SHA-256 (its first eight bytes) or the reported size, the bound and the
scratch size -- over

  pixel items    jpeggpu_ext_encode_header / _bound / _scratch_size: sizes around the block and MCU edges and the extremes, one
                 and three channels, the three subsamplings, four restart intervals, three qualities, optimise and
                 progressive on and off; and calls of several items, as a plain and as a budget call;
  transcodes     jpeggpu_ext_transcode_*: the sources of tests/transcode_cases.py in the encoder's layouts and those of
                 tests/transcode_frame_cases.py and tests/coefficients_ref.py with their own frame;
  coefficients   jpeggpu_ext_write_coefficients_*: the sources of tests/coefficients_ref.py.

The pins say what a commit computes, so they are made with the library of the commit to compare against: check it out, build
it, and run this file with JPEGGPU_LIB naming that library. tests/test_encode_plan_host.py asserts that the shipped library
gives the same values.

    JPEGGPU_LIB=/path/to/the/other/libjpeggpu.so python tools/make_encode_plan_pins.py
"""
import ctypes as C
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LENGTHS = (1, 7, 8, 9, 15, 16, 17, 33)
SIZES = [(w, h) for w in LENGTHS for h in LENGTHS] + [(65535, 1), (1, 65535)]
FAKE = 4096  # a device address that is never followed


def _digest(data):
    return int.from_bytes(hashlib.sha256(data).digest()[:8], "little")


def _row(status, size, head, bound, scratch):
    """status, the header's digest (status 0) or the reported size, bound, scratch size"""
    return [int(status), _digest(head[:size]) if status == 0 else size, bound, scratch]


def pixel_items():
    from jpeggpu_amd import api

    for optimize, progressive in ((0, 0), (1, 0), (0, 1), (1, 1)):
        for quality in (50, 1, 100):
            for w, h in SIZES if quality == 50 else ((1, 1), (17, 9), (33, 33)):
                for channels in (1, 3):
                    for subsampling in range(3):
                        for restart in (0, 1, 2, 65535):
                            it = api.EncodeItem()
                            it.data, it.width, it.height, it.channels, it.progressive, it.optimize = FAKE, w, h, channels, progressive, optimize
                            it.quality, it.subsampling, it.restart_interval = quality, subsampling, restart
                            yield it


def pixel_calls():
    """Calls of 2 and 5 items mixing the kinds: none progressive, all progressive, an optimised item first and last."""
    items = list(pixel_items())
    kinds = {(o, p): [it for it in items if (it.optimize, it.progressive) == (o, p) and it.quality == 50][7::97] for o in (0, 1) for p in (0, 1)}
    for k in range(12):
        plain, opt, prog, both = (kinds[key][k] for key in ((0, 0), (1, 0), (0, 1), (1, 1)))
        yield [plain, opt]
        yield [prog, both]
        yield [opt, plain, prog, plain, opt]
        yield [plain, prog, both, opt, plain]


def pixel(L):
    from jpeggpu_amd import api

    rows, buf = [], C.create_string_buffer(4096)
    for it in pixel_items():
        size = C.c_size_t(4096)
        st = L.jpeggpu_ext_encode_header(C.byref(it), buf, C.byref(size))
        rows.append(_row(st, size.value, buf.raw, L.jpeggpu_ext_encode_bound(C.byref(it)), L.jpeggpu_ext_encode_scratch_size((api.EncodeItem * 1)(it), 1)))
    calls = []
    for call in pixel_calls():
        arr = (api.EncodeItem * len(call))(*call)
        fit = (api.EncodeFitItem * len(call))()
        for f, it in zip(fit, call):
            f.item, f.max_bytes, f.quality_min, f.quality_max = it, 1000, 10, 90
        calls.append([L.jpeggpu_ext_encode_scratch_size(arr, len(call)), L.jpeggpu_ext_encode_fit_scratch_size(fit, len(call))])
    return np.asarray(rows, np.uint64), np.asarray(calls, np.uint64)


def transcode_sources():
    """(name, file, keeps its source's frame)"""
    from tests import coefficients_ref, transcode_cases, transcode_frame_cases

    pins = transcode_cases.pins()[0]
    for case in transcode_cases.cases():
        for kind in "ABC":
            yield "%s-%s" % (case["name"], kind), pins[case["name"]][kind], False
    for name, data in sorted(transcode_frame_cases.pins().items()):
        if name.startswith("S_") and name.endswith("-A"):
            yield name, data, True
    for name, data in sorted(coefficients_ref.sources().items()):
        yield "coefficients_" + name, data, True


OPTIONS = (dict(), dict(restart_interval=0), dict(restart_interval=2), dict(optimize=1), dict(progressive=1, restart_interval=3), dict(optimize=1, progressive=1))


def transcode(L):
    import jpeggpu_amd
    from jpeggpu_amd import api

    rows, names, buf = [], [], C.create_string_buffer(4096)
    for name, data, keep in transcode_sources():
        dec = jpeggpu_amd.Decoder()
        try:
            dec.set_progressive(True)
            if keep:
                dec.set_transcode_frame(1)
            dec.parse_header(data)
            for options in OPTIONS:
                it = api.TranscodeItem()
                it.decoder, it.optimize, it.progressive = dec._h, options.get("optimize", 0), options.get("progressive", 0)
                it.restart_interval = options.get("restart_interval", -1)
                size = C.c_size_t(4096)
                st = L.jpeggpu_ext_transcode_header(C.byref(it), buf, C.byref(size))
                rows.append(_row(st, size.value, buf.raw, L.jpeggpu_ext_transcode_bound(C.byref(it)),
                                 L.jpeggpu_ext_transcode_scratch_size((api.TranscodeItem * 1)(it), 1)))
                names.append(name)
        finally:
            dec.cleanup()
    return np.asarray(rows, np.uint64), names


def coefficients(L):
    from jpeggpu_amd import api
    from tests import coefficients_ref as K

    rows, buf = [], C.create_string_buffer(4096)
    for name, data in sorted(K.sources().items()):
        co = K.read(data)
        for options in OPTIONS:
            it = api.CoefficientItem()
            it.width, it.height, it.components, it.color_space = co.w, co.h, len(co.coef), co.color
            for c in range(len(co.coef)):
                it.h[c], it.v[c] = co.sampling[c]
                it.coef[c] = FAKE
                for k in range(64):
                    it.qtable[c][k] = int(co.qtables[c][k])
            it.optimize, it.progressive, it.restart_interval = options.get("optimize", 0), options.get("progressive", 0), options.get("restart_interval", 0)
            size = C.c_size_t(4096)
            st = L.jpeggpu_ext_write_coefficients_header(C.byref(it), buf, C.byref(size))
            rows.append(_row(st, size.value, buf.raw, L.jpeggpu_ext_write_coefficients_bound(C.byref(it)),
                             L.jpeggpu_ext_write_coefficients_scratch_size((api.CoefficientItem * 1)(it), 1)))
    return np.asarray(rows, np.uint64)


def collect(L):
    """{array name: values} of the loaded library `L`: what the fixture holds."""
    px, calls = pixel(L)
    tr, _ = transcode(L)
    return dict(pixel=px, pixel_calls=calls, transcode=tr, coefficients=coefficients(L))


def main():
    import jpeggpu_amd

    if sys.argv[1:]:
        raise SystemExit(__doc__)
    out = collect(jpeggpu_amd.lib())
    path = os.path.join(ROOT, "tests", "golden", "encode_plan_pins.npz")
    np.savez_compressed(path, **out)
    print("%s: library %s; %s; %d bytes" % (path, os.environ.get("JPEGGPU_LIB", "(the tree's)"),
                                           ", ".join("%d %s" % (len(v), k) for k, v in out.items()), os.path.getsize(path)))


if __name__ == "__main__":
    main()
