"""Builds and binds tests/syncprobe/syncprobe.cpp: the product's widened (sync pack) tables and step counts of the
state-only symbol loop, on the host."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(_HERE))
_LIB = os.path.join(_HERE, "libjgsyncprobe.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        csrc = os.path.join(ROOT, "jpeggpu_amd", "csrc")
        srcs = [os.path.join(_HERE, "syncprobe.cpp"), os.path.join(csrc, "jg_reader.cpp")]
        deps = srcs + [os.path.join(csrc, h) for h in ("jg_huff_core.h", "jg_defs.h", "jg_reader.hpp", "jg_bytes.h")]
        if not os.path.exists(_LIB) or any(os.path.getmtime(d) > os.path.getmtime(_LIB) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-I" + csrc] + srcs + ["-o", _LIB])
        _lib = C.CDLL(_LIB)
        _lib.probe_widen.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        _lib.probe_count_steps.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p]
    return _lib


def widen(bits, vals, is_dc=False, strict=False):
    """uint32 [2^index bits]: low half the single-symbol entry, high half the multi-symbol entry (jg_defs.h) of the table
    with the DHT payload (bits: 16 counts, vals); strict: high halves by the rule that keeps every symbol inside the index."""
    bits = np.ascontiguousarray(bits, np.uint8)
    vals = np.ascontiguousarray(vals, np.uint8)
    assert bits.size == 16 and vals.size == int(bits.sum())
    out = np.zeros(lib().probe_lut_entries(int(is_dc)), np.uint32)
    lib().probe_widen(bits.ctypes.data, vals.ctypes.data, vals.size, int(is_dc), int(strict), out.ctypes.data)
    return out


class Steps:
    pass


def count_steps(data, subseq_bytes=256, max_segments=0):
    """Steps of the state-only loop over scan 0 of `data` (syncprobe.cpp, probe_count_steps)."""
    out = np.zeros(10, np.int64)
    rc = lib().probe_count_steps(data, len(data), subseq_bytes, max_segments, out.ctypes.data)
    assert rc == 0, rc
    r = Steps()
    r.steps, r.main_steps, r.multi_steps = (int(x) for x in out[0:3])
    r.strict_steps, r.strict_main_steps, r.strict_multi_steps = (int(x) for x in out[3:6])
    r.symbols, r.subsequences, r.state_mismatches, r.longest_multi = (int(x) for x in out[6:10])
    return r


def dht_tables(data):
    """[(class (0 DC, 1 AC), id, bits uint8[16], vals uint8[n])] of every DHT segment in front of the first scan."""
    out, i = [], 2
    while i + 4 <= len(data) and data[i] == 0xFF:
        m, ln = data[i + 1], (data[i + 2] << 8) | data[i + 3]
        if m == 0xC4:
            j, end = i + 4, i + 2 + ln
            while j < end:
                bits = np.frombuffer(data, np.uint8, 16, j + 1)
                n = int(bits.sum())
                out.append((data[j] >> 4, data[j] & 15, bits.copy(), np.frombuffer(data, np.uint8, n, j + 17).copy()))
                j += 17 + n
        if m == 0xDA:
            break
        i += 2 + ln
    return out
