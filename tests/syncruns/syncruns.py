"""Builds and binds tests/syncruns/syncruns.cpp: the batched sequence kernel's schedule with runs of subsequences per
lane (jpeggpu_amd/csrc/jg_sync_runs.h), one lane at a time on the host."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(_HERE))
CSRC = os.path.join(ROOT, "jpeggpu_amd", "csrc")
SOURCES = [os.path.join(_HERE, "syncruns.cpp"), os.path.join(CSRC, "jg_reader.cpp")]
FLAGS = ["-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC]
_LIB = os.path.join(_HERE, "libjgsyncruns.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        deps = SOURCES + [os.path.join(CSRC, h) for h in ("jg_sync_runs.h", "jg_huff_core.h", "jg_defs.h", "jg_reader.hpp", "jg_bytes.h")]
        if not os.path.exists(_LIB) or any(os.path.getmtime(d) > os.path.getmtime(_LIB) for d in deps):
            subprocess.check_call(["g++", "-O2", "-shared", "-fPIC"] + FLAGS + SOURCES + ["-o", _LIB])
        _lib = C.CDLL(_LIB)
        _lib.probe_sync_runs.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_void_p]
        _lib.probe_num_subseq.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_int]
    return _lib


class Runs:
    pass


def num_subseq(data, subseq_bytes, scan=0):
    return lib().probe_num_subseq(data, len(data), subseq_bytes, scan)


def run(data, subseq_bytes, r, scan=0):
    """The run schedule over one scan of `data` (syncruns.cpp, probe_sync_runs)."""
    out = np.zeros(24, np.int64)
    rc = lib().probe_sync_runs(data, len(data), subseq_bytes, scan, r, out.ctypes.data)
    assert rc == 0, rc
    x = Runs()
    (x.subsequences, x.groups, x.spec_decodes, x.flow_decodes, x.wrong_states, x.marks, x.marks_inside_runs, x.wrong_after_tail,
     x.differ_from_today, x.tail_decodes, x.never_stored, x.segments) = (int(v) for v in out[:12])
    x.opens_at = [int(v) for v in out[12:16]]           # segments that open at subsequence index % 4 == k
    x.segments_of = {k: int(out[16 + k]) for k in range(1, 8)}  # segments of k subsequences
    return x
