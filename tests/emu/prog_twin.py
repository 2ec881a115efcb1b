"""Builds and binds tests/emu/prog_twin.cpp: the host twin of the progressive kernels (the product's parser and
jg_prog_core.h, driven level by level as the kernels are)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(_HERE))
CSRC = os.path.join(ROOT, "jpeggpu_amd", "csrc")
_LIB = os.path.join(_HERE, "libjgprogtwin.so")
_lib = None
MAX_SCANS = 64


class Info(C.Structure):
    _fields_ = [("num_comp", C.c_int), ("num_scans", C.c_int), ("num_levels", C.c_int), ("color_space", C.c_int),
                ("size_x", C.c_int * 4), ("size_y", C.c_int * 4), ("blocks_x", C.c_int * 4), ("blocks_y", C.c_int * 4),
                ("vis_x", C.c_int * 4), ("vis_y", C.c_int * 4), ("scan_level", C.c_int * MAX_SCANS),
                ("scan_segments", C.c_int * MAX_SCANS)]


def sources():
    return [os.path.join(_HERE, "prog_twin.cpp"), os.path.join(CSRC, "jg_reader.cpp")]


def compile_args():
    return ["-std=c++17", "-fwrapv", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC]


def lib():
    global _lib
    if _lib is None:
        deps = sources() + [os.path.join(CSRC, h) for h in ("jg_prog_core.h", "jg_prog_plan.hpp", "jg_huff_core.h", "jg_defs.h", "jg_reader.hpp")]
        if not os.path.exists(_LIB) or any(os.path.getmtime(d) > os.path.getmtime(_LIB) for d in deps):
            subprocess.check_call(["g++", "-O2", "-shared", "-fPIC"] + compile_args() + sources() + ["-o", _LIB])
        _lib = C.CDLL(_LIB)
        _lib.prog_twin_run.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_int, C.POINTER(Info), C.c_void_p, C.c_void_p]
        _lib.prog_twin_work.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p]
    return _lib


IDLE = 0xFFFFFFFF  # the scan number of an idle work item (jg_prog_core.h, kProgNoScan)


def work_list(data: bytes):
    """(items, level_item) as the blob holds them: items uint32 [n, 2] of (scan, segment), IDLE for a padding item;
    level_item uint32 [MAX_SCANS + 1], the first item of each level (and one past the last level's)."""
    level_item = np.zeros(MAX_SCANS + 1, np.uint32)
    n = lib().prog_twin_work(data, len(data), None, 0, level_item.ctypes.data)
    assert n >= 0, n
    items = np.zeros((n, 2), np.uint32)
    assert lib().prog_twin_work(data, len(data), items.ctypes.data, n, level_item.ctypes.data) == n
    return items, level_item


def parse(data: bytes, progressive=True, shard_world=1):
    """(status, Info) of the product's parser."""
    info = Info()
    return lib().prog_twin_run(data, len(data), int(progressive), shard_world, C.byref(info), None, None), info


def decode(data: bytes):
    """(status, Info, coef, back): coef[c] int16 [blocks_y, blocks_x, 64] over the MCU-padded grid, back[c] int16
    [vis_y, vis_x, 64]: the visible blocks after the hand-over's pack and the way back from the symbol stream."""
    st, info = parse(data)
    if st or not info.num_scans:
        return st, info, None, None
    n = info.num_comp
    coef = [np.zeros((info.blocks_y[c], info.blocks_x[c], 64), np.int16) for c in range(n)]
    back = [np.zeros((info.vis_y[c], info.vis_x[c], 64), np.int16) for c in range(n)]
    cp = (C.c_void_p * 4)(*[a.ctypes.data for a in coef])
    bp = (C.c_void_p * 4)(*[a.ctypes.data for a in back])
    st = lib().prog_twin_run(data, len(data), 1, 1, C.byref(info), cp, bp)
    return st, info, coef, back
