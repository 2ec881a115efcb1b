"""ctypes binding of tools/jpegsynth.c: seeded synthetic baseline JPEGs for tests and bench."""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "libjpegsynth.so")


class _Params(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("ncomp", C.c_int),
                ("hs", C.c_int * 4), ("vs", C.c_int * 4),
                ("interleaved", C.c_int), ("restart_interval", C.c_int), ("quality", C.c_int),
                ("optimize", C.c_int), ("noise", C.c_int), ("fill_bytes", C.c_int), ("seed", C.c_uint64), ("qmax", C.c_int)]


class _Custom(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("ncomp", C.c_int),
                ("hs", C.c_int * 4), ("vs", C.c_int * 4), ("bw", C.c_int * 4), ("bh", C.c_int * 4),
                ("dc_tab", C.c_int * 4), ("ac_tab", C.c_int * 4), ("q_tab", C.c_int * 4),
                ("interleaved", C.c_int), ("restart_interval", C.c_int)]


def build(force=False):
    src = os.path.join(_HERE, "jpegsynth.c")
    if force or not os.path.exists(_LIB) or os.path.getmtime(_LIB) < os.path.getmtime(src):
        subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", "-o", _LIB, src, "-lm"])
    return _LIB


_lib = None


def _load():
    global _lib
    if _lib is None:
        build()
        _lib = C.CDLL(_LIB)
        _lib.js_encode.restype = C.c_size_t
        _lib.js_encode.argtypes = [C.POINTER(_Params), C.c_void_p, C.c_size_t]
        _lib.js_encode_blocks_opt.restype = C.c_size_t
        _lib.js_encode_blocks_opt.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
        _lib.js_encode_custom.restype = C.c_size_t
        _lib.js_encode_custom.argtypes = [C.POINTER(_Custom), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    return _lib


def encode_blocks(coef, blocks_x, q, restart_interval=0, optimize=False) -> bytes:
    """Grayscale JPEG whose data units are the given quantised coefficient blocks: `coef` int16 [n, 64] in
    natural order (n a multiple of blocks_x), `q` uint8 [64] natural order. Block b lands at block row
    b // blocks_x, column b % blocks_x. `optimize`: Huffman tables fitted to these blocks instead of Annex K's."""
    import numpy as np

    coef = np.ascontiguousarray(coef, dtype=np.int16).reshape(-1, 64)
    q = np.ascontiguousarray(q, dtype=np.uint8).reshape(64)
    n = len(coef)
    assert n % blocks_x == 0
    cap = 4096 + n * 64 * 4
    buf = C.create_string_buffer(cap)
    m = _load().js_encode_blocks_opt(coef.ctypes.data, blocks_x, n // blocks_x, q.ctypes.data, restart_interval, int(optimize), buf, cap)
    if m == 0:
        raise RuntimeError("jpegsynth: encode_blocks failed")
    return buf.raw[:m]


def encode_custom(width, height, sampling, blocks, dc_tables, ac_tables, tables=None, qtables=None, interleaved=True,
                  restart_interval=0) -> bytes:
    """A baseline JPEG of the given quantised blocks coded with the given Huffman tables.

    sampling: one (h, v) pair per component (1..4); blocks: per component int16 [blocks_y, blocks_x, 64], natural order,
    DC absolute, at least the component's blocks (whole MCUs of an interleaved scan); dc_tables / ac_tables: up to four
    (BITS, HUFFVAL) pairs each, BITS 16 counts of codes per length; tables: (dc id, ac id) per component, default the
    component index; qtables: up to four uint8 [64] natural order; component c uses qtables[c] if there is one, else
    table 0 (all ones when qtables is None).
    interleaved=False: one scan per component. Raises if a symbol the blocks need has no code."""
    import numpy as np

    nc = len(sampling)
    assert 1 <= nc <= 4 and len(blocks) == nc
    p = _Custom()
    p.width, p.height, p.ncomp = width, height, nc
    p.interleaved, p.restart_interval = int(interleaved), restart_interval
    tables = tables or [(c, c) for c in range(nc)]
    keep = []
    ptrs = (C.c_void_p * 4)()
    for c, (h, v) in enumerate(sampling):
        b = np.ascontiguousarray(blocks[c], dtype=np.int16)
        assert b.ndim == 3 and b.shape[2] == 64
        keep.append(b)
        ptrs[c] = b.ctypes.data
        p.hs[c], p.vs[c], p.bh[c], p.bw[c] = h, v, b.shape[0], b.shape[1]
        p.dc_tab[c], p.ac_tab[c] = tables[c]
        p.q_tab[c] = c if qtables is not None and len(qtables) > c else 0
    tabs = np.zeros((8, 272), np.uint8)
    for k, (bits, vals) in enumerate(list(dc_tables)[:4]):
        tabs[k, :16], tabs[k, 16:16 + len(vals)] = bits, vals
    for k, (bits, vals) in enumerate(list(ac_tables)[:4]):
        tabs[4 + k, :16], tabs[4 + k, 16:16 + len(vals)] = bits, vals
    q = np.ones((4, 64), np.uint8)
    for k, t in enumerate(qtables or []):
        q[k] = t
    cap = 4096 + sum(b.size for b in keep) * 4
    buf = C.create_string_buffer(cap)
    n = _load().js_encode_custom(C.byref(p), ptrs, tabs.ctypes.data, q.ctypes.data, buf, cap)
    if n == 0:
        raise RuntimeError("jpegsynth: encode_custom failed (bad parameters, a symbol without a code, or a full buffer)")
    return buf.raw[:n]


def encode(width, height, sampling=((2, 2), (1, 1), (1, 1)), interleaved=True, restart_interval=0,
           quality=75, optimize=False, noise=6, fill_bytes=0, seed=0, qmax=0) -> bytes:
    """sampling: one (h, v) pair per component (1..4 components)."""
    _load()
    p = _Params()
    p.width, p.height, p.ncomp = width, height, len(sampling)
    for c, (h, v) in enumerate(sampling):
        p.hs[c], p.vs[c] = h, v
    p.interleaved, p.restart_interval, p.quality = int(interleaved), restart_interval, quality
    p.optimize, p.noise, p.fill_bytes, p.seed, p.qmax = int(optimize), noise, fill_bytes, seed, qmax
    cap = 1024 + width * height * len(sampling) * 3
    buf = C.create_string_buffer(cap)
    n = _lib.js_encode(C.byref(p), buf, cap)
    if n == 0:
        raise RuntimeError("jpegsynth: encode failed (bad parameters or buffer too small)")
    return buf.raw[:n]


# The five BASELINE.json configurations, at full size and at a reduced size for oracle-speed tests.
def config(idx: int, seed: int = 0, small: bool = False) -> bytes:
    if idx in (1, 2, 3):  # 12 MP 4:2:0 interleaved, one restart interval per MCU row
        w, h = (4032, 3024) if not small else (496, 360)
        return encode(w, h, ((2, 2), (1, 1), (1, 1)), True, (w + 15) // 16, quality=88, noise=9, seed=seed)
    if idx == 4:  # 39 MP 4:4:4, three single-component scans, no restart markers
        w, h = (7216, 5408) if not small else (456, 344)
        return encode(w, h, ((1, 1), (1, 1), (1, 1)), False, 0, quality=80, noise=6, seed=seed)
    if idx == 5:  # 4 components (2x1,1x1,1x1,2x1), 4 DC + 4 AC tables, no restart markers
        w, h = (4032, 3024) if not small else (504, 376)
        return encode(w, h, ((2, 1), (1, 1), (1, 1), (2, 1)), True, 0, quality=85, optimize=True, noise=6, seed=seed)
    raise ValueError(idx)
