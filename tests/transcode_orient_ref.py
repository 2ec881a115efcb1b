"""CPU restatement of the lossless transcode with an orientation (jpeggpu_ext_set_transcode_orientation;
jpeggpu_amd.transcode_jpeg(..., orientation=, trim=)): jpegtran's -flip, -rotate, -transpose and -transverse on the
source's quantised coefficients, built on tests/transcode_ref.py and the three restatements of the encoder as
transcode_ref.transcode is.

    orient_pixels(a, o)   the DISPLAYED image of the stored image `a` (H x W [x C]) under EXIF orientation o, by the table at
                          jpeggpu_ext_get_orientation:  O[y][x] = S[...]
    orient_blocks(g, o)   the same in the coefficient domain: `g` [by, bx, 64] (natural order) -> the target's grid. A real
                          block of the target is the source's block under the table, taken on block grids; 5..8 transpose the
                          block (natural index 8 v + u takes the source's 8 u + v); a mirrored displayed x (2, 3, 6, 7)
                          negates odd horizontal frequencies u, a mirrored displayed y (3, 4, 7, 8) odd v
    target_size(w, h, hs, vs, o, trim) -> (w', h') of the trimmed SOURCE; Unsupported by the edge rules: the stored x is
                          mirrored for 2, 3, 7, 8 (w a multiple of 8 hs), the stored y for 3, 4, 6, 7 (h of 8 vs); `trim`
                          cuts to the largest such multiple, and an axis below one iMCU stays refused
    transform(src, o, trim=False, optimize=False, progressive=False, restart_interval=None) -> bytes. With o == 1 it is
                          transcode_ref.transcode (the source's dummy blocks are kept). Otherwise the dummy blocks of the
                          target are the encoder's (63 zeros and the DC of the block in front in the MCU's order), both
                          quantisation tables are transposed for 5..8, the size becomes H x W, luma's factors swap (4:2:2 is
                          refused there: it would be 4:4:0) and a grey file's sampling byte has its nibbles exchanged.
                          Unsupported where the library refuses or marks the item uncodable; the coding limits follow the
                          TARGET's prediction order."""
import functools

import numpy as np

from oracle import oracle
from tests import encode_opt_ref as O
from tests import encode_prog_ref as G
from tests import encode_ref as E
from tests import progressive_ref as P
from tests import transcode_ref as R

Unsupported = R.Unsupported
TRANSPOSED = (5, 6, 7, 8)
MIRROR_X = (2, 3, 6, 7)  # of the DISPLAYED axes
MIRROR_Y = (3, 4, 7, 8)
STORED_X = (2, 3, 7, 8)  # of the source's stored axes: what the edge rules are about
STORED_Y = (3, 4, 6, 7)
INVERSE = {1: 1, 2: 2, 3: 3, 4: 4, 5: 5, 6: 8, 7: 7, 8: 6}


def orient_pixels(a, o):
    a = np.asarray(a)
    if o in TRANSPOSED:  # O = T mirrored, T[y][x] = S[x][y]
        a = np.swapaxes(a, 0, 1)
    if o in MIRROR_X:
        a = a[:, ::-1]
    if o in MIRROR_Y:
        a = a[::-1]
    return a


def orient_blocks(g, o):
    by, bx = g.shape[:2]
    g = np.asarray(g).reshape(by, bx, 8, 8)  # [.., v, u]
    if o in TRANSPOSED:
        g = g.transpose(1, 0, 3, 2)
    sign = np.ones((8, 8), np.int64)
    if o in MIRROR_X:
        g = g[:, ::-1]
        sign[:, 1::2] *= -1
    if o in MIRROR_Y:
        g = g[::-1]
        sign[1::2, :] *= -1
    return (g * sign).reshape(g.shape[0], g.shape[1], 64)


def target_size(w, h, hs, vs, o, trim=False):
    if o not in range(1, 9):
        raise ValueError("orientation")
    for axis, stored in ((0, STORED_X), (1, STORED_Y)):
        size, unit = (w, 8 * hs) if axis == 0 else (h, 8 * vs)
        if o in stored and size % unit:
            if not trim or size < unit:
                raise Unsupported("a mirrored edge with a partial iMCU")
            size -= size % unit
        w, h = (size, h) if axis == 0 else (w, size)
    return w, h


def _encode(co, tabs, subsampling, factors, r, optimize, progressive):
    """The file of a `coefficients` dict behind a header with the tables `tabs` (natural order) and the sampling byte that
    `factors` gives component 0, as transcode_ref.transcode codes it."""
    saved = E.coefficients, E.quant_table
    try:  # the three encoders read these through the module when they are called
        E.coefficients = lambda *a, **k: co
        E.quant_table = lambda base, quality: tabs[0] if base is E.BASE_LUMA else tabs[-1]
        E.SUBSAMPLINGS[subsampling] = factors
        if progressive:
            return G.encode(None, None, subsampling, r)
        if optimize:
            return O.encode(None, None, subsampling, r)
        return E.encode(None, None, subsampling, r)
    finally:
        E.coefficients, E.quant_table = saved
        del E.SUBSAMPLINGS[subsampling]


@functools.lru_cache(maxsize=32)
def _grids(src, progressive):
    """The source's coefficient arrays [by, bx, 64] in natural order, per component (decoded once per source)."""
    return tuple(np.asarray(g, np.int64) for g in (P.decode(src).coef if progressive else oracle.decode(src).coef))


def transform(src, orientation, trim=False, optimize=False, progressive=False, restart_interval=None):
    o = orientation
    info = R._checked(src)
    nc, hs, vs = len(info["comps"]), info["hs"], info["vs"]
    w, h = target_size(info["w"], info["h"], hs, vs, o, trim)
    if o in TRANSPOSED and (hs, vs) == (2, 1):
        raise Unsupported("4:2:2 would become 4:4:0")
    if o == 1:
        return R.transcode(src, optimize, progressive, restart_interval)
    grids = _grids(bytes(src), info["progressive"])
    out = []
    for c in range(nc):
        cw, ch = (w, h) if c == 0 else (-(-w // hs), -(-h // vs))
        out.append(orient_blocks(np.asarray(grids[c], np.int64)[:-(-ch // 8), :-(-cw // 8)], o))  # the real blocks of the trimmed source
    if o in TRANSPOSED:
        w, h, hs, vs = h, w, vs, hs
    _, _, mx, my, per_mcu = E.geometry(w, h, nc, hs, vs)
    n = mx * my * per_mcu
    coefs, comp, dummy = np.zeros((n, 64), np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    gw, gh = -(-w // 8), -(-h // 8)
    assert out[0].shape[:2] == (gh, gw) and all(g.shape[:2] == (my, mx) for g in out[1:])
    k = 0
    for m in range(mx * my):
        ymcu, xmcu = divmod(m, mx)
        for yo in range(vs):
            for xo in range(hs):
                bx, by = xmcu * hs + xo, ymcu * vs + yo
                if bx < gw and by < gh:
                    coefs[k] = out[0][by, bx][E.ZIGZAG]
                else:  # the encoder's dummy block (tests/encode_ref.py, jccoefct.c)
                    coefs[k, 0] = coefs[k - 1, 0]
                    dummy[k] = (1 if bx >= gw else 0) | (2 if by >= gh else 0)
                k += 1
        for c in range(1, nc):
            coefs[k], comp[k] = out[c][ymcu, xmcu][E.ZIGZAG], c
            k += 1
    co = dict(coefs=coefs.astype(np.int16), comp=comp, mcu=np.repeat(np.arange(mx * my), per_mcu), dummy=dummy, w=w, h=h, ncomp=nc, hs=hs, vs=vs,
              mcus_x=mx, mcus_y=my, per_mcu=per_mcu, quality=None)
    if np.abs(coefs[:, 1:]).max(initial=0) >= 1024:
        raise Unsupported("an AC coefficient of category above 10")
    r = info["restart"] if restart_interval is None else restart_interval
    if np.abs(R.dc_differences(co, r)).max(initial=0) >= 2048:
        raise Unsupported("a DC difference of category above 11")
    inverse = np.argsort(E.ZIGZAG)
    tabs = [np.array(info["qtabs"][c["q"]])[inverse] for c in info["comps"][:2]]
    if o in TRANSPOSED:
        tabs = [t.reshape(8, 8).T.reshape(64) for t in tabs]
    byte = info["comps"][0]["sampling"]
    if o in TRANSPOSED:
        byte = (byte << 4 | byte >> 4) & 0xFF
    return _encode(co, tabs, ("oriented", byte), (byte >> 4, byte & 15), r, optimize, progressive)
