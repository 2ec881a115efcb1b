"""CPU restatement of the lossless transcode (jpeggpu_amd.transcode_jpeg): the source's quantised coefficients -- the
oracle's for a baseline file, tests/progressive_ref's for a progressive one -- as the `coefficients` dict of
tests/encode_ref.py, coded by the three restatements of the encoder (encode_ref, encode_opt_ref, encode_prog_ref) behind a
header that holds the source's quantisation tables. It equals Pillow on every pin (tests/test_transcode_ref.py) and is the
reference for sources Pillow cannot write.

    parse(src) -> what the header says: size, components (sampling byte, table), tables, the DRI at the first scan
    coefficients(src) -> the dict; a dummy block keeps the source's values where a scan of the source codes it (an
                         interleaved scan, a progressive file's interleaved DC scans) and is 64 zeros where none does
    transcode(src, optimize=False, progressive=False, restart_interval=None) -> bytes; Unsupported for what the library
                         refuses or marks uncodable: an AC coefficient of magnitude 1024 or more, a DC difference -- in the
                         TARGET's prediction order, per component, from 0 at every `restart_interval` MCUs -- of 2048 or more"""
import numpy as np

from oracle import oracle
from tests import encode_opt_ref as O
from tests import encode_prog_ref as G
from tests import encode_ref as E
from tests import progressive_ref as P

GREY_SUBSAMPLING = {0x11: "4:4:4", 0x21: "4:2:2", 0x22: "4:2:0"}
COLOUR_SUBSAMPLING = {(1, 1): "4:4:4", (2, 1): "4:2:2", (2, 2): "4:2:0"}


class Unsupported(ValueError):
    pass


def parse(src):
    out = dict(qtabs={}, pq={}, restart=0, progressive=False)
    i = 2
    while True:
        assert src[i] == 0xFF
        m = src[i + 1]
        if m == 0xFF:
            i += 1
            continue
        n = src[i + 2] << 8 | src[i + 3]
        seg = src[i + 4:i + 2 + n]
        i += 2 + n
        if m in (0xC0, 0xC1, 0xC2):
            out["progressive"] = m == 0xC2
            out["h"], out["w"], nc = seg[1] << 8 | seg[2], seg[3] << 8 | seg[4], seg[5]
            out["comps"] = [dict(id=seg[6 + 3 * c], sampling=seg[7 + 3 * c], q=seg[8 + 3 * c]) for c in range(nc)]
        elif m == 0xDB:
            k = 0
            while k < len(seg):
                pq, t = seg[k] >> 4, seg[k] & 15
                size = 128 if pq else 64
                vals = [seg[k + 1 + 2 * j] << 8 | seg[k + 2 + 2 * j] for j in range(64)] if pq else list(seg[k + 1:k + 65])
                out["qtabs"][t], out["pq"][t] = vals, pq  # zigzag order, as the file holds them
                k += 1 + size
        elif m == 0xDD:
            out["restart"] = seg[0] << 8 | seg[1]
        elif m == 0xDA:
            return out


def _checked(src):
    info = parse(src)
    comps = info["comps"]
    if len(comps) == 3:
        f = [(c["sampling"] >> 4, c["sampling"] & 15) for c in comps]
        if f[1] != (1, 1) or f[2] != (1, 1) or f[0] not in COLOUR_SUBSAMPLING or comps[1]["q"] != comps[2]["q"]:
            raise Unsupported("sampling or tables")
        info["subsampling"], info["hs"], info["vs"] = COLOUR_SUBSAMPLING[f[0]], f[0][0], f[0][1]
    elif len(comps) == 1:
        if comps[0]["sampling"] not in GREY_SUBSAMPLING:
            raise Unsupported("the restatements write three sampling bytes for grey")
        info["subsampling"], info["hs"], info["vs"] = GREY_SUBSAMPLING[comps[0]["sampling"]], 1, 1
    else:
        raise Unsupported("components")
    if any(info["pq"][c["q"]] for c in comps):
        raise Unsupported("Pq = 1")
    return info


def coefficients(src, info=None):
    info = info or _checked(src)
    nc, w, h, hs, vs = len(info["comps"]), info["w"], info["h"], info["hs"], info["vs"]
    grids = P.decode(src).coef if info["progressive"] else oracle.decode(src).coef  # [by, bx, 64], natural order
    _, _, mx, my, per_mcu = E.geometry(w, h, nc, hs, vs)
    n = mx * my * per_mcu
    coefs, comp = np.zeros((n, 64), np.int64), np.zeros(n, np.int64)
    gw, gh = -(-w // 8), -(-h // 8)
    dummy = np.zeros(n, np.int64)

    def block(c, by, bx):
        g = grids[c]
        return g[by, bx][E.ZIGZAG] if by < g.shape[0] and bx < g.shape[1] else np.zeros(64, np.int64)

    k = 0
    for m in range(mx * my):
        ymcu, xmcu = divmod(m, mx)
        for yo in range(vs):
            for xo in range(hs):
                bx, by = xmcu * hs + xo, ymcu * vs + yo
                coefs[k] = block(0, by, bx)
                dummy[k] = (1 if bx >= gw else 0) | (2 if by >= gh else 0)
                k += 1
        for c in range(1, nc):
            coefs[k], comp[k] = block(c, ymcu, xmcu), c
            k += 1
    return dict(coefs=coefs.astype(np.int16), comp=comp, mcu=np.repeat(np.arange(mx * my), per_mcu), dummy=dummy, w=w, h=h, ncomp=nc, hs=hs, vs=vs,
                mcus_x=mx, mcus_y=my, per_mcu=per_mcu, quality=None)


def dc_differences(co, restart_interval):
    """The DC differences a target with that restart interval codes, per block of the MCU stream: each component predicts
    from its previous block, and from 0 in the first MCU of the file and of every `restart_interval` MCUs."""
    dc = co["coefs"][:, 0].astype(np.int64)
    out = np.zeros_like(dc)
    for c in range(co["ncomp"]):
        idx = np.flatnonzero(co["comp"] == c)
        d = dc[idx].copy()
        d[1:] -= dc[idx[:-1]]
        if restart_interval:
            mcu = co["mcu"][idx]
            opens = (mcu % restart_interval == 0) & np.r_[True, mcu[1:] != mcu[:-1]]  # the component's first block of such an MCU
            d[opens] = dc[idx][opens]
        out[idx] = d
    return out


def transcode(src, optimize=False, progressive=False, restart_interval=None):
    info = _checked(src)
    co = coefficients(src, info)
    if np.abs(co["coefs"][:, 1:].astype(np.int64)).max(initial=0) >= 1024:
        raise Unsupported("an AC coefficient of category above 10")
    r = info["restart"] if restart_interval is None else restart_interval
    if np.abs(dc_differences(co, r)).max(initial=0) >= 2048:  # whatever the target's first DC scan shifts away: jpeggpu_ext.h
        raise Unsupported("a DC difference of category above 11")
    inverse = np.argsort(E.ZIGZAG)
    tabs = [np.array(info["qtabs"][c["q"]])[inverse] for c in info["comps"][:2]]  # natural order, as quant_table returns them
    saved = E.coefficients, E.quant_table
    try:  # the three encoders read both through the module when they are called
        E.coefficients = lambda *a, **k: co
        E.quant_table = lambda base, quality: tabs[0] if base is E.BASE_LUMA else tabs[-1]
        if progressive:
            return G.encode(None, None, info["subsampling"], r)
        if optimize:
            return O.encode(None, None, info["subsampling"], r)
        return E.encode(None, None, info["subsampling"], r)
    finally:
        E.coefficients, E.quant_table = saved
