"""CPU restatement of the lossless transcode with a crop (jpeggpu_ext_set_transcode_crop; jpeggpu_amd.transcode_jpeg(...,
crops=, expand=)): jpegtran's -crop on the source's quantised coefficients, built on tests/transcode_orient_ref.py.

    target_geometry(w, h, hs, vs, o, trim) -> (W', H', hs', vs') of the UNCROPPED target: the trimmed source, turned
    checked(rect, W', H', hs', vs')  the library's rules on a rectangle (x, y, w, h) of that image: Invalid for a negative
                          value, an empty rectangle or one that leaves the image (JPEGGPU_INVALID_ARGUMENT), Unsupported for
                          an x or y that is no multiple of the target's iMCU (JPEGGPU_NOT_SUPPORTED)
    expanded(rect, hs', vs')  jpegtran's rule: x and y rounded down to the iMCU, w and h grown by what was cut
    source_rect(rect, W', H', o)  the rectangle of stored source pixels that `rect` shows
    transform(src, rect, o=1, trim=False, optimize=False, progressive=False, restart_interval=None) -> bytes. rect None: the
                          uncropped transform of transcode_orient_ref. Otherwise the oriented grids of the real blocks of the
                          (trimmed) source are sliced from block (x / 8, y / 8) of luma and (x / (8 hs'), y / (8 vs')) of
                          chroma on, to the real grid of a w x h image; the dummy blocks of that image are the encoder's (63
                          zeros and the DC of the block in front in the MCU's order) -- at orientation 1 and for a crop of
                          the whole image too; tables, sampling byte and restart interval as for the orientation alone; the
                          coding limits follow the cropped target's prediction order."""
import numpy as np

from tests import encode_ref as E
from tests import transcode_orient_ref as X
from tests import transcode_ref as R

Unsupported = X.Unsupported


class Invalid(ValueError):
    """What the library answers with JPEGGPU_INVALID_ARGUMENT."""


def target_geometry(w, h, hs, vs, o, trim=False):
    w, h = X.target_size(w, h, hs, vs, o, trim)
    if o in X.TRANSPOSED:
        if (hs, vs) == (2, 1):
            raise Unsupported("4:2:2 would become 4:4:0")
        return h, w, vs, hs
    return w, h, hs, vs


def checked(rect, tw, th, ths, tvs):
    x, y, w, h = rect
    if min(x, y, w, h) < 0 or w == 0 or h == 0:
        raise Invalid("a negative value or an empty rectangle")
    if x + w > tw or y + h > th:
        raise Invalid("the rectangle leaves the image")
    if x % (8 * ths) or y % (8 * tvs):
        raise Unsupported("the rectangle does not start on an iMCU boundary")
    return rect


def expanded(rect, ths, tvs):
    x, y, w, h = rect
    return x - x % (8 * ths), y - y % (8 * tvs), w + x % (8 * ths), h + y % (8 * tvs)


def source_rect(rect, tw, th, o):
    x, y, w, h = rect
    if o in X.MIRROR_X:
        x = tw - x - w
    if o in X.MIRROR_Y:
        y = th - y - h
    return (y, x, h, w) if o in X.TRANSPOSED else (x, y, w, h)


def transform(src, rect, orientation=1, trim=False, optimize=False, progressive=False, restart_interval=None):
    o = orientation
    if rect is None:
        return X.transform(src, o, trim, optimize, progressive, restart_interval)
    info = R._checked(src)
    nc, hs, vs = len(info["comps"]), info["hs"], info["vs"]
    sw, sh = X.target_size(info["w"], info["h"], hs, vs, o, trim)  # the trimmed source
    tw, th, ths, tvs = target_geometry(info["w"], info["h"], hs, vs, o, trim)
    x, y, w, h = checked(tuple(int(v) for v in rect), tw, th, ths, tvs)
    grids = X._grids(bytes(src), info["progressive"])
    out = []
    for c in range(nc):
        cw, ch = (sw, sh) if c == 0 else (-(-sw // hs), -(-sh // vs))
        g = X.orient_blocks(np.asarray(grids[c], np.int64)[:-(-ch // 8), :-(-cw // 8)], o)  # the uncropped target's real blocks
        ox, oy = (x // 8, y // 8) if c == 0 else (x // (8 * ths), y // (8 * tvs))
        nx, ny = (-(-w // 8), -(-h // 8)) if c == 0 else (-(-(-(-w // ths)) // 8), -(-(-(-h // tvs)) // 8))
        assert oy + ny <= g.shape[0] and ox + nx <= g.shape[1]
        out.append(g[oy:oy + ny, ox:ox + nx])
    hs, vs = ths, tvs
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
    if o in X.TRANSPOSED:
        tabs = [t.reshape(8, 8).T.reshape(64) for t in tabs]
    byte = info["comps"][0]["sampling"]
    if o in X.TRANSPOSED:
        byte = (byte << 4 | byte >> 4) & 0xFF
    return X._encode(co, tabs, ("cropped", byte), (byte >> 4, byte & 15), r, optimize, progressive)
