"""CPU restatement of the lossless transcode that keeps the SOURCE's frame layout (jpeggpu_ext_set_transcode_frame(SOURCE);
jpeggpu_amd.transcode_jpeg(..., frame="source")): the file libjpeg writes after jpeg_copy_critical_parameters, as jpegtran
does, for any sampling factors, one to four components, up to four quantisation tables of 8 or 16 bits and every colour
model the decoder tells apart. Built on the earlier restatements, which it imports and does not change.

    parse(src)            transcode_ref.parse and the colour model by libjpeg's rules (jdapimin.c): "grey", "ycbcr", "rgb",
                          "cmyk", "ycck", "unknown"
    in_encoder_range(src, info, orientation)   the file is one the other mode takes, numbered as the encoder numbers its tables:
                          then SOURCE mode gives the other mode's bytes (transcode_crop_ref.transform)
    header(info, w, h, factors, tables, restart, dhts, sof) -> SOI .. SOS by the rules of jpeggpu_ext.h
    mcu_stream(grids, factors, w, h, mapped)   the `coefficients` dict of tests/encode_ref.py for any layout: the
                          components' blocks of an MCU one after the other, each h x v row by row. A block beyond its
                          component's real grid is, for an unmapped item, the source's where the grid holds it and zeros
                          where not; for a mapped one 63 zeros and the DC of the block in front of it in the MCU
    transcode(src, optimize=False, progressive=False, restart_interval=None, orientation=1, trim=False, crop=None) -> bytes;
                          Unsupported for what the library refuses or marks uncodable. `progressive`: three-component
                          YCbCr keeps libjpeg's ten scans, a single component the six, everything else gets
                          jpeg_simple_progression's all-purpose script of 2 + 4 n scans (script, progressive_file)"""
import numpy as np

from oracle import oracle
from tests import encode_opt_ref as O
from tests import encode_prog_ref as G
from tests import encode_ref as E
from tests import progressive_ref as P
from tests import transcode_crop_ref as C
from tests import transcode_orient_ref as X
from tests import transcode_ref as R
from tests.progressive_ref import script_pillow_like

Unsupported = R.Unsupported
Invalid = C.Invalid


def parse(src):
    info = R.parse(src)
    jfif = adobe = None
    i = 2
    while src[i + 1] != 0xDA:
        n = src[i + 2] << 8 | src[i + 3]
        seg = src[i + 4:i + 2 + n]
        if src[i + 1] == 0xE0 and seg[:5] == b"JFIF\0":
            jfif = True
        if src[i + 1] == 0xEE and seg[:5] == b"Adobe" and len(seg) >= 12:
            adobe = seg[11]
        i += 2 + n
    ids = bytes(c["id"] for c in info["comps"])
    nc = len(ids)
    if nc == 1:
        cs = "grey"
    elif nc == 3:
        cs = "ycbcr" if jfif else ("rgb" if adobe == 0 else "ycbcr") if adobe is not None else "rgb" if ids == b"RGB" else "ycbcr"
    elif nc == 4:
        cs = "cmyk" if adobe in (None, 0) else "ycck"
    else:
        cs = "unknown"
    info["color"] = cs
    info["factors"] = [(c["sampling"] >> 4, c["sampling"] & 15) if nc > 1 else (1, 1) for c in info["comps"]]
    return info


def in_encoder_range(src, info, orientation=1):
    try:
        R._checked(src)
    except Unsupported:
        return False
    if info["color"] not in ("grey", "ycbcr"):
        return False
    if any(v > 255 for c in info["comps"] for v in info["qtabs"][c["q"]]):
        return False
    return not (orientation in X.TRANSPOSED and info["factors"][0] == (2, 1) and len(info["comps"]) == 3)


def _ids(cs, nc):
    return {"grey": [1], "ycbcr": [1, 2, 3], "rgb": list(b"RGB"), "cmyk": list(b"CMYK"), "ycck": [1, 2, 3, 4]}.get(cs, list(range(nc)))


def selectors(cs, nc):
    return [1 if cs in ("ycbcr", "ycck") and c in (1, 2) else 0 for c in range(nc)]


def _segment(out, marker, payload):
    out += bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def header(info, w, h, bytes_, tables, restart, dhts=None, progressive=False):
    """SOI .. SOS. bytes_: the sampling byte per component; tables: {number: 64 zigzag values}; dhts: (DC0, AC0, DC1, AC1)
    as (bits, values), None: Annex K's. progressive: SOI .. SOF2 only."""
    cs, nc = info["color"], len(info["comps"])
    out = bytearray(b"\xff\xd8")
    if cs in ("grey", "ycbcr"):
        _segment(out, 0xE0, b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    elif cs in ("rgb", "cmyk", "ycck"):
        _segment(out, 0xEE, b"Adobe\0\x64\0\0\0\0" + bytes([2 if cs == "ycck" else 0]))
    sent, wide = [], False
    for c in info["comps"]:
        if c["q"] in sent:
            continue
        sent.append(c["q"])
        t = [int(v) for v in tables[c["q"]]]
        if max(t) > 255:
            wide = True
            _segment(out, 0xDB, bytes([0x10 | c["q"]]) + b"".join(v.to_bytes(2, "big") for v in t))
        else:
            _segment(out, 0xDB, bytes([c["q"]]) + bytes(t))
    ids, sel = _ids(cs, nc), selectors(cs, nc)
    sof = bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([nc])
    for c in range(nc):
        sof += bytes([ids[c], bytes_[c], info["comps"][c]["q"]])
    _segment(out, 0xC2 if progressive else 0xC1 if wide else 0xC0, sof)
    if progressive:
        return bytes(out)
    dhts = dhts or (E.DC_LUMA, E.AC_LUMA, E.DC_CHROMA, E.AC_CHROMA)
    for cls_id, table in ((0x00, dhts[0]), (0x10, dhts[1]), (0x01, dhts[2]), (0x11, dhts[3]))[:4 if any(sel) else 2]:
        _segment(out, 0xC4, bytes([cls_id]) + bytes(table[0]) + bytes(table[1]))
    if restart:
        _segment(out, 0xDD, restart.to_bytes(2, "big"))
    sos = bytes([nc])
    for c in range(nc):
        sos += bytes([ids[c], 0x11 if sel[c] else 0x00])
    _segment(out, 0xDA, sos + b"\x00\x3f\x00")
    return bytes(out)


def comp_blocks(pixels, f, fmax):
    """The real blocks along one axis of a component with factor f in a frame of `pixels` whose largest factor is fmax."""
    return -(-(-(-pixels * f // fmax)) // 8)


def mcu_stream(grids, factors, w, h, mapped):
    """grids[c]: [by, bx, 64] natural order, at least the component's real blocks (an unmapped item: whatever the source's
    scans code beyond them too)."""
    nc = len(factors)
    hmax, vmax = max(f[0] for f in factors), max(f[1] for f in factors)
    mx, my = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    per_mcu = sum(f[0] * f[1] for f in factors)
    n = mx * my * per_mcu
    coefs, comp, dummy = np.zeros((n, 64), np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    k = 0
    for m in range(mx * my):
        ymcu, xmcu = divmod(m, mx)
        for c, (fh, fv) in enumerate(factors):
            g = grids[c]
            gw, gh = comp_blocks(w, fh, hmax), comp_blocks(h, fv, vmax)
            for yo in range(fv):
                for xo in range(fh):
                    bx, by = xmcu * fh + xo, ymcu * fv + yo
                    comp[k] = c
                    if bx < gw and by < gh:
                        coefs[k] = g[by, bx][E.ZIGZAG]
                    else:
                        dummy[k] = (1 if bx >= gw else 0) | (2 if by >= gh else 0)
                        if mapped:  # the encoder's dummy block: the block in front is the component's, a dummy never opens one
                            assert xo or yo
                            coefs[k, 0] = coefs[k - 1, 0]
                        elif by < g.shape[0] and bx < g.shape[1]:
                            coefs[k] = g[by, bx][E.ZIGZAG]
                    k += 1
    return dict(coefs=coefs.astype(np.int16), comp=comp, mcu=np.repeat(np.arange(mx * my), per_mcu), dummy=dummy, w=w, h=h, ncomp=nc,
                mcus_x=mx, mcus_y=my, per_mcu=per_mcu, quality=None)


def entropy(co, select, restart, optimize):
    """(DHT tables, entropy-coded bytes): the coders of encode_ref and encode_opt_ref on DC differences made here, so that
    their rule "component 0 is table 0, every other table 1" never applies: `comp` becomes the block's selector and no
    component is left for them to predict."""
    d = dict(co)
    coefs = co["coefs"].astype(np.int64).copy()
    coefs[:, 0] = R.dc_differences(co, restart)
    d["coefs"], d["comp"], d["ncomp"] = coefs, np.asarray(select, np.int64)[co["comp"]], 0
    saved = E.DC_LUMA, E.AC_LUMA, E.DC_CHROMA, E.AC_CHROMA
    try:
        if optimize:
            dhts = O.tables_of_counts(O.symbol_counts(d, restart), 3 if any(select) else 1)
            E.DC_LUMA, E.AC_LUMA = dhts[0], dhts[1]
            if dhts[2] is not None:
                E.DC_CHROMA, E.AC_CHROMA = dhts[2], dhts[3]
        dhts = (E.DC_LUMA, E.AC_LUMA, E.DC_CHROMA, E.AC_CHROMA)
        return dhts, E.entropy_code(d, restart)
    finally:
        E.DC_LUMA, E.AC_LUMA, E.DC_CHROMA, E.AC_CHROMA = saved


def script(cs, nc):
    """jpeg_simple_progression: (components, Ss, Se, Ah, Al) per scan."""
    if nc == 1 or (nc == 3 and cs == "ycbcr"):
        return script_pillow_like(nc)
    every = tuple(range(nc))
    out = [(every, 0, 0, 0, 1)]
    out += [((c,), 1, 5, 0, 2) for c in every] + [((c,), 6, 63, 0, 2) for c in every] + [((c,), 1, 63, 2, 1) for c in every]
    out += [(every, 0, 0, 1, 0)]
    return out + [((c,), 1, 63, 1, 0) for c in every]


def progressive_file(info, co, factors, w, h, bytes_, tables, restart):
    """jcphuff.c on the script over any layout: an interleaved scan walks the MCU stream, a component's own scan its real
    blocks row by row; every scan brings the tables its symbols need, numbered by its components' selectors."""
    cs, nc = info["color"], len(factors)
    ids, sel = _ids(cs, nc), selectors(cs, nc)
    hmax, vmax = max(f[0] for f in factors), max(f[1] for f in factors)
    coefs, comp, per_mcu, mx = co["coefs"].astype(np.int64), co["comp"], co["per_mcu"], co["mcus_x"]
    k0 = np.cumsum([0] + [f[0] * f[1] for f in factors])
    st = dict(scans=[], cap_flushes=0, be_flushes=0, max_run=0, refine_zrl=0, refine_long_tail=0)
    out = bytearray(header(info, w, h, bytes_, tables, restart, progressive=True))
    for number, (comps, ss, se, ah, al) in enumerate(script(cs, nc)):
        if len(comps) > 1:
            order, step = np.arange(coefs.shape[0]), per_mcu
        else:
            fh, fv = factors[comps[0]]
            by, bx = np.mgrid[0:comp_blocks(h, fv, vmax), 0:comp_blocks(w, fh, hmax)]
            order, step = (((by // fv) * mx + bx // fh) * per_mcu + k0[comps[0]] + (by % fv) * fh + bx % fh).ravel(), 1
        step = restart * step if restart else len(order)
        segments = []
        for a in range(0, len(order), step):
            part = order[a:a + step]
            if ss:
                segments.append(G._segment_events(co, coefs, part, comp, (comps, ss, se, ah, al), st))
                continue
            events, pred = [], {}
            for i in part:
                v = int(coefs[i, 0]) >> al
                if ah:
                    events.append((-1, v & 1, 1))
                    continue
                d = v - pred.get(comp[i], 0)
                pred[comp[i]] = v
                n = int(abs(d)).bit_length()
                events.append((0, n | (0x100 if sel[comp[i]] else 0), 0))
                if n:
                    events.append((-1, (d - 1 if d < 0 else d) & ((1 << n) - 1), n))
            segments.append(events)
        counts = {}
        for seg in segments:
            for e in seg:
                if e[0] >= 0:
                    key = (e[0], (e[1] >> 8) if ss == 0 else sel[comps[0]], e[1] & 0xFF)
                    counts[key] = counts.get(key, 0) + 1
        codes = {}
        for cls, tid in sorted({k[:2] for k in counts}):
            freq = np.zeros(256, np.int64)
            for (c, t, sym), v in counts.items():
                if (c, t) == (cls, tid):
                    freq[sym] = v
            bits, values, status = O.gen_optimal_table(freq)
            if status == O.OVERFLOW:
                raise O.TableOverflow("scan %d class %d table %d" % (number, cls, tid))
            _segment(out, 0xC4, bytes([cls << 4 | tid]) + bytes(bits) + bytes(values))
            for sym, cl in E.huff_codes((bits, values)).items():
                codes[cls, sym | (0x100 if ss == 0 and tid else 0)] = cl
        if number == 0 and restart:
            _segment(out, 0xDD, restart.to_bytes(2, "big"))
        sos = bytes([len(comps)])
        for c in comps:
            sos += bytes([ids[c], (sel[c] << 4 if ah == 0 else 0) if ss == 0 else sel[c]])
        _segment(out, 0xDA, sos + bytes([ss, se, ah << 4 | al]))
        for i, seg in enumerate(segments):
            if i:
                out += bytes([0xFF, 0xD0 + (i - 1) % 8])
            out += G._pack(seg, codes)
    return bytes(out) + b"\xff\xd9"


def source_grids(src, info):
    return [np.asarray(g, np.int64) for g in (P.decode(src).coef if info["progressive"] else oracle.decode(src).coef)]


def target_geometry(info, o, trim=False):
    """(w, h) of the trimmed SOURCE, (W', H') and the factors of the uncropped target; the edge rules on the iMCU."""
    factors = info["factors"]
    hmax, vmax = max(f[0] for f in factors), max(f[1] for f in factors)
    w, h = X.target_size(info["w"], info["h"], hmax, vmax, o, trim)
    if o in X.TRANSPOSED:
        return (w, h), (h, w), [(f[1], f[0]) for f in factors]
    return (w, h), (w, h), list(factors)


def transcode(src, optimize=False, progressive=False, restart_interval=None, orientation=1, trim=False, crop=None):
    src = bytes(src)
    info = parse(src)
    o = orientation
    if in_encoder_range(src, info, o):
        return C.transform(src, crop, o, trim, optimize, progressive, restart_interval)
    nc = len(info["comps"])
    (w, h), (tw, th), tf = target_geometry(info, o, trim)
    hmax, vmax = max(f[0] for f in info["factors"]), max(f[1] for f in info["factors"])
    thmax, tvmax = max(f[0] for f in tf), max(f[1] for f in tf)
    grids = source_grids(src, info)
    mapped = o != 1 or crop is not None
    if mapped:
        out = []
        for c, (fh, fv) in enumerate(info["factors"]):
            g = grids[c][:comp_blocks(h, fv, vmax), :comp_blocks(w, fh, hmax)]  # the real blocks of the trimmed source
            out.append(X.orient_blocks(g, o) if o != 1 else g)
        grids = out
        if crop is not None:
            x, y, cw, ch = C.checked(crop, tw, th, thmax, tvmax)
            grids = [g[y // (8 * tvmax) * f[1]:, x // (8 * thmax) * f[0]:] for g, f in zip(grids, tf)]
            tw, th = cw, ch
    co = mcu_stream(grids, tf, tw, th, mapped)
    if np.abs(co["coefs"][:, 1:].astype(np.int64)).max(initial=0) >= 1024:
        raise Unsupported("an AC coefficient of category above 10")
    r = info["restart"] if restart_interval is None else restart_interval
    if np.abs(R.dc_differences(co, r)).max(initial=0) >= 2048:
        raise Unsupported("a DC difference of category above 11")
    tables = {}
    inverse = np.argsort(E.ZIGZAG)
    for c in info["comps"]:
        t = np.array(info["qtabs"][c["q"]])
        if o in X.TRANSPOSED:
            t = t[inverse].reshape(8, 8).T.reshape(64)[E.ZIGZAG]
        tables[c["q"]] = t
    bytes_ = [f[0] << 4 | f[1] for f in tf]
    if nc == 1:  # written back as it came, the nibbles exchanged with the axes
        b = info["comps"][0]["sampling"]
        bytes_ = [(b << 4 | b >> 4) & 0xFF if o in X.TRANSPOSED else b]
    if progressive:
        return progressive_file(info, co, tf, tw, th, bytes_, tables, r)
    dhts, data = entropy(co, selectors(info["color"], nc), r, optimize)
    return header(info, tw, th, bytes_, tables, r, dhts) + data + b"\xff\xd9"
