"""CPU restatement of the baseline JPEG encoder the library's encode calls implement: libjpeg-turbo's forward path (jccolor,
jcsample, jfdctint, the quantiser, jccoefct's dummy blocks, jchuff with the Annex K tables) in numpy, equal byte for byte to
Pillow's Image.fromarray(a).save(f, "JPEG", quality=q, subsampling=s, restart_marker_blocks=r) on libjpeg-turbo
(tests/golden/encode_pins.npz holds Pillow's files; tests/test_encode_ref.py compares).

    coefficients(img, hs, vs, quality)   quantised coefficients of every block in MCU stream order, zigzag order inside
    encode(img, quality, subsampling, restart_interval) -> bytes
    census(img, quality, subsampling, restart_interval) -> counts of the symbols and edge cases a stream exercises
"""
import numpy as np

# Annex K.1 / K.2, natural order
BASE_LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
             18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
BASE_CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32
# natural index of zigzag position k
ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]

# Annex K.3 - K.6: (bits[1..16], values)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1, 0x08,
    0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6,
    0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2,
    0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
    0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26,
    0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4,
    0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA,
    0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA])

SUBSAMPLINGS = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2), 0: (1, 1), 1: (2, 1), 2: (2, 2)}
PILLOW_SUBSAMPLING = {(1, 1): 0, (2, 1): 1, (2, 2): 2}


def quant_table(base, quality):
    """jpeg_set_quality's table (force_baseline), natural order."""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((np.asarray(base, np.int64) * s + 50) // 100, 1, 255).astype(np.int32)


def huff_codes(table):
    """{symbol: (code, length)} by Annex C."""
    bits, vals = table
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def huff_arrays(table):
    code, size = np.zeros(256, np.int64), np.zeros(256, np.int64)
    for s, (c, n) in huff_codes(table).items():
        code[s], size[s] = c, n
    return code, size


def geometry(w, h, ncomp, hs, vs):
    """MCU grid and per-component block layout of a scan: grey is one block per MCU."""
    if ncomp == 1:
        hs = vs = 1
    mx, my = -(-w // (8 * hs)), -(-h // (8 * vs))
    per_mcu = hs * vs + (2 if ncomp == 3 else 0)
    return hs, vs, mx, my, per_mcu


def _ycc(rgb):
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def _pad(p, rows, cols):
    return np.pad(p, ((0, rows - p.shape[0]), (0, cols - p.shape[1])), mode="edge")


def _downsample(p, hs, vs, w, h, mx, my, bottom_rule):
    """jcsample.c on one full-size component plane p (h x w): the plane of the MCU-padded block grid."""
    pw = mx * 8 * hs  # columns: the input row repeats its last sample up to the MCU-padded width
    if bottom_rule == "libjpeg":  # rows: the input only to a multiple of vs; the last DOWNSAMPLED row fills the grid
        p = _pad(p, -(-h // vs) * vs, pw)
    else:  # the simpler, wrong rule: the input padded to the MCU height first
        p = _pad(p, my * 8 * vs, pw)
    if (hs, vs) == (2, 1):
        bias = np.arange(p.shape[1] // 2) & 1
        p = (p[:, 0::2] + p[:, 1::2] + bias) >> 1
    elif (hs, vs) == (2, 2):
        bias = 1 + (np.arange(p.shape[1] // 2) & 1)
        p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
    return _pad(p, my * 8, p.shape[1])


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_1d(d, first):
    """One pass of jpeg_fdct_islow over the last axis."""
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., i] for i in range(8))
    t0, t7, t1, t6, t2, t5, t3, t4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    o = [None] * 8
    o[0] = (t10 + t11) << 2 if first else _descale(t10 + t11, 2)
    o[4] = (t10 - t11) << 2 if first else _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    o[2] = _descale(z1 + t13 * 6270, n)
    o[6] = _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = -z1 * 7373, -z2 * 20995, -z3 * 16069 + z5, -z4 * 3196 + z5
    o[7], o[5], o[3], o[1] = _descale(t4 + z1 + z3, n), _descale(t5 + z2 + z4, n), _descale(t6 + z2 + z3, n), _descale(t7 + z1 + z4, n)
    return np.stack(o, axis=-1)


def fdct_islow(blocks):
    """jpeg_fdct_islow of level-shifted blocks [..., 8 rows, 8 cols] (int64): 8 times the true DCT."""
    rows = _fdct_1d(blocks, True)
    return np.swapaxes(_fdct_1d(np.swapaxes(rows, -1, -2), False), -1, -2)


def quantise(c, q):
    d = 8 * q
    t = (np.abs(c) + (d >> 1)) // d
    return np.where(c < 0, -t, t)


def _plane_blocks(p, q):
    """Quantised coefficients [by, bx, 64] (zigzag order) of a plane whose sides are multiples of 8."""
    by, bx = p.shape[0] // 8, p.shape[1] // 8
    b = p.reshape(by, 8, bx, 8).swapaxes(1, 2).astype(np.int64) - 128
    c = quantise(fdct_islow(b).reshape(by, bx, 64), q.astype(np.int64))
    return c[..., ZIGZAG]


def coefficients(img, hs, vs, quality, bottom_rule="libjpeg"):
    """img: H x W x 3 (RGB) or H x W (grey) uint8. Returns a dict: `coefs` int16 [blocks, 64], MCU stream order, zigzag
    order inside a block, dummy blocks resolved (jccoefct.c); `comp` the component of each block; `mcu` its MCU; `dummy`
    0 for a real block, 1 right edge, 2 bottom edge, 3 both; plus the geometry."""
    img = np.asarray(img)
    h, w = img.shape[:2]
    ncomp = 1 if img.ndim == 2 else 3
    hs, vs, mx, my, per_mcu = geometry(w, h, ncomp, hs, vs)
    ql, qc = quant_table(BASE_LUMA, quality), quant_table(BASE_CHROMA, quality)
    if ncomp == 1:
        planes = [_pad(img.astype(np.int64), my * 8, mx * 8)]
    else:
        y, cb, cr = _ycc(img)
        planes = [_pad(y, my * 8 * vs, mx * 8 * hs)] + [_downsample(p, hs, vs, w, h, mx, my, bottom_rule) for p in (cb, cr)]
    grids = [_plane_blocks(planes[0], ql)] + [_plane_blocks(p, qc) for p in planes[1:]]
    gw, gh = -(-w // 8), -(-h // 8)  # the luma component's real blocks
    n = mx * my * per_mcu
    coefs, comp, dummy = np.zeros((n, 64), np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    mcu = np.repeat(np.arange(mx * my), per_mcu)
    k = 0
    for m in range(mx * my):
        ymcu, xmcu = divmod(m, mx)
        first = k
        for yo in range(vs):
            for xo in range(hs):
                bx, by = xmcu * hs + xo, ymcu * vs + yo
                if bx < gw and by < gh:
                    coefs[k] = grids[0][by, bx]
                else:  # 63 zeros and the DC of the block before it in the MCU's order
                    coefs[k, 0] = coefs[k - 1, 0]
                    dummy[k] = (1 if bx >= gw else 0) | (2 if by >= gh else 0)
                    assert k > first
                k += 1
        for c in range(1, ncomp):
            coefs[k], comp[k] = grids[c][ymcu, xmcu], c
            k += 1
    return dict(coefs=coefs.astype(np.int16), comp=comp, mcu=mcu, dummy=dummy, w=w, h=h, ncomp=ncomp, hs=hs, vs=vs, mcus_x=mx, mcus_y=my,
                per_mcu=per_mcu, quality=quality)


def _segment(buf, marker, payload):
    buf += bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload


def header(w, h, ncomp, hs, vs, quality, restart_interval):
    """SOI .. end of SOS, as libjpeg writes it for Pillow. A grey file's only component carries the sampling factors that
    were asked for (Pillow sets them whatever the mode); with one component they change nothing but that byte."""
    out = bytearray(b"\xff\xd8")
    _segment(out, 0xE0, b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for i, base in enumerate((BASE_LUMA, BASE_CHROMA)[:1 if ncomp == 1 else 2]):
        q = quant_table(base, quality)
        _segment(out, 0xDB, bytes([i]) + bytes(int(q[z]) for z in ZIGZAG))
    sof = bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([ncomp])
    for c in range(ncomp):
        sof += bytes([c + 1, (hs << 4 | vs) if c == 0 else 0x11, 0 if c == 0 else 1])
    _segment(out, 0xC0, sof)
    for cls_id, table in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA))[:2 if ncomp == 1 else 4]:
        _segment(out, 0xC4, bytes([cls_id]) + bytes(table[0]) + bytes(table[1]))
    if restart_interval:
        _segment(out, 0xDD, restart_interval.to_bytes(2, "big"))
    sos = bytes([ncomp])
    for c in range(ncomp):
        sos += bytes([c + 1, 0x00 if c == 0 else 0x11])
    _segment(out, 0xDA, sos + b"\x00\x3f\x00")
    return bytes(out)


def _bitlen(a):
    """Bits of each non-negative int64 in `a` (0 for 0)."""
    n = np.zeros(a.shape, np.int64)
    for b in range(16):
        n += (a >> b) > 0
    return n


def entropy_code(co, restart_interval, stats=None):
    """The entropy-coded bytes of stream-ordered coefficients (a `coefficients` dict): stuffed, with restart markers, without
    EOI. Vectorised: every code is a token (value, length, sort key); the tokens' bits are laid out with one cumulative sum."""
    coefs = co["coefs"].astype(np.int64)
    n = coefs.shape[0]
    comp, mcu = co["comp"], co["mcu"]
    seg = mcu // restart_interval if restart_interval else np.zeros(n, np.int64)
    tbl = (comp > 0).astype(np.int64)
    dc_code, dc_size = zip(huff_arrays(DC_LUMA), huff_arrays(DC_CHROMA))
    ac_code, ac_size = zip(huff_arrays(AC_LUMA), huff_arrays(AC_CHROMA))
    dc_code, dc_size, ac_code, ac_size = (np.stack(x) for x in (dc_code, dc_size, ac_code, ac_size))
    # DC differences: the previous block of the same component, 0 at the start of a segment
    diff = coefs[:, 0].copy()
    for c in range(co["ncomp"]):
        idx = np.nonzero(comp == c)[0]
        prev = np.concatenate([[0], coefs[idx[:-1], 0]])
        prev[np.concatenate([[True], seg[idx[1:]] != seg[idx[:-1]]])] = 0
        diff[idx] -= prev
    keys, vals, lens = [], [], []

    def coded(v):  # category and the value bits: a negative v is sent as v - 1 in s bits
        s = _bitlen(np.abs(v))
        return s, np.where(v < 0, v - 1, v) & ((1 << s) - 1)

    blk = np.arange(n)
    s, bits = coded(diff)
    keys.append(blk * 256)
    vals.append(dc_code[tbl, s] << s | bits)
    lens.append(dc_size[tbl, s] + s)
    b, k = np.nonzero(coefs[:, 1:])
    k = k + 1
    prev_k = np.concatenate([[0], k[:-1]])
    prev_k[np.concatenate([[True], b[1:] != b[:-1]])] = 0
    run = k - prev_k - 1
    s, bits = coded(coefs[b, k])
    t = tbl[b]
    nz = run >> 4
    zb = nz > 0
    zc, zs = ac_code[t[zb], 0xF0], ac_size[t[zb], 0xF0]
    zv = np.zeros(zc.shape, np.int64)
    for i in range(3):
        zv = np.where(nz[zb] > i, zv << zs | zc, zv)
    keys.append(b[zb] * 256 + 2 * k[zb])
    vals.append(zv)
    lens.append(zs * nz[zb])
    sym = (run & 15) << 4 | s
    keys.append(b * 256 + 2 * k + 1)
    vals.append(ac_code[t, sym] << s | bits)
    lens.append(ac_size[t, sym] + s)
    last = np.zeros(n, np.int64)
    np.maximum.at(last, b, k)
    eob = np.nonzero(last < 63)[0]
    keys.append(eob * 256 + 200)
    vals.append(ac_code[tbl[eob], 0])
    lens.append(ac_size[tbl[eob], 0])
    keys, vals, lens = np.concatenate(keys), np.concatenate(vals), np.concatenate(lens)
    # padding ones at the end of every segment
    blk_bits = np.bincount(keys >> 8, weights=lens, minlength=n).astype(np.int64)
    nseg = int(seg[-1]) + 1
    seg_bits = np.bincount(seg, weights=blk_bits, minlength=nseg).astype(np.int64)
    pad = -seg_bits % 8
    seg_last = np.concatenate([np.nonzero(seg[1:] != seg[:-1])[0], [n - 1]])
    keys = np.concatenate([keys, seg_last * 256 + 201])
    vals = np.concatenate([vals, (1 << pad) - 1])
    lens = np.concatenate([lens, pad])
    order = np.argsort(keys, kind="stable")
    vals, lens = vals[order], lens[order]
    total = int(lens.sum())
    tok = np.repeat(np.arange(len(lens), dtype=np.int64), lens)
    start = np.cumsum(lens) - lens
    off = np.arange(total, dtype=np.int64) - start[tok]
    bit = ((vals[tok] >> (lens[tok] - 1 - off)) & 1).astype(np.uint8)
    raw = np.packbits(bit).tobytes()
    seg_end = np.cumsum(seg_bits + pad) // 8
    out, p = [], 0
    for i in range(nseg):
        if i:
            out.append(bytes([0xFF, 0xD0 + (i - 1) % 8]))
        out.append(raw[p:seg_end[i]].replace(b"\xff", b"\xff\x00"))
        p = int(seg_end[i])
    if stats is not None:
        ends = np.frombuffer(raw, np.uint8)[seg_end - 1]
        stats.update(
            zrl=int(nz.sum()), no_eob=int(n - len(eob)), max_dc_category=int(_bitlen(np.abs(diff)).max()),
            max_ac_category=int(s.max()) if len(s) else 0, stuffed_bytes=raw.count(b"\xff"),
            stuffed_padding_bytes=int(((ends == 0xFF) & (pad > 0)).sum()), restart_markers=nseg - 1,
            dummy_right=int((co["dummy"] == 1).sum()), dummy_bottom=int((co["dummy"] == 2).sum()), dummy_corner=int((co["dummy"] == 3).sum()),
            blocks=n, unstuffed_bytes=len(raw))
    return b"".join(out)


def encode(img, quality=75, subsampling="4:2:0", restart_interval=0, stats=None, bottom_rule="libjpeg"):
    """The whole file. img: H x W x 3 or H x W uint8; subsampling "4:4:4" | "4:2:2" | "4:2:0" (or Pillow's 0, 1, 2)."""
    hs, vs = SUBSAMPLINGS[subsampling]
    co = coefficients(img, hs, vs, quality, bottom_rule)
    return header(co["w"], co["h"], co["ncomp"], hs, vs, quality, restart_interval) + entropy_code(co, restart_interval, stats) + b"\xff\xd9"


def census(img, quality=75, subsampling="4:2:0", restart_interval=0):
    """What a stream exercises: ZRLs, blocks without EOB, the largest DC and AC categories, stuffed bytes, stuffed bytes that
    the padding ones completed, restart markers, dummy blocks by edge (right, bottom, the corner chain)."""
    stats = {}
    encode(img, quality, subsampling, restart_interval, stats)
    return stats


def worst_case_stream(w, h, ncomp, hs, vs, restart_interval):
    """The stream of this geometry in which every coefficient takes the longest code of its table -- crafted coefficients,
    not an image: what jpeggpu_ext_encode_bound must cover."""
    hs, vs, mx, my, per_mcu = geometry(w, h, ncomp, hs, vs)
    n = mx * my * per_mcu
    comp = np.tile(np.concatenate([np.zeros(hs * vs, np.int64), np.arange(1, ncomp)]), mx * my)
    coefs = np.zeros((n, 64), np.int64)
    longest = {}
    for t, table in enumerate((AC_LUMA, AC_CHROMA)):  # the run-0 symbol with the longest code + value bits
        codes = huff_codes(table)
        longest[t] = max((s for s in codes if s >> 4 == 0 and s), key=lambda s: codes[s][1] + (s & 15))
    for t in (0, 1):
        coefs[comp > 0 if t else comp == 0, 1:] = -((1 << (longest[t] & 15)) - 1)  # negative: the value bits are zeros
    # DC differences of category 11 in every block: alternate +-1023 around 0 (diff = +-2046, 11 bits)
    for c in range(ncomp):
        idx = np.nonzero(comp == c)[0]
        coefs[idx, 0] = np.where(np.arange(len(idx)) % 2 == 0, 1023, -1023)
    co = dict(coefs=coefs, comp=comp, mcu=np.repeat(np.arange(mx * my), per_mcu), dummy=np.zeros(n, np.int64), ncomp=ncomp)
    return header(w, h, ncomp, hs, vs, 75, restart_interval) + entropy_code(co, restart_interval) + b"\xff\xd9"
