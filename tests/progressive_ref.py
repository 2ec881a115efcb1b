"""Progressive JPEG (SOF2, Huffman) restated in plain Python / numpy from T.81 Annex G, independent of the product's code:

  * decode(data): the file's coefficients, per component int16 [blocks_y, blocks_x, 64] over the MCU-padded block grid,
    natural order inside a block, and each scan's level (0 if no earlier scan touches its coefficients, else one more
    than the highest level among those that do);
  * encode(...): a progressive file from quantised coefficients, a scan script and a restart interval, with flat code
    tables -- for the scripts no encoder at hand writes (tests/test_progressive_host.py, tests/test_gpu_progressive.py).

Slow and simple on purpose; most files of the tests are a few blocks large, and the decoder takes a second or two for the
largest (tests/golden/progressive_large.npz). decode(data, stats) also says what each scan's data exercised: end-of-band
runs by category, correction bits inside runs, codes longer than 9 bits.
"""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
                   21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53,
                   60, 61, 54, 47, 55, 62, 63])


def ceil_div(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------
# decoder
# ------------------------------------------------------------------------------------------------

class _Bits:
    """Bits of one restart interval's bytes, stuffing removed, zeros behind the end."""

    def __init__(self, raw):
        out, i = bytearray(), 0
        while i < len(raw):
            out.append(raw[i])
            i += 2 if raw[i] == 0xFF else 1  # FF 00 stands for FF
        self.b, self.pos = bytes(out), 0
        self.symbols = self.long_codes = 0  # Huffman symbols read so far, and those of more than 9 bits (statistics)

    def bit(self):
        byte = self.pos >> 3
        v = (self.b[byte] >> (7 - (self.pos & 7))) & 1 if byte < len(self.b) else 0
        self.pos += 1
        return v

    def bits(self, n):
        v = 0
        for _ in range(n):
            v = v << 1 | self.bit()
        return v


def _huff_codes(counts, vals):
    """{(length, code): value} of a DHT table (T.81 Annex C)."""
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            table[(length, code)] = vals[k]
            code += 1
            k += 1
        code <<= 1
    return table


def _decode_symbol(br, table):
    code = 0
    for length in range(1, 17):
        code = code << 1 | br.bit()
        if (length, code) in table:
            br.symbols += 1
            br.long_codes += length > 9
            return table[(length, code)]
    raise ValueError("no code matches")


def _extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


class Decoded:
    pass


def decode(data: bytes, stats=None) -> Decoded:
    """`stats`: a list that gets one dict per scan, in file order -- what the scan's entropy-coded data exercised:
         eob_categories  [15]: how many end-of-band run symbols of each category r (a run of 2^r .. 2^(r+1) - 1 blocks)
         runs            [(length, n)]: every run in order, with n the number of the run symbol among the Huffman symbols
                         of its restart segment (two runs with consecutive n: the second symbol stands right behind the
                         first one's blocks)
         longest_run     the longest of them (0: none)
         correction_bits_in_runs  correction bits read for blocks that an end-of-band run covers (refinement scans)
         long_codes      Huffman codes of more than 9 bits
       Nothing else changes with it."""
    i = 2
    assert data[:2] == b"\xff\xd8"
    out = Decoded()
    out.scans, out.levels = [], []
    dc_tabs, ac_tabs, restart = {}, {}, 0
    comps = None
    touched = {}
    while True:
        assert data[i] == 0xFF, i
        m = data[i + 1]
        if m == 0xFF:
            i += 1
            continue
        if m == 0xD9:
            break
        n = data[i + 2] << 8 | data[i + 3]
        seg = data[i + 4:i + 2 + n]
        i += 2 + n
        if m == 0xC2:
            out.height, out.width = seg[1] << 8 | seg[2], seg[3] << 8 | seg[4]
            nc = seg[5]
            comps = [dict(id=seg[6 + 3 * c], h=seg[7 + 3 * c] >> 4, v=seg[7 + 3 * c] & 15, q=seg[8 + 3 * c]) for c in range(nc)]
            if nc == 1:
                comps[0]["h"] = comps[0]["v"] = 1
            hmax, vmax = max(c["h"] for c in comps), max(c["v"] for c in comps)
            for c in comps:
                c["w"], c["ht"] = ceil_div(out.width * c["h"], hmax), ceil_div(out.height * c["v"], vmax)
                c["bx"] = max(ceil_div(out.width, 8 * hmax) * c["h"], ceil_div(c["w"], 8))
                c["by"] = max(ceil_div(out.height, 8 * vmax) * c["v"], ceil_div(c["ht"], 8))
                c["coef"] = np.zeros((c["by"], c["bx"], 64), np.int64)
            out.comps = comps
        elif m == 0xC4:
            k = 0
            while k < len(seg):
                tc, th = seg[k] >> 4, seg[k] & 15
                counts = list(seg[k + 1:k + 17])
                total = sum(counts)
                (ac_tabs if tc else dc_tabs)[th] = _huff_codes(counts, list(seg[k + 17:k + 17 + total]))
                k += 17 + total
        elif m == 0xDD:
            restart = seg[0] << 8 | seg[1]
        elif m == 0xDA:
            ns = seg[0]
            sel = []
            for a in range(ns):
                ci = [c["id"] for c in comps].index(seg[1 + 2 * a])
                sel.append((ci, seg[2 + 2 * a] >> 4, seg[2 + 2 * a] & 15))
            ss, se, ah, al = seg[1 + 2 * ns], seg[2 + 2 * ns], seg[3 + 2 * ns] >> 4, seg[3 + 2 * ns] & 15
            # entropy-coded data up to the next marker that is neither stuffing nor a restart marker
            j, parts, start = i, [], i
            while True:
                if data[j] == 0xFF and data[j + 1] != 0:
                    if 0xD0 <= data[j + 1] <= 0xD7:
                        parts.append(data[start:j])
                        j += 2
                        start = j
                        continue
                    if data[j + 1] != 0xFF:
                        break
                j += 1
            parts.append(data[start:j])
            i = j
            level = 0
            for ci, _, _ in sel:
                for k in range(ss, se + 1):
                    if (ci, k) in touched:
                        level = max(level, touched[(ci, k)] + 1)
            for ci, _, _ in sel:
                for k in range(ss, se + 1):
                    touched[(ci, k)] = level
            out.levels.append(level)
            out.scans.append(dict(comps=[s[0] for s in sel], ss=ss, se=se, ah=ah, al=al, segments=len(parts)))
            st = None
            if stats is not None:
                st = dict(eob_categories=[0] * 15, runs=[], longest_run=0, correction_bits_in_runs=0, long_codes=0)
                stats.append(st)
            _decode_scan(comps, sel, ss, se, ah, al, restart, parts, dc_tabs, ac_tabs, st)
    out.coef = [c["coef"].astype(np.int16) for c in comps]
    out.visible = [(ceil_div(c["ht"], 8), ceil_div(c["w"], 8)) for c in comps]
    return out


def _decode_scan(comps, sel, ss, se, ah, al, restart, parts, dc_tabs, ac_tabs, st=None):
    if len(sel) > 1:  # interleaved: MCUs of h x v blocks per component
        ci0 = sel[0][0]
        mx, my = ceil_div(comps[ci0]["w"], 8 * comps[ci0]["h"]), ceil_div(comps[ci0]["ht"], 8 * comps[ci0]["v"])
        units = [(ci, td, ta, x, y) for ci, td, ta in sel for y in range(comps[ci]["v"]) for x in range(comps[ci]["h"])]
    else:
        ci0 = sel[0][0]
        mx, my = ceil_div(comps[ci0]["w"], 8), ceil_div(comps[ci0]["ht"], 8)
        units = [(ci0, sel[0][1], sel[0][2], 0, 0)]
    total = mx * my
    per = restart if restart else total
    assert len(parts) == ceil_div(total, per), (len(parts), total, per)
    for g, raw in enumerate(parts):
        br = _Bits(raw)
        pred = {ci: 0 for ci, _, _ in sel}
        eobrun = 0
        for mcu in range(g * per, min((g + 1) * per, total)):
            for ci, td, ta, x, y in units:
                c = comps[ci]
                if len(sel) > 1:
                    blk = c["coef"][(mcu // mx) * c["v"] + y, (mcu % mx) * c["h"] + x]
                else:
                    blk = c["coef"][mcu // mx, mcu % mx]
                if ss == 0:
                    if ah == 0:  # G.1.2.1: the difference of the point-transformed DC values
                        s = _decode_symbol(br, dc_tabs[td])
                        pred[ci] += _extend(br.bits(s), s)
                        blk[0] = pred[ci] * (1 << al)
                    elif br.bit():
                        blk[0] |= 1 << al
                elif ah == 0:
                    eobrun = _ac_first(br, ac_tabs[ta], blk, ss, se, al, eobrun, st)
                else:
                    eobrun = _ac_refine(br, ac_tabs[ta], blk, ss, se, al, eobrun, st)
        if st is not None:
            st["long_codes"] += br.long_codes


def _count_run(st, br, r, length):
    if st is not None:
        st["eob_categories"][r] += 1
        st["runs"].append((length, br.symbols))
        st["longest_run"] = max(st["longest_run"], length)


def _ac_first(br, table, blk, ss, se, al, eobrun, st=None):
    """G.1.2.2: one block of a first AC scan; returns the end-of-band run left for the blocks behind it."""
    if eobrun:
        return eobrun - 1
    k = ss
    while k <= se:
        rs = _decode_symbol(br, table)
        r, s = rs >> 4, rs & 15
        if s == 0:
            if r == 15:
                k += 16
                continue
            run = (1 << r) + br.bits(r)
            _count_run(st, br, r, run)
            return run - 1
        k += r
        blk[ZIGZAG[k]] = _extend(br.bits(s), s) * (1 << al)
        k += 1
    return 0


def _ac_refine(br, table, blk, ss, se, al, eobrun, st=None):
    """G.1.2.3 (figure G.7): one block of an AC refinement scan."""
    p1 = 1 << al

    def correct(z):
        if br.bit() and not (abs(int(blk[z])) & p1):
            blk[z] += p1 if blk[z] > 0 else -p1

    k = ss
    if not eobrun:
        while k <= se:
            rs = _decode_symbol(br, table)
            r, s = rs >> 4, rs & 15
            value = 0
            if s:
                assert s == 1
                value = p1 if br.bit() else -p1  # the sign comes in front of the correction bits
            elif r != 15:
                eobrun = (1 << r) + br.bits(r)
                _count_run(st, br, r, eobrun)
                break
            while k <= se:  # pass r zero-history coefficients; the non-zero ones on the way take a correction bit each
                z = ZIGZAG[k]
                if blk[z]:
                    correct(z)
                else:
                    if r == 0:
                        break
                    r -= 1
                k += 1
            if value:
                blk[ZIGZAG[k]] = value
            k += 1
    if eobrun:
        while k <= se:
            if blk[ZIGZAG[k]]:
                correct(ZIGZAG[k])
                if st is not None:
                    st["correction_bits_in_runs"] += 1
            k += 1
        eobrun -= 1
    return eobrun


# ------------------------------------------------------------------------------------------------
# encoder
# ------------------------------------------------------------------------------------------------

class _Writer:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, value, nbits):
        for k in range(nbits - 1, -1, -1):
            self.acc = self.acc << 1 | ((value >> k) & 1)
            self.n += 1
            if self.n == 8:
                self.out.append(self.acc)
                if self.acc == 0xFF:
                    self.out.append(0)
                self.acc, self.n = 0, 0

    def flush(self):
        while self.n:
            self.put(1, 1)  # pad with ones (T.81 F.1.2.3)


def _flat_table(nsym, length):
    """(DHT counts, values, {value: (code, length)}) of a table whose `nsym` symbols all have `length` bits -- but for the
    last one of 256, which has one bit more: a DHT count is a byte."""
    counts = [0] * 16
    first = min(nsym, 255)
    assert first < (1 << length)
    counts[length - 1] = first
    vals = list(range(nsym))
    codes = {v: (v, length) for v in vals[:first]}
    if nsym > first:
        counts[length] = 1
        codes[255] = (first << 1, length + 1)
    return counts, vals, codes


def _category(v):
    return int(abs(int(v))).bit_length()


def _magnitude_bits(v, s):
    return (v if v >= 0 else v - 1) & ((1 << s) - 1)


def encode(width, height, sampling, qtabs, qidx, coef, script, restart=0, dc_len=5, ac_len=9, ids=None, jfif=True):
    """A progressive file. `sampling`: (h, v) per component; `qtabs`: {index: 64 values in natural order}; `coef[c]`:
    int [rows, cols, 64] in natural order, at least the component's ceil(size / 8) blocks (blocks an interleaved scan
    needs beyond them are zero); `script`: scans (component indices, Ss, Se, Ah, Al); `restart`: MCUs per restart interval
    of every scan (0: none). Flat code tables: `dc_len` bits for the 16 DC symbols, `ac_len` for the 256 AC symbols."""
    nc = len(sampling)
    ids = list(ids) if ids else list(range(1, nc + 1))
    if nc == 1:
        sampling = [(1, 1)]
    hmax, vmax = max(h for h, _ in sampling), max(v for _, v in sampling)
    comps = []
    for c in range(nc):
        h, v = sampling[c]
        w, ht = ceil_div(width * h, hmax), ceil_div(height * v, vmax)
        bx, by = max(ceil_div(width, 8 * hmax) * h, ceil_div(w, 8)), max(ceil_div(height, 8 * vmax) * v, ceil_div(ht, 8))
        full = np.zeros((by, bx, 64), np.int64)
        src = np.asarray(coef[c])
        ry, rx = min(by, src.shape[0]), min(bx, src.shape[1])
        full[:ry, :rx] = src[:ry, :rx]
        comps.append(dict(h=h, v=v, w=w, ht=ht, coef=full))
    out = bytearray(b"\xff\xd8")
    if jfif:
        out += b"\xff\xe0\x00\x10JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00"
    for t in sorted(qtabs):
        q = np.asarray(qtabs[t]).reshape(64)
        assert q.max() < 256
        out += b"\xff\xdb\x00\x43" + bytes([t]) + bytes(int(q[ZIGZAG[k]]) for k in range(64))
    out += b"\xff\xc2" + (8 + 3 * nc).to_bytes(2, "big") + b"\x08" + height.to_bytes(2, "big") + width.to_bytes(2, "big") + bytes([nc])
    for c in range(nc):
        out += bytes([ids[c], sampling[c][0] << 4 | sampling[c][1], qidx[c]])
    dcc, dcv, dcode = _flat_table(16, dc_len)
    acc, acv, acode = _flat_table(256, ac_len)
    out += b"\xff\xc4" + (2 + 17 + 16).to_bytes(2, "big") + b"\x00" + bytes(dcc) + bytes(dcv)
    out += b"\xff\xc4" + (2 + 17 + 256).to_bytes(2, "big") + b"\x10" + bytes(acc) + bytes(acv)
    if restart:
        out += b"\xff\xdd\x00\x04" + restart.to_bytes(2, "big")
    for sel, ss, se, ah, al in script:
        out += b"\xff\xda" + (6 + 2 * len(sel)).to_bytes(2, "big") + bytes([len(sel)])
        for ci in sel:
            out += bytes([ids[ci], 0x00])
        out += bytes([ss, se, ah << 4 | al])
        out += _encode_scan(comps, sel, ss, se, ah, al, restart, dcode, acode)
    return bytes(out + b"\xff\xd9")


def _encode_scan(comps, sel, ss, se, ah, al, restart, dcode, acode):
    if len(sel) > 1:
        c0 = comps[sel[0]]
        mx, my = ceil_div(c0["w"], 8 * c0["h"]), ceil_div(c0["ht"], 8 * c0["v"])
        units = [(ci, x, y) for ci in sel for y in range(comps[ci]["v"]) for x in range(comps[ci]["h"])]
    else:
        c0 = comps[sel[0]]
        mx, my = ceil_div(c0["w"], 8), ceil_div(c0["ht"], 8)
        units = [(sel[0], 0, 0)]
    total = mx * my
    per = restart if restart else total
    data = bytearray()
    for g in range(ceil_div(total, per)):
        w = _Writer()
        state = dict(eobrun=0, pending=[])  # correction bits that wait behind an end-of-band run

        def sym(table, s):
            w.put(*table[s])

        def flush_eobrun():
            if state["eobrun"]:
                nb = state["eobrun"].bit_length() - 1
                sym(acode, nb << 4)
                w.put(state["eobrun"] & ((1 << nb) - 1), nb)
                state["eobrun"] = 0
            for b in state["pending"]:
                w.put(b, 1)
            state["pending"] = []

        pred = {ci: 0 for ci in sel}
        for mcu in range(g * per, min((g + 1) * per, total)):
            for ci, x, y in units:
                c = comps[ci]
                blk = c["coef"][(mcu // mx) * c["v"] + y, (mcu % mx) * c["h"] + x] if len(sel) > 1 else c["coef"][mcu // mx, mcu % mx]
                if ss == 0:
                    if ah == 0:
                        v = int(blk[0]) >> al  # the DC point transform is an arithmetic shift
                        d = v - pred[ci]
                        pred[ci] = v
                        s = _category(d)
                        sym(dcode, s)
                        w.put(_magnitude_bits(d, s), s)
                    else:
                        w.put((int(blk[0]) >> al) & 1, 1)
                    continue
                vals = [int(blk[ZIGZAG[k]]) for k in range(64)]
                mags = [abs(v) >> al for v in vals]  # the AC point transform divides, rounding towards zero
                if ah == 0:
                    r = 0
                    for k in range(ss, se + 1):
                        if mags[k] == 0:
                            r += 1
                            continue
                        flush_eobrun()
                        while r > 15:
                            sym(acode, 0xF0)
                            r -= 16
                        s = mags[k].bit_length()
                        sym(acode, r << 4 | s)
                        w.put(_magnitude_bits(mags[k] if vals[k] > 0 else -mags[k], s), s)
                        r = 0
                    if r:
                        state["eobrun"] += 1
                        if state["eobrun"] == 0x7FFF:
                            flush_eobrun()
                else:
                    last_new = max([k for k in range(ss, se + 1) if mags[k] == 1], default=-1)
                    r, buffered = 0, []
                    for k in range(ss, se + 1):
                        if mags[k] == 0:
                            r += 1
                            continue
                        while r > 15 and k <= last_new:
                            flush_eobrun()
                            sym(acode, 0xF0)
                            r -= 16
                            for b in buffered:
                                w.put(b, 1)
                            buffered = []
                        if mags[k] > 1:
                            buffered.append(mags[k] & 1)
                            continue
                        flush_eobrun()
                        sym(acode, r << 4 | 1)
                        w.put(1 if vals[k] > 0 else 0, 1)
                        for b in buffered:
                            w.put(b, 1)
                        buffered, r = [], 0
                    if r or buffered:
                        state["eobrun"] += 1
                        state["pending"] += buffered
                        if state["eobrun"] == 0x7FFF:
                            flush_eobrun()
        flush_eobrun()
        w.flush()
        data += w.out
        if g + 1 < ceil_div(total, per):
            data += bytes([0xFF, 0xD0 + g % 8])
    return bytes(data)


# scan scripts: (component indices, Ss, Se, Ah, Al)

def script_pillow_like(nc):
    """libjpeg's default script for three components (jcparam.c, jpeg_simple_progression), or its analogue."""
    if nc == 3:
        return [((0, 1, 2), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((2,), 1, 63, 0, 1), ((1,), 1, 63, 0, 1), ((0,), 6, 63, 0, 2),
                ((0,), 1, 63, 2, 1), ((0, 1, 2), 0, 0, 1, 0), ((2,), 1, 63, 1, 0), ((1,), 1, 63, 1, 0), ((0,), 1, 63, 1, 0)]
    out = [(tuple(range(nc)), 0, 0, 0, 1)]
    for c in range(nc):
        out += [((c,), 1, 5, 0, 2), ((c,), 6, 63, 0, 2), ((c,), 1, 63, 2, 1)]
    out.append((tuple(range(nc)), 0, 0, 1, 0))
    out += [((c,), 1, 63, 1, 0) for c in range(nc)]
    return out


def script_plain(nc):
    """No successive approximation at all: a non-interleaved DC scan and one AC scan per component, Al = 0 throughout."""
    out = []
    for c in range(nc):
        out += [((c,), 0, 0, 0, 0), ((c,), 1, 63, 0, 0)]
    return out


def script_three_refinements(nc):
    """Three refinement passes, for DC and AC alike."""
    out = [(tuple(range(nc)), 0, 0, 0, 3)]
    out += [((c,), 1, 63, 0, 3) for c in range(nc)]
    for al in (2, 1, 0):
        out.append((tuple(range(nc)), 0, 0, al + 1, al))
        out += [((c,), 1, 63, al + 1, al) for c in range(nc)]
    return out


def script_single_bands(nc):
    """Bands of one coefficient for the low frequencies (first scans and refinements), the rest in one band."""
    out = [(tuple(range(nc)), 0, 0, 0, 0)]
    for c in range(nc):
        out += [((c,), k, k, 0, 1) for k in range(1, 6)]
        out.append(((c,), 6, 63, 0, 1))
        out += [((c,), k, k, 1, 0) for k in range(1, 4)]
        out.append(((c,), 4, 63, 1, 0))
    return out


def script_early_stop(nc):
    """A script that stops early: the last bit of every coefficient is never sent, and the highest band of component 0 is never coded."""
    out = [(tuple(range(nc)), 0, 0, 0, 2)]
    out += [((c,), 1, 40 if c == 0 else 63, 0, 2) for c in range(nc)]
    out.append((tuple(range(nc)), 0, 0, 2, 1))
    out += [((c,), 1, 40 if c == 0 else 63, 2, 1) for c in range(nc)]
    return out
