"""CPU restatement of progressive encoding (Image.save(f, "JPEG", progressive=True) on libjpeg-turbo), on top of
tests/encode_ref.coefficients and tests/encode_opt_ref.gen_optimal_table: jpeg_simple_progression's script and jcphuff.c's
four scan coders in Python (tests/golden/encode_prog_pins.npz holds Pillow's files; tests/test_encode_prog_ref.py compares).

    encode(img, quality, subsampling, restart_interval, stats=None) -> bytes
    edge_cases() -> (case dict, image) pairs: the inputs that reach each path of the run logic

`stats`, if given, receives `scans` (per scan a dict {(class, table id, symbol): count}), `cap_flushes` (runs ended by
EOBRUN == 0x7FFF), `be_flushes` (runs ended by more than 937 pending correction bits), `max_run`, `refine_zrl` (ZRLs of
refinement scans) and `refine_long_tail` (coefficients met in a refinement scan behind the block's last newly non-zero one
with more than 15 zeros pending, where no ZRL is sent)."""
import numpy as np

from tests import encode_opt_ref as O
from tests import encode_ref as E
from tests.progressive_ref import script_pillow_like

MAX_RUN = 0x7FFF
MAX_PENDING_BITS = 937  # MAX_CORR_BITS - DCTSIZE2 + 1


def scan_blocks(co, comps):
    """Indices into co["coefs"] of a scan's blocks in the scan's order, and the blocks per MCU of the scan: an interleaved
    scan walks the MCU stream, dummy blocks included; a scan of one component its real blocks only, row by row."""
    hs, vs, mx, per_mcu = co["hs"], co["vs"], co["mcus_x"], co["per_mcu"]
    if len(comps) > 1:
        return np.arange(co["coefs"].shape[0]), per_mcu
    c = comps[0]
    if c:
        return np.arange(mx * co["mcus_y"]) * per_mcu + hs * vs + c - 1, 1
    by, bx = np.mgrid[0:-(-co["h"] // 8), 0:-(-co["w"] // 8)]
    return (((by // vs) * mx + bx // hs) * per_mcu + (by % vs) * hs + bx % hs).ravel(), 1


def _bits(v):
    return int(v).bit_length()


class _Run:
    """The pending end-of-band run of a scan: its length and the correction bits that follow its symbol."""

    def __init__(self, out, stats):
        self.out, self.stats, self.n, self.bits = out, stats, 0, []

    def flush(self):
        if self.n:
            nb = _bits(self.n) - 1
            self.out.append((1, nb << 4, 0))
            if nb:
                self.out.append((-1, self.n & ((1 << nb) - 1), nb))
            self.stats["max_run"] = max(self.stats["max_run"], self.n)
            self.n = 0
        self.out.extend((-1, b, 1) for b in self.bits)
        self.bits = []


def _segment_events(co, coefs, order, comp, scan, stats):
    """The symbols (class, symbol, 0) and raw bits (-1, value, length) of one restart segment, in order. For a DC scan the
    class is 0 and the symbol's table follows the component: the caller tells them apart by `comp`."""
    comps, ss, se, ah, al = scan
    out = []
    if ss == 0:
        pred = {}
        for i in order:
            v = int(coefs[i, 0]) >> al
            if ah:
                out.append((-1, v & 1, 1))
                continue
            d = v - pred.get(comp[i], 0)
            pred[comp[i]] = v
            s = _bits(abs(d))
            out.append((0, s | (0x100 if comp[i] else 0), 0))  # bit 8: the chroma table
            if s:
                out.append((-1, (d - 1 if d < 0 else d) & ((1 << s) - 1), s))
        return out
    band = coefs[order, ss:se + 1]
    mag = np.abs(band) >> al
    busy = mag.any(1)
    run = _Run(out, stats)
    for row in range(len(order)):
        buf = []
        if not busy[row]:
            r = se - ss + 1
        else:
            m = mag[row]
            nz = np.flatnonzero(m)
            eob = int(nz[m[nz] == 1][-1]) if ah and (m[nz] == 1).any() else -1
            r, prev = 0, -1
            for k in nz:
                k = int(k)
                r += k - prev - 1
                prev = k
                t = int(m[k])
                if ah == 0:
                    run.flush()
                    while r > 15:
                        out.append((1, 0xF0, 0))
                        r -= 16
                    s = _bits(t)
                    v = -t if band[row, k] < 0 else t
                    out.append((1, r << 4 | s, 0))
                    out.append((-1, (v - 1 if v < 0 else v) & ((1 << s) - 1), s))
                    r = 0
                    continue
                while r > 15 and k <= eob:
                    run.flush()
                    out.append((1, 0xF0, 0))
                    stats["refine_zrl"] += 1
                    r -= 16
                    out.extend((-1, b, 1) for b in buf)
                    buf = []
                if t > 1:
                    if r > 15:
                        stats["refine_long_tail"] += 1
                    buf.append(t & 1)
                    continue
                run.flush()
                out.append((1, r << 4 | 1, 0))
                out.append((-1, 0 if band[row, k] < 0 else 1, 1))
                out.extend((-1, b, 1) for b in buf)
                buf = []
                r = 0
            r += se - ss - prev
        if r > 0 or buf:
            run.n += 1
            run.bits += buf
            if run.n == MAX_RUN or len(run.bits) > MAX_PENDING_BITS:
                stats["cap_flushes" if run.n == MAX_RUN else "be_flushes"] += 1
                run.flush()
    run.flush()
    return out


def _pack(events, codes):
    """The bytes of a segment: codes and raw bits in order, padded with ones, 0xFF stuffed."""
    vals = np.array([codes[e[0], e[1]][0] if e[0] >= 0 else e[1] for e in events], np.int64)
    lens = np.array([codes[e[0], e[1]][1] if e[0] >= 0 else e[2] for e in events], np.int64)
    total = int(lens.sum())
    tok = np.repeat(np.arange(len(lens)), lens)
    off = np.arange(total) - (np.cumsum(lens) - lens)[tok]
    bit = ((vals[tok] >> (lens[tok] - 1 - off)) & 1).astype(np.uint8)
    bit = np.concatenate([bit, np.ones(-total % 8, np.uint8)])
    return np.packbits(bit).tobytes().replace(b"\xff", b"\xff\x00")


def encode(img, quality=75, subsampling="4:2:0", restart_interval=0, stats=None):
    """The whole file. img: H x W x 3 or H x W uint8."""
    hs, vs = E.SUBSAMPLINGS[subsampling]
    co = E.coefficients(img, hs, vs, quality)
    coefs, comp, nc = co["coefs"].astype(np.int64), co["comp"], co["ncomp"]
    st = dict(scans=[], cap_flushes=0, be_flushes=0, max_run=0, refine_zrl=0, refine_long_tail=0)
    head = E.header(co["w"], co["h"], nc, hs, vs, quality, 0)
    at = 2 + 18 + 69 * (1 if nc == 1 else 2)  # SOI, APP0 and the DQTs lie in front of the frame header
    assert head[at:at + 2] == b"\xff\xc0"
    out = bytearray(head[:at] + b"\xff\xc2" + head[at + 2:at + 10 + 3 * nc])  # SOI .. SOF2, no table, no SOS
    for number, scan in enumerate(script_pillow_like(nc)):
        comps, ss, se, ah, al = scan
        order, per_mcu = scan_blocks(co, comps)
        step = restart_interval * per_mcu if restart_interval else len(order)
        segments = [_segment_events(co, coefs, order[a:a + step], comp, scan, st) for a in range(0, len(order), step)]
        counts = {}
        for seg in segments:
            for e in seg:
                if e[0] >= 0:
                    key = (e[0], (e[1] >> 8) if ss == 0 else int(comps[0] > 0), e[1] & 0xFF)
                    counts[key] = counts.get(key, 0) + 1
        st["scans"].append(counts)
        codes = {}
        for cls, tid in sorted({k[:2] for k in counts}):
            freq = np.zeros(256, np.int64)
            for (c, t, s), v in counts.items():
                if (c, t) == (cls, tid):
                    freq[s] = v
            bits, values, status = O.gen_optimal_table(freq)
            if status == O.OVERFLOW:
                raise O.TableOverflow("scan %d class %d table %d" % (number, cls, tid))
            E._segment(out, 0xC4, bytes([cls << 4 | tid]) + bytes(bits) + bytes(values))
            for s, cl in E.huff_codes((bits, values)).items():
                codes[cls, s | (0x100 if ss == 0 and tid else 0)] = cl
        if number == 0 and restart_interval:
            E._segment(out, 0xDD, restart_interval.to_bytes(2, "big"))
        sos = bytes([len(comps)])
        for c in comps:
            sos += bytes([c + 1, (0x10 if c else 0x00) if ss == 0 and ah == 0 else 0x00 if ss == 0 else int(c > 0)])
        E._segment(out, 0xDA, sos + bytes([ss, se, ah << 4 | al]))
        for i, seg in enumerate(segments):
            if i:
                out += bytes([0xFF, 0xD0 + (i - 1) % 8])
            out += _pack(seg, codes)
    if stats is not None:
        stats.update(st)
    return bytes(out) + b"\xff\xd9"


def long_tail_image():
    """32 x 32 grey for quality 100: per block one large coefficient early in the band, a gap of more than 16 zeros, a
    coefficient of magnitude 1 (newly non-zero in the last refinement), again more than 16 zeros and a large coefficient:
    the first gap costs a ZRL in refinement, the second does not (it lies behind the block's last new coefficient)."""
    x = np.arange(8)
    img = np.full((32, 32), 128.0)

    def basis(k):
        v, u = divmod(E.ZIGZAG[k], 8)
        return np.cos((2 * x[None, :] + 1) * u * np.pi / 16) * np.cos((2 * x[:, None] + 1) * v * np.pi / 16)

    for by in range(4):
        for bx in range(4):
            f = 6.0 * basis(2 + bx) + 0.30 * basis(24 + by) + 6.0 * basis(50 + bx + by)
            img[8 * by:8 * by + 8, 8 * bx:8 * bx + 8] += f
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def edge_cases():
    """(case dict, image) pairs; the case dicts have encode_cases' keys."""
    from tests import encode_cases as K

    rng = np.random.default_rng(777)
    two_tiles = rng.integers(0, 256, (136, 136), dtype=np.uint8)  # (the first draw: the pixels of encode_opt_ref's two-tile image)
    noise_block = np.full((1456, 1456), 128, np.uint8)
    noise_block[700:708, 300:308] =np.random.default_rng(5).integers(0, 256, (8, 8), dtype=np.uint8)
    binary = np.random.default_rng(1).integers(0, 2, (256, 256), dtype=np.uint8) * 255
    return [
        (K._case("prog_zero_8x8_grey", 8, 8, True, "prog_edge", 75, "4:4:4", 0), np.zeros((8, 8), np.uint8)),
        (K._case("prog_flat_16x16_rgb", 16, 16, False, "prog_edge", 75, "4:2:0", 0), np.full((16, 16, 3), 128, np.uint8)),
        (K._case("prog_37x53_rgb_420", 37, 53, False, "prog_edge", 75, "4:2:0", 0), rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)),
        (K._case("prog_33x17_rgb_420_r1", 33, 17, False, "prog_edge", 85, "4:2:0", 1), rng.integers(0, 256, (33, 17, 3), dtype=np.uint8)),
        (K._case("prog_two_tiles_136x136_grey_r3", 136, 136, True, "prog_edge", 90, "4:4:4", 3), two_tiles),
        (K._case("prog_flat_1456_grey", 1456, 1456, True, "prog_edge", 75, "4:4:4", 0), np.full((1456, 1456), 128, np.uint8)),
        (K._case("prog_flat_1456_grey_one_block", 1456, 1456, True, "prog_edge", 75, "4:4:4", 0), noise_block),
        (K._case("prog_binary_256_grey_q100", 256, 256, True, "prog_edge", 100, "4:4:4", 0), binary),
        (K._case("prog_binary_256_grey_q100_r40", 256, 256, True, "prog_edge", 100, "4:4:4", 40), binary),
        (K._case("prog_long_tail_32_grey_q100", 32, 32, True, "prog_edge", 100, "4:4:4", 0), long_tail_image()),
        # runs of 100 blocks that restart segments end: the walk's steps of eight blocks stop short of a segment's first block
        (K._case("prog_flat_400_grey_r100", 400, 400, True, "prog_edge", 75, "4:4:4", 100), np.full((400, 400), 128, np.uint8)),
    ]


_pins = None


def pins():
    """{name: dict(length, sha256, data or None)} and the recorded versions, from tests/golden/encode_prog_pins.npz."""
    global _pins
    if _pins is None:
        import json
        import os

        z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encode_prog_pins.npz"))
        meta = json.loads(z["meta"].tobytes().decode())
        table = {e["name"]: dict(length=e["length"], sha256=e["sha256"], data=z["file_" + e["name"]].tobytes() if e["whole"] else None) for e in meta["cases"]}
        _pins = (table, {k: v for k, v in meta.items() if k != "cases"})
    return _pins


def equals_pin(name, data):
    import hashlib

    pin = pins()[0][name]
    if pin["data"] is not None:
        return data == pin["data"]
    return len(data) == pin["length"] and hashlib.sha256(data).hexdigest() == pin["sha256"]
