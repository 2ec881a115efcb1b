"""CPU restatement of how libjpeg decodes a baseline JPEG that ends early, as Pillow shows it with
ImageFile.LOAD_TRUNCATED_IMAGES (JpegImagePlugin.load_read hands libjpeg one fake FF D9 when the file runs dry, and libjpeg
takes its "hit a marker" path: jdhuff.c, jpeg_fill_bit_buffer / decode_mcu / process_restart).

The rule ("Truncated files"; checked against Pillow at every cut offset by tests/test_truncated_ref.py):

  1. everything up to and including the first SOS header must be whole;
  2. the entropy-coded data of a scan is what lies between its header and the next marker or the end of the file; a trailing
     FF (the first half of an FF 00 pair or of a marker) is not data;
  3. behind the last real bit the bit reader delivers zero bits. The first MCU that needs a bit that does not exist is
     finished from those zero bits;
  4. every MCU behind that one, to the end of the scan, is not decoded: all its coefficients are zero, DC included;
  5. restart intervals that are wholly missing are such MCUs; where the data ends with an interval and no bit was missing
     yet, the first MCU of the next interval is the one decoded from zero bits (DC predictors reset);
  6. a scan that is not there at all leaves its components' coefficients zero;
  7. a file that lacks only its EOI equals the whole file.

`decode(data)` returns an object with the fields of oracle.Decoded that the other restatements read (tests/libjpeg_ref.py,
tests/draft_ref.py, tests/color_ref.py), so truncated coefficients go through the same IDCT and colour code as whole ones.
"""
import functools
import hashlib
import io
import os

import numpy as np

ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
          57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)


class Truncated(Exception):
    """The file ends in front of the end of its first SOS header (rule 1)."""


class Decoded:
    """The fields of oracle.Decoded that the CPU restatements read, plus what the cut did."""


@functools.lru_cache(maxsize=64)
def _lookup(payload):
    """DHT payload (16 counts + values) -> 65536-entry list: 16-bit window -> (code length, symbol). A window that starts no
    code (an incomplete table) reads as a 16-bit code of symbol 0, which no file of these tests reaches."""
    counts, vals = payload[:16], payload[16:]
    table = [(16, 0)] * 65536
    code, k = 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            lo = code << (16 - length)
            table[lo:lo + (1 << (16 - length))] = [(length, vals[k])] * (1 << (16 - length))
            code += 1
            k += 1
        code <<= 1
    return table


def _extend(bits, s):
    return bits if s == 0 or bits >> (s - 1) else bits - (1 << s) + 1


class _Bits:
    """The bits of one restart interval, zeros behind them; `short` says a read went past the last real bit."""

    def __init__(self, data):
        self.real = 8 * len(data)
        self.total = self.real + 64
        self.value = int.from_bytes(data, "big") << 64 if data else 0
        self.pos = 0
        self.short = False

    def peek16(self):
        shift = self.total - self.pos - 16
        return (self.value >> shift) & 0xFFFF if shift >= 0 else (self.value << -shift) & 0xFFFF

    def take(self, n):
        """n <= 16 bits; the position may run past `total` (all zeros there)."""
        shift = self.total - self.pos - n
        v = (self.value >> shift) & ((1 << n) - 1) if shift >= 0 else (self.value << -shift) & ((1 << n) - 1)
        self.pos += n
        if self.pos > self.real:
            self.short = True
        return v


def _segments(data, begin):
    """The scan's restart intervals as destuffed byte strings, the offset of what follows the scan, and how the scan ended:
    "marker" (a marker other than RSTn follows), "eof" (the file ended in or behind the data)."""
    segs, cur, i, n = [], bytearray(), begin, len(data)
    while True:
        j = data.find(b"\xff", i)
        if j < 0 or j + 1 >= n:  # no more markers: data to the end, a trailing FF is not data (rule 2)
            cur += data[i:n if j < 0 else j]
            segs.append(bytes(cur))
            return segs, n, "eof"
        cur += data[i:j]
        m = data[j + 1]
        if m == 0:
            cur.append(0xFF)
            i = j + 2
            continue
        k = j + 1
        while k < n and data[k] == 0xFF:  # fill bytes
            k += 1
        if k >= n:
            segs.append(bytes(cur))
            return segs, n, "eof"
        m = data[k]
        segs.append(bytes(cur))
        if 0xD0 <= m <= 0xD7:
            cur = bytearray()
            i = k + 1
            continue
        return segs, k - 1, "marker"


def decode(data):
    """The quantised coefficients of `data` by the rule above, as a Decoded. Baseline and extended-sequential Huffman files."""
    n = len(data)
    if n < 4 or data[:2] != b"\xff\xd8":
        raise Truncated("no SOI")
    qtab = np.zeros((4, 64), np.int64)
    dht = {}
    frame = None
    restart = 0
    out = Decoded()
    out.nscans = 0
    out.ended = "eoi"          # "eoi", or "eof": the file ended without an EOI marker
    out.cut_mcu = None         # (scan, MCU) decoded from missing bits, if any
    out.scan_bytes = []
    i = 2
    seen = set()
    while True:
        if i + 2 > n:
            if out.nscans == 0:
                raise Truncated("header")
            out.ended = "eof"
            break
        if data[i] != 0xFF:
            raise ValueError("marker expected at %d" % i)
        while i < n and data[i] == 0xFF:
            i += 1
        if i >= n:
            if out.nscans == 0:
                raise Truncated("header")
            out.ended = "eof"
            break
        m = data[i]
        i += 1
        if m == 0xD9:
            break
        if i + 2 > n:
            if out.nscans == 0:
                raise Truncated("header")
            out.ended = "eof"
            break
        length = data[i] << 8 | data[i + 1]
        if i + length > n:
            if out.nscans == 0:
                raise Truncated("header")
            out.ended = "eof"  # a cut inside a later scan's tables or header: that scan is not there (rule 6)
            break
        body = data[i + 2:i + length]
        i += length
        if m == 0xDB:
            k = 0
            while k < len(body):
                pq, tq = body[k] >> 4, body[k] & 15
                k += 1
                for z in range(64):
                    qtab[tq, ZIGZAG[z]] = (body[k] << 8 | body[k + 1]) if pq else body[k]
                    k += 2 if pq else 1
        elif m == 0xC4:
            k = 0
            while k < len(body):
                cnt = sum(body[k + 1:k + 17])
                dht[body[k]] = bytes(body[k + 1:k + 17 + cnt])
                k += 17 + cnt
        elif m in (0xC0, 0xC1):
            h, w, nc = body[1] << 8 | body[2], body[3] << 8 | body[4], body[5]
            frame = [(body[6 + 3 * c], body[7 + 3 * c] >> 4, body[7 + 3 * c] & 15, body[8 + 3 * c]) for c in range(nc)]
            out.width, out.height, out.ncomp = w, h, nc
            out.hs = [1] if nc == 1 else [f[1] for f in frame]
            out.vs = [1] if nc == 1 else [f[2] for f in frame]
            out.qidx = [f[3] for f in frame]
            hmax, vmax = max(out.hs), max(out.vs)
            mx, my = -(-w // (8 * hmax)), -(-h // (8 * vmax))
            out.coef = [np.zeros((my * v, mx * hh, 64), np.int16) for hh, v in zip(out.hs, out.vs)]
            out.planes = [np.zeros((-(-h * v // vmax), -(-w * hh // hmax)), np.uint8) for hh, v in zip(out.hs, out.vs)]
        elif m == 0xDD:
            restart = body[0] << 8 | body[1]
        elif m == 0xC2 or 0xC5 <= m <= 0xCF and m not in (0xC8, 0xCC):
            raise NotImplementedError("SOF%d" % (m - 0xC0))
        elif m == 0xDA:
            ns = body[0]
            comps = []
            for a in range(ns):
                ci = next(c for c, f in enumerate(frame) if f[0] == body[1 + 2 * a])
                comps.append((ci, _lookup(dht[body[2 + 2 * a] >> 4]), _lookup(dht[0x10 | body[2 + 2 * a] & 15])))
            segs, i, how = _segments(data, i)
            out.scan_bytes.append(sum(len(s) for s in segs))
            _decode_scan(out, out.nscans, comps, segs, how, restart)
            out.nscans += 1
            seen.update(c for c, _, _ in comps)
            if how == "eof":
                out.ended = "eof"
                break
    out.restart_interval = restart
    out.qtab = qtab
    return out


def _decode_scan(out, scan_idx, comps, segs, how, restart):
    hmax, vmax = max(out.hs), max(out.vs)
    if len(comps) > 1:
        mx, my = -(-out.width // (8 * hmax)), -(-out.height // (8 * vmax))
        units = [(ci, dc, ac, x, y, out.hs[ci], out.vs[ci]) for ci, dc, ac in comps for y in range(out.vs[ci]) for x in range(out.hs[ci])]
    else:  # one component: its own block grid, one unit per MCU
        ci, dc, ac = comps[0]
        mx = -(-(-(-out.width * out.hs[ci] // hmax)) // 8)
        my = -(-(-(-out.height * out.vs[ci] // vmax)) // 8)
        units = [(ci, dc, ac, 0, 0, 1, 1)]
    total = mx * my
    interval = restart if restart else total
    insufficient = False  # jdhuff.c: entropy->insufficient_data
    for mcu in range(total):
        k, first = divmod(mcu, interval)
        if first == 0:
            pred = [0] * 4
            if k < len(segs):
                bits = _Bits(segs[k])
                # only the file's last interval can run dry: a whole one that does is a damaged file, out of scope
                last = how == "eof" and k == len(segs) - 1
            else:
                bits, last = _Bits(b""), True
        if insufficient:
            continue  # rule 4
        for ci, dc, ac, x, y, hh, vv in units:
            block = out.coef[ci][(mcu // mx) * vv + y, (mcu % mx) * hh + x]
            length, s = dc[bits.peek16()]
            bits.take(length)
            pred[ci] += _extend(bits.take(s), s) if s else 0
            block[0] = ((pred[ci] + 32768) & 0xFFFF) - 32768  # int16 wrap
            z = 1
            while z < 64:
                length, rs = ac[bits.peek16()]
                bits.take(length)
                r, s = rs >> 4, rs & 15
                if s == 0:
                    if r != 15:
                        break
                    z += 16
                    continue
                z += r
                v = _extend(bits.take(s), s)
                block[ZIGZAG[z] if z < 64 else 63] = v  # jdhuff.c: jpeg_natural_order is padded with 63s for an overshooting run
                z += 1
        if last and bits.short:
            insufficient = True
            out.cut_mcu = (scan_idx, mcu)


# ------------------------------------------------------------------------------------------------
# pixels
# ------------------------------------------------------------------------------------------------

def islow_planes_of(dec):
    """tests/libjpeg_ref.islow_planes_of, transforming only the blocks that hold a coefficient: an all-zero block is 64 samples
    of 128 under jpeg_idct_islow (every sum is 0, and the range limit of 0 is 128), and behind a cut most blocks are such."""
    from tests import libjpeg_ref

    out = []
    for c in range(dec.ncomp):
        coef = dec.coef[c]
        bh, bw = coef.shape[:2]
        flat = coef.reshape(-1, 64)
        blocks = np.full((bh * bw, 8, 8), 128, np.uint8)
        some = flat.any(axis=1)
        if some.any():
            blocks[some] = libjpeg_ref.idct_islow(flat[some], dec.qtab[dec.qidx[c]])
        full = blocks.reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)
        h, w = dec.planes[c].shape
        out.append(np.ascontiguousarray(full[:h, :w]))
    return out


def rgb_of(dec, data, d=1):
    """Pillow's convert("RGB") of a truncated file's Decoded (at 1 / d after draft())."""
    from tests import color_ref, draft_ref

    if d > 1:
        return color_ref.color_rgb_of(dec, model_of(data), d)
    hs, vs = draft_ref.factors_of(dec)
    return color_ref.convert(color_ref.upsampled(islow_planes_of(dec), hs, vs, dec.width, dec.height, True), model_of(data))


def model_of(data):
    """The colour model (tests/color_ref.py) from the segments in front of the first scan; the scan itself may be cut."""
    from tests import color_ref

    return color_ref.model_of_file(data[:scan_begin(data)] + b"\xff\xd9")


def rgb(data, d=1):
    return rgb_of(decode(data), data, d)


def pillow_rgb(data, d=1, mode="RGB"):
    """np.asarray(Image.open(..).convert(mode)) with ImageFile.LOAD_TRUNCATED_IMAGES set for the call and restored."""
    from PIL import Image, ImageFile

    old = ImageFile.LOAD_TRUNCATED_IMAGES
    ImageFile.LOAD_TRUNCATED_IMAGES = True
    try:
        im = Image.open(io.BytesIO(data))
        if d > 1:
            im.draft(mode if mode == "L" else "RGB", (max(im.size[0] // d, 1), max(im.size[1] // d, 1)))
        return np.asarray(im.convert(mode))
    finally:
        ImageFile.LOAD_TRUNCATED_IMAGES = old


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ------------------------------------------------------------------------------------------------
# files
# ------------------------------------------------------------------------------------------------

LAYOUTS = (("gray", "L", None, 48, 32), ("s444", "RGB", 0, 48, 32), ("s422", "RGB", 1, 64, 40), ("s420", "RGB", 2, 64, 48))
VARIANTS = (("plain", {}), ("opt", {"optimize": True}), ("rst1", {"restart_marker_blocks": 1}), ("rstrow", {"restart_marker_rows": 1}),
            ("rst5", {"restart_marker_blocks": 5}))


def picture(w, h, seed, noise=10):
    """A smooth picture with some noise: a scan of a few hundred bytes with short and long codes."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 100 * np.sin(x / 7.0 + seed) * np.cos(y / 5.0), 128 + 90 * np.cos(x / 11.0) * np.sin(y / 9.0 + 1), 40 + 3 * x + 2 * y], axis=-1)
    return np.clip(base + rng.normal(0, noise, base.shape), 0, 255).astype(np.uint8)


def encode(mode, subsampling, w, h, seed, quality=60, noise=10, **kw):
    from PIL import Image

    a = picture(w, h, seed, noise)
    im = Image.fromarray(a if mode == "RGB" else a[:, :, 0])
    buf = io.BytesIO()
    if subsampling is not None:
        kw["subsampling"] = subsampling
    im.save(buf, "JPEG", quality=quality, **kw)
    return buf.getvalue()


def scan_begin(data):
    """Offset of the first entropy-coded byte of the first scan."""
    i = 2
    while True:
        assert data[i] == 0xFF
        m = data[i + 1]
        length = data[i + 2] << 8 | data[i + 3]
        i += 2 + length
        if m == 0xDA:
            return i


@functools.lru_cache(maxsize=1)
def files():
    """name -> bytes: every layout in every variant (needs Pillow), and one file whose scan holds stuffed FF 00 pairs."""
    out = {}
    for k, (lname, mode, sub, w, h) in enumerate(LAYOUTS):
        for j, (vname, kw) in enumerate(VARIANTS):
            out["%s_%s" % (lname, vname)] = encode(mode, sub, w, h, seed=10 * k + j, **kw)
    for seed in range(200):  # high quality, much noise: long codes of ones
        data = encode("RGB", 2, 48, 32, seed=1000 + seed, quality=95, noise=60, restart_marker_blocks=2)
        if data.count(b"\xff\x00", scan_begin(data)) >= 2:
            out["s420_stuffed"] = data
            break
    assert "s420_stuffed" in out
    return out


def cuts(data):
    """Every length from the end of the first SOS header to the whole file."""
    return range(scan_begin(data), len(data) + 1)


def special_cuts(data):
    """name -> file length, for the ends the rule leaves open: a lone trailing FF, inside FF 00, inside and right behind a
    restart marker, exactly at an interval's end, and the file without its EOI. Entries the file does not have are missing."""
    b = scan_begin(data)
    out = {"no_eoi": len(data) - 2, "eoi_ff": len(data) - 1}
    i = data.find(b"\xff\x00", b)
    if i >= 0:
        out["in_ff00"] = i + 1      # the FF of the pair is the last byte
        out["behind_ff00"] = i + 2
    for m in range(0xD0, 0xD8):
        i = data.find(bytes([0xFF, m]), b)
        if i >= 0 and (m == 0xD0):
            out["interval_end"] = i  # the data of interval 0, nothing of the marker
            out["in_rst"] = i + 1    # the marker's FF is the last byte
            out["behind_rst"] = i + 2
    return out


# ------------------------------------------------------------------------------------------------
# where Pillow's IDCT is not jidctint.c's
# ------------------------------------------------------------------------------------------------

def simd_comparable(coef, q):
    """bool [n]: the units [n, 64] on which libjpeg-turbo's SIMD jpeg_idct_islow (what Pillow runs) computes what jidctint.c
    -- the library's ISLOW transform and tests/libjpeg_ref.py -- computes. The SIMD code keeps the dequantised inputs, the sums
    in0 +- in4, in1 + in5, in3 + in7, in2 + in6 and the workspace in 16 bits, and it saturates its result where jidctint.c wraps
    it to 10 bits first (tests/test_idct_cases_host.py, pillow_comparable_units: the same rule). The unit a cut file's MCU
    is finished from zero bits in can hold 63 coefficients of -(2^s - 1) and fall outside; units of whole data do not."""
    from tests import libjpeg_ref
    from tests.scaled_ref import CONST_BITS, PASS1_BITS, descale

    d = (coef.astype(np.int64) * q.astype(np.int64)[None, :]).reshape(-1, 8, 8)

    def fits(x, axis):
        a = np.abs(np.moveaxis(x, axis, 1))
        return ((a[:, 0] + a[:, 4] <= 32767) & (a[:, 1] + a[:, 5] <= 32767) & (a[:, 3] + a[:, 7] <= 32767) & (a[:, 2] + a[:, 6] <= 32767)).all(axis=1) & (a <= 32767).all(axis=(1, 2))

    ws = np.empty(d.shape, np.int64)
    out = libjpeg_ref.islow_1d([d[:, k, :] for k in range(8)])
    for k in range(8):
        ws[:, k, :] = descale(out[k], CONST_BITS - PASS1_BITS)
    v = np.empty(d.shape, np.int64)
    out = libjpeg_ref.islow_1d([ws[:, :, k] for k in range(8)])
    for k in range(8):
        v[:, :, k] = descale(out[k], CONST_BITS + PASS1_BITS + 3)
    return fits(d, 1) & fits(ws, 2) & ((v >= -512) & (v <= 511)).all(axis=(1, 2))


def cut_mcu_rect(dec, margin=2):
    """(x0, y0, x1, y1) in pixels of the MCU that was finished from zero bits, `margin` pixels wider on every side (what a
    fancy-upsampled chroma sample of it reaches), or None. For a file of one interleaved scan or of one component."""
    if dec.cut_mcu is None:
        return None
    mw, mh = 8 * max(dec.hs), 8 * max(dec.vs)
    mx = -(-dec.width // mw)
    m = dec.cut_mcu[1]
    x0, y0 = (m % mx) * mw, (m // mx) * mh
    return max(x0 - margin, 0), max(y0 - margin, 0), min(x0 + mw + margin, dec.width), min(y0 + mh + margin, dec.height)


def pillow_comparable(dec):
    """Whether every unit of the MCU finished from zero bits is one Pillow's SIMD IDCT computes as jidctint.c does."""
    if dec.cut_mcu is None:
        return True
    m = dec.cut_mcu[1]
    mx = -(-dec.width // (8 * max(dec.hs)))
    for c in range(dec.ncomp):
        h, v = dec.hs[c], dec.vs[c]
        units = dec.coef[c][(m // mx) * v:(m // mx) * v + v, (m % mx) * h:(m % mx) * h + h].reshape(-1, 64)
        if not simd_comparable(units, dec.qtab[dec.qidx[c]]).all():
            return False
    return True


# ------------------------------------------------------------------------------------------------
# pins: the files themselves and Pillow's answers at some cuts, so that the GPU tests need no Pillow
# ------------------------------------------------------------------------------------------------

PINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "truncated_pins.npz")
PINNED_CUTS = 12  # evenly spread over the scan, besides the special ends


def pin_cuts(data):
    """The cuts of a file that are pinned: PINNED_CUTS spread over the scan and every special end it has -- those at which
    Pillow's SIMD IDCT computes the cut MCU as jidctint.c does (pillow_comparable): the others are Pillow's arithmetic on
    out-of-range blocks, not the rule."""
    b, n = scan_begin(data), len(data)
    want = sorted(set([b + (n - b) * k // PINNED_CUTS for k in range(PINNED_CUTS)] + list(special_cuts(data).values())))
    return [c for c in want if pillow_comparable(decode(data[:c]))]


@functools.lru_cache(maxsize=1)
def pinned():
    """name -> (file bytes, [cut], [sha256 of Pillow's RGB at that cut]) from tests/golden/truncated_pins.npz."""
    z = np.load(PINS)
    out = {}
    for key in z.files:
        kind, _, name = key.partition("/")
        if kind == "jpeg":
            out[name] = (z[key].tobytes(), [int(c) for c in z["cuts/" + name]], [str(s) for s in z["sha/" + name]])
    return out


def pinned_files():
    """name -> bytes of the pinned files: files() without Pillow."""
    return {name: v[0] for name, v in pinned().items()}


# ------------------------------------------------------------------------------------------------
# larger files (the synthetic encoder: no Pillow) and the cuts around subsequence boundaries
# ------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=1)
def large_files():
    """512 x 384, 4:2:0: one without restart markers, one with a marker per MCU row; and the smallest sizes whose scan of
    one segment has two sequences at 32-byte subsequences (more than 240 of them)."""
    from tools import jpegsynth

    out = {"plain": jpegsynth.encode(512, 384, quality=75, noise=6, seed=71), "rstrow": jpegsynth.encode(512, 384, restart_interval=32, quality=75, noise=6, seed=72)}
    for side in range(64, 513, 16):
        data = jpegsynth.encode(side, side, quality=90, noise=12, seed=73)
        if len(data) - scan_begin(data) > 250 * 32:
            out["twoseq"] = data
            break
    return out


def destuffed_offsets(data):
    """[(file offset of a data byte, restart interval, its offset in the interval's destuffed data)] of the first scan."""
    out, i, n, seg, k = [], scan_begin(data), len(data), 0, 0
    while i < n:
        if data[i] == 0xFF:
            m = data[i + 1]
            if m == 0:
                out.append((i, seg, k))
                k += 1
                i += 2
                continue
            if 0xD0 <= m <= 0xD7:
                seg, k = seg + 1, 0
                i += 2
                continue
            break
        out.append((i, seg, k))
        k += 1
        i += 1
    return out


def boundary_cuts(data, subseq_bytes, around=2, segments=(0,), rows=(1, 5)):
    """File lengths whose last destuffed byte is the last byte of a subsequence, or the first byte of one, for the
    subsequences `rows` of the restart intervals `segments`, and the `around` lengths to either side of each; plus a cut in the
    first subsequence of each of those intervals and one in its last."""
    offs = destuffed_offsets(data)
    cuts = set()
    for seg in segments:
        mine = [(o, k) for o, s, k in offs if s == seg]
        if not mine:
            continue
        by_k = {k: o for o, k in mine}
        last_k = mine[-1][1]
        for r in rows:
            for k in (r * subseq_bytes - 1, r * subseq_bytes):  # the byte that ends a subsequence, the byte that starts one
                if k in by_k:
                    for d in range(-around, around + 1):
                        cuts.add(by_k[k] + 1 + d)
        cuts.add(by_k[min(3, last_k)] + 1)
        cuts.add(by_k[max(last_k - 2, 0)] + 1)
    b = scan_begin(data)
    return sorted(c for c in cuts if b <= c <= len(data))
