"""EXIF orientation restated: which Orientation a JPEG file carries, as Pillow reads it, and what the eight values do to an
image. The library's jpeggpu_ext_get_orientation, jpeggpu_ext_orient_size / _rect and its oriented outputs must agree.

The rule (jg_reader.cpp, exif_orientation), checked against Image.open(f).getexif().get(0x0112) and
ImageOps.exif_transpose on every case of cases() (tests/test_exif_ref.py):

  * the APP1 segments in front of the first scan that begin "Exif\\0\\0" hold the data: the first one's, with the data of
    every later one (behind its six bytes) appended, as Pillow joins them; so the first segment decides unless it is cut short;
  * behind the six bytes a TIFF header of 8 bytes: "II" (little endian) with the number 42 in either byte order, or "MM"
    with 42 in either order or 43 (Pillow's list of prefixes), and the offset of IFD0 from the header;
  * IFD0 is a 16-bit entry count and 12-byte entries (tag, type, count, value), read one by one while whole entries lie in
    the data: a count that says more than there is does not matter;
  * an entry with tag 0x0112, a TIFF type 1..13 or 16, count x size of the type not 0 and its value inside the data (at the
    offset the value field holds if it takes more than 4 bytes) sets the value -- the first of `count` -- and a later such
    entry replaces an earlier. Types SHORT, LONG, SSHORT and SLONG give an integer, and 1..8 are the orientation;
  * everything else is orientation 1: no segment, a truncated or malformed one, an offset outside it, a BYTE (Pillow gets
    bytes, which are no orientation), the values 0 and 9..65535. (A RATIONAL or FLOAT of value 6 Pillow would take for 6;
    neither this restatement nor the library does.)
Pillow's fallback to an XMP tiff:Orientation attribute is not restated (the library does not read XMP).

The eight values, with S the stored image W x H and O the displayed one:
    1  O[y][x] = S[y][x]            5  O[y][x] = S[x][y]              (5..8: O is H x W)
    2  S[y][W-1-x]                  6  S[H-1-x][y]
    3  S[H-1-y][W-1-x]              7  S[H-1-x][W-1-y]
    4  S[H-1-y][x]                  8  S[x][W-1-y]
"""
import struct

import numpy as np

TAG = 0x0112
BYTE, SHORT, LONG = 1, 3, 4
SIZES = {BYTE: 1, SHORT: 2, LONG: 4}


# ------------------------------------------------------------------------------------------------
# bytes
# ------------------------------------------------------------------------------------------------

def ifd_entry(endian, tag, typ, count, value):
    """A 12-byte IFD entry whose value is stored inline, left-justified as TIFF does."""
    e = "<" if endian == "II" else ">"
    fmt = {BYTE: "B", SHORT: "H", LONG: "I"}[typ]
    inline = struct.pack(e + fmt * min(count, 4 // SIZES[typ]), *([value] * min(count, 4 // SIZES[typ])))
    return struct.pack(e + "HHI", tag, typ, count) + inline.ljust(4, b"\0")


def tiff(endian="II", entries=(), ifd_offset=8, entry_count=None, magic=42):
    """A TIFF header and IFD0 with the given entries at `ifd_offset` (a gap of zeros in front if it is more than 8);
    `entry_count`: what the count field says, if not the truth."""
    e = "<" if endian == "II" else ">"
    n = len(entries) if entry_count is None else entry_count
    body = struct.pack(e + "H", n) + b"".join(entries) + struct.pack(e + "I", 0)
    return endian.encode() + struct.pack(e + "HI", magic, ifd_offset) + b"\0" * max(ifd_offset - 8, 0) + body


def app1_exif(payload, length=None):
    """An APP1 segment "Exif\\0\\0" + payload; `length` cuts it short (the field says `length`, and so many bytes follow)."""
    body = b"Exif\0\0" + payload
    n = len(body) + 2 if length is None else length
    return b"\xff\xe1" + struct.pack(">H", n) + body[:n - 2]


def orientation_segment(value, endian="II", typ=SHORT, count=1, where="only", ifd_offset=8):
    """An Exif segment whose IFD0 holds the Orientation tag with `value`: alone, or first / last among other tags."""
    o = ifd_entry(endian, TAG, typ, count, value)
    a = ifd_entry(endian, 0x0100, LONG, 1, 40)
    b = ifd_entry(endian, 0x0131, SHORT, 1, 7)
    c = ifd_entry(endian, 0x011A, SHORT, 1, 3)
    entries = {"only": [o], "first": [o, b, c], "last": [a, c, o], "absent": [a, b]}[where]
    return app1_exif(tiff(endian, entries, ifd_offset))


def splice(data, *segments, before=None):
    """`segments` put behind SOI, or in front of the first marker `before`."""
    assert data[:2] == b"\xff\xd8"
    at = 2 if before is None else data.index(bytes([0xFF, before]))
    return data[:at] + b"".join(segments) + data[at:]


def splice_after_first(data, marker, *segments):
    """`segments` put behind the first segment with `marker`."""
    at = data.index(bytes([0xFF, marker]))
    at += 2 + (data[at + 2] << 8 | data[at + 3])
    return data[:at] + b"".join(segments) + data[at:]


def segments():
    """{name: (bytes to splice behind SOI, expected orientation)}: the list of Exif segments every layer is tested on."""
    from tests.color_ref import app0_jfif, app14_adobe

    out = {}
    for en in ("II", "MM"):
        for v in range(1, 9):
            out["%s short %d" % (en, v)] = (orientation_segment(v, en), v)
        out["%s long 6" % en] = (orientation_segment(6, en, LONG), 6)
        out["%s byte 6" % en] = (orientation_segment(6, en, BYTE), 1)
        out["%s count 2" % en] = (orientation_segment(6, en, SHORT, 2), 6)  # Pillow takes the first of two
        out["%s first 3" % en] = (orientation_segment(3, en, where="first"), 3)
        out["%s last 8" % en] = (orientation_segment(8, en, where="last"), 8)
        out["%s absent" % en] = (orientation_segment(8, en, where="absent"), 1)
        out["%s value 0" % en] = (orientation_segment(0, en), 1)
        out["%s value 9" % en] = (orientation_segment(9, en), 1)
        out["%s value 0x0106" % en] = (orientation_segment(0x0106, en), 1)
        out["%s long 0x10006" % en] = (orientation_segment(0x10006, en, LONG), 1)
        out["%s ifd gap" % en] = (orientation_segment(5, en, ifd_offset=20), 5)
        t = tiff(en, [ifd_entry(en, TAG, SHORT, 1, 6)])
        out["%s ifd past the end" % en] = (app1_exif(t[:4] + struct.pack("<I" if en == "II" else ">I", 4000) + t[8:]), 1)
        out["%s entry count too large" % en] = (app1_exif(tiff(en, [ifd_entry(en, TAG, SHORT, 1, 6)], entry_count=40)), 6)
        out["%s wrong magic" % en] = (app1_exif(tiff(en, [ifd_entry(en, TAG, SHORT, 1, 6)], magic=43)), 1 if en == "II" else 6)  # "MM" 00 2B is on Pillow's list
        full = orientation_segment(6, en)
        for n in (8, 13, 14):
            out["%s length %d" % (en, n)] = (app1_exif(tiff(en, [ifd_entry(en, TAG, SHORT, 1, 6)]), length=n), 1)
        out["%s entry cut" % en] = (full[:2] + struct.pack(">H", 8 + 8 + 2 + 10) + full[4:4 + 6 + 8 + 2 + 10], 1)
        out["%s behind JFIF" % en] = (app0_jfif() + orientation_segment(7, en), 7)
        out["%s behind Adobe" % en] = (app14_adobe(1) + orientation_segment(4, en), 4)
        out["%s two segments" % en] = (orientation_segment(6, en) + orientation_segment(3, en), 6)
        out["%s bad first, good second" % en] = (app1_exif(tiff(en, [ifd_entry(en, TAG, SHORT, 1, 6)], magic=43)) + orientation_segment(3, en),
                                                   1 if en == "II" else 6)
    out["no byte order"] = (app1_exif(b"XX" + tiff("II", [ifd_entry("II", TAG, SHORT, 1, 6)])[2:]), 1)
    out["not Exif"] = (b"\xff\xe1" + struct.pack(">H", 2 + 29) + b"http://ns.adobe.com/xap/1.0/\0", 1)
    out["none"] = (b"", 1)
    return out


def cases(base):
    """{name: (file, expected orientation)} of `base` (a baseline or progressive file) with every segment of segments()
    behind SOI, and one segment put behind the first DQT."""
    out = {name: (splice(base, seg), want) for name, (seg, want) in segments().items()}
    out["after a DQT"] = (splice_after_first(base, 0xDB, orientation_segment(8, "MM")), 8)
    return out


# ------------------------------------------------------------------------------------------------
# the rule
# ------------------------------------------------------------------------------------------------

UNITS = {1: 1, 2: 1, 3: 2, 4: 4, 5: 8, 6: 1, 7: 1, 8: 2, 9: 4, 10: 8, 11: 4, 12: 8, 13: 4, 16: 8}  # TIFF types Pillow reads
INTS = {3: "H", 4: "I", 8: "h", 9: "i"}
PREFIXES = (b"II\x2a\x00", b"II\x00\x2a", b"MM\x00\x2a", b"MM\x2a\x00", b"MM\x00\x2b")


def orientation_of_exif(d):
    """The orientation of Exif data: the first Exif segment's data with that of later ones (behind their six bytes)."""
    while d[:6] == b"Exif\0\0":
        d = d[6:]
    if len(d) < 8 or d[:4] not in PREFIXES:
        return 1
    e = "<" if d[:2] == b"II" else ">"
    (ifd,) = struct.unpack(e + "I", d[4:8])
    if ifd > len(d) or len(d) - ifd < 2:
        return 1
    (n,) = struct.unpack(e + "H", d[ifd:ifd + 2])
    value = 1
    for i in range(n):
        at = ifd + 2 + 12 * i
        if len(d) - at < 12:
            break  # entries are read one by one while whole ones are there
        tag, typ, count = struct.unpack(e + "HHI", d[at:at + 8])
        if tag != TAG or typ not in UNITS:
            continue
        size = count * UNITS[typ]
        if size == 0:
            continue
        at += 8
        if size > 4:
            (at,) = struct.unpack(e + "I", d[at:at + 4])
            if at > len(d) or len(d) - at < size:
                continue
        value = struct.unpack(e + INTS[typ], d[at:at + UNITS[typ]])[0] if typ in INTS else 1  # a later entry replaces
    return value if 1 <= value <= 8 else 1


def orientation_of_file(data):
    """The orientation of a JPEG file, from the Exif APP1 segments in front of its first scan."""
    i, exif = 2, None
    while i + 4 <= len(data):
        if data[i] != 0xFF:
            break
        m = data[i + 1]
        if m == 0xFF:
            i += 1
            continue
        if m in (0xDA, 0xD9):
            break
        n = data[i + 2] << 8 | data[i + 3]
        if m == 0xE1 and n >= 8 and i + 2 + n <= len(data) and data[i + 4:i + 10] == b"Exif\0\0":
            exif = data[i + 4:i + 2 + n] if exif is None else exif + data[i + 10:i + 2 + n]
        i += 2 + n
    return 1 if exif is None else orientation_of_exif(exif)


# ------------------------------------------------------------------------------------------------
# the eight values
# ------------------------------------------------------------------------------------------------

def transposes(o):
    return o >= 5


def orient_size(o, w, h):
    return (h, w) if transposes(o) else (w, h)


def apply(img, o):
    """The displayed image of a stored (H, W[, C]) array: the table of the module's docstring."""
    if o == 1:
        return img
    if o == 2:
        return img[:, ::-1]
    if o == 3:
        return img[::-1, ::-1]
    if o == 4:
        return img[::-1]
    t = np.swapaxes(img, 0, 1)  # t[y][x] = S[x][y]
    if o == 5:
        return t
    if o == 6:
        return t[:, ::-1]  # S[H-1-x][y]
    if o == 7:
        return t[::-1, ::-1]
    if o == 8:
        return t[::-1]  # S[x][W-1-y]
    raise ValueError(o)


def orient_rect(o, w, h, x, y, rw, rh):
    """The stored rectangle (x, y, w, h) of the displayed rectangle (x, y, rw, rh) of a stored w x h image."""
    ow, oh = orient_size(o, w, h)
    assert 0 <= x and 0 <= y and rw >= 1 and rh >= 1 and x + rw <= ow and y + rh <= oh
    if o == 1:
        return x, y, rw, rh
    if o == 2:
        return w - x - rw, y, rw, rh
    if o == 3:
        return w - x - rw, h - y - rh, rw, rh
    if o == 4:
        return x, h - y - rh, rw, rh
    if o == 5:
        return y, x, rh, rw
    if o == 6:
        return y, h - x - rw, rh, rw
    if o == 7:
        return w - y - rh, h - x - rw, rh, rw
    return w - y - rh, x, rh, rw


# ------------------------------------------------------------------------------------------------
# the files and resize cases of the GPU tests (tools/make_exif_pins.py pins Pillow's outputs for them)
# ------------------------------------------------------------------------------------------------

SCALES = (1, 2, 8)
TILE = 64  # the transposing conversion's tile side (jg_output.hpp, kOrientTile): sizes one less and one more are cases
S420, S422, S440, S444 = ((2, 2), (1, 1), (1, 1)), ((2, 1), (1, 1), (1, 1)), ((1, 2), (1, 1), (1, 1)), ((1, 1),) * 3
FILTERS = ("bilinear", "bicubic")
RESIZE_FILES = ("s420", "wide")
RESIZE_SIZES = ((24, 16), (16, 24))  # (width, height)


def gpu_files():
    """name -> (file without Exif, its baseline twin for the restatement): 53 x 37 in every sampling layout, grey and
    YCCK; 17 x 9; one pixel wide and one high; 300 x 20 and 20 x 300, across the row kernel's 256-wide tile and the
    transposing tile both ways; a width and a height one less and one more than that tile; one progressive file."""
    import os

    from tests.color_ref import app14_adobe, splice as color_splice
    from tools import jpegsynth

    enc = lambda w, h, s, seed: jpegsynth.encode(w, h, s, quality=90, noise=8, seed=seed)
    out = {
        "s420": enc(53, 37, S420, 700), "s422": enc(53, 37, S422, 701), "s440": enc(53, 37, S440, 702),
        "s444": enc(53, 37, S444, 703), "gray": enc(53, 37, ((1, 1),), 704),
        "ycck": color_splice(enc(53, 37, ((2, 2), (1, 1), (1, 1), (2, 2)), 705), app14_adobe(2)),
        "odd": enc(17, 9, S420, 706), "col": enc(1, 40, S420, 707), "row": enc(40, 1, S420, 708),
        "wide": enc(300, 20, S420, 709), "tall": enc(20, 300, S420, 710),
        "t63x65": enc(TILE - 1, TILE + 1, S420, 711), "t65x63": enc(TILE + 1, TILE - 1, S422, 712),
    }
    out = {k: (v, v) for k, v in out.items()}
    pins = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "progressive_pins.npz"))
    out["prog"] = (pins["prog/p420"].tobytes(), pins["twin/p420"].tobytes())
    return out


def frame_size(data):
    """(width, height) from the frame header of a baseline or progressive file."""
    i = 2
    while data[i + 1] not in (0xC0, 0xC1, 0xC2):
        i += 2 + (data[i + 2] << 8 | data[i + 3])
    return data[i + 7] << 8 | data[i + 8], data[i + 5] << 8 | data[i + 6]


def with_orientation(data, o):
    """The file with an Exif segment of orientation `o` behind SOI (byte order by the value's parity)."""
    return splice(data, orientation_segment(o, "MM" if o % 2 else "II"))


def batch_cases():
    """The eight-image batch of decode_resized(exif_transpose=True): (file name, orientation, displayed crop (x, y, w, h))
    with seeded crops, one image per orientation."""
    files = gpu_files()
    rng = np.random.default_rng(812)
    names = ("s420", "wide", "gray", "tall", "ycck", "s422", "t65x63", "prog")
    out = []
    for o, name in zip(range(1, 9), names):
        w, h = orient_size(o, *frame_size(files[name][0]))
        cw, ch = int(rng.integers(max(w // 2, 1), w + 1)), int(rng.integers(max(h // 2, 1), h + 1))
        out.append((name, o, (int(rng.integers(0, w - cw + 1)), int(rng.integers(0, h - ch + 1)), cw, ch)))
    return out


def resize_swapped(a, out_w, out_h, filt):
    """pillow_resample_ref.resize with the passes in the wrong order: the vertical, rounded pass first. A resize case
    whose result this does not change proves nothing about the order of the passes."""
    from tests import pillow_resample_ref as R

    return np.swapaxes(R.resize(np.swapaxes(a, 0, 1), out_h, out_w, filt), 0, 1)
