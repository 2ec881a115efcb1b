"""Colour models of JPEG files restated: which model libjpeg (and so Pillow) takes a file for, and the RGB that
Image.open(f).convert("RGB") makes of each -- after draft() too. Built on the upsampling of tests/libjpeg_ref.py and
tests/draft_ref.py; the library's jpeggpu_ext_get_color_space and its jpeggpu_ext_*_cs calls must agree with it.

  * the model (jdapimin.c, default_decompress_parms): one component is grey; of three, a JFIF APP0 segment says YCbCr even
    beside an Adobe segment, else an Adobe APP14 segment's transform (0: RGB, anything else: YCbCr), else the component
    ids ('R', 'G', 'B': RGB, anything else: YCbCr); of four, an Adobe transform other than 0 says YCCK, everything else CMYK;
  * RGB-coded files: the upsampled samples as they are;
  * CMYK: Pillow reads every CMYK JPEG as Adobe's inverted samples ("CMYK;I") and converts with cmyk2rgb (Convert.c):
    with the stored samples s_i, the inks c_i = 255 - s_i and K = s_3, out_i = K - MULDIV255(c_i, K), MULDIV255(a, b) =
    ((t >> 8) + t) >> 8 for t = a b + 128;
  * YCCK: libjpeg's ycck_cmyk_convert hands out 255 - r, 255 - g, 255 - b of jdcolor.c's YCbCr conversion in place of the
    stored samples, and K unchanged; Pillow inverts them like any CMYK file's: the CMYK rule with the inks c_i = r, g, b.

Also the byte helpers that make such files of tools.jpegsynth's: application segments spliced in behind SOI, component ids
patched in the frame and scan headers.
"""
import functools

import numpy as np

from tests import draft_ref, libjpeg_ref

UNKNOWN, GRAY, YCBCR, RGB, CMYK, YCCK = range(6)  # enum jpeggpu_ext_color_space
NAMES = ("UNKNOWN", "GRAY", "YCBCR", "RGB", "CMYK", "YCCK")
SCALES = (1, 2, 4, 8)
IDS_RGB = (82, 71, 66)


# ------------------------------------------------------------------------------------------------
# bytes
# ------------------------------------------------------------------------------------------------

def app0_jfif(length=16):
    """A JFIF APP0 segment (version 1.01, no thumbnail); `length` below 16 cuts it short."""
    body = b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00"
    return b"\xff\xe0" + bytes([length >> 8, length & 255]) + body[:length - 2]


def app14_adobe(transform, length=14):
    """An Adobe APP14 segment (version 100, no flags) with the given transform byte; `length` 13 ends in front of it."""
    body = b"Adobe\x00\x64\x00\x00\x00\x00" + bytes([transform])
    return b"\xff\xee" + bytes([length >> 8, length & 255]) + body[:length - 2]


def splice(data, *segments):
    """`segments` put behind the SOI marker, in that order."""
    assert data[:2] == b"\xff\xd8"
    return data[:2] + b"".join(segments) + data[2:]


def segments_of(data):
    """[(marker, offset of the length field, length)] of the marker segments of a baseline file, entropy-coded data and
    stand-alone markers skipped."""
    out, i = [], 2
    while i + 4 <= len(data):
        assert data[i] == 0xFF, i
        m = data[i + 1]
        if m == 0xFF:  # fill byte
            i += 1
            continue
        if m == 0xD9:
            break
        n = data[i + 2] << 8 | data[i + 3]
        out.append((m, i + 2, n))
        i += 2 + n
        if m == 0xDA:  # entropy-coded data up to the next marker that is neither stuffing nor a restart marker
            while not (data[i] == 0xFF and data[i + 1] != 0 and not 0xD0 <= data[i + 1] <= 0xD7 and data[i + 1] != 0xFF):
                i += 1
    return out


def patch_ids(data, ids):
    """The frame's component ids replaced by `ids`, in the SOF segment and in every scan header."""
    b = bytearray(data)
    old = None
    for m, off, n in segments_of(data):
        if m in (0xC0, 0xC1):
            nc = b[off + 7]
            assert nc == len(ids)
            old = [b[off + 8 + 3 * c] for c in range(nc)]
            for c in range(nc):
                b[off + 8 + 3 * c] = ids[c]
        elif m == 0xDA:
            for a in range(b[off + 2]):
                b[off + 3 + 2 * a] = ids[old.index(b[off + 3 + 2 * a])]
    return bytes(b)


def model_of(ncomp, ids=(1, 2, 3, 4), jfif=False, adobe=None):
    """libjpeg's choice; `adobe`: the transform byte of an Adobe segment, None without one."""
    if ncomp == 1:
        return GRAY
    if ncomp == 3:
        if jfif:
            return YCBCR
        if adobe is not None:
            return RGB if adobe == 0 else YCBCR
        return RGB if tuple(ids[:3]) == IDS_RGB else YCBCR
    if ncomp == 4:
        return YCCK if adobe is not None and adobe != 0 else CMYK
    return UNKNOWN


def model_of_file(data):
    """model_of from the file's own segments (those in front of the first scan)."""
    jfif, adobe, ids = False, None, ()
    for m, off, n in segments_of(data):
        body = data[off + 2:off + n]
        if m == 0xE0 and n >= 16 and body[:5] == b"JFIF\0":
            jfif = True
        elif m == 0xEE and n >= 14 and body[:5] == b"Adobe":
            adobe = body[11]
        elif m in (0xC0, 0xC1):
            ids = tuple(data[off + 8 + 3 * c] for c in range(data[off + 7]))
        elif m == 0xDA:
            break
    return model_of(len(ids), ids, jfif, adobe)


# ------------------------------------------------------------------------------------------------
# pixels
# ------------------------------------------------------------------------------------------------

def muldiv255(a, b):
    t = a * b + 128
    return ((t >> 8) + t) >> 8


def cmyk_to_rgb(ink, k):
    """Pillow's cmyk2rgb: `ink` (H, W, 3) the inks (255 - the samples libjpeg hands out), `k` (H, W) the stored fourth."""
    ink, k = ink.astype(np.int64), k.astype(np.int64)[:, :, None]
    return np.clip(k - muldiv255(ink, k), 0, 255).astype(np.uint8)


def convert(full, model):
    """(H, W, 3) uint8 of the upsampled planes `full` read as `model`."""
    want = {GRAY: 1, YCBCR: 3, RGB: 3, CMYK: 4, YCCK: 4}[model]
    assert len(full) == want, (len(full), NAMES[model])
    if model == GRAY:
        return np.repeat(full[0][:, :, None], 3, axis=2)
    if model == YCCK:
        return cmyk_to_rgb(libjpeg_ref.ycc_to_rgb(*full[:3]), full[3])
    if model == CMYK:
        return cmyk_to_rgb(255 - np.stack(full[:3], axis=-1).astype(np.int64), full[3])
    return libjpeg_ref.ycc_to_rgb(*full) if model == YCBCR else np.stack(full, axis=-1)


def upsampled(planes, eh, ev, width, height, fancy):
    """Every plane at the image's size: libjpeg's fancy upsamplers, or replication (1/8 in libjpeg's scale mode)."""
    hm, vm = max(eh), max(ev)
    assert all(hm % h == 0 for h in eh) and all(vm % v == 0 for v in ev), "non-integral ratio"
    if fancy:
        return [libjpeg_ref.upsample_fancy(p, hm // h, vm // v, width, height) for p, h, v in zip(planes, eh, ev)]
    return [np.repeat(np.repeat(p, vm // v, axis=0), hm // h, axis=1)[:height, :width] for p, h, v in zip(planes, eh, ev)]


def color_rgb_of(dec, model, d=1):
    """Pillow's convert("RGB") of an oracle.Decoded read as `model`, at 1 / d (d > 1: after draft())."""
    hs, vs = draft_ref.factors_of(dec)
    eh, ev = draft_ref.effective_factors(hs, vs, d) if d > 1 else (hs, vs)
    width, height = draft_ref.ceil_div(dec.width, d), draft_ref.ceil_div(dec.height, d)
    return convert(upsampled(draft_ref.draft_planes_of(dec, d), eh, ev, width, height, d == 1 or draft_ref.fancy(d)), model)


def color_rgb(data, d=1):
    from oracle import oracle

    return color_rgb_of(oracle.decode(data), model_of_file(data), d)


def pillow_rgb(data, d=1):
    """(np.asarray(im.convert("RGB")), im.size), after im.draft("RGB", (W // d, H // d)) if d > 1. Needs Pillow."""
    if d == 1:
        a = libjpeg_ref.pillow_rgb(data)
        return a, (a.shape[1], a.shape[0])
    return draft_ref.pillow_draft_rgb(data, d)


def draft_comparable(width, height, d):
    """draft() returns the image at 1 / d (tests/draft_ref.pillow_comparable's size rule)."""
    s = draft_ref.pillow_scale(width, height, (max(width // d, 1), max(height // d, 1)))
    return (draft_ref.ceil_div(width, s), draft_ref.ceil_div(height, s)) == (draft_ref.ceil_div(width, d), draft_ref.ceil_div(height, d))


# ------------------------------------------------------------------------------------------------
# the case list
# ------------------------------------------------------------------------------------------------

C444 = ((1, 1),) * 4
C2111_21 = ((2, 1), (1, 1), (1, 1), (2, 1))
C2211_22 = ((2, 2), (1, 1), (1, 1), (2, 2))
C22_21 = ((2, 2), (2, 1), (1, 1), (1, 1))  # component 1 is h1v2
C2111 = ((2, 2), (1, 1), (1, 1), (1, 1))   # K is upsampled
S444 = ((1, 1),) * 3
S420 = ((2, 2), (1, 1), (1, 1))

FOUR = (("c444", C444, 69, 37), ("c21", C2111_21, 264, 200), ("c22", C2211_22, 333, 251), ("c22_21", C22_21, 69, 37),
        ("c22_k1", C2111, 69, 37), ("c22_tiny", C2211_22, 3, 5))
THREE = (("s444", S444, 69, 37), ("s420_seam", S420, 264, 200), ("s420", S420, 333, 251), ("s420_tiny", S420, 3, 5))


@functools.lru_cache(maxsize=1)
def cases():
    """name -> (bytes, model): four components plain, with Adobe transform 0 and with 2; three components with Adobe
    transform 0, with the ids 'R', 'G', 'B', and with Adobe transform 1 (the control: YCbCr); a YCCK file with restart
    markers and one of four scans."""
    from tools import jpegsynth

    out = {}
    for k, (name, sampling, w, h) in enumerate(FOUR):
        base = jpegsynth.encode(w, h, sampling, quality=90, noise=8, seed=300 + k)
        out[name + "_plain"] = (base, CMYK)
        out[name + "_adobe0"] = (splice(base, app14_adobe(0)), CMYK)
        out[name + "_adobe2"] = (splice(base, app14_adobe(2)), YCCK)
    for k, (name, sampling, w, h) in enumerate(THREE):
        base = jpegsynth.encode(w, h, sampling, quality=90, noise=8, seed=320 + k)
        out[name + "_adobe0"] = (splice(base, app14_adobe(0)), RGB)
        out[name + "_ids"] = (patch_ids(base, IDS_RGB), RGB)
        out[name + "_adobe1"] = (splice(base, app14_adobe(1)), YCBCR)
    out["ycck_dri"] = (splice(jpegsynth.encode(333, 251, C2211_22, restart_interval=5, quality=85, noise=8, seed=340), app14_adobe(2)), YCCK)
    out["ycck_ni"] = (splice(jpegsynth.encode(69, 37, C2211_22, interleaved=False, quality=85, noise=8, seed=341), app14_adobe(2)), YCCK)
    return out


def frame_size(data):
    """(width, height) from the frame header."""
    off = next(off for m, off, n in segments_of(data) if m in (0xC0, 0xC1))
    return data[off + 5] << 8 | data[off + 6], data[off + 3] << 8 | data[off + 4]


def comparable(name, d):
    """The one exclusion from comparisons with Pillow: a file and scale for which draft() does not return the 1 / d size
    (the 3 x 5 files at d > 1)."""
    return d == 1 or draft_comparable(*frame_size(cases()[name][0]), d)
