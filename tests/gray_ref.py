"""libjpeg-turbo's grey output restated in numpy: what np.asarray(im) is after Pillow's im.draft("L", (W // d, H // d)), and
what the library's grey calls (decode_to_gray, decode_batch_to_gray, mode="L") must produce.

With out_color_space = JCS_GRAYSCALE a YCbCr file's chroma components are not needed (jdmaster.c), so the grey is component
0 at its own IDCT size (tests/draft_ref.py), upsampled only where its sampling factors are below the frame's largest; a
grey file is its one component; an RGB-coded file is decoded whole and converted by jdcolor.c's rgb_gray_convert. CMYK
and YCCK files have no grey: Pillow's draft("L") leaves them as they are. ImageOps.exif_transpose, crop and resize then
act on an "L" image: tests/exif_ref.py and tests/pillow_resample_ref.py on one band.
"""
import os

import numpy as np

from tests import center_crop_ref, color_ref, draft_ref, exif_ref, libjpeg_ref, pillow_resample_ref

SCALES = (1, 2, 4, 8)
SIZES = ((1, 1), (9, 7), (17, 33), (83, 61), (80, 64))  # (width, height)
S444, S422, S420, S440, S411 = ((1, 1),) * 3, ((2, 1), (1, 1), (1, 1)), ((2, 2), (1, 1), (1, 1)), ((1, 2), (1, 1), (1, 1)), ((4, 1), (1, 1), (1, 1))
LUMA_SMALL = ((1, 1), (2, 2), (1, 1))  # cases.SWEEP_LAYOUTS["y1x1_cb2x2"]: luma itself is upsampled
RESIZES = ((24, 17), (5, 3), (224, 224))  # (width, height), from 83 x 61: down and up


def rgb_to_gray(r, g, b):
    """jdcolor.c, rgb_gray_convert: FIX(0.29900), FIX(0.58700), FIX(0.11400), ONE_HALF, SCALEBITS 16."""
    r, g, b = (np.asarray(v).astype(np.int64) for v in (r, g, b))
    return ((19595 * r + 38470 * g + 7471 * b + 32768) >> 16).astype(np.uint8)


def gray_of(dec, model, d=1):
    """The (H, W) uint8 grey at 1 / d of an oracle.Decoded read as colour model `model` (tests/color_ref.py)."""
    if model not in (color_ref.GRAY, color_ref.YCBCR, color_ref.RGB):
        raise ValueError("no grey of colour model %r" % (model,))
    hs, vs = draft_ref.factors_of(dec)
    eh, ev = draft_ref.effective_factors(hs, vs, d) if d > 1 else (hs, vs)
    width, height = draft_ref.ceil_div(dec.width, d), draft_ref.ceil_div(dec.height, d)
    planes = draft_ref.draft_planes_of(dec, d)
    fancy = d == 1 or draft_ref.fancy(d)
    if model == color_ref.RGB:
        return rgb_to_gray(*color_ref.upsampled(planes, eh, ev, width, height, fancy))
    hr, vr = max(eh) // eh[0], max(ev) // ev[0]
    assert max(eh) % eh[0] == 0 and max(ev) % ev[0] == 0, "non-integral ratio"
    if fancy:
        return libjpeg_ref.upsample_fancy(planes[0], hr, vr, width, height)
    return np.repeat(np.repeat(planes[0], vr, axis=0), hr, axis=1)[:height, :width]


def gray(data, d=1, orientation=1, crop=None):
    """decode_to_gray's result: the grey at 1 / d, displayed by `orientation`, then the rectangle crop = (x, y, w, h)."""
    from oracle import oracle

    a = exif_ref.apply(gray_of(oracle.decode(data), color_ref.model_of_file(data), d), orientation)
    if crop is not None:
        x, y, w, h = crop
        a = a[y:y + h, x:x + w]
    return np.ascontiguousarray(a)


def resize(a, out_w, out_h, filt):
    """Image.fromarray(a).resize((out_w, out_h), filter) of an (H, W) "L" array."""
    return pillow_resample_ref.resize(a, out_w, out_h, filt)


def resize_center_crop(a, size, crop, filt):
    return center_crop_ref.resize_center_crop(a, size, crop, filt)


def pillow_gray(data, d=1, orientation=None):
    """np.asarray(im) after im.draft("L", (W // d, H // d)) (and ImageOps.exif_transpose). Needs Pillow."""
    import io

    from PIL import Image, ImageOps

    im = Image.open(io.BytesIO(data))
    w, h = im.size
    im.draft("L", (max(w // d, 1), max(h // d, 1)))
    if orientation is not None:
        im = ImageOps.exif_transpose(im)
    return np.asarray(im), im.mode


# ------------------------------------------------------------------------------------------------
# the files of the tests (tools/make_gray_pins.py pins Pillow's outputs for them)
# ------------------------------------------------------------------------------------------------

def files():
    """name -> bytes. Every sampling at 83 x 61, 4:2:0 at every size of SIZES, a grey and an RGB-coded file, restart
    intervals of one MCU and of one MCU row, a non-interleaved baseline file, a progressive file, luma smaller than chroma."""
    from tools import jpegsynth

    enc = lambda w, h, s, seed, **kw: jpegsynth.encode(w, h, s, quality=90, noise=8, seed=seed, **kw)
    out = {"s444": enc(83, 61, S444, 900), "s422": enc(83, 61, S422, 901), "s420": enc(83, 61, S420, 902), "s440": enc(83, 61, S440, 903),
           "s411": enc(83, 61, S411, 904), "gray": enc(83, 61, ((1, 1),), 905),
           "rgb": color_ref.patch_ids(enc(83, 61, S444, 906), color_ref.IDS_RGB), "rgb420": color_ref.patch_ids(enc(17, 33, S420, 907), color_ref.IDS_RGB),
           "luma_small": enc(83, 61, LUMA_SMALL, 908), "dri1": enc(83, 61, S420, 909, restart_interval=1),
           "drirow": enc(83, 61, S420, 910, restart_interval=6), "ni": enc(83, 61, S420, 911, interleaved=False)}
    for k, (w, h) in enumerate(SIZES):
        out["s420_%dx%d" % (w, h)] = enc(w, h, S420, 920 + k)
        out["s422_%dx%d" % (w, h)] = enc(w, h, S422, 930 + k)
    pins = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "progressive_pins.npz"))
    out["prog"] = pins["prog/p420"].tobytes()
    out["prog_twin"] = pins["twin/p420"].tobytes()
    return out


def frame_size(data):
    return exif_ref.frame_size(data)


def twin(files_, name):
    """The baseline file whose coefficients are `name`'s: what the oracle decodes for a progressive file."""
    return files_["prog_twin"] if name == "prog" else files_[name]


def names(files_):
    return [n for n in files_ if n != "prog_twin"]


ORIENT_FILE, ORIENT_SCALE = "s420", 2     # Pillow's exif_transpose of an "L" draft: every orientation of one file
RESIZE_FILE = "s420"                       # Pillow's resize of the "L" image, both filters, RESIZES
FILTERS = pillow_resample_ref.FILTERS


def pin_keys(files_):
    """Every pinned array: (key, function of nothing that makes Pillow's array). Scales where Pillow's draft picks another
    size than 1 / d (tiny images: color_ref.draft_comparable) are not pinned."""
    out = []
    for name in names(files_):
        data = files_[name]
        w, h = frame_size(data)
        for d in SCALES:
            if d == 1 or color_ref.draft_comparable(w, h, d):
                out.append(("L/%s/%d" % (name, d), lambda data=data, d=d: pillow_gray(data, d)[0]))
    for o in range(1, 9):
        data = exif_ref.with_orientation(files_[ORIENT_FILE], o)
        out.append(("exif/%d" % o, lambda data=data: pillow_gray(data, ORIENT_SCALE, orientation=True)[0]))
    for filt in FILTERS:
        for ow, oh in RESIZES:
            out.append(("resize/%s/%dx%d" % (filt, ow, oh),
                        lambda filt=filt, ow=ow, oh=oh: pillow_resample_ref.pillow_resize(pillow_gray(files_[RESIZE_FILE], 1)[0], ow, oh, filt)))
    return out


PIN_ARRAY_MAX = 6000  # larger arrays are pinned by their shape and SHA-256


def to_pin(a):
    import hashlib

    a = np.ascontiguousarray(a, dtype=np.uint8)
    if a.size <= PIN_ARRAY_MAX:
        return a
    return np.concatenate([np.array(a.shape, np.int64).view(np.uint8), np.frombuffer(hashlib.sha256(a.tobytes()).digest(), np.uint8)])


def matches_pin(a, pin):
    """`a` is the pinned array (or has its shape and hash)."""
    return np.array_equal(to_pin(a), pin)


def load_pins():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gray_pins.npz"))
