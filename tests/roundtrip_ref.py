"""CPU restatement of a JPEG round trip (jpeggpu_ext_roundtrip_batch, jpeg_roundtrip): the pixels of
np.asarray(Image.open(buf)) after Image.fromarray(a).save(buf, "JPEG", quality=q, subsampling=s) on Pillow with
libjpeg-turbo, without the file. Entropy coding is lossless, so the chain is the encoder's restatement up to the quantised
coefficients (tests/encode_ref.py) and the decoder's from there (tests/libjpeg_ref.py):

    encode_ref.coefficients   jccolor, jcsample with its edge rules, jpeg_fdct_islow, the quantiser, jpeg_set_quality's tables
    -> natural order, each component's real block grid (a dummy block lies outside the image and is never looked at)
    -> libjpeg_ref.idct_islow         dequantisation, jpeg_idct_islow, the range limit
    -> the component planes at libjpeg's downsampled sizes
    -> libjpeg_ref.planes_to_rgb_fancy  fancy upsampling (replication where the plane is at most 2 samples wide), YCbCr -> RGB

    roundtrip(img, quality, subsampling) -> uint8 array of img's shape
    cases()                              the pinned cases (tests/golden/roundtrip_pins.npz; tools/make_roundtrip_pins.py)
"""
import hashlib

import numpy as np

from tests import encode_ref as E
from tests import libjpeg_ref as L

SIZES = [(1, 1), (2, 3), (3, 2), (5, 4), (7, 5), (8, 8), (9, 17), (16, 16), (17, 33), (33, 6), (64, 48), (250, 131)]  # width, height
PATTERNS = ["noise", "ramp", "checker", "zeros", "ones"]
SUBSAMPLINGS = ["4:4:4", "4:2:2", "4:2:0"]
QUALITIES = [1, 10, 50, 75, 95, 100]
STORED_PIXELS = 64  # a pin of at most this many pixels is stored as an array, a larger one as its SHA-256


# A grey block whose reconstruction at quality 1 (every quantiser 255) overshoots so far that jidctint.c's range limit WRAPS:
# sample [5][3] comes out of the second pass below -512, which the table lookup (x & 1023) turns into 255 and a plain clamp
# into 0. Found by a hill climb on max |reconstruction|; none of the pinned patterns, the 0/255 checkerboard included, gets
# beyond the +-384 of overshoot it takes (at quantisers up to 100 no input can). libjpeg-turbo's SIMD IDCT saturates instead
# of looking the table up, so Pillow on a SIMD build returns 0 here and 255 with JSIMD_FORCENONE=1; the library's ISLOW
# decoder, and so the round trip, is jidctint.c's. The block is therefore no pin: it is compared with the decode chain.
WRAP_BLOCK = np.array([[255, 0, 0, 255, 255, 255, 0, 0], [124, 255, 255, 237, 255, 255, 255, 255], [250, 255, 0, 0, 73, 255, 255, 82],
                       [255, 0, 255, 0, 255, 100, 38, 0], [0, 18, 148, 0, 255, 255, 0, 255], [255, 255, 255, 0, 0, 0, 0, 0],
                       [255, 0, 214, 255, 255, 81, 0, 255], [255, 0, 255, 255, 255, 0, 255, 21]], np.uint8)
WRAP_AT = (5, 3)


def planes(img, quality, subsampling):
    """The decoded component planes (uint8, libjpeg's downsampled sizes) and the sampling factors (hs, vs) of each."""
    img = np.asarray(img)
    hs, vs = E.SUBSAMPLINGS[subsampling]
    co = E.coefficients(img, hs, vs, quality)
    hs, vs, mx, my, per = co["hs"], co["vs"], co["mcus_x"], co["mcus_y"], co["per_mcu"]
    h, w = co["h"], co["w"]
    natural = np.zeros((co["coefs"].shape[0], 64), np.int64)
    natural[:, E.ZIGZAG] = co["coefs"]  # zigzag position k holds natural index ZIGZAG[k]
    stream = natural.reshape(my, mx, per, 64)
    tables = [E.quant_table(E.BASE_LUMA, quality), E.quant_table(E.BASE_CHROMA, quality)]
    out = []
    for c in range(co["ncomp"]):
        if c == 0:  # the MCU's hs x vs luma blocks, row by row, back on the padded grid
            grid = stream[:, :, :hs * vs].reshape(my, mx, vs, hs, 64).transpose(0, 2, 1, 3, 4).reshape(my * vs, mx * hs, 64)
            pw, ph = w, h
        else:
            grid = stream[:, :, hs * vs + c - 1]
            pw, ph = -(-w // hs), -(-h // vs)
        gh, gw = -(-ph // 8), -(-pw // 8)  # the real blocks: a luma block beyond them is a dummy and never read
        grid = grid[:gh, :gw]
        px = L.idct_islow(grid.reshape(-1, 64), tables[c > 0]).reshape(gh, gw, 8, 8).transpose(0, 2, 1, 3).reshape(gh * 8, gw * 8)
        out.append(np.ascontiguousarray(px[:ph, :pw]))
    return out, ([hs, 1, 1], [vs, 1, 1]) if co["ncomp"] == 3 else ([1], [1])


def roundtrip(img, quality=75, subsampling="4:2:0"):
    """img: H x W (grey) or H x W x 3 (RGB) uint8 -> the array Pillow returns after save and open."""
    img = np.asarray(img)
    p, (hs, vs) = planes(img, quality, subsampling)
    if img.ndim == 2:
        return p[0]
    return L.planes_to_rgb_fancy(p, hs, vs, img.shape[1], img.shape[0])


def pattern(kind, w, h, channels, seed):
    """The inputs of the pins. `checker`: 0 / 255 by pixel, the largest coefficients and the range limit's overshoot."""
    shape = (h, w) if channels == 1 else (h, w, 3)
    if kind == "noise":
        return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    if kind == "ramp":
        base = [(x * 255) // max(w - 1, 1), (y * 255) // max(h - 1, 1), ((x + y) * 255) // max(w + h - 2, 1)]
    elif kind == "checker":
        base = [((x + y) & 1) * 255, ((x + y + 1) & 1) * 255, (x & 1) * 255]
    else:
        v = 0 if kind == "zeros" else 255
        base = [np.full((h, w), v)] * 3
    a = np.stack(base, axis=-1).astype(np.uint8)
    return np.ascontiguousarray(a[..., 0] if channels == 1 else a)


def cases():
    """[(name, width, height, channels, pattern, subsampling, quality, seed)]: every size, grey and RGB, every pattern and
    quality; grey has no chroma, so it takes one subsampling."""
    out = []
    for w, h in SIZES:
        for ch in (1, 3):
            for kind in PATTERNS:
                for ss in SUBSAMPLINGS if ch == 3 else SUBSAMPLINGS[2:]:
                    for q in QUALITIES:
                        name = "%dx%d_%s_%s_%s_q%d" % (w, h, "rgb" if ch == 3 else "grey", kind, ss.replace(":", ""), q)
                        seed = int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little")
                        out.append((name, w, h, ch, kind, ss, q, seed))
    return out


def case_input(case):
    _, w, h, ch, kind, _, _, seed = case
    return pattern(kind, w, h, ch, seed)


def case_table(all_cases):
    """The cases' parameters as the pins store them: int64 [n, 7] of width, height, channels, the indices of the pattern and
    the subsampling, quality, seed."""
    return np.array([[w, h, ch, PATTERNS.index(kind), SUBSAMPLINGS.index(ss), q, seed] for _, w, h, ch, kind, ss, q, seed in all_cases], np.int64)


def matches_pin(pins, i, a):
    """Does `a` equal Pillow's output of case i? By the stored array where the pins hold one (cases of at most
    STORED_PIXELS pixels: `small` from small_off[i] to small_off[i + 1]), and by its SHA-256 for every case."""
    a = np.ascontiguousarray(a)
    w, h, ch = (int(v) for v in pins["cases"][i][:3])
    if a.dtype != np.uint8 or a.shape != ((h, w) if ch == 1 else (h, w, 3)):
        return False
    lo, hi = (int(v) for v in pins["small_off"][i:i + 2])
    if hi > lo and not np.array_equal(a.ravel(), pins["small"][lo:hi]):
        return False
    return hashlib.sha256(a.tobytes()).digest() == pins["sha256"][i].tobytes()
