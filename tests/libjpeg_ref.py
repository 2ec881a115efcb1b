"""CPU restatement of libjpeg-compatible full-size decoding (jpeggpu_ext_set_idct's ISLOW mode and
jpeggpu_ext_planes_to_rgbi_fancy), applied to the coefficients of the CPU oracle.

Written from the algorithms, in numpy:
  * libjpeg-turbo's jpeg_idct_islow (jidctint.c): DEQUANTIZE in full int, 64-bit intermediates (JLONG),
    CONST_BITS = 13, PASS1_BITS = 2, a 32-bit (int) workspace between the passes, DESCALE by 11 after the column pass
    and by 18 after the row pass, then the 10-bit-wrapping range limit. The shortcuts jidctint.c takes for columns and
    rows whose AC terms are zero are the same expressions with the zero terms dropped, so they are not restated;
  * the fancy upsamplers of jdsample.c (h2v1, h2v2, h1v2; replication for the other integral ratios and for 2x1 / 2x2
    planes at most 2 samples wide), with the samples beyond a plane's edges copies of the edge samples;
  * the integer YCbCr -> RGB conversion of jdcolor.c (ycc_rgb_convert).
"""
import functools

import numpy as np

from tests.scaled_ref import CONST_BITS, PASS1_BITS, descale, int32, range_limit

FIX_0_298631336 = 2446
FIX_0_390180644 = 3196
FIX_0_541196100 = 4433
FIX_0_765366865 = 6270
FIX_0_899976223 = 7373
FIX_1_175875602 = 9633
FIX_1_501321110 = 12299
FIX_1_847759065 = 15137
FIX_1_961570560 = 16069
FIX_2_053119869 = 16819
FIX_2_562915447 = 20995
FIX_3_072711026 = 25172


def islow_1d(x):
    """One 8-point pass of jpeg_idct_islow on int64 inputs x[0..7] (arrays): the eight outputs before their DESCALE."""
    # even part
    z2, z3 = x[2], x[6]
    z1 = (z2 + z3) * FIX_0_541196100
    tmp2 = z1 + z3 * -FIX_1_847759065
    tmp3 = z1 + z2 * FIX_0_765366865
    tmp0 = (x[0] + x[4]) << np.int64(CONST_BITS)
    tmp1 = (x[0] - x[4]) << np.int64(CONST_BITS)
    tmp10, tmp13 = tmp0 + tmp3, tmp0 - tmp3
    tmp11, tmp12 = tmp1 + tmp2, tmp1 - tmp2
    # odd part
    t0, t1, t2, t3 = x[7], x[5], x[3], x[1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * FIX_1_175875602
    t0 = t0 * FIX_0_298631336
    t1 = t1 * FIX_2_053119869
    t2 = t2 * FIX_3_072711026
    t3 = t3 * FIX_1_501321110
    z1 = z1 * -FIX_0_899976223
    z2 = z2 * -FIX_2_562915447
    z3 = z3 * -FIX_1_961570560 + z5
    z4 = z4 * -FIX_0_390180644 + z5
    t0 = t0 + z1 + z3
    t1 = t1 + z2 + z4
    t2 = t2 + z2 + z3
    t3 = t3 + z1 + z4
    return [tmp10 + t3, tmp11 + t2, tmp12 + t1, tmp13 + t0, tmp13 - t0, tmp12 - t1, tmp11 - t2, tmp10 - t3]


def idct_islow(coef, q):
    """jpeg_idct_islow: [n, 64] natural-order coefficients x [64] quantisers -> [n, 8, 8] uint8 (row, column)."""
    d = (coef.astype(np.int64) * q.astype(np.int64)[None, :]).reshape(-1, 8, 8)
    ws = np.empty(d.shape, np.int64)
    out = islow_1d([d[:, k, :] for k in range(8)])  # columns: output k is row k
    for k in range(8):
        ws[:, k, :] = int32(descale(out[k], CONST_BITS - PASS1_BITS))
    px = np.empty(d.shape, np.uint8)
    out = islow_1d([ws[:, :, k] for k in range(8)])  # rows: output k is column k
    for k in range(8):
        px[:, :, k] = range_limit(descale(out[k], CONST_BITS + PASS1_BITS + 3))
    return px


def islow_planes_of(dec):
    """Full-size planes of an oracle.Decoded with the ISLOW IDCT, cropped like the oracle's planes."""
    out = []
    for c in range(dec.ncomp):
        coef = dec.coef[c]
        bh, bw = coef.shape[:2]
        blocks = idct_islow(coef.reshape(-1, 64), dec.qtab[dec.qidx[c]])
        full = blocks.reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)
        h, w = dec.planes[c].shape
        out.append(np.ascontiguousarray(full[:h, :w]))
    return out


def islow_planes(data: bytes):
    """Per-component uint8 planes of `data` decoded at full size with the ISLOW IDCT."""
    from oracle import oracle

    return islow_planes_of(oracle.decode(data))


def _neighbours(a, axis):
    """(previous, next) along `axis` with the edge samples repeated."""
    n = a.shape[axis]
    prev = np.take(a, np.clip(np.arange(n) - 1, 0, n - 1), axis=axis)
    nxt = np.take(a, np.clip(np.arange(n) + 1, 0, n - 1), axis=axis)
    return prev, nxt


def _interleave(even, odd, axis):
    shape = list(even.shape)
    shape[axis] *= 2
    out = np.empty(shape, even.dtype)
    idx = [slice(None)] * even.ndim
    idx[axis] = slice(0, None, 2)
    out[tuple(idx)] = even
    idx[axis] = slice(1, None, 2)
    out[tuple(idx)] = odd
    return out


def upsample_fancy(plane, hr, vr, width, height):
    """One component's plane (its h x w samples, libjpeg's downsampled size) at (height, width) output pixels, for the
    ratio hr = h_max / h_c, vr = v_max / v_c (jdsample.c with do_fancy_upsampling)."""
    s = plane.astype(np.int64)
    h, w = s.shape
    if (hr, vr) == (2, 1) and w > 2:  # h2v1_fancy_upsample
        left, right = _neighbours(s, 1)
        out = _interleave((3 * s + left + 1) >> 2, (3 * s + right + 2) >> 2, 1)
    elif (hr, vr) == (2, 2) and w > 2:  # h2v2_fancy_upsample: column sums 3 near + far row, then across
        up, down = _neighbours(s, 0)
        cols = _interleave(3 * s + up, 3 * s + down, 0)
        left, right = _neighbours(cols, 1)
        out = _interleave((3 * cols + left + 8) >> 4, (3 * cols + right + 7) >> 4, 1)
    elif (hr, vr) == (1, 2):  # h1v2_fancy_upsample
        up, down = _neighbours(s, 0)
        out = _interleave((3 * s + up + 1) >> 2, (3 * s + down + 2) >> 2, 0)
    else:  # int_upsample (1x1 included): replication
        out = np.repeat(np.repeat(s, vr, axis=0), hr, axis=1)
    assert out.shape[0] >= height and out.shape[1] >= width
    return out[:height, :width].astype(np.uint8)


def ycc_to_rgb(y, cb, cr):
    """jdcolor.c ycc_rgb_convert on uint8 planes -> (H, W, 3) uint8."""
    y = y.astype(np.int64)
    cb = cb.astype(np.int64) - 128
    cr = cr.astype(np.int64) - 128
    half = np.int64(1 << 15)
    r = y + ((91881 * cr + half) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + half) >> 16)
    b = y + ((116130 * cb + half) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def planes_to_rgb_fancy(planes, hs, vs, width, height):
    """What jpeggpu_ext_planes_to_rgbi_fancy computes: 1 or 3 planes with sampling factors hs, vs -> (H, W, 3) uint8."""
    hmax, vmax = max(hs), max(vs)
    assert all(hmax % h == 0 for h in hs) and all(vmax % v == 0 for v in vs), "non-integral ratio"
    full = [upsample_fancy(p, hmax // h, vmax // v, width, height) for p, h, v in zip(planes, hs, vs)]
    if len(full) == 1:
        return np.repeat(full[0][:, :, None], 3, axis=2)
    return ycc_to_rgb(*full)


def libjpeg_rgb_of(dec):
    """libjpeg-turbo's RGB output (jpeg_read_scanlines, JCS_RGB) of a 1- or 3-component oracle.Decoded."""
    return planes_to_rgb_fancy(islow_planes_of(dec), list(dec.hs), list(dec.vs), dec.width, dec.height)


def libjpeg_rgb(data: bytes):
    from oracle import oracle

    return libjpeg_rgb_of(oracle.decode(data))


def pillow_rgb(data: bytes):
    """np.asarray(Image.open(f).convert("RGB")). Needs Pillow; used by the pin tool and tests."""
    import io

    from PIL import Image

    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


@functools.lru_cache(maxsize=1)
def _matrix():
    from tests import cases

    return cases.matrix()


def pinned_jpeg(pins, name):
    """The input file of a pin of tests/golden/libjpeg_pins.npz: stored bytes, or the tests/cases.matrix() file whose
    SHA-256 the pins hold (regenerated; a change of the synthetic encoder fails here rather than as a wrong pin)."""
    import hashlib

    if "jpeg/" + name in pins.files:
        return pins["jpeg/" + name].tobytes()
    data = _matrix()[name]
    assert hashlib.sha256(data).hexdigest() == str(pins["jpeg_sha256/" + name]), (name, "input differs from the pinned one")
    return data


def pinned_arrays(pins, kind):
    """[(name, component or None, array or None, sha256 or None)] of the `kind` ("planes" or "rgb") pins."""
    out = []
    for key in pins.files:
        k, _, rest = key.partition("/")
        if k not in (kind, kind + "_sha256"):
            continue
        name, _, c = rest.partition("/")
        stored = k == kind
        out.append((name, int(c) if c else None, pins[key] if stored else None, None if stored else str(pins[key])))
    return out


def matches_pin(a, array, sha):
    import hashlib

    if array is not None:
        return a.shape == array.shape and np.array_equal(a, array)
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest() == sha
