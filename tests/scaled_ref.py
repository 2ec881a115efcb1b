"""CPU restatement of scaled decoding (jpeggpu_ext_set_scale): the reduced inverse DCTs of libjpeg-turbo's jidctred.c
(jpeg_idct_4x4, jpeg_idct_2x2, jpeg_idct_1x1) and its range limit, applied to the coefficients of the CPU oracle.

Written from the algorithm, in numpy; the arithmetic it reproduces is:
  * DEQUANTIZE: coefficient * quantiser in full int (no int16 truncation);
  * 64-bit intermediates (JLONG), CONST_BITS = 13, PASS1_BITS = 2, DESCALE(x, n) = (x + 2^(n-1)) >> n;
  * a 32-bit (int) workspace between the two passes;
  * the output goes through the post-IDCT range-limit table: index x & 1023 (RANGE_MASK), i.e. x wrapped to a 10-bit
    signed value, clamped to -128..127, plus 128.
Column 4 (and row 4 of the 4x4's second pass) never contributes to the 4x4 output; the 2x2 uses rows and columns
0, 1, 3, 5, 7 only. The shortcuts jidctred.c takes for columns and rows whose AC terms are zero give the same numbers as
the full formulas (exactly: they are the same expressions with the zero terms dropped), so they are not restated.
"""
import numpy as np

SCALES = (1, 2, 4, 8)

CONST_BITS = 13
PASS1_BITS = 2

FIX_0_211164243 = 1730
FIX_0_509795579 = 4176
FIX_0_601344887 = 4926
FIX_0_720959822 = 5906
FIX_0_765366865 = 6270
FIX_0_850430095 = 6967
FIX_0_899976223 = 7373
FIX_1_061594337 = 8697
FIX_1_272758580 = 10426
FIX_1_451774981 = 11893
FIX_1_847759065 = 15137
FIX_2_172734803 = 17799
FIX_2_562915447 = 20995
FIX_3_624509785 = 29692


def descale(x, n):
    return (x + (np.int64(1) << np.int64(n - 1))) >> np.int64(n)


def range_limit(x):
    """libjpeg's post-IDCT range limit: table[x & 1023] = clamp(wrap10(x), -128, 127) + 128."""
    x = np.asarray(x, np.int64) & 1023
    x = np.where(x >= 512, x - 1024, x)
    return (np.clip(x, -128, 127) + 128).astype(np.uint8)


def int32(x):
    """The int workspace of jidctred.c: the 64-bit result of a pass-1 DESCALE kept in 32 bits (two's complement)."""
    return ((x + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def _dequant(coef, q):
    """[n, 64] natural-order coefficients x [64] quantisers -> [n, 8, 8] int64 (row, column)."""
    return (coef.astype(np.int64) * q.astype(np.int64)[None, :]).reshape(-1, 8, 8)


def idct_1x1(coef, q):
    """jpeg_idct_1x1: [n, 64] -> [n, 1, 1]."""
    dc = coef[:, 0].astype(np.int64) * np.int64(q[0])
    return range_limit(descale(dc, 3)).reshape(-1, 1, 1)


def idct_2x2(coef, q):
    """jpeg_idct_2x2: [n, 64] -> [n, 2, 2]."""
    d = _dequant(coef, q)
    # pass 1: columns 0, 1, 3, 5, 7 -> workspace rows 0 and 1
    ws = np.zeros((d.shape[0], 2, 8), np.int64)
    for col in (0, 1, 3, 5, 7):
        c = d[:, :, col]
        tmp10 = c[:, 0] << np.int64(CONST_BITS + 2)
        tmp0 = (c[:, 7] * -FIX_0_720959822 + c[:, 5] * FIX_0_850430095
                + c[:, 3] * -FIX_1_272758580 + c[:, 1] * FIX_3_624509785)
        ws[:, 0, col] = int32(descale(tmp10 + tmp0, CONST_BITS - PASS1_BITS + 2))
        ws[:, 1, col] = int32(descale(tmp10 - tmp0, CONST_BITS - PASS1_BITS + 2))
    # pass 2: the two workspace rows
    out = np.empty((d.shape[0], 2, 2), np.uint8)
    for row in range(2):
        w = ws[:, row, :]
        tmp10 = w[:, 0] << np.int64(CONST_BITS + 2)
        tmp0 = (w[:, 7] * -FIX_0_720959822 + w[:, 5] * FIX_0_850430095
                + w[:, 3] * -FIX_1_272758580 + w[:, 1] * FIX_3_624509785)
        out[:, row, 0] = range_limit(descale(tmp10 + tmp0, CONST_BITS + PASS1_BITS + 3 + 2))
        out[:, row, 1] = range_limit(descale(tmp10 - tmp0, CONST_BITS + PASS1_BITS + 3 + 2))
    return out


def _idct4(v0, v1, v2, v3, v5, v6, v7):
    """The 4-point even / odd parts of jpeg_idct_4x4 (both passes): (tmp10, tmp12, tmp0, tmp2)."""
    tmp0 = v0 << np.int64(CONST_BITS + 1)
    tmp2 = v2 * FIX_1_847759065 + v6 * -FIX_0_765366865
    tmp10, tmp12 = tmp0 + tmp2, tmp0 - tmp2
    z1, z2, z3, z4 = v7, v5, v3, v1
    o0 = z1 * -FIX_0_211164243 + z2 * FIX_1_451774981 + z3 * -FIX_2_172734803 + z4 * FIX_1_061594337
    o2 = z1 * -FIX_0_509795579 + z2 * -FIX_0_601344887 + z3 * FIX_0_899976223 + z4 * FIX_2_562915447
    return tmp10, tmp12, o0, o2


def idct_4x4(coef, q):
    """jpeg_idct_4x4: [n, 64] -> [n, 4, 4]."""
    d = _dequant(coef, q)
    ws = np.zeros((d.shape[0], 4, 8), np.int64)
    for col in (0, 1, 2, 3, 5, 6, 7):
        c = d[:, :, col]
        tmp10, tmp12, o0, o2 = _idct4(c[:, 0], c[:, 1], c[:, 2], c[:, 3], c[:, 5], c[:, 6], c[:, 7])
        n = CONST_BITS - PASS1_BITS + 1
        ws[:, 0, col] = int32(descale(tmp10 + o2, n))
        ws[:, 3, col] = int32(descale(tmp10 - o2, n))
        ws[:, 1, col] = int32(descale(tmp12 + o0, n))
        ws[:, 2, col] = int32(descale(tmp12 - o0, n))
    out = np.empty((d.shape[0], 4, 4), np.uint8)
    for row in range(4):
        w = ws[:, row, :]
        tmp10, tmp12, o0, o2 = _idct4(w[:, 0], w[:, 1], w[:, 2], w[:, 3], w[:, 5], w[:, 6], w[:, 7])
        n = CONST_BITS + PASS1_BITS + 3 + 1
        out[:, row, 0] = range_limit(descale(tmp10 + o2, n))
        out[:, row, 3] = range_limit(descale(tmp10 - o2, n))
        out[:, row, 1] = range_limit(descale(tmp12 + o0, n))
        out[:, row, 2] = range_limit(descale(tmp12 - o0, n))
    return out


_IDCT = {2: idct_4x4, 4: idct_2x2, 8: idct_1x1}


def scaled_size(full, d):
    """Plane size at 1 / d: ceil(W * h_c / (h_max * d)) == ceil(ceil(W * h_c / h_max) / d)."""
    return -(-full // d)


def scaled_planes_of(dec, d):
    """Planes at 1 / d from an oracle.Decoded (coefficients + quantisation tables)."""
    if d == 1:
        return [p.copy() for p in dec.planes]
    n = 8 // d
    out = []
    for c in range(dec.ncomp):
        coef = dec.coef[c]
        bh, bw = coef.shape[:2]
        blocks = _IDCT[d](coef.reshape(-1, 64), dec.qtab[dec.qidx[c]])
        full = blocks.reshape(bh, bw, n, n).transpose(0, 2, 1, 3).reshape(bh * n, bw * n)
        h, w = dec.planes[c].shape
        out.append(np.ascontiguousarray(full[:scaled_size(h, d), :scaled_size(w, d)]))
    return out


def scaled_planes(data: bytes, d: int):
    """Per-component uint8 planes of `data` decoded at 1 / d (d in 1, 2, 4, 8); d = 1 is the oracle's full decode."""
    from oracle import oracle

    return scaled_planes_of(oracle.decode(data), d)


def pillow_draft(data: bytes, d: int):
    """Pillow's (libjpeg-turbo's) scaled decode of a grayscale or 4:4:4 file as planes: draft() at (W // d, H // d) with
    the colour transform switched off (mode 'YCbCr' for three components). Needs Pillow; used by the pin tool and tests."""
    import io

    from PIL import Image

    im = Image.open(io.BytesIO(data))
    w, h = im.size
    mode = "L" if im.mode == "L" else "YCbCr"
    im.draft(mode, (max(w // d, 1), max(h // d, 1)))
    a = np.asarray(im)
    if a.ndim == 2:
        return [a.copy()]
    return [np.ascontiguousarray(a[:, :, c]) for c in range(a.shape[2])]
