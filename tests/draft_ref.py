"""libjpeg-turbo's scaled decoding restated in numpy: what Pillow's im.draft("RGB", (W // d, H // d)); im.convert("RGB")
returns, and what the library's JPEGGPU_EXT_SCALE_LIBJPEG mode must produce.

jdmaster.c gives every component its own IDCT output size S_c (DCT_scaled_size), so that the IDCT does as much of the
chroma upsampling as it can; what subsampling is left is upsampled as at full size (jdsample.c), except that fancy
upsampling is off when the smallest block size is 1 (1/8 scale), where libjpeg replicates. The IDCTs, the fancy
upsamplers and the colour conversion are those of tests/scaled_ref.py and tests/libjpeg_ref.py.
"""
import numpy as np

from tests import libjpeg_ref, scaled_ref

SCALES = (2, 4, 8)
_IDCT = {8: libjpeg_ref.idct_islow, 4: scaled_ref.idct_4x4, 2: scaled_ref.idct_2x2, 1: scaled_ref.idct_1x1}


def ceil_div(a, b):
    return -(-a // b)


def block_sizes(hs, vs, d):
    """S_c per component at scale 1 / d (jdmaster.c, jpeg_calc_output_dimensions)."""
    hmax, vmax = max(hs), max(vs)
    mn = 8 // d
    out = []
    for h, v in zip(hs, vs):
        s = mn
        while s < 8 and (hmax * mn) % (h * s * 2) == 0 and (vmax * mn) % (v * s * 2) == 0:
            s *= 2
        out.append(s)
    return out


def effective_factors(hs, vs, d):
    """(eh, ev): the sampling factors the planes have at the scale, h_c S_c / S_min and v_c S_c / S_min."""
    mn = 8 // d
    sizes = block_sizes(hs, vs, d)
    return [h * s // mn for h, s in zip(hs, sizes)], [v * s // mn for v, s in zip(vs, sizes)]


def plane_sizes(width, height, hs, vs, d):
    """[(w, h)] per component: ceil(W h_c S_c / (8 h_max)), ceil(H v_c S_c / (8 v_max))."""
    hmax, vmax = max(hs), max(vs)
    return [(ceil_div(width * h * s, hmax * 8), ceil_div(height * v * s, vmax * 8)) for h, v, s in zip(hs, vs, block_sizes(hs, vs, d))]


def factors_of(dec):
    """The frame's sampling factors as the library sees them: a single component's are ignored (1 x 1)."""
    if dec.ncomp == 1:
        return [1], [1]
    return list(dec.hs), list(dec.vs)


def fancy(d):
    """jdsample.c: do_fancy_upsampling && min_DCT_scaled_size > 1."""
    return 8 // d > 1


def draft_planes_of(dec, d):
    """Planes at 1 / d of an oracle.Decoded, each component with its own IDCT size (size 8: jpeg_idct_islow)."""
    if d == 1:
        return libjpeg_ref.islow_planes_of(dec)
    hs, vs = factors_of(dec)
    sizes = block_sizes(hs, vs, d)
    out = []
    for c, ((w, h), s) in enumerate(zip(plane_sizes(dec.width, dec.height, hs, vs, d), sizes)):
        coef = dec.coef[c]
        bh, bw = coef.shape[:2]
        blocks = _IDCT[s](coef.reshape(-1, 64), dec.qtab[dec.qidx[c]])
        full = blocks.reshape(bh, bw, s, s).transpose(0, 2, 1, 3).reshape(bh * s, bw * s)
        assert full.shape[0] >= h and full.shape[1] >= w
        out.append(np.ascontiguousarray(full[:h, :w]))
    return out


def planes_to_rgb(planes, eh, ev, width, height, d):
    """libjpeg's RGB of such planes: fancy upsampling of what subsampling is left, or replication at 1/8."""
    if fancy(d):
        return libjpeg_ref.planes_to_rgb_fancy(planes, eh, ev, width, height)
    hm, vm = max(eh), max(ev)
    assert all(hm % h == 0 for h in eh) and all(vm % v == 0 for v in ev), "non-integral ratio"
    full = [np.repeat(np.repeat(p, vm // v, axis=0), hm // h, axis=1)[:height, :width] for p, h, v in zip(planes, eh, ev)]
    if len(full) == 1:
        return np.repeat(full[0][:, :, None], 3, axis=2)
    return libjpeg_ref.ycc_to_rgb(*full)


def has_rgb(dec):
    """1 or 3 components with integral ratios: what the RGB calls accept."""
    hs, vs = factors_of(dec)
    return dec.ncomp in (1, 3) and all(max(hs) % h == 0 for h in hs) and all(max(vs) % v == 0 for v in vs)


def needs_replication(dec, d):
    """1/8 with subsampling left: libjpeg replicates, which the batched resize does not reproduce."""
    eh, ev = effective_factors(*factors_of(dec), d)
    return d == 8 and (len(set(eh)) > 1 or len(set(ev)) > 1)


def draft_rgb_of(dec, d):
    """(H, W, 3) uint8: libjpeg-turbo's RGB output at 1 / d of a 1- or 3-component oracle.Decoded."""
    hs, vs = factors_of(dec)
    eh, ev = effective_factors(hs, vs, d)
    return planes_to_rgb(draft_planes_of(dec, d), eh, ev, ceil_div(dec.width, d), ceil_div(dec.height, d), d)


def draft_rgb(data: bytes, d: int):
    from oracle import oracle

    return draft_rgb_of(oracle.decode(data), d)


def crop_windows(width, height, hs, vs, d, rect):
    """The windows of a cropped decode in this mode (jpeggpu_ext.h): [(origin_x, origin_y, size_x, size_y)] per component
    and the frame's MCU range (mx0, my0, mx1, my1). The rectangle is in pixels of the image at 1 / d; every component
    gets a one-sample halo; an MCU column is h_c S_c samples of component c."""
    x, y, w, h = rect
    hmax, vmax = max(hs), max(vs)
    sizes = block_sizes(hs, vs, d) if d > 1 else [8] * len(hs)
    eh, ev = effective_factors(hs, vs, d) if d > 1 else (list(hs), list(vs))
    full = plane_sizes(width, height, hs, vs, d) if d > 1 else [(ceil_div(width * a, hmax), ceil_div(height * b, vmax)) for a, b in zip(hs, vs)]
    n = len(hs)
    lo_x = [max(x * eh[c] // hmax - 1, 0) for c in range(n)]
    hi_x = [min((x + w - 1) * eh[c] // hmax + 1, full[c][0] - 1) for c in range(n)]
    lo_y = [max(y * ev[c] // vmax - 1, 0) for c in range(n)]
    hi_y = [min((y + h - 1) * ev[c] // vmax + 1, full[c][1] - 1) for c in range(n)]
    mx0 = min(lo_x[c] // (sizes[c] * hs[c]) for c in range(n))
    mx1 = max(hi_x[c] // (sizes[c] * hs[c]) + 1 for c in range(n))
    my0 = min(lo_y[c] // (sizes[c] * vs[c]) for c in range(n))
    my1 = max(hi_y[c] // (sizes[c] * vs[c]) + 1 for c in range(n))
    win = []
    for c in range(n):
        ox, oy = mx0 * sizes[c] * hs[c], my0 * sizes[c] * vs[c]
        win.append((ox, oy, hi_x[c] + 1 - ox, hi_y[c] + 1 - oy))
    return win, (mx0, my0, mx1, my1)


def pillow_draft_rgb(data: bytes, d: int):
    """(np.asarray(im.convert("RGB")), im.size) after im.draft("RGB", (W // d, H // d)). Needs Pillow."""
    import io

    from PIL import Image

    im = Image.open(io.BytesIO(data))
    w, h = im.size
    im.draft("RGB", (max(w // d, 1), max(h // d, 1)))
    return np.asarray(im.convert("RGB")), im.size


def pillow_comparable(name, dec, d):
    """The cases Pillow's draft() can be compared on. Excluded, and nothing else: dense_escapes at 1/2 (libjpeg-turbo's
    SIMD jpeg_idct_4x4 differs from jidctred.c on that file's coefficients, as its SIMD ISLOW does at full size), and
    files smaller than d in a direction for which draft() cannot be made to return the image at 1 / d: asked for
    (max(W // d, 1), max(H // d, 1)) it picks a smaller denominator, and an image of another size."""
    if not has_rgb(dec):
        return False
    if name == "dense_escapes" and d == 2:
        return False
    s = pillow_scale(dec.width, dec.height, (max(dec.width // d, 1), max(dec.height // d, 1)))
    return (ceil_div(dec.width, s), ceil_div(dec.height, s)) == (ceil_div(dec.width, d), ceil_div(dec.height, d))


def pillow_scale(width, height, requested):
    """JpegImageFile.draft's choice: min(width // rw, height // rh) rounded down to 8, 4, 2 or 1."""
    s = min(width // requested[0], height // requested[1])
    return next((k for k in (8, 4, 2) if s >= k), 1)


def inputs():
    """name -> bytes: the matrix, the sampling sweep ("sweep:" in front of its names, the file parse_header and the
    oracle refuse left out) and the photo."""
    import os

    from tests import cases

    files = dict(cases.matrix())
    for k, v in cases.sampling_sweep().items():
        if not cases.sweep_is_refused(k):
            files["sweep:" + k] = v
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "IMG_6510.JPG"), "rb") as f:
        files["photo"] = f.read()
    return files
