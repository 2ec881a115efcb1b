"""CPU restatement of Pillow's im.thumbnail((rw, rh), BILINEAR | BICUBIC, reducing_gap) on a JPEG file, the chain
jpeggpu_ext_thumbnail_plan and jpeggpu_ext_thumbnail_to_rgb reproduce. Written from the algorithm, in numpy:
  1. the final size (x, y): thumbnail's preserve_aspect_ratio, in doubles, with round_aspect's tie rule and a floor of 1;
     None when the request holds the image (nothing happens: the thumbnail is the full-scale decode);
  2. with a gap g: draft() for (int(rw g), int(rh g)) picks the scale s in 8, 4, 2, 1; the decode has ceil(W / s) x
     ceil(H / s) pixels and the box is (W / s, H / s), in doubles;
  3. the decode is the thumbnail when it already has the final size;
  4. with a gap: fx = int(bx / x / g) or 1, fy alike; when either exceeds 1, Image.reduce((fx, fy)) of the whole decode --
     an output pixel over nx x ny source pixels (fx x fy, fewer in the last column or row) is ((sum + n // 2) * m) >> 24 per
     channel, n = nx ny, m = uint32(float32(2^24) / float32(n)) -- and the box is divided by the factors;
  5. ImagingResample of that image to (x, y) from the box, which passes through C as binary32: per direction scale =
     extent / out, then tests/pillow_resample_ref.py's rule with `extent` in place of the input size and the taps clamped
     at the input size; a direction is skipped only when out == in and extent == in;
  6. an image more than 100 times taller than wide that gets shorter takes the vertical pass first in Pillow; refused here.
"""
import math

import numpy as np

from tests import pillow_resample_ref as R

FILTERS = R.FILTERS


class Refused(ValueError):
    """A thumbnail the library refuses with JPEGGPU_NOT_SUPPORTED (a tall image: step 6)."""


def final_size(w, h, rw, rh):
    """thumbnail's preserve_aspect_ratio: (x, y), or None when the request holds the image."""
    def round_aspect(number, key):
        return max(min(math.floor(number), math.ceil(number), key=key), 1)

    x, y = rw, rh
    if x >= w and y >= h:
        return None
    aspect = w / h
    if x / y >= aspect:
        x = round_aspect(y * aspect, key=lambda n: abs(aspect - n / y))
    else:
        y = round_aspect(x / aspect, key=lambda n: 0 if n == 0 else abs(aspect - x / n))
    return x, y


def draft_scale(w, h, req_w, req_h):
    """JpegImagePlugin.draft's scale for the requested size."""
    scale = min(w // req_w, h // req_h)
    for s in (8, 4, 2, 1):
        if scale >= s:
            return s
    return 1


class Plan:
    """What jpeggpu_ext_thumbnail_plan reports: scale, the decoded size, the reduction factors and the reduced size, the
    resize's extents as binary32 values, the final size, and whether the decode is the thumbnail."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def astuple(self):
        return (self.scale, self.dec_w, self.dec_h, self.fx, self.fy, self.red_w, self.red_h, float(self.box_w), float(self.box_h), self.out_w,
                self.out_h, int(self.identity))


def plan(w, h, rw, rh, gap=2.0):
    """The plan of a w x h file for the request (rw, rh), gap None or >= 1. Raises Refused for step 6."""
    rw, rh = math.floor(rw), math.floor(rh)
    fs = final_size(w, h, rw, rh)
    if fs is None:
        return Plan(scale=1, dec_w=w, dec_h=h, fx=1, fy=1, red_w=w, red_h=h, box_w=np.float32(w), box_h=np.float32(h), out_w=w, out_h=h,
                    identity=True)
    x, y = fs
    s = 1
    if gap is not None:
        s = draft_scale(w, h, int(rw * gap), int(rh * gap))
    dw, dh = -(-w // s), -(-h // s)
    bx, by = w / s, h / s
    if (dw, dh) == (x, y):
        return Plan(scale=s, dec_w=dw, dec_h=dh, fx=1, fy=1, red_w=dw, red_h=dh, box_w=np.float32(dw), box_h=np.float32(dh), out_w=x, out_h=y,
                    identity=True)
    fx = fy = 1
    if gap is not None:
        fx = int(bx / x / gap) or 1
        fy = int(by / y / gap) or 1
    r_w, r_h = -(-dw // fx), -(-dh // fy)
    if fx > 1 or fy > 1:
        bx, by = bx / fx, by / fy
    if r_h > r_w * 100 and y < r_h:
        raise Refused("vertical pass first")
    return Plan(scale=s, dec_w=dw, dec_h=dh, fx=fx, fy=fy, red_w=r_w, red_h=r_h, box_w=np.float32(bx), box_h=np.float32(by), out_w=x, out_h=y,
                identity=False)


def reduce_multiplier(n):
    """Reduce.c's division_UINT32(n, 8): a binary32 division, truncated."""
    return int(np.float32(1 << 24) / np.float32(n))


def reduce(a, fx, fy):
    """Image.reduce((fx, fy)) of an (H, W) or (H, W, C) uint8 array, the whole image as the box."""
    squeeze = a.ndim == 2
    if squeeze:
        a = a[:, :, None]
    h, w, c = a.shape
    ow, oh = -(-w // fx), -(-h // fy)
    p = np.zeros((oh * fy, ow * fx, c), np.int64)
    p[:h, :w] = a
    sums = p.reshape(oh, fy, ow, fx, c).sum(axis=(1, 3))
    nx = np.minimum(fx, w - np.arange(ow) * fx)
    ny = np.minimum(fy, h - np.arange(oh) * fy)
    n = ny[:, None] * nx[None, :]
    m = np.vectorize(reduce_multiplier)(n).astype(np.int64)
    v = (sums + (n // 2)[:, :, None]) * m[:, :, None]
    assert v.max() < 2 ** 32  # the product fits uint32
    out = (v >> 24).astype(np.uint8)
    return out[:, :, 0] if squeeze else out


def box_max_taps(extent, out_size, filt):
    fs = max(float(extent) / out_size, 1.0)
    return 2 * int(math.ceil(R.SUPPORT[filt] * fs)) + 1


def box_weights(in_size, extent, out_size, filt):
    """pillow_resample_ref.weights with a fractional extent: scale = extent / out, taps clamped at in_size. `extent` is
    used as given (round it to binary32 first, as the box is when it passes through C)."""
    f = R._FILTER[filt]
    scale = float(extent) / out_size
    fs = max(scale, 1.0)
    support = R.SUPPORT[filt] * fs
    ss = 1.0 / fs
    k = box_max_taps(extent, out_size, filt)
    first = np.zeros(out_size, np.int32)
    count = np.zeros(out_size, np.int32)
    w = np.zeros((out_size, k), np.int32)
    for x in range(out_size):
        center = (x + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), in_size) - lo
        ws = [f((j + lo - center + 0.5) * ss) for j in range(n)]
        total = 0.0
        for v in ws:
            total += v
        if total != 0.0:
            ws = [v / total for v in ws]
        first[x], count[x] = lo, n
        for j, v in enumerate(ws):
            w[x, j] = int(v * (1 << R.PRECISION_BITS) - 0.5) if v < 0 else int(v * (1 << R.PRECISION_BITS) + 0.5)
    return first, count, w


def box_resize(a, box_w, box_h, out_w, out_h, filt):
    """ImagingResample of `a` to (out_w, out_h) from the box (0, 0, box_w, box_h): the horizontal pass first, over the rows
    the vertical taps read; a direction is skipped when nothing changes in it."""
    squeeze = a.ndim == 2
    if squeeze:
        a = a[:, :, None]
    h, w = a.shape[:2]
    need_x = not (out_w == w and float(box_w) == w)
    need_y = not (out_h == h and float(box_h) == h)
    y0 = 0
    if need_y:
        fy, cy, wy = box_weights(h, box_h, out_h, filt)
        y0, y1 = int(fy[0]), int(fy[-1] + cy[-1])
    if need_x:
        fx, cx, wx = box_weights(w, box_w, out_w, filt)
        a = R._pass(a[y0:y1] if need_y else a, fx, cx, wx, 1)
    elif need_y:
        a = a[y0:y1]
    if need_y:
        a = R._pass(a, fy - y0, cy, wy, 0)
    return a[:, :, 0] if squeeze else a


def thumbnail(decode, w, h, rw, rh, filt="bicubic", gap=2.0):
    """The thumbnail of a w x h file: `decode(scale)` gives the pixels Pillow has after draft() at that scale, (H, W) or
    (H, W, 3) uint8. Returns (array, plan)."""
    p = plan(w, h, rw, rh, gap)
    a = decode(p.scale)
    assert a.shape[:2] == (p.dec_h, p.dec_w), (a.shape, p.astuple())
    if p.identity:
        return a, p
    if p.fx > 1 or p.fy > 1:
        a = reduce(a, p.fx, p.fy)
        assert a.shape[:2] == (p.red_h, p.red_w)
    return box_resize(a, p.box_w, p.box_h, p.out_w, p.out_h, filt), p


def pillow_decode(data):
    """decode(scale) for `thumbnail`, by Pillow's own draft (raises ImportError without Pillow)."""
    import io

    from PIL import Image

    def decode(s):
        im = Image.open(io.BytesIO(data))
        if s != 1:
            im.draft(None, (im.size[0] // s, im.size[1] // s))  # W // (W // s) lies in [s, 2 s): draft settles on s
        im.load()
        return np.asarray(im)

    return decode


def pillow_thumbnail(data, rw, rh, filt="bicubic", gap=2.0):
    """Pillow's own thumbnail of the file, as an array."""
    import io

    from PIL import Image

    f = {"bilinear": Image.Resampling.BILINEAR, "bicubic": Image.Resampling.BICUBIC}[filt]
    im = Image.open(io.BytesIO(data))
    im.thumbnail((rw, rh), f, reducing_gap=gap)
    return np.asarray(im)
