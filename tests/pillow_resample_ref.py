"""CPU restatement of Pillow's 8-bit resampling (Image.resize with BILINEAR or BICUBIC, no box, no reducing_gap), the
arithmetic jpeggpu_ext_resize_to_rgb reproduces. Written from the algorithm, in numpy:
  * per output coordinate, in double: scale = in / out, fs = max(scale, 1), support = filter support * fs,
    center = (x + 0.5) * scale, first = max(int(center - support + 0.5), 0), count = min(int(center + support + 0.5), in)
    - first; tap j weighs filter((j + first - center + 0.5) * (1 / fs)); the weights are summed in tap order and divided
    by the sum when it is not 0;
  * each weight in fixed point with 22 fraction bits, rounded half away from zero and truncated: int(w * 2^22 + 0.5),
    or int(w * 2^22 - 0.5) for a negative weight;
  * a pass computes clamp_0..255((2^21 + sum w_j p_j) >> 22) in int32 (arithmetic shift);
  * the horizontal pass first, over the rows the vertical taps read only; its result is uint8; then the vertical pass.
    A direction whose size does not change is skipped.
"""
import numpy as np

PRECISION_BITS = 22
FILTERS = ("bilinear", "bicubic")
SUPPORT = {"bilinear": 1.0, "bicubic": 2.0}


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


_FILTER = {"bilinear": _bilinear, "bicubic": _bicubic}


def max_taps(in_size, out_size, filt):
    """The most taps any output coordinate gets: 2 ceil(support) + 1 (Pillow's ksize)."""
    fs = max(in_size / out_size, 1.0)
    return 2 * int(np.ceil(SUPPORT[filt] * fs)) + 1


def weights(in_size, out_size, filt):
    """(first[out], count[out], weights[out, max_taps]) in fixed point, int32; weights beyond count are 0."""
    f = _FILTER[filt]
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = SUPPORT[filt] * fs
    ss = 1.0 / fs
    k = max_taps(in_size, out_size, filt)
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
            w[x, j] = int(v * (1 << PRECISION_BITS) - 0.5) if v < 0 else int(v * (1 << PRECISION_BITS) + 0.5)
    return first, count, w


def _pass(a, first, count, w, axis):
    """One pass along `axis` (0 rows, 1 columns) of an (H, W, C) uint8 array."""
    a = np.moveaxis(a, axis, 0).astype(np.int64)
    out = np.zeros((len(first),) + a.shape[1:], np.int64)
    for x in range(len(first)):
        n = int(count[x])
        seg = a[first[x]:first[x] + n]
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(w[x, :n].astype(np.int64), seg, axes=(0, 0))
        out[x] = acc
    assert np.abs(out).max(initial=0) < 2 ** 31  # the sum fits int32
    out = np.clip(out >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def resize(a, out_w, out_h, filt):
    """Image.fromarray(a).resize((out_w, out_h), BILINEAR | BICUBIC) of an (H, W, 3) or (H, W) uint8 array."""
    squeeze = a.ndim == 2
    if squeeze:
        a = a[:, :, None]
    h, w = a.shape[:2]
    if out_w != w:
        fy, cy, wy = weights(h, out_h, filt)
        y0, y1 = (int(fy[0]), int(fy[-1] + cy[-1])) if out_h != h else (0, h)
        fx, cx, wx = weights(w, out_w, filt)
        a = _pass(a[y0:y1], fx, cx, wx, 1)
        if out_h != h:
            a = _pass(a, fy - y0, cy, wy, 0)
    elif out_h != h:
        fy, cy, wy = weights(h, out_h, filt)
        a = _pass(a, fy, cy, wy, 0)
    return a[:, :, 0] if squeeze else a


def pillow_resize(a, out_w, out_h, filt):
    """Pillow's own Image.resize of the same array (raises ImportError without Pillow)."""
    from PIL import Image

    f = {"bilinear": Image.Resampling.BILINEAR, "bicubic": Image.Resampling.BICUBIC}[filt]
    return np.asarray(Image.fromarray(a).resize((out_w, out_h), f))
