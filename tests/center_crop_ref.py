"""CPU restatement of torchvision's Resize + CenterCrop on a Pillow image, the transform jpeggpu_ext_resize_view_to_tensor
reproduces, on top of the restatement of Pillow's resampling (tests/pillow_resample_ref.py):
  * Resize(s) of a w x h image: the shorter side becomes s, the longer one int(s * long / short) (true division, truncated);
    a pair (rh, rw) is used as given (torchvision's _compute_resized_output_size);
  * CenterCrop(cw x ch) of the resized rw x rh image: where cw <= rw the window starts at int(round((rw - cw) / 2.0)) --
    Python's round, half to even --; where cw > rw the image is padded with (cw - rw) // 2 zero columns on the left and
    (cw - rw + 1) // 2 on the right, so the window starts at -((cw - rw) // 2); rows alike (torchvision's center_crop);
  * a window pixel inside the resized image is Pillow's Image.resize pixel, one outside is 0 in every channel.
window_tables says which taps such a window reads: the slices of the full tables that the kernels are handed.
"""
import numpy as np

from tests import pillow_resample_ref as R


def resized_size(w, h, size):
    """(rw, rh) of Resize(size): int -> the shorter side; a pair is (rh, rw)."""
    if not isinstance(size, int):
        rh, rw = size
        return int(rw), int(rh)
    short, long = (w, h) if w <= h else (h, w)
    new_long = int(size * long / short)
    return (size, new_long) if w <= h else (new_long, size)


def _corner(r, c):
    return int(round((r - c) / 2.0)) if c <= r else -((c - r) // 2)


def center_crop_window(rw, rh, cw, ch):
    """(x, y) of the cw x ch centre window in the rw x rh image; negative where the image is padded."""
    return _corner(rw, cw), _corner(rh, ch)


def window(a, x, y, cw, ch):
    """The cw x ch window at (x, y) of the (H, W, C) or (H, W) array `a`, zeros outside it."""
    h, w = a.shape[:2]
    out = np.zeros((ch, cw) + a.shape[2:], a.dtype)
    x0, x1, y0, y1 = max(x, 0), min(x + cw, w), max(y, 0), min(y + ch, h)
    if x0 < x1 and y0 < y1:
        out[y0 - y:y1 - y, x0 - x:x1 - x] = a[y0:y1, x0:x1]
    return out


def resize_view(a, rw, rh, x, y, cw, ch, filt):
    """The cw x ch window at (x, y) of Image.fromarray(a).resize((rw, rh), filter), zeros outside the resized image."""
    return window(R.resize(a, rw, rh, filt), x, y, cw, ch)


def resize_center_crop(a, size, crop, filt):
    """torchvision's Resize(size) + CenterCrop(crop) of the array; `crop`: int or (ch, cw)."""
    ch, cw = (crop, crop) if isinstance(crop, int) else crop
    h, w = a.shape[:2]
    rw, rh = resized_size(w, h, size)
    x, y = center_crop_window(rw, rh, cw, ch)
    return resize_view(a, rw, rh, x, y, cw, ch, filt)


def full_table(in_size, resized, filt):
    """pillow_resample_ref.weights, or the skipped direction's one tap of weight 1."""
    if in_size == resized:
        k = R.max_taps(in_size, resized, filt)
        w = np.zeros((resized, k), np.int32)
        w[:, 0] = 1 << R.PRECISION_BITS
        return np.arange(resized, dtype=np.int32), np.ones(resized, np.int32), w
    return R.weights(in_size, resized, filt)


def window_tables(in_size, resized, x0, count_out, filt):
    """(first, count, weights, inside) for output coordinates x0 .. x0 + count_out - 1 of in_size -> resized: the rows of the
    full table for the coordinates in [0, resized) (`inside`), count 0 and weights 0 for the others (their `first` is
    left 0: what it carries is the kernels' business)."""
    f, c, w = full_table(in_size, resized, filt)
    first, count = np.zeros(count_out, np.int32), np.zeros(count_out, np.int32)
    wt = np.zeros((count_out, w.shape[1]), np.int32)
    inside = np.zeros(count_out, bool)
    for e in range(count_out):
        x = x0 + e
        if 0 <= x < resized:
            first[e], count[e], wt[e], inside[e] = f[x], c[x], w[x], True
    return first, count, wt, inside


def tap_range(in_size, resized, x0, count_out, filt):
    """Samples [lo, hi) that the taps of the window's coordinates read, or None if no coordinate lies in the image."""
    first, count, _, inside = window_tables(in_size, resized, x0, count_out, filt)
    if not inside.any():
        return None
    return int(first[inside].min()), int((first[inside] + count[inside]).max())
