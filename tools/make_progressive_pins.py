"""Writes tests/golden/progressive_pins.npz: small progressive JPEGs that Pillow (libjpeg-turbo) writes, each with its
baseline twin -- the same pixels, quality, sampling and optimize=True, progressive=False -- and what Pillow decodes them to:
np.asarray(im.convert("RGB")) at full size and after im.draft("RGB", (W // d, H // d)) at d = 2, 4, 8.

    python tools/make_progressive_pins.py          (needs Pillow; written with Pillow 12.2)

libjpeg's progressive mode changes the entropy coding only, so a file and its twin hold the same coefficients: the
generator ASSERTS that Pillow decodes both to the same pixels at all four scales and fails otherwise. The cases:

    40x24 4:2:0, 17x9 4:2:0, 33x31 4:4:4, 24x40 4:2:2, 31x17 grey, 48x32 CMYK 4:2:0 (18 scans),
    136x72 4:2:0 with a restart marker behind every MCU / block (153 segments in luma's AC scans: more than a wave),
    67x45 4:2:2 with a restart marker per MCU row (libjpeg then writes a new DRI in front of every scan),
    and two files made of Pillow's by the byte edits of tests/color_ref.py: a YCCK file (the CMYK file's Adobe transform
    set to 2) and an RGB-coded one (a 4:4:4 file without its JFIF segment, component ids 'R', 'G', 'B').

Arrays: prog/<name>, twin/<name>: the files as uint8; rgb/<name>/<d>: Pillow's RGB; names: the case names.
"""
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "tests", "golden", "progressive_pins.npz")
SCALES = (1, 2, 4, 8)

CASES = (
    ("p420", 40, 24, "RGB", dict(subsampling=2)),
    ("p420_odd", 17, 9, "RGB", dict(subsampling=2)),
    ("p444", 33, 31, "RGB", dict(subsampling=0)),
    ("p422", 24, 40, "RGB", dict(subsampling=1)),
    ("pgray", 31, 17, "L", dict()),
    ("pcmyk", 48, 32, "CMYK", dict(subsampling=2)),
    ("p420_rst1", 136, 72, "RGB", dict(subsampling=2, restart_marker_blocks=1)),
    ("p422_rstrow", 67, 45, "RGB", dict(subsampling=1, restart_marker_rows=1)),
)


def picture(width, height, mode, seed):
    """Smooth shapes with some texture: a few coefficients per block, every scan of the script with something to code.
    The two larger pictures are flat tiles of 24 x 24 pixels, a few of them textured: what Pillow decodes them to is most
    of the pins' bytes, and flat areas compress."""
    from PIL import Image

    n = {"L": 1, "RGB": 3, "CMYK": 4}[mode]
    rng = np.random.default_rng(seed)
    if width * height >= 2000:
        ty, tx = height // 24 + 1, width // 24 + 1
        spread = lambda t: np.repeat(np.repeat(t, 24, 0), 24, 1)[:height, :width]
        a = spread(rng.integers(30, 226, (ty, tx, n))).astype(np.float64)
        a += spread(rng.random((ty, tx)) < 0.15)[..., None] * rng.normal(0, 25, (height, width, n))
    else:
        y, x = np.mgrid[0:height, 0:width].astype(np.float64)
        planes = []
        for c in range(n):
            p = 128 + 70 * np.sin(x / (5.0 + c) + c) + 50 * np.cos(y / (4.0 + 2 * c)) + 30 * ((x // 7 + y // 5) % 2)
            planes.append(p + rng.normal(0, 6, (height, width)))
        a = np.stack(planes, -1)
    a = np.clip(a, 0, 255).astype(np.uint8)
    return Image.fromarray(a[..., 0] if n == 1 else a, mode)


def save(im, **kw):
    b = io.BytesIO()
    im.save(b, "JPEG", quality=85, optimize=True, **kw)
    return b.getvalue()


def pillow_rgb(data, d):
    from PIL import Image

    im = Image.open(io.BytesIO(data))
    w, h = im.size
    if d > 1:
        im.draft("RGB", (max(w // d, 1), max(h // d, 1)))
    out = np.asarray(im.convert("RGB"))
    assert out.shape[:2] == (-(-h // d), -(-w // d)), (out.shape, w, h, d)
    return out


def to_ycck(data):
    """The Adobe segment's transform byte set to 2 (tests/color_ref.app14_adobe)."""
    i = data.index(b"\xff\xee")
    assert data[i + 4:i + 9] == b"Adobe"
    return data[:i + 15] + b"\x02" + data[i + 16:]


def to_rgb_coded(data):
    """Without the JFIF segment, and with the component ids 'R', 'G', 'B' in the frame and scan headers (tests/color_ref.patch_ids)."""
    from tests import color_ref

    assert data[2:4] == b"\xff\xe0" and data[6:11] == b"JFIF\0"
    b = bytearray(data[:2] + data[4 + (data[4] << 8 | data[5]):])
    i, old = 2, None
    while b[i + 1] != 0xD9:
        assert b[i] == 0xFF
        m, n = b[i + 1], b[i + 2] << 8 | b[i + 3]
        if m in (0xC0, 0xC2):
            old = [b[i + 10 + 3 * c] for c in range(3)]
            for c in range(3):
                b[i + 10 + 3 * c] = color_ref.IDS_RGB[c]
        i += 2 + n
        if m == 0xDA:
            for a in range(b[i - n + 2]):
                b[i - n + 3 + 2 * a] = color_ref.IDS_RGB[old.index(b[i - n + 3 + 2 * a])]
            while not (b[i] == 0xFF and b[i + 1] != 0 and not 0xD0 <= b[i + 1] <= 0xD7 and b[i + 1] != 0xFF):
                i += 1
    return bytes(b)


def main():
    files = {}
    for k, (name, w, h, mode, kw) in enumerate(CASES):
        im = picture(w, h, mode, 500 + k)
        files[name] = (save(im, progressive=True, **kw), save(im, progressive=False, **kw))
    files["pycck"] = tuple(to_ycck(f) for f in files["pcmyk"])
    files["prgb"] = tuple(to_rgb_coded(f) for f in files["p444"])
    arrays = {"names": np.array(sorted(files))}
    for name, (prog, twin) in files.items():
        assert b"\xff\xc2" in prog and b"\xff\xc2" not in twin[:600]
        arrays["prog/" + name] = np.frombuffer(prog, np.uint8)
        arrays["twin/" + name] = np.frombuffer(twin, np.uint8)
        for d in SCALES:
            a, b = pillow_rgb(prog, d), pillow_rgb(twin, d)
            assert np.array_equal(a, b), "Pillow decodes %s and its twin differently at 1/%d" % (name, d)
            arrays["rgb/%s/%d" % (name, d)] = a
    np.savez_compressed(OUT, **arrays)
    print("%d cases, %d bytes" % (len(files), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
