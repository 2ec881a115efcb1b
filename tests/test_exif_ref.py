"""The EXIF restatement (tests/exif_ref.py) against Pillow itself: for every case of its list, spliced into a baseline
and a progressive file, orientation_of_file is what Image.open(f).getexif().get(0x0112) amounts to, and exif_ref.apply is
ImageOps.exif_transpose. Where Pillow and the written rule disagreed on a crafted case, the rule was changed. Skipped
without Pillow; no GPU needed."""
import io
import os
import warnings

import numpy as np
import pytest

from tests import exif_ref
from tests.conftest import GOLDEN

PIL = pytest.importorskip("PIL")


@pytest.fixture(scope="module")
def bases():
    from tools import jpegsynth

    return {"baseline": jpegsynth.encode(40, 24, ((2, 2), (1, 1), (1, 1)), seed=3),
            "progressive": np.load(os.path.join(GOLDEN, "progressive_pins.npz"))["prog/p420"].tobytes()}


def pillow_orientation(im):
    v = im.getexif().get(0x0112)
    return v if isinstance(v, int) and 1 <= v <= 8 else 1  # what exif_transpose's table of the values 2..8 makes of it


@pytest.mark.parametrize("kind", ("baseline", "progressive"))
def test_every_case_against_pillow(bases, kind):
    from PIL import Image, ImageOps

    n = 0
    for name, (data, want) in exif_ref.cases(bases[kind]).items():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # Pillow warns about the truncated ones, and opens them
            im = Image.open(io.BytesIO(data))
            got = pillow_orientation(im)
            shown = np.asarray(ImageOps.exif_transpose(im).convert("RGB"))
        assert got == want, (name, "the list's expectation is not Pillow's")
        assert exif_ref.orientation_of_file(data) == want, (name, "the rule")
        stored = np.asarray(Image.open(io.BytesIO(bases[kind])).convert("RGB"))
        assert np.array_equal(shown, exif_ref.apply(stored, want)), (name, "the table")
        n += 1
    assert n >= 60


def test_the_list_holds_what_it_must():
    """Both byte orders; the tag first, last and absent; SHORT, LONG, BYTE and count 2; the values 0, 9 and 0x0106; IFD
    offsets 8, with a gap and past the end; too many entries; lengths 8, 13 and 14; behind JFIF, Adobe and a DQT; two segments."""
    names = set(exif_ref.segments())
    for en in ("II", "MM"):
        for part in ("short 1", "short 8", "long 6", "byte 6", "count 2", "first 3", "last 8", "absent", "value 0", "value 9",
                     "value 0x0106", "ifd gap", "ifd past the end", "entry count too large", "length 8", "length 13", "length 14",
                     "behind JFIF", "behind Adobe", "two segments"):
            assert "%s %s" % (en, part) in names
    from tools import jpegsynth

    assert "after a DQT" in exif_ref.cases(jpegsynth.encode(16, 16, ((1, 1),), seed=1))
    assert sorted({w for _, w in exif_ref.segments().values()}) == list(range(1, 9))


def test_the_eight_values_are_the_written_table():
    h, w = 5, 7
    s = np.arange(h * w).reshape(h, w)
    f = {1: lambda x, y: s[y][x], 2: lambda x, y: s[y][w - 1 - x], 3: lambda x, y: s[h - 1 - y][w - 1 - x], 4: lambda x, y: s[h - 1 - y][x],
         5: lambda x, y: s[x][y], 6: lambda x, y: s[h - 1 - x][y], 7: lambda x, y: s[h - 1 - x][w - 1 - y], 8: lambda x, y: s[x][w - 1 - y]}
    for o in range(1, 9):
        d = exif_ref.apply(s, o)
        ow, oh = exif_ref.orient_size(o, w, h)
        assert d.shape == (oh, ow)
        assert all(d[y][x] == f[o](x, y) for y in range(oh) for x in range(ow)), o
