"""tests/transcode_frame_ref.py against Pillow: the restatement of a pinned source with a kind's options is, byte for byte,
Pillow's file of the same pixels with those options, and with an orientation Pillow's file of the turned pixels. No GPU."""
import pytest

from tests import transcode_frame_cases as K
from tests import transcode_frame_ref as F

PINS = K.pins()
SOURCES = sorted({k[2:].rsplit("-", 1)[0] for k in PINS if k.startswith("S_")})
ORIENTED = sorted({k[2:].rsplit("-", 1)[0] for k in PINS if k.startswith("O_")})


def test_the_pins_are_the_cases():
    assert SOURCES == sorted(K.sources()) and ORIENTED == sorted(K.oriented())
    assert len(SOURCES) == 16 and all("S_%s-%s" % (s, k) in PINS for s in SOURCES for k in K.KINDS)


def test_what_the_pins_are():
    """The sources lie outside the encoder's layouts, each for the reason it was made for."""
    for name in SOURCES:
        src = PINS["S_%s-A" % name]
        info = F.parse(src)
        assert not F.in_encoder_range(src, info), name
        kind = name.split("_")[0]
        assert info["color"] == {"cmyk": "cmyk", "rgb": "rgb"}.get(kind, "ycbcr"), name
        if kind in ("t3", "t16"):
            assert [c["q"] for c in info["comps"]] == [0, 1, 2] and info["qtabs"][1] != info["qtabs"][2], name
            assert (max(info["qtabs"][2]) > 255) == (kind == "t16") and src[src.index(b"\xff\xdb") + 4] >> 4 == (kind == "t16"), name
            assert (b"\xff\xc1" in src[:700]) == (kind == "t16"), name


@pytest.mark.parametrize("name", SOURCES)
def test_options(name):
    src = PINS["S_%s-A" % name]
    for kind, options in K.OPTIONS.items():
        assert F.transcode(src, **options) == PINS["S_%s-%s" % (name, kind)], (name, kind)
    assert F.transcode(src) == src, "restart_interval None keeps the source's"
    again = PINS["S_%s-Br" % name]  # an optimised source with restart markers back to the plain file
    assert F.transcode(again, restart_interval=0) == src, name


@pytest.mark.parametrize("name", ORIENTED)
def test_orientations(name):
    src = PINS["O_%s-1" % name]
    for o in range(2, 9):
        assert F.transcode(src, orientation=o) == PINS["O_%s-%d" % (name, o)], (name, o)
        assert F.transcode(src, optimize=True, orientation=o) != PINS["O_%s-%d" % (name, o)]


def test_the_scripts():
    """Pillow's progressive files have 2 + 4 n scans, and the ten of three-component YCbCr; and they come back plain."""
    for name, scans in (("cmyk_80x64", 18), ("rgb_80x64", 14), ("t3_422_80x64", 10), ("t16_420_75x53", 10)):
        for kind in ("C", "Cr"):
            assert PINS["S_%s-%s" % (name, kind)].count(b"\xff\xda") == scans, name
            assert F.transcode(PINS["S_%s-%s" % (name, kind)], restart_interval=0) == PINS["S_%s-A" % name], (name, kind)
