"""tests/transcode_orient_ref.py: the orientation rules in the coefficient domain against the float IDCT, an orientation
and its inverse against the plain transcode, and every pinned and every freshly written Pillow file of a transposed image
(tests/transcode_orient_cases.py) against transform() of Pillow's file of the image itself."""
import io

import numpy as np
import pytest

from tests import encode_ref as E
from tests import transcode_orient_cases as K
from tests import transcode_orient_ref as X
from tests import transcode_ref as R

PIN_CASES = K.pin_cases()


def _idct(blocks):
    """The float IDCT of [n, 64] natural-order blocks: [n, 8, 8] samples (without level shift)."""
    x, u = np.mgrid[0:8, 0:8]
    basis = np.where(u == 0, np.sqrt(0.125), 0.5) * np.cos((2 * x + 1) * u * np.pi / 16)  # [x, u]
    return np.einsum("yv,nvu,xu->nyx", basis, blocks.reshape(-1, 8, 8).astype(np.float64), basis)


def test_idct_identity():
    """The IDCT of the oriented block is the oriented IDCT of the block. 1e-8 absolute on |coefficient| < 1024: double
    rounding over 64 terms of magnitude below 2^10 is some 1e-12; four orders of room."""
    rng = np.random.default_rng(20261101)
    blocks = rng.integers(-1023, 1024, (3, 4, 64))
    pixels = _idct(blocks.reshape(-1, 64)).reshape(3, 4, 8, 8).transpose(0, 2, 1, 3).reshape(24, 32)  # the image of the grid
    worst = 0.0
    for o in range(1, 9):
        got = X.orient_blocks(blocks, o)
        by, bx = got.shape[:2]
        image = _idct(got.reshape(-1, 64)).reshape(by, bx, 8, 8).transpose(0, 2, 1, 3).reshape(8 * by, 8 * bx)
        want = X.orient_pixels(pixels, o)
        assert image.shape == want.shape
        worst = max(worst, float(np.abs(image - want).max()))
        assert np.abs(image - want).max() < 1e-8, o
    print("largest difference: %.3g" % worst)
    assert (X.orient_blocks(blocks, 1) == blocks).all()
    for o in range(1, 9):  # the DC never changes sign, and the inverse orientation undoes the blocks
        assert (np.sort(X.orient_blocks(blocks, o)[..., 0].ravel()) == np.sort(blocks[..., 0].ravel())).all()
        assert (X.orient_blocks(X.orient_blocks(blocks, o), X.INVERSE[o]) == blocks).all()


def test_orient_pixels_is_the_table():
    s = np.arange(3 * 5).reshape(3, 5)  # H = 3, W = 5
    h, w = s.shape
    table = {1: lambda y, x: s[y, x], 2: lambda y, x: s[y, w - 1 - x], 3: lambda y, x: s[h - 1 - y, w - 1 - x], 4: lambda y, x: s[h - 1 - y, x],
             5: lambda y, x: s[x, y], 6: lambda y, x: s[h - 1 - x, y], 7: lambda y, x: s[h - 1 - x, w - 1 - y], 8: lambda y, x: s[x, w - 1 - y]}
    for o, f in table.items():
        got = X.orient_pixels(s, o)
        assert got.shape == ((w, h) if o >= 5 else (h, w))
        assert all(got[y, x] == f(y, x) for y in range(got.shape[0]) for x in range(got.shape[1])), o


def test_edge_rules():
    for o in range(1, 9):
        assert X.target_size(32, 48, 2, 2, o) == (32, 48)
    assert X.target_size(17, 40, 2, 2, 5) == (17, 40) and X.target_size(17, 40, 1, 1, 6) == (17, 40)
    for o in (2, 3, 7, 8):
        with pytest.raises(X.Unsupported):
            X.target_size(17, 40, 1, 1, o)
        assert X.target_size(17, 40, 1, 1, o, trim=True) == (16, 40)
        with pytest.raises(X.Unsupported):
            X.target_size(40, 16, 2, 1, o)  # 4:2:2: 16 pixels to the iMCU
        assert X.target_size(40, 16, 2, 1, o, trim=True) == (32, 16)
        with pytest.raises(X.Unsupported):
            X.target_size(5, 16, 1, 1, o, trim=True)
    for o in (3, 4, 6, 7):
        with pytest.raises(X.Unsupported):
            X.target_size(16, 35, 1, 1, o)
        assert X.target_size(16, 35, 2, 2, o, trim=True) == (16, 32)
        with pytest.raises(X.Unsupported):
            X.target_size(16, 15, 2, 2, o, trim=True)
    assert X.target_size(35, 21, 2, 2, 3, trim=True) == (32, 16)


def _round_trip_sources():
    rng = np.random.default_rng(20261102)
    for k, (w, h, sampling) in enumerate([(32, 16, "4:2:0"), (16, 48, "4:4:4"), (24, 8, "grey"), (48, 32, "4:2:0"), (32, 32, "4:2:2"), (16, 16, "4:2:0")]):
        img = rng.integers(0, 256, (h, w) if sampling == "grey" else (h, w, 3), dtype=np.uint8)
        yield (w, h, sampling), E.encode(img, [60, 95, 30][k % 3], "4:4:4" if sampling == "grey" else sampling, k % 3)


def test_an_orientation_and_its_inverse():
    """Sizes of whole iMCUs on both axes: o and then its inverse give the plain transcode of the source, byte for byte, for
    every kind of file in between and at the end; the file in between differs from it."""
    n = 0
    for what, src in _round_trip_sources():
        for o in range(1, 9):
            if what[2] == "4:2:2" and o >= 5:
                with pytest.raises(X.Unsupported):
                    X.transform(src, o)
                continue
            for options in (dict(), dict(optimize=True), dict(progressive=True), dict(restart_interval=2)):
                between = X.transform(src, o, progressive=bool(n % 2), optimize=bool(n % 3 == 0))
                assert X.transform(between, X.INVERSE[o], **dict(dict(restart_interval=R.parse(src)["restart"]), **options)) == \
                    R.transcode(src, **dict(dict(restart_interval=R.parse(src)["restart"]), **options)), (what, o, options)
                n += 1
            if o != 1:
                assert X.transform(src, o) != R.transcode(src)
                info, head = R.parse(src), R.parse(X.transform(src, o))
                assert (head["w"], head["h"]) == ((info["h"], info["w"]) if o >= 5 else (info["w"], info["h"]))
    assert n == 4 * (5 * 8 + 4)


def test_tables_and_sampling_byte():
    """5..8 transpose both tables and exchange the nibbles of component 0's sampling byte, a grey file's included."""
    rng = np.random.default_rng(7)
    inverse = np.argsort(E.ZIGZAG)
    for sampling, nc in (("4:2:0", 3), ("4:4:4", 3), ("4:2:2", 1), ("4:2:0", 1)):
        img = rng.integers(0, 256, (16, 32) if nc == 1 else (16, 32, 3), dtype=np.uint8)
        src = E.encode(img, 50, sampling, 0)
        info = R.parse(src)
        for o in (2, 5, 6):
            head = R.parse(X.transform(src, o))
            for t in info["qtabs"]:
                q, p = np.array(info["qtabs"][t])[inverse].reshape(8, 8), np.array(head["qtabs"][t])[inverse].reshape(8, 8)
                assert (p == (q.T if o >= 5 else q)).all() and (t != 0 or not (q == q.T).all())  # (Annex K's chroma table is symmetric)
            b = info["comps"][0]["sampling"]
            assert head["comps"][0]["sampling"] == (((b << 4 | b >> 4) & 0xFF) if o >= 5 else b)
    assert R.parse(X.transform(E.encode(img, 50, "4:2:2", 0), 5))["comps"][0]["sampling"] == 0x12


def test_pins_cover_the_cases():
    sources, want, _ = K.pins()
    assert sorted(sources) == sorted(c["name"] for c in PIN_CASES)
    assert {(c["w"], c["h"]) for c in PIN_CASES} == set(K.SIZES) and {c["sampling"] for c in PIN_CASES} == set(K.SAMPLINGS)
    equal = refused = 0
    for c in PIN_CASES:
        for o in range(1, 9):
            perfect, trimmed = K.allowed(c, o, False) is not None, K.allowed(c, o, True) is not None
            assert trimmed or not perfect
            for k in K.KINDS:
                assert ((c["name"], o, False, k) in want) == perfect and ((c["name"], o, True, k) in want) == (trimmed and not perfect), (c["name"], o)
            equal, refused = equal + 3 * (perfect + trimmed), refused + 3 * (2 - perfect - trimmed)
    print("combinations: %d pinned, %d refused" % (equal, refused))
    assert any(k[2] for k in want) and any(k[1] == 5 and k[0].startswith("17x40") for k in want)
    for name, data in sources.items():  # the symmetric tables are what the parsed DQT holds
        if name.endswith("_sym"):
            inverse = np.argsort(E.ZIGZAG)
            tabs = R.parse(data)["qtabs"]
            for t, q in tabs.items():
                assert (np.array(q)[inverse] == np.array(K.SYM_TABLES[t])).all() and (np.array(q)[inverse].reshape(8, 8) == np.array(q)[inverse].reshape(8, 8).T).all()


@pytest.mark.parametrize("case", PIN_CASES, ids=[c["name"] for c in PIN_CASES])
def test_pins_equal_pillow(case):
    """transform of Pillow's file of the pixels is Pillow's file of Image.transpose of the (cut) pixels, for every
    orientation the rules allow, plain, optimised and progressive, without and with trim; and refused where they refuse."""
    src = K.pins()[0][case["name"]]
    for o in range(1, 9):
        for trim in (False, True):
            if K.allowed(case, o, trim) is None:
                with pytest.raises(X.Unsupported):
                    X.transform(src, o, trim)
                continue
            for kind, options in K.KINDS.items():
                assert X.transform(src, o, trim, **options) == K.expected(case["name"], o, trim, kind), (o, trim, kind)


def test_live_pillow_sweep():
    """The same against the Pillow at hand, on freshly drawn cell images of the pin sizes and a few more, with restart
    intervals.

    Not a pass criterion, and not asserted: Pillow's decode of a transformed NOISE file against the transposed decode of its
    source. It is not exact -- libjpeg's ISLOW IDCT does not round alike along rows and columns, and clamping and the colour
    conversion follow it -- and differed by up to 3 levels on at most 5.9 % of the samples (64 x 64 noise, 4:4:4 and grey,
    qualities 75 and 95, Pillow's decode): the transposing orientations on 5.6 to 5.9 %, the mirrors alone on at most 0.01 %."""
    Image = pytest.importorskip("PIL.Image")
    from PIL import ImageFile, features

    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("this Pillow is not built on libjpeg-turbo")
    saved = ImageFile.MAXBLOCK
    ImageFile.MAXBLOCK = 1 << 24

    def save(im, params, **more):
        f = io.BytesIO()
        im.save(f, "JPEG", **params, **more)
        return f.getvalue()

    rng = np.random.default_rng(20261103)
    equal = refused = 0
    try:
        for w, h in K.SIZES + [(24, 56), (50, 33), (96, 16)]:
            for sampling in K.SAMPLINGS:
                case = dict(w=w, h=h, sampling=sampling, tables=["q100", "sym"][int(rng.integers(0, 2))])
                img = K.cell_image(case) ^ np.uint8(rng.integers(0, 256))
                assert (img == np.repeat(np.repeat(img[::16, ::16], 16, 0), 16, 1)[:h, :w]).all()
                params = dict(K.save_params(case), restart_marker_blocks=int(rng.integers(0, 3)))
                src = save(Image.fromarray(img), params)
                for o in range(1, 9):
                    for trim in (False, True):
                        size = K.allowed(case, o, trim)
                        if size is None:
                            with pytest.raises(X.Unsupported):
                                X.transform(src, o, trim)
                            refused += 3
                            continue
                        im = Image.fromarray(img[:size[1], :size[0]])
                        if o != 1:
                            im = im.transpose(getattr(Image.Transpose, K.PIL_METHOD[o]))
                        assert (np.asarray(im) == X.orient_pixels(img[:size[1], :size[0]], o)).all()
                        for kind, options in K.KINDS.items():
                            assert X.transform(src, o, trim, **options) == save(im, params, **options), (case, o, trim, kind)
                            equal += 1
    finally:
        ImageFile.MAXBLOCK = saved
    print("live: %d equal, %d refused" % (equal, refused))
