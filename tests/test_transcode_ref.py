"""tests/transcode_ref.py against Pillow: every direction of a transcode on every pinned source
(tests/golden/transcode_pins.npz) gives, byte for byte, the file Pillow wrote for the same pixels with the other options; and
the same on a seeded sweep of other sizes against the Pillow at hand, where there is one."""
import io

import numpy as np
import pytest

from tests import transcode_cases as T
from tests import transcode_ref as R

CASES = T.cases()
DIRECTIONS = T.DIRECTIONS


def test_pins_cover_the_cases():
    files, _ = T.pins()
    assert sorted(files) == sorted(c["name"] for c in CASES)
    assert all(files[c["name"]]["R"] is not None for c in CASES if c["restart_to"] is not None)
    sizes = {(c["w"], c["h"]) for c in CASES}
    assert sizes == set(T.SIZES) and {c["sampling"] for c in CASES} == set(T.SAMPLINGS)
    assert {c["quality"] for c in CASES} == {1, 75, 100, None}
    assert {0, 1, 3} <= {c["restart_interval"] for c in CASES} and any(c["restart_interval"] == T.mcus_x(c) > 3 for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_every_direction_equals_pillow(case):
    files = T.pins()[0][case["name"]]
    for src, options, want in DIRECTIONS:
        assert R.transcode(files[src], **options) == files[want], (src, options, want)
    if case["restart_to"] is not None:
        assert R.transcode(files["A"], restart_interval=case["restart_to"]) == files["R"]
        assert R.transcode(files["R"], restart_interval=case["restart_interval"]) == files["A"]


def test_live_pillow_on_a_seeded_sweep():
    """Sizes the pins do not have, every sampling, qualities 1..100 and custom tables, restart intervals 0..5 on both sides:
    each source is saved plain, optimised and progressive, and every direction, with and without a new interval, is Pillow's
    file."""
    Image = pytest.importorskip("PIL.Image")
    from PIL import ImageFile, features

    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("this Pillow is not built on libjpeg-turbo")
    rng = np.random.default_rng(20261021)
    saved = ImageFile.MAXBLOCK
    ImageFile.MAXBLOCK = 1 << 24

    def save(img, params, restart, **more):
        f = io.BytesIO()
        Image.fromarray(img).save(f, "JPEG", restart_marker_blocks=restart, **params, **more)
        return f.getvalue()

    try:
        for k in range(40):
            h, w = (int(v) for v in rng.integers(1, 91, 2))
            grey = bool(rng.integers(0, 2))
            img = rng.integers(0, 256, (h, w) if grey else (h, w, 3), dtype=np.uint8)
            kind = int(rng.integers(0, 3))
            if kind == 1:
                img = (img // 64 * 64).astype(np.uint8)
            elif kind == 2:  # nearly flat: long end-of-band runs
                img = (120 + (img > 250) * 60).astype(np.uint8)
            params = dict(subsampling=int(rng.integers(0, 3)))
            if k % 5 == 4:  # custom tables, drawn too
                tabs = [[int(v) for v in rng.integers(1, 256, 64)] for _ in range(2)]
                params["qtables"] = tabs[:1 if grey else 2]
            else:
                params["quality"] = int(rng.integers(1, 101))
            r, to = (int(v) for v in rng.integers(0, 6, 2))
            what = (h, w, grey, kind, params, r, to)
            files = dict(A=save(img, params, r), B=save(img, params, r, optimize=True), C=save(img, params, r, progressive=True))
            for src, options, want in DIRECTIONS:
                assert R.transcode(files[src], **options) == files[want], (what, src, options)
            for src in "ABC":  # another interval, from every kind of source to every kind of file
                assert R.transcode(files[src], restart_interval=to) == save(img, params, to), (what, src)
            assert R.transcode(files["A"], optimize=True, restart_interval=to) == save(img, params, to, optimize=True), what
            assert R.transcode(files["B"], progressive=True, restart_interval=to) == save(img, params, to, progressive=True), what
    finally:
        ImageFile.MAXBLOCK = saved


def test_escapes_are_exercised():
    """Quality 100 on noise and the custom tables reach AC categories of 10: the decoder's escape entries."""
    files, _ = T.pins()
    top = {c["name"]: int(np.abs(R.coefficients(files[c["name"]]["A"])["coefs"][:, 1:]).max()) for c in CASES if c["kind"] == "noise" and c["quality"] in (100, None)}
    assert max(top.values()) >= 512, top
