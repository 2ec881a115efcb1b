"""The numpy restatement of libjpeg-turbo's scaled decoding (tests/draft_ref.py) against Pillow: the pinned outputs of
tests/golden/draft_pins.npz for every pinned case, and live Pillow when it imports. No GPU needed."""
import hashlib
import os

import numpy as np
import pytest

from tests import draft_ref
from tests.conftest import GOLDEN


@pytest.fixture(scope="module")
def pins():
    return np.load(os.path.join(GOLDEN, "draft_pins.npz"))


@pytest.fixture(scope="module")
def decoded():
    from oracle import oracle

    return {name: (data, oracle.decode(data)) for name, data in draft_ref.inputs().items()}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def test_block_size_rule():
    # 4:2:0: chroma one size above luma; 4:2:2, 4:4:0 and 4:4:4 keep one size (both directions must allow the doubling)
    S420, S422, S440, S444 = ([2, 1, 1], [2, 1, 1]), ([2, 1, 1], [1, 1, 1]), ([1, 1, 1], [2, 1, 1]), ([1, 1, 1], [1, 1, 1])
    assert [draft_ref.block_sizes(*S420, d) for d in (2, 4, 8)] == [[4, 8, 8], [2, 4, 4], [1, 2, 2]]
    for s in (S422, S440, S444):
        assert [draft_ref.block_sizes(*s, d) for d in (2, 4, 8)] == [[4] * 3, [2] * 3, [1] * 3]
    # 4x4 luma over 1x1 chroma: two doublings at 1/4, three at 1/8
    assert [draft_ref.block_sizes([4, 1, 1], [4, 1, 1], d) for d in (2, 4, 8)] == [[4, 8, 8], [2, 8, 8], [1, 4, 4]]
    assert draft_ref.effective_factors(*S420, 2) == ([2, 2, 2], [2, 2, 2])
    assert draft_ref.effective_factors(*S422, 8) == ([2, 1, 1], [1, 1, 1])
    assert draft_ref.plane_sizes(4032, 3024, *S420, 2) == [(2016, 1512)] * 3
    assert draft_ref.plane_sizes(17, 9, *S420, 8) == [(3, 2)] * 3
    assert [draft_ref.fancy(d) for d in (2, 4, 8)] == [True, True, False]


def test_inputs_are_the_pinned_ones(pins, decoded):
    names = {k.partition("/")[2] for k in pins.files if k.startswith("jpeg_sha256/")}
    assert names == set(decoded)
    for name, (data, _) in decoded.items():
        assert hashlib.sha256(data).hexdigest() == str(pins["jpeg_sha256/" + name]), (name, "input differs from the pinned one")


def test_restatement_equals_the_pins(pins, decoded):
    n = 0
    for name, (data, dec) in decoded.items():
        for d in draft_ref.SCALES:
            key = "%s/%d" % (name, d)
            if not draft_ref.pillow_comparable(name, dec, d):
                assert "rgb/" + key not in pins.files and "rgb_sha256/" + key not in pins.files
                continue
            got = draft_ref.draft_rgb_of(dec, d)
            if "rgb/" + key in pins.files:
                want = pins["rgb/" + key]
                assert got.shape == want.shape and np.array_equal(got, want), (key, int((got != want).sum()) if got.shape == want.shape else got.shape)
            else:
                assert sha(got) == str(pins["rgb_sha256/" + key]), key
            n += 1
    assert n == sum(k.startswith(("rgb/", "rgb_sha256/")) for k in pins.files) >= 299


def test_exclusions_are_the_two_kinds_only(decoded):
    """Not compared with Pillow: dense_escapes at 1/2 and files smaller than d in a direction -- nothing else."""
    excluded = [(name, d) for name, (_, dec) in decoded.items() if draft_ref.has_rgb(dec) for d in draft_ref.SCALES
                if not draft_ref.pillow_comparable(name, dec, d)]
    assert ("dense_escapes", 2) in excluded
    for name, d in excluded:
        dec = decoded[name][1]
        assert (name, d) == ("dense_escapes", 2) or dec.width < d or dec.height < d, (name, d)
    assert len(excluded) == 19


def test_restatement_equals_live_pillow(decoded):
    pytest.importorskip("PIL")
    n = 0
    for name, (data, dec) in decoded.items():
        for d in draft_ref.SCALES:
            if not draft_ref.pillow_comparable(name, dec, d):
                continue
            want, size = draft_ref.pillow_draft_rgb(data, d)
            assert size == (draft_ref.ceil_div(dec.width, d), draft_ref.ceil_div(dec.height, d)), (name, d, size)
            got = draft_ref.draft_rgb_of(dec, d)
            assert got.shape == want.shape and np.array_equal(got, want), (name, d)
            n += 1
    assert n >= 299


def test_uniform_scaling_is_not_pillows(decoded):
    """What the library did before this mode (one size for all components, then fancy upsampling) differs from Pillow on
    the subsampled layouts the rule changes: the photo at all three scales among them."""
    from tests import libjpeg_ref, scaled_ref

    data, dec = decoded["photo"]
    for d in draft_ref.SCALES:
        old = libjpeg_ref.planes_to_rgb_fancy(scaled_ref.scaled_planes_of(dec, d), list(dec.hs), list(dec.vs),
                                              draft_ref.ceil_div(dec.width, d), draft_ref.ceil_div(dec.height, d))
        assert not np.array_equal(old, draft_ref.draft_rgb_of(dec, d)), d


def test_crop_windows_hold_every_sample_the_rectangle_reads(decoded):
    rng = np.random.default_rng(7)
    for name in ("ss_2x2", "ss_2x1", "sweep:y4x2_a", "sweep:y1x1_cb2x2_a", "gray"):
        dec = decoded[name][1]
        hs, vs = draft_ref.factors_of(dec)
        for d in draft_ref.SCALES:
            W, H = draft_ref.ceil_div(dec.width, d), draft_ref.ceil_div(dec.height, d)
            eh, ev = draft_ref.effective_factors(hs, vs, d)
            full = draft_ref.plane_sizes(dec.width, dec.height, hs, vs, d)
            for _ in range(20):
                w, h = int(rng.integers(1, W + 1)), int(rng.integers(1, H + 1))
                x, y = int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1))
                win, _ = draft_ref.crop_windows(dec.width, dec.height, hs, vs, d, (x, y, w, h))
                for c, (ox, oy, sx, sy) in enumerate(win):
                    hr, vr = max(eh) // eh[c], max(ev) // ev[c]
                    assert ox <= max(x // hr - 1, 0) and ox + sx - 1 >= min((x + w - 1) // hr + 1, full[c][0] - 1)
                    assert oy <= max(y // vr - 1, 0) and oy + sy - 1 >= min((y + h - 1) // vr + 1, full[c][1] - 1)
                    assert ox + sx <= full[c][0] and oy + sy <= full[c][1]
