"""The numpy restatement of Pillow's Image.thumbnail on JPEG files (tests/thumbnail_ref.py) against Pillow: the pinned outputs
of tests/golden/thumbnail_pins.npz for every case of tests/thumbnail_cases.py, and live Pillow on a seeded sweep when it
imports. No GPU needed."""
import hashlib

import numpy as np
import pytest

from tests import thumbnail_cases as TC
from tests import thumbnail_ref as T


@pytest.fixture(scope="module")
def pins():
    return TC.load_pins()


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def frame(data):
    from tests import exif_ref

    return exif_ref.frame_size(data)


def cpu_decode(data):
    """decode(scale) for thumbnail_ref.thumbnail by the CPU restatement of libjpeg's (scaled) decoding; a grey file gives
    one channel. None for a progressive file, which that restatement does not read."""
    from tests import color_ref

    if b"\xff\xc2" in data[:1024]:
        return None

    def decode(s):
        a = color_ref.color_rgb(data, s)
        return a[:, :, 0] if color_ref.model_of_file(data) == color_ref.GRAY else a

    return decode


# what every case is in the list for: (scale, (fx, fy), (out_w, out_h), identity) and, where it matters, more
EXPECT = {
    "noop": (1, (1, 1), (40, 30), True), "rw_only": (1, (1, 1), (27, 20), False), "draft2": (2, (1, 1), (48, 36), False),
    "draft4": (4, (1, 1), (16, 12), False), "draft8": (8, (1, 1), (24, 17), False), "hit8": (8, (1, 1), (80, 60), True),
    "hit4": (4, (1, 1), (80, 60), True), "reduce_eq": (4, (2, 2), (10, 8), False), "reduce_ne": (8, (4, 3), (10, 8), False),
    "reduce_ne_gray": (8, (4, 3), (10, 8), False), "reduce_440": (4, (2, 2), (10, 8), False), "reduce_422_8": (8, (4, 3), (5, 4), False),
    "reduce_deep": (1, (33, 31), (5, 4), False), "reduce_rgb": (1, (3, 3), (10, 5), False), "reduce_fy1": (8, (2, 1), (10, 8), False),
    "one": (2, (17, 10), (10, 1), False), "white_reduce": (1, (10, 10), (10, 8), False), "white_draft": (8, (2, 2), (10, 8), False),
    "checker": (1, (6, 6), (10, 8), False), "gap_none": (1, (1, 1), (48, 36), False), "gap_none_big": (1, (1, 1), (96, 69), False),
    "gap3": (4, (2, 2), (24, 18), False), "gap1": (4, (2, 2), (24, 18), False),
}


def test_cases_are_what_they_are_listed_for(pins):
    assert {c[0] for c in TC.CASES} == set(EXPECT)
    plans = {}
    for case, src, req, gap in TC.CASES:
        w, h = frame(TC.source(pins, src))
        assert (w, h) == tuple(TC.SOURCES[src][1:3]) or TC.SOURCES[src][0] == "pillow" and (w, h) == tuple(TC.SOURCES[src][2:4])
        p = plans[case] = T.plan(w, h, req[0], req[1], gap)
        assert (p.scale, (p.fx, p.fy), (p.out_w, p.out_h), bool(p.identity)) == EXPECT[case], (case, p.astuple())
    frac = lambda p: float(p.box_w) != p.red_w or float(p.box_h) != p.red_h  # noqa: E731
    assert all(frac(plans[c]) for c in ("draft2", "draft4", "draft8", "reduce_eq", "reduce_ne_gray", "reduce_422_8"))
    ragged = lambda p: p.dec_w % p.fx != 0 or p.dec_h % p.fy != 0  # noqa: E731
    assert all(ragged(plans[c]) for c in ("reduce_eq", "reduce_ne_gray", "reduce_deep", "checker", "one")) and not ragged(plans["reduce_ne"])
    # binary32 matters: a box that is no float value
    assert float(plans["reduce_422_8"].box_w) == float(np.float32(333 / 8 / 4)) and float(plans["reduce_ne_gray"].box_h) != 479 / 8 / 3


def test_restatement_equals_the_pins(pins):
    n = passed_over = 0
    for case, src, req, gap in TC.CASES:
        data = TC.source(pins, src)
        decode = cpu_decode(data)
        if decode is None:
            try:
                import PIL  # noqa: F401
            except ImportError:
                passed_over += 1
                continue
            decode = T.pillow_decode(data)
        w, h = frame(data)
        for filt in TC.FILTERS:
            got, _ = T.thumbnail(decode, w, h, req[0], req[1], filt, gap)
            k = TC.key(case, filt)
            if "out/" + k in pins.files:
                want = pins["out/" + k]
                assert got.shape == want.shape and np.array_equal(got, want), (case, filt, got.shape, want.shape)
            else:
                assert (got.shape[1], got.shape[0]) == tuple(pins["size/" + k]) and sha(got) == str(pins["out_sha256/" + k]), (case, filt)
            n += 1
    assert n >= 2 * (len(TC.CASES) - 3) and passed_over <= 3


def test_saturated_sources_stay_saturated(pins):
    """Image.reduce is not a rounded mean, but 255 everywhere must stay 255 through it (and black and white squares of one
    pixel become the multiplier's idea of a half)."""
    for filt in TC.FILTERS:
        assert (pins["out/" + TC.key("white_reduce", filt)] >= 254).all()
    a = np.full((7, 13), 255, np.uint8)
    assert (T.reduce(a, 3, 2) == 255).all() and (T.reduce(a, 13, 7) == 255).all() and (T.reduce(a, 5, 5) == 255).all()
    b = (np.indices((6, 6)).sum(0) & 1).astype(np.uint8) * 255
    assert T.reduce(b, 3, 3).tolist() == [[113, 142], [142, 113]]  # (4 * 255 + 4) * m >> 24 and (5 * 255 + 4) * m >> 24, m = 1864135
    assert T.reduce_multiplier(9) == 1864135 and T.reduce_multiplier(4) == 1 << 22 and T.reduce_multiplier(1) == 1 << 24


def test_reduce_equals_pillow():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(41)
    shapes = [(1, 1, 1, 1), (7, 13, 3, 2), (60, 81, 3, 4), (39, 51, 2, 2), (20, 348, 10, 17), (251, 333, 31, 33), (96, 128, 6, 6), (30, 40, 1, 2),
              (5, 9, 7, 11)]
    shapes += [tuple(int(v) for v in (*rng.integers(1, 200, 2), *rng.integers(1, 40, 2))) for _ in range(40)]
    for i, (h, w, fy, fx) in enumerate(shapes):
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        if i % 4 == 1:
            a[:] = 255
        if i % 4 == 2:
            a[:] = ((np.indices((h, w)).sum(0) & 1) * 255)[:, :, None]
        assert np.array_equal(T.reduce(a, fx, fy), np.asarray(Image.fromarray(a).reduce((fx, fy)))), (h, w, fy, fx)
        assert np.array_equal(T.reduce(a[:, :, 0], fx, fy), np.asarray(Image.fromarray(a[:, :, 0]).reduce((fx, fy)))), (h, w, fy, fx, "L")


def test_sweep_equals_pillow():
    pytest.importorskip("PIL")
    seen = {k: 0 for k in ("files", "noop", "hit", "draft2", "draft4", "draft8", "fractional", "reduce_eq", "reduce_ne", "ragged", "one", "gap_none",
                           "bilinear", "bicubic", "gray", "color", "replicate_reduce", "refused", "444", "420", "422", "440")}
    datas = set()
    for data, w, h, req, filt, gap, layout in TC.sweep():
        datas.add(data)
        try:
            got, p = T.thumbnail(T.pillow_decode(data), w, h, req[0], req[1], filt, gap)
        except T.Refused:
            seen["refused"] += 1
            continue
        want = T.pillow_thumbnail(data, req[0], req[1], filt, gap)
        assert got.shape == want.shape and np.array_equal(got, want), (w, h, req, filt, gap, p.astuple(), got.shape, want.shape)
        reduces = p.fx > 1 or p.fy > 1
        seen["noop"] += req[0] >= w and req[1] >= h
        seen["hit"] += bool(p.identity) and p.scale > 1
        seen["draft%d" % p.scale if p.scale > 1 and not reduces and not p.identity else "files"] += 1
        seen["fractional"] += not p.identity and (float(p.box_w) != p.red_w or float(p.box_h) != p.red_h)
        seen["reduce_eq"] += reduces and p.fx == p.fy
        seen["reduce_ne"] += reduces and p.fx != p.fy
        seen["ragged"] += reduces and (p.dec_w % p.fx != 0 or p.dec_h % p.fy != 0)
        seen["one"] += p.out_w == 1 or p.out_h == 1
        seen["gap_none"] += gap is None
        seen[filt] += 1
        seen["gray" if got.ndim == 2 else "color"] += 1
        seen["replicate_reduce"] += reduces and p.scale == 8 and layout in ("422", "440")
        seen[layout] += 1
    seen["files"] = len(datas)
    assert seen["refused"] == 0  # no file here is a hundred times taller than wide
    assert seen["files"] >= 300 and sum(seen[k] for k in ("bilinear", "bicubic")) >= 300
    low = {k: v for k, v in seen.items() if k != "refused" and v < (3 if k in ("one", "hit") else 8)}
    assert not low, seen
