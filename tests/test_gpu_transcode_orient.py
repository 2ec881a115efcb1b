"""The oriented transcode on the device (jpeggpu_ext_set_transcode_orientation; gather_blocks<true> of jg_encode.hip): every
pinned Pillow file of a transposed image, a sweep of source kinds, layouts, restart intervals, sizes and orientations
against tests/transcode_orient_ref.transform, the DC limit in the target's prediction order, the Python layer and a round
trip on the device. Every output slot lies between guard bytes (transcode_guarded of tests/test_gpu_transcode.py)."""
import numpy as np
import pytest

import jpeggpu_amd
from jpeggpu_amd import JpegGpuError
from oracle import oracle
from tests import encode_ref as E
from tests import exif_ref
from tests import progressive_ref as P
from tests import transcode_cases as T
from tests import transcode_orient_cases as K
from tests import transcode_orient_ref as X
from tests import transcode_ref as R
from tests.test_gpu_transcode import torch, transcode_guarded  # noqa: F401 (torch is a fixture)

pytestmark = pytest.mark.gpu

KIND_OPTIONS = [dict(), dict(optimize=True), dict(progressive=True)]


def run(torch, plan):
    """plan: (source, orientation, trim, options) per item, in ONE call. Returns (files, sizes, status)."""
    return transcode_guarded(
        torch, [p[0] for p in plan], orientation=[p[1] for p in plan], trim=[p[2] for p in plan], optimize=[bool(p[3].get("optimize")) for p in plan],
        progressive=[bool(p[3].get("progressive")) for p in plan], restart_interval=[p[3].get("restart_interval") for p in plan])


def test_every_pin(torch):
    """Every pinned source at every orientation the rules allow, without and with trim, in three calls that give each item
    another output kind each time: Pillow's file of the transposed pixels, byte for byte. Items of orientation 1 lie between
    the oriented ones."""
    sources = K.pins()[0]
    items = [(c, o, trim) for c in K.pin_cases() for o in range(1, 9) for trim in (False, True) if K.allowed(c, o, trim) is not None]
    assert len(items) > 350 and sum(o == 1 for _, o, _ in items) == 2 * len(sources)
    for shift in range(3):
        kinds = ["ABC"[(i + shift) % 3] for i in range(len(items))]
        got, _, status = run(torch, [(sources[c["name"]], o, trim, K.KINDS[k]) for (c, o, trim), k in zip(items, kinds)])
        assert status == [0] * len(items)
        wrong = [(c["name"], o, trim, k) for (c, o, trim), k, g in zip(items, kinds, got) if g != K.expected(c["name"], o, trim, k)]
        assert not wrong, wrong[:10]


def _sweep_source(kind, sampling, w, h, content, seed, restart):
    """One source of the sweep: the quantised coefficients of a seeded image, written the way `kind` says."""
    grey = sampling == "grey"
    img = K.sweep_image(w, h, grey, content, seed)
    a = E.encode(img, [35, 80, 92][seed % 3], "4:4:4" if grey else sampling, restart)
    if kind == "interleaved":
        return a
    grids = [np.asarray(g) for g in oracle.decode(a).coef]
    factors = [(1, 1)] if grey else [K.FACTORS[sampling], (1, 1), (1, 1)]
    nc = len(factors)
    if kind == "own_scans":  # unit quantisers: the file holds the same coefficients
        from tools import jpegsynth

        return jpegsynth.encode_custom(w, h, factors, grids, [P._flat_table(16, 5)[:2]], [P._flat_table(256, 9)[:2]], tables=[(0, 0)] * nc, interleaved=False,
                                       restart_interval=restart)
    inverse = np.argsort(E.ZIGZAG)
    info = R.parse(a)
    qtabs = {t: np.array(q)[inverse] for t, q in info["qtabs"].items()}
    return P.encode(w, h, factors, qtabs, [0, 1, 1][:nc], grids, P.script_pillow_like(nc), restart=restart)


@pytest.mark.parametrize("sampling", ["grey", "4:4:4", "4:2:0", "4:2:2"])
@pytest.mark.parametrize("kind", K.SOURCE_KINDS)
def test_sweep(torch, kind, sampling):
    """Seeded noise and photograph-like sources of one kind and layout, every size, every orientation the rules allow
    (with trim where the size needs it, and orientation 5 without), the restart intervals 0, 1, one MCU row of the target and
    the source's own, the output kinds in turn: one call, every file equal to the reference's."""
    sizes = K.SWEEP_SIZES + ([K.SWEEP_LARGE] if sampling == "4:2:0" else [])
    hs, vs = K.FACTORS[sampling]
    plan, what = [], []
    n = 0
    for w, h in sizes:
        case = dict(w=w, h=h, sampling=sampling)
        src = {r: _sweep_source(kind, sampling, w, h, ["noise", "photo"][(len(plan) + r) % 2], n + r, r) for r in (0, 2)}
        perfect = all(K.allowed(case, o, False) is not None for o in (2, 4))
        for o in range(1, 9):
            for trim in ((False,) if perfect else (False, True)):
                size = K.allowed(case, o, trim)
                if size is None:
                    continue
                tw = size[1] if o >= 5 else size[0]
                row = -(-tw // (8 * (vs if o >= 5 else hs)))
                for restart in (0, 1, row, None):
                    options = dict(KIND_OPTIONS[n % 3], restart_interval=restart)
                    plan.append((src[2 if restart is None else 0], o, trim, options))
                    what.append((w, h, o, trim, options))
                    n += 1
    assert len(plan) >= (60 if sampling == "4:2:2" else 120)
    got, _, status = run(torch, plan)
    assert status == [0] * len(plan)
    wrong = [w for p, w, g in zip(plan, what, got) if g != X.transform(p[0], p[1], p[2], **p[3])]
    assert not wrong, wrong[:10]


def test_the_large_size_spans_two_tiles():
    assert T.blocks_of(*K.SWEEP_LARGE, "4:2:0") == (336, 2) and T.blocks_of(K.SWEEP_LARGE[1], K.SWEEP_LARGE[0], "4:2:0") == (336, 2)
    assert K.SWEEP_LARGE[0] % 16 == 0 and K.SWEEP_LARGE[1] % 16 == 0 and K.SWEEP_LARGE[0] != K.SWEEP_LARGE[1]


def test_dc_limit_follows_the_target(torch):
    """A crafted source whose DC difference of 2048 lies between neighbours of one block row: uncodable as it stands, codable
    once transposed, where the two are a row apart -- and the other way round for the transposed file. Status 4 and size 0
    for that item only."""
    found = None
    for s in T.limit_sources():
        if s["where"][1] == 0 and s["sampling"] == "grey":
            def codable(o):
                try:
                    return X.transform(s["data"], o, restart_interval=0)
                except X.Unsupported:
                    return None
            if codable(1) is None and codable(5) is not None:
                found = s, codable(5)
                break
    assert found, "no source of limit_sources() is refused at orientation 1 and coded at 5"
    s, turned = found
    twin = next(t for t in T.limit_sources() if t["name"] == s["name"].rsplit("_", 1)[0] + "_progressive")  # the coefficient-array branch
    assert s["route"] == "baseline" and (R.coefficients(twin["data"])["coefs"] == R.coefficients(s["data"])["coefs"]).all()
    good = K.pins()[0]["32x32_grey_q100"]
    for options in KIND_OPTIONS:
        options = dict(options, restart_interval=0)
        for data in (s["data"], twin["data"]):
            got, sizes, status = run(torch, [(good, 6, False, options), (data, 1, False, options), (data, 5, False, options), (good, 1, False, options)])
            assert status == [0, 4, 0, 0] and sizes[1] == 0, (s["name"], options)
            assert got[2] == X.transform(data, 5, **options) and got[0] == X.transform(good, 6, **options) and got[3] == R.transcode(good, **options)
    # the transposed file holds the pair a row apart; transposing it back brings them together again
    with pytest.raises(X.Unsupported):
        X.transform(turned, 5, restart_interval=0)
    got, sizes, status = run(torch, [(turned, 5, False, dict(restart_interval=0)), (turned, 1, False, dict(restart_interval=0))])
    assert status == [4, 0] and sizes[0] == 0 and got[1] == R.transcode(turned, restart_interval=0)


def test_python_layer():
    """exif_transpose=True on files that carry the tags 1..8 is orientation= with the same numbers; no Exif segment is left;
    an imperfect file raises JpegGpuError naming the item before anything is enqueued; naming both is a ValueError."""
    sources = K.pins()[0]
    base = [sources["48x32_420_q100"], sources["32x32_grey_q100"], sources["64x48_444_q100"], sources["16x64_420_q100"]]
    tagged = [exif_ref.with_orientation(base[o % len(base)], o) for o in range(1, 9)]
    assert all(b"Exif\0\0" in t for t in tagged)
    plain = [base[o % len(base)] for o in range(1, 9)]
    for options in KIND_OPTIONS:
        got = jpeggpu_amd.transcode_jpeg(tagged, exif_transpose=True, **options)
        assert got == jpeggpu_amd.transcode_jpeg(plain, orientation=list(range(1, 9)), **options)
        assert got == [X.transform(p, o, **options) for p, o in zip(plain, range(1, 9))]
        assert not any(b"Exif" in g for g in got)
    assert jpeggpu_amd.transcode_jpeg(tagged[5:6])[0] == R.transcode(plain[5])  # the tag alone changes nothing
    mixed = jpeggpu_amd.transcode_jpeg(tagged[:3], orientation=[None, None, 4], exif_transpose=[True, False, False])
    assert mixed == [X.transform(plain[0], 1), R.transcode(plain[1]), X.transform(plain[2], 4)]
    imperfect = sources["35x21_444_q100"]
    with pytest.raises(JpegGpuError, match="item 1"):
        jpeggpu_amd.transcode_jpeg([base[0], imperfect, base[1]], orientation=3)
    assert jpeggpu_amd.transcode_jpeg([base[0], imperfect, base[1]], orientation=3, trim=True)[1] == K.expected("35x21_444_q100", 3, True, "A")
    with pytest.raises(JpegGpuError, match="item 0"):
        jpeggpu_amd.transcode_jpeg([sources["32x32_422_q100"]], orientation=6)
    with pytest.raises(ValueError):
        jpeggpu_amd.transcode_jpeg(tagged[:2], orientation=[None, 2], exif_transpose=True)
    buf, offsets, sizes = jpeggpu_amd.transcode_jpeg_to_device([imperfect], orientation=5, progressive=True)
    assert buf[offsets[0]:offsets[0] + sizes[0]].cpu().numpy().tobytes() == K.expected("35x21_444_q100", 5, False, "C")


def test_round_trip_on_the_device():
    """The output of o fed back with the inverse orientation is the plain transcode of the source; the decoders' setting does
    not leak into a later call on other decoders."""
    sources = K.pins()[0]
    noise = [_sweep_source(kind, "4:2:0", 48, 32, "noise", 3 + i, i) for i, kind in enumerate(K.SOURCE_KINDS)]
    datas = [sources["64x48_420_q100"], sources["48x32_420_sym"]] + noise + [_sweep_source("interleaved", "grey", 32, 48, "photo", 9, 0)]
    for o in range(1, 9):
        there = jpeggpu_amd.transcode_jpeg(datas, orientation=o, progressive=[i % 2 == 0 for i in range(len(datas))], restart_interval=0)
        back = jpeggpu_amd.transcode_jpeg(there, orientation=X.INVERSE[o], restart_interval=0)
        assert back == jpeggpu_amd.transcode_jpeg(datas, restart_interval=0) == [R.transcode(d, restart_interval=0) for d in datas], o
        if o != 1:
            assert all(t != b for t, b in zip(there, back))
