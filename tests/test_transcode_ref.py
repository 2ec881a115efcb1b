"""tests/transcode_ref.py against Pillow: every direction of a transcode on every pinned source
(tests/golden/transcode_pins.npz) gives, byte for byte, the file Pillow wrote for the same pixels with the other options; and
the same on a seeded sweep of other sizes against the Pillow at hand, where there is one."""
import hashlib
import io
import json

import numpy as np
import pytest

from tests import progressive_ref as P
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


def _hashed(data):
    return dict(size=len(data), sha256=hashlib.sha256(data).hexdigest())


def test_large_sources_are_what_they_are_there_for():
    files = T.large()
    want = {"photo": (1024, 768, "4:2:0", 0, 18432, 72), "photo_rst": (512, 384, "4:2:0", 1, 4608, 18), "eob_cap": (1456, 1448, "grey", 0, 32942, 129),
            "eob_ladder": (1456, 1448, "grey", 0, 32942, 129), "camera": (4032, 3024, "4:2:0", 252, 285768, 1117)}
    for name, (w, h, sampling, restart, blocks, tiles) in want.items():
        for src in (name, name + "_twin") if name + "_twin" in files else (name,):
            info = R._checked(files[src])
            assert (info["w"], info["h"], info["restart"]) == (w, h, restart), src
            assert ("grey" if len(info["comps"]) == 1 else info["subsampling"]) == sampling, src
            assert info["progressive"] == (src != "camera" and not src.endswith("_twin")), src
        assert T.blocks_of(w, h, sampling) == (blocks, tiles), name
    assert b"Exif\0\0" in files["camera"][:64]
    assert T.LARGE_ROW == {"photo": T.mcus_x(dict(w=1024, sampling="4:2:0")), "photo_rst": T.mcus_x(dict(w=512, sampling="4:2:0"))}
    # a data unit's entries are its DC and its non-zero AC coefficients, 16 entries to a sector of the symbol stream: a unit
    # with 16 non-zero AC coefficients lies in two sectors wherever it begins -- sym_advance's stride -- and one with 32 in three
    for src, sectors in (("photo_twin", 3), ("photo_rst_twin", 3)):
        nonzero = (R.coefficients(files[src])["coefs"][:, 1:] != 0).sum(1)
        assert nonzero.max() >= 16 * (sectors - 1), (src, int(nonzero.max()))
        assert (nonzero >= 16).sum() > 100, src


def test_photos_and_their_twins():
    """Pillow's progressive file and its optimised baseline twin hold the same coefficients: each is the other's transcode."""
    files = T.large()
    for name in ("photo", "photo_rst"):
        assert R.transcode(files[name], optimize=True) == files[name + "_twin"], name
        assert R.transcode(files[name + "_twin"], progressive=True) == files[name], name


def test_large_pins():
    """tests/golden/transcode_large_pins.json, recomputed: the EOB files' entries and the photos' from their baseline twins
    (the progressive photos' entries are the same pins, and test_photos_and_their_twins says they hold the same coefficients).
    The camera file's two entries are recomputed only by tools/make_transcode_large_pins.py: the restatement takes half a
    minute over them. The pins are the restatement's output, not Pillow's."""
    files = T.large()
    pins, _ = T.large_pins()
    assert sorted(pins) == sorted("%s/%s" % (s, label) for s, label, _, expected in T.LARGE_PAIRS if expected is None)
    for source, label, options, expected in T.LARGE_PAIRS:
        if expected is None and source not in ("camera", "photo", "photo_rst"):
            assert _hashed(R.transcode(files[source], **options)) == pins["%s/%s" % (source, label)], (source, label)
    for name in ("photo", "photo_rst"):
        for label in ("plain", "row"):
            assert pins["%s/%s" % (name, label)] == pins["%s_twin/%s" % (name, label)]
    with open(T.LARGE_PINS) as f:
        assert json.load(f)["sources"] == {k: _hashed(v) for k, v in files.items()}  # the camera's pins are of THIS file


OPTION_SETS = (dict(), dict(optimize=True), dict(progressive=True), dict(restart_interval=2))


def test_crafted_progressive_sources():
    """Every crafted progressive file transcodes (but the four-component one). Those that hold their baseline source's
    coefficients give the bytes that source gives; the others differ from it, and where they differ is what the case is
    there for: dummy blocks no scan of the progressive file codes, bits and a band its script never sends."""
    crafted = T.crafted_progressive()
    assert set(T.CRAFTED_EQUAL) < set(crafted) and T.CRAFTED_REFUSED in crafted and len(crafted) == 15
    with pytest.raises(R.Unsupported):
        R.transcode(crafted[T.CRAFTED_REFUSED][0])
    seen = dict(dummy=0, unrefined=0, chroma_ac=0)
    for name, (prog, base) in crafted.items():
        if name == T.CRAFTED_REFUSED:
            continue
        own = R.parse(prog)["restart"]
        a, b = R.coefficients(prog), R.coefficients(base)
        ca, cb = a["coefs"].astype(np.int64), b["coefs"].astype(np.int64)
        real = a["dummy"] == 0
        if name in T.CRAFTED_EQUAL:
            assert (ca == cb).all(), name
            for options in OPTION_SETS:  # (the baseline source has no interval of its own: the target's is named)
                options = dict(dict(restart_interval=own), **options)
                assert R.transcode(prog, **options) == R.transcode(base, **options), (name, options)
            continue
        assert (ca != cb).any(), name
        assert all(R.transcode(prog, **o) for o in OPTION_SETS), name
        assert R.transcode(prog, restart_interval=own) != R.transcode(base, restart_interval=own), name
        if name.startswith("early_stop"):  # Al = 1 is never refined: the DC floors, an AC magnitude truncates; luma's band 41..63 is never coded
            want = np.sign(cb) * (np.abs(cb) >> 1 << 1)
            want[:, 0] = cb[:, 0] >> 1 << 1
            want[a["comp"] == 0, 41:] = 0
            assert (ca[real] == want[real]).all(), name
            seen["unrefined"] += int((cb[real] & 1).any())
        elif name == "sixty_four_scans":  # only component 0 has AC scans
            assert (ca[real & (a["comp"] == 0)] == cb[real & (a["comp"] == 0)]).all() and (ca[real][:, 0] == cb[real][:, 0]).all()
            assert not ca[a["comp"] > 0, 1:].any() and cb[a["comp"] > 0, 1:].any()
            seen["chroma_ac"] += 1
        else:
            assert (ca[real] == cb[real]).all(), name
        if (~real).any():  # a dummy block keeps what an interleaved scan codes of it -- the DC, or nothing -- and is zero beyond
            interleaved_dc = len(P.decode(prog).scans[0]["comps"]) > 1
            assert not ca[~real, 1:].any() and (interleaved_dc or not ca[~real].any()), name
            if interleaved_dc:
                assert (ca[~real, 0] >> 3 == cb[~real, 0] >> 3).all(), name  # (as far down as any script here sends it)
            seen["dummy"] += int((ca[~real] != cb[~real]).any())
    assert seen["dummy"] >= 4 and seen["unrefined"] == 2 and seen["chroma_ac"] == 1, seen


def test_coding_limits():
    """limit_sources(): each file holds the value it is named for at the block it is named for; the restatement refuses
    exactly the uncodable ones, by the TARGET's restart interval; the structural cases have their structure."""
    sources = T.limit_sources()
    by_name = {s["name"]: s for s in sources}
    assert len(by_name) == len(sources) and {s["route"] for s in sources} == {"baseline", "progressive"}
    for s in sources:
        info = R.parse(s["data"])
        assert info["progressive"] == (s["route"] == "progressive") and info["restart"] == 0, s["name"]
        co = R.coefficients(s["data"])
        block, zz, value = s["where"]
        assert int(co["coefs"][block, zz]) == value, s["name"]
        assert len(co["coefs"]) == T.blocks_of(s["w"], s["h"], s["sampling"])[0]
        twin = by_name[s["name"].rsplit("_", 1)[0] + ("_progressive" if s["route"] == "baseline" else "_baseline")]
        assert (R.coefficients(twin["data"])["coefs"] == co["coefs"]).all(), s["name"]  # both routes carry every value
        for r, codable in s["codable"].items():
            if not codable:
                with pytest.raises(R.Unsupported):
                    R.transcode(s["data"], restart_interval=r)
                continue
            for options in ({}, dict(optimize=True), dict(progressive=True)):
                out = R.transcode(s["data"], restart_interval=r, **options)
                assert (R.coefficients(out)["coefs"] == co["coefs"]).all(), (s["name"], r, options)
        if zz:  # an AC case: nothing else in the file is near a limit
            rest = co["coefs"].astype(np.int64).copy()
            rest[block, zz] = 0
            assert np.abs(rest).max() < 64 and np.abs(R.dc_differences(co, 0)).max() < 128
        else:  # a DC case: the named difference is the only one at the limit, and no AC coefficient is
            d = R.dc_differences(co, 0)
            assert abs(int(d[block])) in (2047, 2048) and (np.abs(np.delete(d, block)) < 2047).all(), s["name"]
            assert np.abs(co["coefs"][:, 1:]).max() < 64
    for s in sources:
        n, tiles = T.blocks_of(s["w"], s["h"], s["sampling"])
        if "second_tile" in s["name"]:
            assert tiles == 2 and s["where"][0] >= T.TILE_BLOCKS
        if "chroma" in s["name"]:
            assert R.coefficients(s["data"])["comp"][s["where"][0]] > 0
        if "luma" in s["name"]:
            assert R.coefficients(s["data"])["comp"][s["where"][0]] == 0 and s["sampling"] == "4:2:0"
    for v in T.AC_CODABLE + T.AC_UNCODABLE:
        for zz in (1, 63):
            for route in ("baseline", "progressive"):
                s = by_name["ac_%d_zz%d_%s" % (v, zz, route)]
                assert s["where"] == (2, zz, v) and s["codable"] == {0: abs(v) <= 1023}
    # the DC rule follows the target's interval: the same pair is refused at 0 and coded at 1; a difference across an MCU
    # row's end and one between chroma blocks of neighbouring MCUs are differences like any other
    for name in ("dc_restart_pair", "dc_restart_pair_chroma"):
        for route in ("baseline", "progressive"):
            s = by_name["%s_%s" % (name, route)]
            co = R.coefficients(s["data"])
            assert s["codable"] == {0: False, 1: True}
            assert np.abs(R.dc_differences(co, 0)).max() == 2048 and np.abs(R.dc_differences(co, 1)).max() == 1025
            assert (np.abs(R.dc_differences(co, 2)).max() == 2048) == (name == "dc_restart_pair")  # MCUs 0|1 of one interval, 1|2 of two
    co = R.coefficients(by_name["dc_row_2048_baseline"]["data"])
    assert co["mcus_x"] == 2 and by_name["dc_row_2048_baseline"]["where"][0] == 2
    assert np.abs(R.dc_differences(co, 2)).max() < 2048  # (an interval of one MCU row resets in front of it)


def test_dc_rule_on_the_pins():
    """No pinned file is near the limit, in any prediction order: the rule changes nothing Pillow wrote."""
    files, _ = T.pins()
    for c in CASES:
        co = R.coefficients(files[c["name"]]["A"])
        for r in (0, 1, 3):
            assert np.abs(R.dc_differences(co, r)).max() < 2048
    co = R.coefficients(files["17x13_420_q75_r0_noise"]["A"])  # the differences are the encoder's: per component, reset per interval
    d0, d1 = R.dc_differences(co, 0), R.dc_differences(co, 1)
    dc = co["coefs"][:, 0].astype(np.int64)
    assert (d1[co["comp"] > 0] == dc[co["comp"] > 0]).all() and d0[0] == dc[0] and d0[1] == dc[1] - dc[0]
    assert d0[6] == dc[6] - dc[3] and d1[6] == dc[6] and d1[7] == dc[7] - dc[6] and d0[10] == dc[10] - dc[4]


def test_escapes_are_exercised():
    """Quality 100 on noise and the custom tables reach AC categories of 10: the decoder's escape entries."""
    files, _ = T.pins()
    top = {c["name"]: int(np.abs(R.coefficients(files[c["name"]]["A"])["coefs"][:, 1:]).max()) for c in CASES if c["kind"] == "noise" and c["quality"] in (100, None)}
    assert max(top.values()) >= 512, top
