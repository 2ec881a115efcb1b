"""The lossless transcode at scale and at its limits (gather_blocks of jg_encode.hip, jpeggpu_ext_transcode_batch): sources
of tens to a thousand 256-block tiles of both kinds -- a symbol stream over many sectors and symbol tiles, coefficient
arrays -- against Pillow's files and the pins of tests/golden/transcode_large_pins.json; progressive sources with scan
scripts Pillow cannot write against tests/transcode_ref.py; a decode that ran its IDCT stage in front of the transcode;
hundreds of items in one call and more calls in flight than the staging ring holds; and the coding limits on both
branches of the gather, value by value. Every output slot lies between guard bytes (transcode_guarded)."""
import functools
import hashlib

import numpy as np
import pytest

import jpeggpu_amd
from jpeggpu_amd import JpegGpuError, Status
from tests import transcode_cases as T
from tests import transcode_ref as R
from tests.test_gpu_transcode import DEV, GUARD, G, transcode_guarded

pytestmark = pytest.mark.gpu

CASES = T.cases()
KINDS = (dict(), dict(optimize=True), dict(progressive=True))
OPTION_SETS = KINDS + (dict(restart_interval=2),)


@pytest.fixture(scope="module")
def torch(gpu_lib):
    import torch

    assert torch.cuda.is_available()
    return torch


@functools.lru_cache(maxsize=None)
def _restated(data, optimize=False, progressive=False, restart_interval=None):
    """tests/transcode_ref.transcode, computed once per (file, options) for all the tests here."""
    return R.transcode(data, optimize=optimize, progressive=progressive, restart_interval=restart_interval)


def _large_expected(source, label, expected):
    """What a pair of T.LARGE_PAIRS is to give: (size, SHA-256), of Pillow's file or from the pins."""
    if expected is not None:
        data = T.large()[expected]
        return len(data), hashlib.sha256(data).hexdigest()
    pin = T.large_pins()[0]["%s/%s" % (source, label)]
    return pin["size"], pin["sha256"]


def _check_large(pairs, got, sizes, status):
    assert status == [0] * len(pairs), status
    for (source, label, _, expected), g, size in zip(pairs, got, sizes):
        assert (size, hashlib.sha256(g).hexdigest()) == _large_expected(source, label, expected), (source, label)


def _pairs(*sources):
    return [p for p in T.LARGE_PAIRS if p[0] in sources]


def _one_call_per_pair(torch, pairs):
    files = T.large()
    for pair in pairs:
        got, sizes, status = transcode_guarded(torch, [files[pair[0]]], **pair[2])
        _check_large([pair], got, sizes, status)


@pytest.mark.parametrize("name", ["photo", "photo_rst"])
def test_large_photos_from_both_source_kinds(torch, name):
    """The progressive file to optimize=True is Pillow's twin and the twin to progressive=True Pillow's progressive file;
    both to plain and to a restart interval of one MCU row are the pins. 72 and 18 tiles; the twin's symbol stream runs over
    several symbol tiles and its units over sector boundaries (tests/test_transcode_ref.py)."""
    pairs = _pairs(name, name + "_twin")
    assert len(pairs) == 6
    _one_call_per_pair(torch, pairs)


@pytest.mark.parametrize("name", ["eob_cap", "eob_ladder"])
def test_large_eob_files(torch, name):
    """129 tiles of coefficient arrays, to plain and to progressive: the encoder's EOBRUN cap of 32 767 behind a gather."""
    pairs = _pairs(name)
    assert [p[1] for p in pairs] == ["plain", "progressive"]
    _one_call_per_pair(torch, pairs)


@pytest.mark.parametrize("label", ["optimize", "progressive"])
def test_large_camera_file(torch, label):
    """1 117 tiles from one symbol stream of 252-MCU restart segments, the target with the source's own interval."""
    pairs = [p for p in _pairs("camera") if p[1] == label]
    assert len(pairs) == 1 and "restart_interval" not in pairs[0][2]
    _one_call_per_pair(torch, pairs)


def test_all_large_sources_in_one_call(torch):
    """The five large sources (the photos from their baseline twins as well) in one call that mixes the output kinds and the
    restart intervals; the odd items in slots of exactly the expected length."""
    files = T.large()
    pairs = [p for p in T.LARGE_PAIRS if (p[0], p[1]) in (("photo", "optimize"), ("photo_twin", "row"), ("photo_rst", "plain"), ("photo_rst_twin", "progressive"),
                                                         ("eob_cap", "progressive"), ("eob_ladder", "plain"), ("camera", "progressive"))]
    assert len(pairs) == 7
    datas = [files[p[0]] for p in pairs]
    caps = [_large_expected(p[0], p[1], p[3])[0] if i % 2 else 2 * len(d) + 2048 for i, (p, d) in enumerate(zip(pairs, datas))]
    got, sizes, status = transcode_guarded(torch, datas, caps, optimize=[bool(p[2].get("optimize")) for p in pairs],
                                           progressive=[bool(p[2].get("progressive")) for p in pairs], restart_interval=[p[2].get("restart_interval") for p in pairs])
    _check_large(pairs, got, sizes, status)


@pytest.mark.parametrize("options", OPTION_SETS, ids=["plain", "optimize", "progressive", "restart 2"])
def test_crafted_progressive_sources(torch, options):
    """Non-interleaved DC scans (dummy blocks no scan codes, through the arrays' row length), bands of one coefficient, three
    refinement levels, 64 scans, 14 DC levels, restart intervals inside progressive scans, coefficients never fully refined."""
    crafted = T.crafted_progressive()
    names = [n for n in crafted if n != T.CRAFTED_REFUSED]
    assert len(names) == 14
    got, _, status = transcode_guarded(torch, [crafted[n][0] for n in names], **options)
    assert status == [0] * len(names)
    for n, g in zip(names, got):
        assert g == _restated(crafted[n][0], **options), (n, options)
    with pytest.raises(JpegGpuError) as e:  # four components: refused on the host, before anything is enqueued
        jpeggpu_amd.transcode_jpeg([crafted[names[0]][0], crafted[T.CRAFTED_REFUSED][0]], **options)
    assert e.value.status == Status.NOT_SUPPORTED and "item 1" in str(e.value)


def _slots(torch, capacities):
    """One guarded buffer with a slot per capacity: (buffer, offsets)."""
    offsets, total = [], G
    for cap in capacities:
        offsets.append(total)
        total += cap + G
    return torch.full((total,), GUARD, dtype=torch.uint8, device=DEV), offsets


def _read_slots(buf, offsets, sizes, status):
    """The files of a guarded buffer once the stream is done; asserts that nothing outside them was written."""
    host = buf.cpu().numpy()
    sizes, status = sizes.cpu().tolist(), status.cpu().tolist()
    untouched = np.ones(len(host), bool)
    files = []
    for o, size, st in zip(offsets, sizes, status):
        if st == 0:
            untouched[o:o + size] = False
        files.append(host[o:o + size].tobytes() if st == 0 else None)
    assert (host[untouched] == GUARD).all(), "bytes outside the files were written"
    return files, sizes, status


def _into_slots(torch, bd, capacities, **options):
    buf, offsets = _slots(torch, capacities)
    sizes, status = jpeggpu_amd.transcode_into(bd, [buf[o:o + cap] for o, cap in zip(offsets, capacities)], **options)
    return buf, offsets, sizes, status


def _twelve_sources():
    files, crafted, large = T.pins()[0], T.crafted_progressive(), T.large()
    return [files["136x120_420_q75_r0_smooth"]["A"], files["33x17_422_qtab_r0_noise"]["B"], files["136x120_grey_q75_r0_smooth"]["A"], large["photo_rst_twin"],
            files["136x120_420_q75_r0_smooth"]["C"], files["17x13_420_q100_r1_noise"]["C"], files["33x17_grey_q100_r3_noise"]["C"], large["photo"],
            crafted["plain_420"][0], crafted["three_refinements_rst"][0], crafted["early_stop_420"][0], crafted["sixty_four_scans"][0]]


def test_decoded_without_coefficients_only(torch):
    """jpeggpu_ext.h: the decode may have run "with jpeggpu_ext_batch_set_coefficients_only or without". A plain batched decode
    -- planes allocated, the IDCT stage run -- leaves the symbol streams and the progressive sources' coefficient arrays as a
    transcode needs them: the same bytes as by the coefficients-only route, for the three output kinds; and the planes are
    those of a decode that no transcode followed."""
    datas = _twelve_sources()
    assert len(datas) == 12 and sum(R.parse(d)["progressive"] for d in datas) == 8
    caps = [2 * len(d) + 2048 for d in datas]
    want = [transcode_guarded(torch, datas, **options)[0] for options in KINDS]
    with jpeggpu_amd.BatchDecode(datas, DEV) as bd:
        bd.decode()
        runs = [_into_slots(torch, bd, caps, **options) for options in KINDS]
        torch.cuda.synchronize(DEV)
        planes = [[p.cpu() for p in item] for item in bd.planes]
        for options, w, run in zip(KINDS, want, runs):
            got, _, status = _read_slots(*run)
            assert status == [0] * 12, options
            assert [i for i in range(12) if got[i] != w[i]] == [], options
    assert want[1][3] == T.large()["photo_rst_twin"] and want[2][3] == T.large()["photo_rst"]  # (the routes agree on the RIGHT bytes)
    with jpeggpu_amd.BatchDecode(datas, DEV) as fresh:
        fresh.decode()
        torch.cuda.synchronize(DEV)
        for i, (a, b) in enumerate(zip(planes, fresh.planes)):
            assert len(a) == len(b) > 0 and all(bool((x == y.cpu()).all()) for x, y in zip(a, b)), i
    assert all(int(p.max()) > int(p.min()) for p in planes[7])  # (the photo's planes hold a picture)


@pytest.mark.parametrize("reverse", [False, True], ids=["in order", "reversed"])
def test_many_items_in_one_call(torch, reverse):
    """All 40 cases x 8 directions, 320 items in one call: every file is its pin; the odd items have slots of exactly the
    pinned length; three slots are a byte short -- status 1, the size the item needs, the slot as it was."""
    files = T.pins()[0]
    plan = [(c["name"], src, options, want) for src, options, want in T.DIRECTIONS for c in CASES]
    assert len(plan) == 320
    if reverse:
        plan.reverse()
    datas = [files[n][src] for n, src, _, _ in plan]
    need = [len(files[n][want]) for n, _, _, want in plan]
    short = (7, 160, 319)
    caps = [need[i] - 1 if i in short else need[i] if i % 2 else need[i] + 100 + 3 * i for i in range(320)]
    got, sizes, status = transcode_guarded(torch, datas, caps, optimize=[bool(o.get("optimize")) for _, _, o, _ in plan],
                                           progressive=[bool(o.get("progressive")) for _, _, o, _ in plan])
    assert status == [int(i in short) for i in range(320)] and sizes == need
    assert [plan[i][:2] for i in range(320) if i not in short and got[i] != files[plan[i][0]][plan[i][3]]] == []


def test_more_calls_in_flight_than_the_staging_ring_holds(torch):
    """Nine transcode calls queued on one stream behind some tens of milliseconds of other work, over three batched decodes of
    different sources, the output kinds mixed within each call; nothing is read before the one synchronisation. The staging
    ring has four buffers: the fifth call and those behind it reuse one, with their own GatherSrc blobs and shadow items."""
    files = T.pins()[0]
    groups = [[c["name"] for c in CASES[k::3]] for k in range(3)]
    kinds = "ABC"
    ballast = torch.zeros(1 << 26, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize(DEV)
    decodes, runs = [], []
    try:
        for k, names in enumerate(groups):
            decodes.append(jpeggpu_amd.BatchDecode([files[n][kinds[(i + k) % 3]] for i, n in enumerate(names)], DEV, coefficients_only=True))
        for _ in range(200):
            ballast.add_(1.0)
        for bd in decodes:
            bd.decode()
        for call in range(9):
            names = groups[call % 3]
            want = [kinds[(i + call // 3) % 3] for i in range(len(names))]  # another mix of kinds in every call over a decode
            need = [len(files[n][w]) for n, w in zip(names, want)]
            run = _into_slots(torch, decodes[call % 3], need, optimize=[w == "B" for w in want], progressive=[w == "C" for w in want])
            runs.append((names, want, need, run))
        torch.cuda.synchronize(DEV)
        for call, (names, want, need, run) in enumerate(runs):
            got, sizes, status = _read_slots(*run)
            assert status == [0] * len(names) and sizes == need, call
            assert [n for n, w, g in zip(names, want, got) if g != files[n][w]] == [], call
    finally:
        for bd in decodes:
            bd.close()


def test_repeat(torch):
    """Two transcodes from one decode, then the transfers and the decode again and a third: the same bytes each time."""
    datas = [T.large()["photo_rst"], T.large()["photo_rst_twin"], T.crafted_progressive()["single_bands_rst"][0], T.pins()[0]["136x120_420_q1_r3_noise"]["A"]]
    caps = [2 * len(d) + 2048 for d in datas]
    options = dict(optimize=[True, False, False, True], progressive=[False, True, True, False])
    with jpeggpu_amd.BatchDecode(datas, DEV, coefficients_only=True) as bd:
        bd.decode()
        runs = [_into_slots(torch, bd, caps, **options), _into_slots(torch, bd, caps, **options)]
        bd.transfer()
        bd.decode()
        runs.append(_into_slots(torch, bd, caps, **options))
        torch.cuda.synchronize(DEV)
        results = [_read_slots(*run) for run in runs]
    for got, _, status in results:
        assert status == [0] * 4
        assert got == results[0][0]
    first = results[0][0]
    assert first[0] == T.large()["photo_rst_twin"] and first[1] == T.large()["photo_rst"]
    assert first[2] == _restated(datas[2], progressive=True) and first[3] == T.pins()[0]["136x120_420_q1_r3_noise"]["B"]


# ---- the coding limits: |AC| = 1023 and |DC difference| = 2047 are coded, one more is JPEGGPU_EXT_ENCODE_UNCODABLE ----

LIMITS = T.limit_sources()


@pytest.mark.parametrize("options", KINDS, ids=["plain", "optimize", "progressive"])
@pytest.mark.parametrize("route", ["baseline", "progressive"])
def test_coding_limits(torch, route, options):
    """Every source of limit_sources() of one route -- the symbol-stream branch or the coefficient-array branch of the gather
    -- in ONE call: the codable ones are the restatement's bytes, the others status 4 with size 0 and an untouched slot (the
    guard check of transcode_guarded covers a slot whose status is not 0), whatever their neighbours in the call are. A
    progressive target's first DC scan codes the differences shifted down by one, and 2048 would fit its code: the contract
    of jpeggpu_ext.h ("a DC difference of category above 11") refuses it all the same, and so does the kernel."""
    sources = [s for s in LIMITS if s["route"] == route]
    assert len(sources) == len(LIMITS) // 2 == 38
    for r in (0, 1):
        some = [s for s in sources if r in s["codable"]]
        got, sizes, status = transcode_guarded(torch, [s["data"] for s in some], restart_interval=r, **options)
        print([(s["name"], st, size) for s, st, size in zip(some, status, sizes)])
        assert [s["name"] for s, st in zip(some, status) if st != (0 if s["codable"][r] else 4)] == [], (r, status)
        for s, g, size in zip(some, got, sizes):
            if s["codable"][r]:
                assert g == _restated(s["data"], restart_interval=r, **options), (s["name"], r)
            else:
                assert size == 0 and g is None, (s["name"], r)
        assert 0 in status and (r == 1 or 4 in status)


def test_restart_dependence_in_one_call(torch):
    """The same source twice in one call, with an interval of 0 and of 1: uncodable and codable side by side."""
    for s in (s for s in LIMITS if s["name"].startswith("dc_restart_pair")):
        for options in KINDS:
            got, sizes, status = transcode_guarded(torch, [s["data"]] * 4, restart_interval=[0, 1, 0, 1], **options)
            assert status == [4, 0, 4, 0] and sizes[0] == sizes[2] == 0, (s["name"], options)
            assert got[1] == got[3] == _restated(s["data"], restart_interval=1, **options), (s["name"], options)
            with pytest.raises(JpegGpuError, match="item 0"):
                jpeggpu_amd.transcode_jpeg([s["data"]], restart_interval=0, **options)
