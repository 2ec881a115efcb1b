"""Encoding to a byte budget on the device (jpeggpu_ext_encode_fit_batch; jg_encode_fit.hip): the chosen quality and the file
against the rule of tests/encode_fit_ref.py over the files the plain encoder writes at every quality, against Pillow's pins
(tests/golden/encode_fit_pins.npz), in calls that mix ranges, budgets, layouts and both kinds of table, with slots that are
too small and without slots, at the arithmetic edges of the stored transform and the device's tables, and behind
thumbnail_jpeg. Every output slot lies between guard bytes."""
import hashlib

import numpy as np
import pytest

import jpeggpu_amd
from jpeggpu_amd import EncodeStatus
from tests import encode_cases as K
from tests import encode_fit_ref as F

pytestmark = pytest.mark.gpu

GUARD, G = 0xA5, 64
DEV = "cuda:0"
CASES = F.cases()
# 300 x 200 noise at 4:4:4: 2 850 blocks in 12 tiles, and a stream of more than one 8 192-byte chunk at high quality -- the
# smallest shape that crosses both the tile and the chunk boundary
BIG = dict(K._case("fit_300x200_noise_rgb_444", 200, 300, False, "noise", 75, "4:4:4", 0, seed=900), optimize=False, lo=1, hi=100)


@pytest.fixture(scope="module")
def torch(gpu_lib):
    import torch

    assert torch.cuda.is_available()
    return torch


def _params(c):
    return dict(subsampling=c["subsampling"], restart_interval=c["restart_interval"], optimize=c["optimize"])


@pytest.fixture(scope="module")
def plain(torch):
    """{case name: (device tensor, {q: the plain encoder's file at quality q})}: ONE encode_jpeg call per image, one item per
    quality. Shared by the tests below and never changed."""
    out = {}
    for c in CASES + [BIG]:
        x = torch.from_numpy(F.image(c)).to(DEV)
        files = jpeggpu_amd.encode_jpeg([x] * 100, quality=list(range(1, 101)), **_params(c))
        out[c["name"]] = (x, dict(zip(range(1, 101), files)))
    return out


def fit_guarded(torch, xs, capacities, budgets, his, los, **params):
    """One jpeggpu_ext_encode_fit_batch call into guarded slots. Returns (files, sizes, status, qualities): files[i] the slot's
    bytes up to its reported size, None where status is not 0. Asserts that nothing outside the files was written."""
    offsets, total = [], G
    for cap in capacities:
        offsets.append(total)
        total += cap + G
    buf = torch.full((total,), GUARD, dtype=torch.uint8, device=DEV)
    sizes, status, qualities = jpeggpu_amd.encode_fit_into(xs, [buf[o:o + cap] for o, cap in zip(offsets, capacities)], budgets, his, los, **params)
    sizes, status, qualities = sizes.cpu().tolist(), status.cpu().tolist(), qualities.cpu().tolist()
    host = buf.cpu().numpy()
    untouched = np.ones(total, bool)
    files = []
    for o, cap, size, st in zip(offsets, capacities, sizes, status):
        if st == 0:
            assert size <= cap
            untouched[o:o + size] = False
        files.append(host[o:o + size].tobytes() if st == 0 else None)
    assert (host[untouched] == GUARD).all(), "bytes outside the files were written"
    return files, sizes, status, qualities


def _expect(files, lo, hi, budget):
    """(quality, file or None, size, status) by the rule over the plain encoder's files."""
    q = F.choose(lambda v: len(files[v]), lo, hi, budget)
    if q is None:
        return lo, None, len(files[lo]), EncodeStatus.OVER_BUDGET
    return q, files[q], len(files[q]), EncodeStatus.OK


@pytest.mark.parametrize("case", CASES + [BIG], ids=lambda c: c["name"])
def test_fit_equals_the_rule_over_the_plain_encoder(torch, plain, case):
    """Per image ONE fit call, one item per budget: size(hi), a byte less, size(lo), a byte less (over budget), the median
    and every dip of the image's own table."""
    x, files = plain[case["name"]]
    table = {q: len(f) for q, f in files.items()}
    lo, hi = case["lo"], case["hi"]
    budgets = F.budgets(table, lo, hi)
    assert len(budgets) >= 2
    n = len(budgets)
    cap = max(table.values())
    got, sizes, status, qualities = fit_guarded(torch, [x] * n, [cap] * n, budgets, hi, lo, **_params(case))
    seen = set()
    for i, b in enumerate(budgets):
        q, want, size, st = _expect(files, lo, hi, b)
        assert (qualities[i], sizes[i], status[i]) == (q, size, st), (case["name"], b, qualities[i], sizes[i], status[i])
        assert got[i] == want, (case["name"], b, q)
        seen.add(st)
    assert seen == {EncodeStatus.OK, EncodeStatus.OVER_BUDGET}
    if case is BIG:
        assert K.counts(case)["tiles"] == 12 and max(table.values()) > K.CHUNK_BYTES


def test_fit_equals_the_pins(torch, plain):
    """Quality, length and hash (the bytes, where stored) of every pinned case and budget, in one call of all of them."""
    pins = F.pins()[0]
    xs, caps, budgets, his, los, params, want = [], [], [], [], [], dict(subsampling=[], restart_interval=[], optimize=[]), []
    for c in CASES:
        for e in pins[c["name"]]["budgets"]:
            xs.append(plain[c["name"]][0])
            caps.append(max(pins[c["name"]]["table"].values()))
            budgets.append(e["budget"]), his.append(c["hi"]), los.append(c["lo"])
            for k in params:
                params[k].append(c[k])
            want.append((c, e))
    got, sizes, status, qualities = fit_guarded(torch, xs, caps, budgets, his, los, **params)
    for i, (c, e) in enumerate(want):
        if e["quality"] < 0:
            assert (status[i], qualities[i], sizes[i], got[i]) == (EncodeStatus.OVER_BUDGET, c["lo"], e["length"], None), (c["name"], e)
            continue
        assert (status[i], qualities[i], sizes[i]) == (EncodeStatus.OK, e["quality"], e["length"]), (c["name"], e, qualities[i], sizes[i])
        assert hashlib.sha256(got[i]).hexdigest() == e["sha256"] and F.equals_pin(c["name"], e, got[i]), (c["name"], e)


def _mixed(torch, plain):
    """Items of one call: ranges of 1, 2 and 100 qualities, different budgets, grey and RGB, both kinds of table, a CHW view
    and a row-padded view. Each: (tensor, layout-free files table, case, lo, hi, budget)."""
    by = {c["name"]: c for c in CASES + [BIG]}
    pick = lambda **kw: next(c for c in CASES if all(c[k] == v for k, v in kw.items()))  # noqa: E731
    a = pick(w=120, h=80, grey=False, optimize=False)
    b = pick(w=37, h=39, grey=False, optimize=True)
    g = pick(w=59, h=24, grey=True)
    g2 = next(c for c in CASES if c["grey"] and c["optimize"] != g["optimize"])
    s = pick(w=1, h=1, grey=False)
    items = []
    for c, lo, hi, where in ((a, 1, 100, 0.5), (b, 1, 100, 0.3), (g, 50, 50, 2.0), (g2, 40, 41, 0.999), (s, 1, 100, 0.9), (BIG, 1, 100, 0.4), (a, 30, 31, 0.1),
                             (b, 75, 75, 0.5), (g, 1, 100, 0.6), (BIG, 90, 90, 1.0)):
        files = plain[c["name"]][1]
        items.append([plain[c["name"]][0], files, by[c["name"]], lo, hi, int(len(files[hi]) * where)])
    # the same pixels through other strides: a CHW tensor seen as HWC, and rows inside a wider allocation
    x = plain[a["name"]][0]
    items[0][0] = x.permute(2, 0, 1).contiguous().permute(1, 2, 0)
    wide = torch.full((a["h"], a["w"] + 13, 3), 77, dtype=torch.uint8, device=DEV)
    wide[:, :a["w"]] = x
    items[6][0] = wide[:, :a["w"]]
    assert not items[0][0].is_contiguous() and not items[6][0].is_contiguous()
    return items


def _run_mixed(torch, items, capacities=None):
    caps = capacities or [max(len(f) for f in it[1].values()) for it in items]
    return fit_guarded(torch, [it[0] for it in items], caps, [it[5] for it in items], [it[4] for it in items], [it[3] for it in items],
                       subsampling=[it[2]["subsampling"] for it in items], restart_interval=[it[2]["restart_interval"] for it in items],
                       optimize=[it[2]["optimize"] for it in items])


def test_mixed_call_and_its_reverse(torch, plain):
    items = _mixed(torch, plain)
    assert {it[4] - it[3] + 1 for it in items} == {1, 2, 100} and {it[2]["grey"] for it in items} == {False, True}
    assert {it[2]["optimize"] for it in items} == {False, True}
    forward = _run_mixed(torch, items)
    backward = _run_mixed(torch, items[::-1])
    statuses = set()
    for i, it in enumerate(items):
        q, want, size, st = _expect(it[1], it[3], it[4], it[5])
        for files, sizes, status, qualities, k in (forward + (i,), backward + (len(items) - 1 - i,)):
            assert (qualities[k], sizes[k], status[k]) == (q, size, st), (i, it[2]["name"], it[3:], qualities[k], sizes[k], status[k])
            assert files[k] == want, (i, it[2]["name"])
        statuses.add(st)
    assert statuses == {EncodeStatus.OK, EncodeStatus.OVER_BUDGET}


def test_a_slot_that_is_too_small_reports_what_it_needs(torch, plain):
    items = _mixed(torch, plain)
    files, sizes, status, qualities = _run_mixed(torch, items)
    short = next(i for i, st in enumerate(status) if st == 0 and sizes[i] > 100)
    caps = [max(len(f) for f in it[1].values()) for it in items]
    caps[short] = sizes[short] - 1
    files2, sizes2, status2, qualities2 = _run_mixed(torch, items, caps)  # (fit_guarded: the short slot kept its pattern)
    assert status2[short] == EncodeStatus.TOO_SMALL and sizes2[short] == sizes[short] and qualities2[short] == qualities[short] and files2[short] is None
    for i in range(len(items)):
        if i != short:
            assert (files2[i], sizes2[i], status2[i], qualities2[i]) == (files[i], sizes[i], status[i], qualities[i]), i


def test_size_only_call(torch, plain):
    """out NULL with capacity 0: the same qualities and sizes as the writing call, status TOO_SMALL where a file would be."""
    items = _mixed(torch, plain)
    files, sizes, status, qualities = _run_mixed(torch, items)
    s, st, q = jpeggpu_amd.encode_fit_into([it[0] for it in items], [None] * len(items), [it[5] for it in items], [it[4] for it in items],
                                           [it[3] for it in items], subsampling=[it[2]["subsampling"] for it in items],
                                           restart_interval=[it[2]["restart_interval"] for it in items], optimize=[it[2]["optimize"] for it in items])
    assert s.cpu().tolist() == sizes and q.cpu().tolist() == qualities
    assert st.cpu().tolist() == [EncodeStatus.TOO_SMALL if v == 0 else v for v in status]


def _edge_images():
    seen, out = set(), []
    for c in K.edge_cases():
        key = (c["content"], c["grey"], c["subsampling"], c["restart_interval"])
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


def test_arithmetic_edges(torch):
    """The basis-pattern and colour-lattice images at quality_min = quality_max in {1, 50, 100} equal plain encode_jpeg: every
    coefficient at its largest value of either sign through the int16 store, and the device's tables at both ends of the
    clamp. The first evaluation of a search uses the tables the host wrote; ranges of two qualities make the device derive them."""
    cases = _edge_images()
    assert {c["content"] for c in cases} == {"basis", "lattice"} and any(c["grey"] for c in cases)
    for c in cases:
        x = torch.from_numpy(K.image(c)).to(DEV)
        params = dict(subsampling=c["subsampling"], restart_interval=c["restart_interval"])
        want = jpeggpu_amd.encode_jpeg([x] * 3, quality=[1, 50, 100], **params)
        got, qualities = jpeggpu_amd.encode_jpeg_fit([x] * 3, 1 << 30, quality=[1, 50, 100], min_quality=[1, 50, 100], **params)
        assert qualities == [1, 50, 100] and got == want, c["name"]
        # tables the DEVICE derives, at both ends of jpeg_set_quality's range and around its change of formula at 50: the
        # search starts at the top of a range of eleven qualities, and the budget is the file at the bottom, or the median one
        ranges = [(1, 11), (45, 55), (90, 100)]
        qs = [q for lo, hi in ranges for q in range(lo, hi + 1)]
        files = dict(zip(qs, jpeggpu_amd.encode_jpeg([x] * len(qs), quality=qs, **params)))
        budgets = [b for lo, hi in ranges for b in (len(files[lo]), sorted(len(files[q]) for q in range(lo, hi + 1))[5])]
        got, qualities = jpeggpu_amd.encode_jpeg_fit([x] * 6, budgets, quality=[hi for _, hi in ranges for _ in (0, 1)],
                                                      min_quality=[lo for lo, _ in ranges for _ in (0, 1)], **params)
        for i, b in enumerate(budgets):
            lo, hi = ranges[i // 2]
            q, want_file, _, st = _expect(files, lo, hi, b)
            assert st == EncodeStatus.OK and (qualities[i], got[i]) == (q, want_file), (c["name"], lo, hi, b, qualities[i])
        if c["content"] == "basis":
            assert qualities[0] < 11 and qualities[2] < 55 and qualities[4] < 100, "the chosen files were made with the device's tables"


def test_over_budget_raises_unless_not_strict(torch, plain):
    c = CASES[3]
    x, files = plain[c["name"]]
    with pytest.raises(jpeggpu_amd.JpegGpuError, match="image 1"):
        jpeggpu_amd.encode_jpeg_fit([x, x], [1 << 20, len(files[1]) - 1], **_params(c))
    got, qualities = jpeggpu_amd.encode_jpeg_fit([x, x], [1 << 20, len(files[5]) - 1], quality=90, min_quality=5, strict=False, **_params(c))
    assert got == [files[90], None] and qualities == [90, 5]


def test_thumbnail_jpeg_with_a_budget(torch, plain):
    """thumbnail_jpeg(..., max_bytes=) equals decode_thumbnails followed by encode_jpeg_fit, on a colour and a grey source."""
    colour = next(c for c in CASES if (c["w"], c["h"]) == (120, 80) and not c["grey"] and not c["optimize"])
    grey = next(c for c in CASES if (c["w"], c["h"]) == (120, 80) and c["grey"])
    datas = [plain[colour["name"]][1][90], plain[grey["name"]][1][90]]
    views = jpeggpu_amd.decode_thumbnails(datas, (48, 48))
    subsampling = ["4:4:4" if v.dim() == 2 else "4:2:0" for v in views]
    full = jpeggpu_amd.encode_jpeg(views, quality=85, subsampling=subsampling)
    least = jpeggpu_amd.encode_jpeg(views, quality=5, subsampling=subsampling)
    budgets = [(len(a) + len(b)) // 2 for a, b in zip(least, full)]
    assert all(len(a) < b < len(f) for a, b, f in zip(least, budgets, full))
    want = jpeggpu_amd.encode_jpeg_fit(views, budgets, quality=85, min_quality=5, subsampling=subsampling)
    got = jpeggpu_amd.thumbnail_jpeg(datas, (48, 48), quality=85, max_bytes=budgets, min_quality=5)
    assert got == want and all(len(f) <= b for f, b in zip(got[0], budgets)) and all(5 <= q < 85 for q in got[1])
    assert jpeggpu_amd.thumbnail_jpeg(datas, (48, 48), quality=85) == full, "without max_bytes the function is what it was"
