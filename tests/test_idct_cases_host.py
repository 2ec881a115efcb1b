"""The crafted IDCT corpus (tests/idct_cases.py) is what it claims to be: every file carries exactly the blocks and
quantisers it was built from, and -- worked out from the coefficients alone -- the units that aim at a branch of
jg_idct.hip really meet that branch's condition. No GPU. tests/test_gpu_idct_cases.py decodes the same files on the GPU.

The corpus counts, per family of files (COUNTS below; DESIGN.md section 5 repeats them). A "group" is an aligned group of
eight stream-consecutive units, what a wave of idct_kernel works on in one iteration:
                                                        pass1_*  counts_*  limit_*  ycc420*  kats16_*
  units ................................................  5,056    17,536    4,352    7,680     6,144
  units with a pass-1 input above 32,767 ...............    577         0        0      742     6,110
  units in groups that hold one (the 64-bit pass 1) ....  2,152         0        0    3,072     6,144
  of them ordinary units beside a special one ..........  1,574         0        0    2,023         0
  groups that mix units with and without an escape .....     32       808        0      276       125
  groups of units with an escape only ..................      4        98        0       13       259
Over-large columns built on purpose in the pass1 files: 448, and the 129 units of the DC ramp. Units of 31 / 32 / 33 entries
without an escape: 24 / 24 / 26 in each counts_plain file. Special units in each 4:2:0 file: 489 luma, 117 Cb, 117 Cr, in
366 of its 640 MCUs; over-large inputs in 138 chroma units of ycc420 and in 384 luma and 220 chroma units of ycc420_q16.
"""
import io

import numpy as np
import pytest

from tests import draft_ref, idct_cases, libjpeg_ref, scaled_ref
from tests.scaled_ref import CONST_BITS, PASS1_BITS, descale, int32

PASS1_FILES = ("pass1_bound", "pass1_edge8", "pass1_q16a", "pass1_q16b", "pass1_dcramp")
# per family: units, units with an over-large input, units in groups with one, ordinary ones among those, mixed and pure escape groups
COUNTS = {"pass1": [5056, 577, 2152, 1574, 32, 4], "counts": [17536, 0, 0, 0, 808, 98], "limit": [4352, 0, 0, 0, 0, 0],
          "ycc420": [7680, 742, 3072, 2023, 276, 13], "kats16": [6144, 6110, 6144, 0, 125, 259]}
LARGE_COLUMNS_BUILT = 448


@pytest.fixture(scope="module")
def corpus():
    return idct_cases.corpus()


@pytest.fixture(scope="module")
def decoded(corpus):
    from oracle import oracle

    return {name: oracle.decode(c.data) for name, c in corpus.items()}


def groups_of_eight(x):
    return np.asarray(x).reshape(-1, 8)


def large(case):
    """bool [n]: the unit holds a dequantised input above kIslowPass1Max."""
    return (np.abs(case.dequantised()) > idct_cases.ISLOW_PASS1_MAX).any(axis=(1, 2))


def pass1_outputs(case):
    """int64 [n, 8 (row), 8 (column)]: the pass-1 outputs of jpeg_idct_islow before their DESCALE."""
    d = case.dequantised()
    return np.stack(libjpeg_ref.islow_1d([d[:, k, :] for k in range(8)]), axis=1)


def islow_before_limit(case, pass1=idct_cases.pass1_exact):
    """int64 [n, 8, 8]: what jpeg_idct_islow hands to the range limit; `pass1`: how the workspace is computed."""
    ws = pass1(pass1_outputs(case))
    out = np.stack(libjpeg_ref.islow_1d([ws[:, :, k] for k in range(8)]), axis=2)
    return descale(out, CONST_BITS + PASS1_BITS + 3)


def test_every_file_decodes_to_the_blocks_and_quantisers_it_was_built_from(corpus, decoded):
    assert len(corpus) == 21
    for name, c in corpus.items():
        d = decoded[name]
        assert len(c.stream) <= 6400, name
        assert d.ncomp == len(c.blocks) and (c.gray or list(zip(d.hs, d.vs)) == [tuple(s) for s in c.sampling]), name
        for k in range(d.ncomp):
            assert np.array_equal(d.coef[k], c.blocks[k]), (name, k)
            assert np.array_equal(d.qtab[d.qidx[k]], c.qtabs[k]), (name, k)
        assert np.array_equal(d.stream_coef[0], c.stream), name
        assert d.restart_interval == c.restart_interval
    for name in ("pass1_q16a", "pass1_q16b", "pass1_dcramp", "ycc420_q16", "kats16_q_ones"):
        assert max(int(q.max()) for q in corpus[name].qtabs) > 255, name


def test_with_qtables16_changes_the_tables_only(corpus):
    from oracle import oracle
    from tools import jpegsynth

    c = corpus["pass1_edge8"]
    q = np.arange(64) * 1000 + 1
    a = oracle.decode(jpegsynth.encode_blocks(c.stream, idct_cases.BLOCKS_X, np.ones(64, np.uint8)))
    b = oracle.decode(idct_cases.with_qtables16(jpegsynth.encode_blocks(c.stream, idct_cases.BLOCKS_X, np.ones(64, np.uint8)), {0: q}))
    assert np.array_equal(a.coef[0], b.coef[0]) and np.array_equal(b.qtab[b.qidx[0]], q) and (a.qtab[a.qidx[0]] == 1).all()


def test_settings_every_special_unit_alone_and_among_its_kind(corpus):
    for name, c in corpus.items():
        g_special, g_setting = groups_of_eight(c.special), groups_of_eight(c.setting)
        a = (g_setting == "a").any(axis=1)
        assert (g_special[a].sum(axis=1) == 1).all(), name  # alone among seven ordinary units
        b = (g_setting == "b").all(axis=1)
        assert g_special[b].all(), name
        if name.startswith("kats16") or name == "pass1_dcramp":
            continue
        assert a.sum() >= 8 and b.sum() >= 1, name
        assert set(np.argmax(g_setting[a] == "a", axis=1)) == set(range(8)), name  # every position of the group
        if not name.startswith(("limit", "ycc")):  # (the sweep of `limit` is its setting (b); ycc420 draws from pools)
            assert set(c.label[c.setting == "a"]) == set(c.label[c.setting == "b"]), name
        # an ordinary unit stays far inside the 32-bit pass
        assert np.abs(c.dequantised()[~c.special]).max() <= idct_cases.ORDINARY_MAX, name


def test_pass1_columns_above_the_bound(corpus):
    first_bad, last_good = idct_cases.pass1_thresholds()
    assert 32768 < last_good and first_bad == last_good + 1 <= 35082
    built = 0
    for name in PASS1_FILES:
        c = corpus[name]
        cols = (np.abs(c.dequantised()) > idct_cases.ISLOW_PASS1_MAX).any(axis=1)  # [n, column]
        assert cols.sum() >= c.notes["large_columns"], name
        built += c.notes["large_columns"]
        # one over-large column sends the whole group through the 64-bit pass: ordinary units beside it
        mixed = groups_of_eight(large(c)).any(axis=1) & ~groups_of_eight(large(c)).all(axis=1)
        if name not in ("pass1_bound", "pass1_dcramp"):
            assert mixed.sum() >= 8 and set(np.argmax(groups_of_eight(large(c))[mixed], axis=1)) == set(range(8)), name
    assert built == LARGE_COLUMNS_BUILT + 129  # (the DC ramp: one column per unit with a DC value)
    # the bound itself: every sign pattern in every column, all of it inside the 32-bit pass
    c = corpus["pass1_bound"]
    d = c.dequantised()[c.setting == "b"]
    assert (np.abs(d) == 32767).all() and not large(c).any()
    for col in range(8):
        assert len({tuple(x) for x in np.sign(d[:, :, col])}) == 256, col
    # L = 32,768 in one row, the other rows small, alone in the unit and among ordinary columns
    c = corpus["pass1_edge8"]
    for what in ("lone", "among"):
        rows = set()
        for u in c.dequantised()[[str(s).startswith("L32768/one-row") and str(s).endswith(what) for s in c.label]]:
            col = np.abs(u).max(axis=0).argmax()
            assert (np.sort(np.abs(u[:, col]))[:-1] <= 128).all() and np.abs(u[:, col]).max() == 32768
            assert (np.delete(u, col, axis=1) != 0).any() == (what == "among")
            rows.add(int(np.abs(u[:, col]).argmax()))
        assert rows == set(range(8)), what


def test_pass1_a_wrongly_taken_32_bit_pass_shows(corpus):
    """For every L of the corpus at or above the first inexact one, a 32-bit pass 1 (restated with scaled_ref.int32)
    differs from jidctint.c's on a column of the file, and the difference reaches the pixels; below it the two agree."""
    first_bad, _ = idct_cases.pass1_thresholds()
    seen = set()
    for name in PASS1_FILES + ("ycc420", "ycc420_q16"):
        c = corpus[name]
        out = pass1_outputs(c)
        differs = (idct_cases.pass1_32bit(out) != idct_cases.pass1_exact(out)).any(axis=1)  # [n, column]
        mag = np.abs(c.dequantised())
        uniform = (mag == mag[:, :1, :]).all(axis=1)  # columns whose eight inputs share a magnitude
        for L in np.unique(mag[:, 0, :][uniform]):
            cols = uniform & (mag[:, 0, :] == L)
            if L >= first_bad:
                assert differs[cols].any(), (name, int(L))
                seen.add(int(L))
            elif L > 0:
                assert not differs[cols].any(), (name, int(L))
        bad_units = differs.any(axis=1)
        if name == "pass1_bound":  # at the bound the 32-bit pass is exact, on every sign pattern in every column
            assert not bad_units.any()
            continue
        pixels_differ = (scaled_ref.range_limit(islow_before_limit(c, idct_cases.pass1_32bit)) != scaled_ref.range_limit(islow_before_limit(c))).any(axis=(1, 2))
        assert not pixels_differ[~bad_units].any(), name
        # (an error in workspace column 0 or 4 is a multiple of 2^21 times 2^13 in pass 2: it never reaches bits 18..27)
        shows = differs[:, [1, 2, 3, 5, 6, 7]].any(axis=1)
        if name == "pass1_dcramp":
            assert not shows.any()
            continue
        assert shows.sum() >= 16 and pixels_differ[shows].mean() >= 0.9, (name, int(shows.sum()), float(pixels_differ[shows].mean()))
        if name.startswith("pass1_q16a"):  # the file that catches a threshold raised to 40,000: setting (a) at L <= 40,000
            caught = pixels_differ & (c.setting == "a") & (mag.max(axis=(1, 2)) <= 40000)
            assert caught.sum() >= 8, int(caught.sum())
    assert seen >= {first_bad, 40000, 65535, 1023 * 255, 1023 * 65535}, seen
    below = {int(L) for name in PASS1_FILES[:4] for L in corpus[name].notes["L"]}
    assert below >= {32766, 32767, 32768, 32769, first_bad - 1}


def test_pass1_the_dc_ramp_wraps_the_workspace(corpus):
    c = corpus["pass1_dcramp"]
    dc = c.stream[:, 0].astype(np.int64)
    assert dc.max() == 32767 and dc.min() == -32768 and np.abs(np.diff(np.concatenate([[0], dc]))).max() <= 2047
    assert int(c.qtabs[0][0]) == 65535
    exact = descale(pass1_outputs(c), CONST_BITS - PASS1_BITS)
    wraps = (exact != int32(exact)).any(axis=(1, 2))
    assert wraps.sum() >= 100 and np.abs(c.dequantised()).max() < 2 ** 31


def test_counts_every_entry_count_and_escape_placement(corpus):
    for suffix in ("packed", "restart"):
        c = corpus["counts_plain_" + suffix]
        cnt, esc = idct_cases.entry_count(c.stream), idct_cases.has_escape(c.stream)
        assert not esc.any()
        for setting in ("a", "b"):
            assert set(cnt[c.setting == setting]) == set(range(1, 65)), (suffix, setting)
        for n in range(2, 65):  # index 63 is used at every count
            assert any(c.stream[i, 63] != 0 for i in np.flatnonzero((cnt == n) & (c.setting == "b"))), n
        one_hot = c.stream[[str(s).startswith("one-hot") for s in c.label]]
        assert {(int(np.flatnonzero(u)[0]), int(np.sign(u[np.flatnonzero(u)[0]]))) for u in one_hot} == {(p, s) for p in range(64) for s in (1, -1)}
        assert (c.label == "flip").sum() == 1 and cnt[c.label == "flip"][0] == 1

        c = corpus["counts_escape_" + suffix]
        cnt, esc = idct_cases.entry_count(c.stream), idct_cases.has_escape(c.stream)
        for setting in ("a", "b"):
            sel = c.setting == setting
            assert set(cnt[sel & esc]) >= set(range(3, 128, 2)), (suffix, setting)  # 1..63 escaped coefficients
            at, last, inner = set(), set(), set()
            for u in c.stream[sel & esc]:
                e = idct_cases.entries_of(u)
                for i, (z, is_esc) in enumerate(e):
                    if is_esc:
                        at.add(i)
                        (last if i == len(e) - 1 else inner).add(i)
                        at.add("zz%d" % z)
            assert at >= set(idct_cases.ESCAPE_ENTRIES) | {"zz1", "zz63"}, (suffix, setting)
            assert last >= set(idct_cases.ESCAPE_ENTRIES) and inner >= set(idct_cases.ESCAPE_ENTRIES), (suffix, setting)
        hot = c.stream[[str(s).startswith("one-hot-escaped") for s in c.label]]
        assert {(int(np.flatnonzero(u)[0]), int(np.sign(u[np.flatnonzero(u)[0]]))) for u in hot} == {(p, s) for p in range(64) for s in (1, -1)}
        # a unit with an escape whose last entry is a plain one, in front of an entry whose index field is 0
        ends = np.flatnonzero([str(s).startswith("escape-then-plain-end") for s in c.label])
        assert len(ends) >= 16 and all(not idct_cases.entries_of(c.stream[i])[-1][1] and esc[i] and c.stream[i + 1, 0] % 64 == 0 for i in ends)
        # mixed and pure groups (the escape ballot of idct_kernel, per aligned group of eight)
        g = groups_of_eight(esc)
        assert (g.any(axis=1) & ~g.all(axis=1)).sum() >= 200 and g.all(axis=1).sum() >= 20, suffix
        # and the same for units above 31 entries beside units the prefetched words cover
        g = groups_of_eight(idct_cases.entry_count(corpus["counts_plain_" + suffix].stream) > 31)
        assert (g.any(axis=1) & ~g.all(axis=1)).sum() >= 64 and g.all(axis=1).sum() >= 4, suffix


def test_counts_predicted_gather_coverage(corpus):
    """The order of the ladder (a seeded shuffle) gives the packed file units of 31, 32 and 33 entries with an even and an
    odd first entry, and every sector offset 0..15 of the first entry among units of 17 entries and more, at both
    subsequence sizes the GPU test uses -- by the model of the data-unit table; the GPU test asserts it on the real one."""
    c = corpus["counts_plain_packed"]
    cnt = idct_cases.entry_count(c.stream)
    for sb in (32, 256):
        _, first = idct_cases.predicted_first_entries(c, sb)
        for n in (31, 32, 33):
            assert set(first[cnt == n] & 1) == {0, 1}, (sb, n)
        assert set(first[cnt >= 17] & 15) == set(range(16)), sb


def test_limit_every_value_in_front_of_the_range_limit(corpus):
    for name in ("limit_dc", "limit_ac"):
        c = corpus[name]
        assert int(c.qtabs[0][0]) == 8
        sweep = c.setting == "b"
        assert np.array_equal(c.stream[sweep, 0], np.arange(-1024, 1024))
        assert (c.stream[sweep, 1:] != 0).any(axis=1).all() == (name == "limit_ac")
        want = set(range(-1024, 1024))
        assert {int(v) for v in islow_before_limit(c)[sweep].reshape(-1)} >= want, name
        assert {int(v) for v in descale(c.dequantised()[sweep, 0, 0], 3)} == want, name
        # and the restatements that serve as the GPU's references give the wrapped, clamped value on both sides of the wrap
        dc = np.arange(-1024, 1024)
        limited = np.clip(((dc + 512) % 1024) - 512, -128, 127) + 128
        assert np.array_equal(scaled_ref.idct_1x1(c.stream[sweep], c.qtabs[0]).reshape(-1), limited), name
        if name == "limit_dc":  # DC only: every sample of every size is that value
            for f, n in ((scaled_ref.idct_2x2, 2), (scaled_ref.idct_4x4, 4), (libjpeg_ref.idct_islow, 8)):
                assert np.array_equal(f(c.stream[sweep], c.qtabs[0]), np.broadcast_to(limited[:, None, None], (2048, n, n))), (name, n)
        edges = {int(str(s)[2:]) for s in c.label[c.setting == "a"]}
        assert edges == set(idct_cases.LIMIT_EDGES), name


def test_ycc420_every_component_holds_special_units(corpus):
    first_bad, _ = idct_cases.pass1_thresholds()
    for name in ("ycc420", "ycc420_q16"):
        c = corpus[name]
        for k in range(3):
            sel = c.special & (c.comp == k)
            labels = {str(s).split("/")[0] for s in c.label[sel]}
            assert sel.sum() >= 100 and labels >= {"count31", "count32", "count33", "escape-entry8", "escape-entry17", "dc-513", "dc512"}, (name, k)
            assert {"a", "b"} <= set(c.setting[sel]), (name, k)
        chroma_large = large(c) & (c.comp > 0)
        assert chroma_large.sum() >= 40, name  # the 8x8 ISLOW class of libjpeg's scale mode at 1/2 gets over-large columns
        mcus = c.special_mcus()
        assert (~mcus).sum() >= 40 and mcus.sum() >= 300, name
    assert (np.abs(corpus["ycc420_q16"].dequantised()).max(axis=(1, 2)) == first_bad).any()


def corpus_counts(corpus):
    out = {}
    for name, c in corpus.items():
        big = large(c)
        g = groups_of_eight(big).any(axis=1)
        e = groups_of_eight(idct_cases.has_escape(c.stream))
        row = [len(c.stream), int(big.sum()), 8 * int(g.sum()), int((np.repeat(g, 8) & ~c.special).sum()),
               int((e.any(axis=1) & ~e.all(axis=1)).sum()), int(e.all(axis=1).sum())]
        family = out.setdefault(name.split("_")[0], [0] * 6)
        for k in range(6):
            family[k] += row[k]
    return out


def test_corpus_counts_are_the_documented_ones(corpus):
    assert corpus_counts(corpus) == COUNTS
    for name in ("counts_plain_packed", "counts_plain_restart"):
        c = corpus[name]
        cnt = idct_cases.entry_count(c.stream)[~idct_cases.has_escape(c.stream)]
        assert [int((cnt == n).sum()) for n in (31, 32, 33)] == [24, 24, 26], name
    for name, big in (("ycc420", [0, 70, 68]), ("ycc420_q16", [384, 103, 117])):
        c = corpus[name]
        assert [int((c.special & (c.comp == k)).sum()) for k in range(3)] == [489, 117, 117]
        assert [int((large(c) & (c.comp == k)).sum()) for k in range(3)] == big
        assert int(c.special_mcus().sum()) == 366 and c.special_mcus().size == 640


def test_every_reference_runs_on_every_file(corpus, decoded):
    for name, c in corpus.items():
        d = decoded[name]
        for k in range(d.ncomp):
            coef, q = c.blocks[k].reshape(-1, 64), c.qtabs[k]
            n = len(coef)
            assert libjpeg_ref.idct_islow(coef, q).shape == (n, 8, 8)
            assert scaled_ref.idct_4x4(coef, q).shape == (n, 4, 4) and scaled_ref.idct_2x2(coef, q).shape == (n, 2, 2)
            assert scaled_ref.idct_1x1(coef, q).shape == (n, 1, 1)
        islow = libjpeg_ref.islow_planes_of(d)
        assert [p.shape for p in islow] == [p.shape for p in d.planes]
        assert all(np.array_equal(a, b) for a, b in zip(draft_ref.draft_planes_of(d, 1), islow))
        for s in (2, 4, 8):
            scaled, draft = scaled_ref.scaled_planes_of(d, s), draft_ref.draft_planes_of(d, s)
            assert np.array_equal(scaled[0], draft[0]), (name, s)  # the component with the maximum factors: block size 8 / s
            if d.ncomp == 3:  # 4:2:0: libjpeg's mode gives chroma the next block size up
                assert draft_ref.block_sizes(d.hs, d.vs, s) == [8 // s, 16 // s, 16 // s]
                assert draft[1].shape == (scaled[1].shape[0] * 2, scaled[1].shape[1] * 2), (name, s)
    # the restatement of the range limit is exercised on both sides of its wrap by the limit files
    c = corpus["limit_dc"]
    px = libjpeg_ref.idct_islow(c.stream[c.setting == "b"], c.qtabs[0])[:, 0, 0].astype(int)
    dc = np.arange(-1024, 1024)
    assert np.array_equal(px, np.clip(((dc + 512) % 1024) - 512, -128, 127) + 128)


def pillow_comparable_units(case):
    """bool [n]: the units on which libjpeg-turbo's SIMD jpeg_idct_islow (what Pillow runs) computes what jidctint.c
    computes. The SIMD code keeps the dequantised inputs, the sums in0 +- in4, in1 + in5 and in3 + in7 and the workspace
    in 16 bits, and it SATURATES its result to a sample where jidctint.c wraps it to 10 bits first (RANGE_MASK). So: all
    of those fit 16 bits in both passes, and the value in front of the range limit lies in -512..511. Nothing else is
    excluded, and nothing because of what either decoder returned."""
    d = case.dequantised()
    ws = idct_cases.pass1_exact(pass1_outputs(case))

    def fits(x, axis):
        a = np.abs(np.moveaxis(x, axis, 1))
        return ((a[:, 0] + a[:, 4] <= 32767) & (a[:, 1] + a[:, 5] <= 32767) & (a[:, 3] + a[:, 7] <= 32767) & (a[:, 2] + a[:, 6] <= 32767)).all(axis=1) & (a <= 32767).all(axis=(1, 2))

    v = islow_before_limit(case)
    return fits(d, 1) & fits(ws, 2) & ((v >= -512) & (v <= 511)).all(axis=(1, 2))


def test_limit_and_counts_islow_planes_equal_pillow(corpus, decoded):
    Image = pytest.importorskip("PIL.Image")
    compared = 0
    for name in ("limit_dc", "limit_ac", "counts_plain_packed", "counts_plain_restart", "counts_escape_packed", "counts_escape_restart"):
        c = corpus[name]
        ours = libjpeg_ref.islow_planes_of(decoded[name])[0]
        theirs = np.asarray(Image.open(io.BytesIO(c.data)))
        assert theirs.shape == ours.shape
        blocks = lambda p: p.reshape(-1, 8, idct_cases.BLOCKS_X, 8).transpose(0, 2, 1, 3).reshape(-1, 8, 8)
        ok = pillow_comparable_units(c)
        assert ok.sum() >= len(ok) // 2, (name, int(ok.sum()))
        bad = np.flatnonzero((blocks(ours)[ok] != blocks(theirs)[ok]).any(axis=(1, 2)))
        assert len(bad) == 0, (name, len(bad), c.label[ok][bad][:5])
        compared += int(ok.sum())
    assert compared >= 15000
