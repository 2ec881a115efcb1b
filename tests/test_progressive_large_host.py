"""The large and the structural progressive inputs without a GPU (tests/progressive_cases.py: large(), structure()):
that each file holds what it is there for -- asserted from the statistics of the Annex G restatement, not taken from the
generator's word --, that the host twin of the scan kernels equals the restatement on them, and that the work list the
device reads follows the rule jg_prog_plan.hpp states."""
import numpy as np

from tests import progressive_cases as pc
from tests import progressive_ref as pr
from tests.emu import prog_twin


def new_files():
    out = {n: l.prog for n, l in pc.large().items()}
    out.update({n: f for n, (f, _) in pc.structure().items()})
    return out


def kind_of(scan):
    """ProgKind of a scan of the restatement: DC first, DC refinement, AC first, AC refinement."""
    return (2 if scan["ss"] else 0) + (1 if scan["ah"] else 0)


def test_the_inputs_are_the_ones_described():
    files = new_files()
    assert sorted(files) == sorted(["eob_ladder", "eob_cap", "photo", "photo_rst"] + [c[0] for c in pc.STRUCTURE])
    assert len(files) == 4 + 5
    for name in ("eob_ladder", "eob_cap"):
        want, _ = pc.restated(files[name])
        assert (want.width, want.height, len(want.comps)) == (1456, 1448, 1)
        assert want.coef[0].shape == (181, 182, 64) and 181 * 182 == 32942
        assert [(s["ss"], s["se"], s["ah"], s["al"], s["segments"]) for s in want.scans] == [
            (0, 0, 0, 1, 1), (1, 5, 0, 1, 1), (6, 63, 0, 1, 1), (0, 0, 1, 0, 1), (1, 5, 1, 0, 1), (6, 63, 1, 0, 1)]
    for name, size in (("photo", (1024, 768)), ("photo_rst", (512, 384))):
        want, _ = pc.restated(files[name])
        assert (want.width, want.height) == size and [(c["h"], c["v"]) for c in want.comps] == [(2, 2), (1, 1), (1, 1)]
        assert len(want.scans) == 10 and max(want.levels) == 2
    assert [s["segments"] for s in pc.restated(files["photo"])[0].scans] == [1] * 10
    # a restart marker behind every MCU: 32 x 24 MCUs in the interleaved DC scans and as many blocks in a chroma scan,
    # 64 x 48 blocks in luma's AC scans -- 48 waves of lanes
    rst = pc.restated(files["photo_rst"])[0]
    assert [s["segments"] for s in rst.scans] == [768 if len(s["comps"]) == 3 or s["comps"][0] else 3072 for s in rst.scans]
    assert sum(s["segments"] == 3072 for s in rst.scans) == 4


def test_eob_ladder_holds_a_run_of_every_category():
    want, stats = pc.restated(pc.large()["eob_ladder"].prog)
    first = [st for s, st in zip(want.scans, stats) if kind_of(s) == 2]
    refine = [st for s, st in zip(want.scans, stats) if kind_of(s) == 3]
    assert len(first) == 2 and len(refine) == 2
    assert all(n >= 1 for n in first[0]["eob_categories"]), first[0]["eob_categories"]    # band 1..5
    assert all(n >= 1 for n in refine[1]["eob_categories"]), refine[1]["eob_categories"]  # band 6..63
    assert first[0]["longest_run"] == 1 << 14 and refine[1]["longest_run"] == 1 << 14
    # every block of band 6..63 has a history, so every block inside a run takes a correction bit: all but the separators
    assert refine[1]["correction_bits_in_runs"] >= 32767
    assert refine[1]["correction_bits_in_runs"] == 32942 - 16
    # ... of both values: the coefficients behind them end up with the low bit set and clear
    low = np.abs(want.coef[0].reshape(-1, 64)[:, pr.ZIGZAG[6]].astype(np.int32))
    assert set(low.tolist()) == {4, 5} and 10000 < int((low == 5).sum()) < 23000
    # band 1..5 of the refinement is one run over all blocks, cut at the cap
    assert refine[0]["longest_run"] == 0x7FFF and refine[0]["correction_bits_in_runs"] == 16


def test_eob_cap_holds_the_longest_run_and_another_behind_it():
    want, stats = pc.restated(pc.large()["eob_cap"].prog)
    ac = [(s, st) for s, st in zip(want.scans, stats) if s["ss"]]
    assert len(ac) == 4
    for s, st in ac:  # the first scans and the refinements alike
        runs = st["runs"]
        at = [i for i, (length, _) in enumerate(runs) if length == 0x7FFF]
        assert len(at) == 1, (s, runs)
        i = at[0]
        assert st["eob_categories"][14] == 1 and st["longest_run"] == 0x7FFF
        assert i + 1 < len(runs) and runs[i + 1][1] == runs[i][1] + 1, (s, runs)  # the next symbol of the scan is a run again
        assert runs[i][0] + runs[i + 1][0] >= 32942 - 101 - 1
    flat = want.coef[0].reshape(-1, 64)
    nonzero = np.flatnonzero(np.any(flat[:, 1:] != 0, axis=1))
    assert nonzero.tolist() == [0, 100, 32941]


def test_photo_has_long_codes_and_stuffed_bytes():
    photo = pc.large()["photo"].prog
    want, stats = pc.restated(photo)
    assert sum(st["long_codes"] for st in stats) >= 1
    assert sum(st["long_codes"] > 0 for st in stats) >= 4  # (in most AC scans, in fact)
    assert photo.count(b"\xff\x00") >= 100
    # scans long enough to matter for one lane: the longest single segment holds tens of KB
    i = [k for k in range(len(photo) - 1) if photo[k] == 0xFF and photo[k + 1] == 0xDA]
    assert max(b - a for a, b in zip(i, i[1:] + [len(photo)])) > 40000
    # more than 256 pack units, by far: 12 288 luma blocks and 2 x 3 072 chroma blocks
    assert sum(vy * vx for vy, vx in want.visible) == 128 * 96 + 2 * 64 * 48


def test_level_structure_of_the_small_files():
    s = pc.structure()
    deep, _ = pc.restated(s["deep_levels"][0])
    assert max(deep.levels) + 1 >= 14
    st, info = prog_twin.parse(s["deep_levels"][0])
    assert st == 0 and info.num_levels == max(deep.levels) + 1 == 14
    many, _ = pc.restated(s["sixty_four_scans"][0])
    assert len(many.scans) == 64 and set(many.levels) == {0}
    st, info = prog_twin.parse(s["sixty_four_scans"][0])
    assert st == 0 and (info.num_scans, info.num_levels) == (64, 1)
    # every band writes something: no scan of the 64 is empty of coefficients
    luma = many.coef[0].reshape(-1, 64)
    assert np.all(np.any(luma != 0, axis=0))
    assert [x["segments"] for x in pc.restated(s["two_large_444"][0])[0].scans] == [81] * 6
    assert [x["segments"] for x in pc.restated(s["threshold_420"][0])[0].scans] == [64, 64, 16, 16, 16, 16]
    assert [x["segments"] for x in pc.restated(s["threshold_420_below"][0])[0].scans] == [43, 43, 11, 11, 11, 11]


def test_host_twin_equals_the_restatement_on_the_new_files():
    """As tests/test_progressive_host.py::test_host_twin_equals_the_restatement: coefficient buffers with the padded
    blocks, levels and segment counts; and the pack round trip of test_pack_round_trip."""
    for name, data in new_files().items():
        want, _ = pc.restated(data)
        st, info, coef, back = prog_twin.decode(data)
        assert st == 0, name
        assert list(info.scan_level[:info.num_scans]) == want.levels, name
        assert info.num_levels == max(want.levels) + 1
        assert [info.scan_segments[k] for k in range(info.num_scans)] == [s["segments"] for s in want.scans], name
        for c in range(info.num_comp):
            assert coef[c].shape == want.coef[c].shape, (name, c)
            bad = np.argwhere(coef[c] != want.coef[c])
            assert len(bad) == 0, (name, c, len(bad), bad[:4].tolist())
            assert np.array_equal(back[c], coef[c][:info.vis_y[c], :info.vis_x[c]]), (name, c)


def test_complete_files_hold_their_sources_coefficients():
    """The restatement's coefficients are those of the baseline file the progressive one was made from (its twin, for a
    photo): what the GPU tests compare with the oracle's decode of that file is the same thing."""
    from oracle import oracle

    pairs = {n: (l.prog, l.twin) for n, l in pc.large().items() if l.twin}
    pairs.update({n: v for n, v in pc.structure().items() if n != "sixty_four_scans"})
    assert len(pairs) == 2 + 4
    for name, (prog, base) in pairs.items():
        want, o = pc.restated(prog)[0], oracle.decode(base)
        for c in range(o.ncomp):
            vy, vx = want.visible[c]
            assert np.array_equal(want.coef[c][:vy, :vx], o.coef[c][:vy, :vx]), (name, c)
    # sixty_four_scans: luma and the DC values, the chroma AC coefficients are never coded
    prog, base = pc.structure()["sixty_four_scans"]
    want, o = pc.restated(prog)[0], oracle.decode(base)
    assert np.array_equal(want.coef[0][:3, :5], o.coef[0][:3, :5])
    for c in (1, 2):
        assert np.array_equal(want.coef[c][:2, :3, 0], o.coef[c][:2, :3, 0]) and not want.coef[c][:, :, 1:].any()
        assert o.coef[c][:2, :3, 1:].any()


def check_work_list(data):
    """The rule of jg_prog_plan.hpp restated: per level, the scans of kProgLaneGroup = 64 segments or more come first in
    file order, each from a multiple of 64 items behind the level's start, with idle items in front of it up to that
    multiple; the scans below 64 follow, grouped by kind, in file order inside a kind. Returns the idle items per level."""
    want, _ = pc.restated(data)
    items, level_item = prog_twin.work_list(data)
    levels = max(want.levels) + 1
    assert level_item[0] == 0 and level_item[levels] == len(items)
    idle = []
    for level in range(levels):
        mine = [k for k in range(len(want.scans)) if want.levels[k] == level]
        large = [k for k in mine if want.scans[k]["segments"] >= 64]
        small = sorted((k for k in mine if want.scans[k]["segments"] < 64), key=lambda k: (kind_of(want.scans[k]), k))
        expect = []
        for k in large:
            expect += [(prog_twin.IDLE, 0)] * (-len(expect) % 64)
            assert len(expect) % 64 == 0
            expect += [(k, g) for g in range(want.scans[k]["segments"])]
        for k in small:
            expect += [(k, g) for g in range(want.scans[k]["segments"])]
        got = [tuple(int(v) for v in it) for it in items[level_item[level]:level_item[level + 1]]]
        assert got == expect, (level, [(i, a, b) for i, (a, b) in enumerate(zip(got, expect)) if a != b][:4], len(got), len(expect))
        # (what the comparison above implies, said on its own: every pair exactly once, and nothing idle but the padding)
        real = [it for it in got if it[0] != prog_twin.IDLE]
        assert sorted(real) == sorted((k, g) for k in mine for g in range(want.scans[k]["segments"])) and len(set(real)) == len(real)
        for k in large:
            assert got.index((k, 0)) % 64 == 0
        idle.append(len(got) - len(real))
    return idle


def test_work_list_follows_the_rule():
    s = pc.structure()
    # script_plain's six scans write disjoint coefficients and are ONE level; each has 81 segments: five paddings of 47
    assert check_work_list(s["two_large_444"][0]) == [5 * 47]
    assert check_work_list(s["threshold_420"][0]) == [0]        # 64 is large: scans 0 and 1 lead, at items 0 and 64
    items, _ = prog_twin.work_list(s["threshold_420"][0])
    assert [int(v) for v in items[[0, 63, 64, 127, 128, 144, 160, 176], 0]] == [0, 0, 1, 1, 2, 4, 3, 5]
    assert check_work_list(s["threshold_420_below"][0]) == [0]  # 43 is not: all six scans by kind
    items, _ = prog_twin.work_list(s["threshold_420_below"][0])
    assert [int(v) for v in items[[0, 43, 54, 65, 108, 119], 0]] == [0, 2, 4, 1, 3, 5]
    check_work_list(pc.pins()["p420_rst1"][0])
    for name, data in new_files().items():  # (photo_rst: five large scans in level 0, all of a multiple of 64 segments)
        check_work_list(data)
