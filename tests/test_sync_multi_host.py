"""The multi-symbol entries of the sync pack (jg_defs.h) whose LAST symbol may end behind the index bits: what the
product's table builder (jg_reader.cpp, widen_huff_table) puts into them, checked entry by entry against walks over the
single entries, and how many steps of the state-only loop (jg_huff_core.h, decode_subsequence) they save against the
rule that kept every symbol inside the index. CPU only (tests/syncprobe compiles the product's sources with g++).

Measured when this test was written (whole images, 256-byte subsequences; test_symbols_per_step prints them, EXPERIMENTS.md
keeps them): cfg 2 seed 0 1.620 -> 1.798 symbols per step (9.9 % fewer steps), the photo 1.509 -> 1.712 (11.9 % fewer);
the crafted file's longest entry stands for 21 bits."""
import numpy as np
import pytest

from tests import cases
from tests.syncprobe import crafted, syncprobe
from tools import jpegsynth

LB = 11           # index bits of an AC table (jg_defs.h, kLutBitsAc)
EOB_ADVANCE = 63  # advance field of an end of block
FILLS = 64        # seeded random fills of the bits behind the index, besides all zeros and all ones


@pytest.fixture(scope="module")
def tables():
    """name -> (class, bits, vals): the four Annex K tables (a file jpegsynth writes without optimize carries them), every
    distinct table of the tests/cases.matrix() inputs -- the fitted ones of its optimize=True files among them -- and the
    crafted file's."""
    out, seen = {}, set()

    def take(prefix, data):
        for tc, th, bits, vals in syncprobe.dht_tables(data):
            key = (tc, bits.tobytes(), vals.tobytes())
            if key not in seen:
                seen.add(key)
                out["%s_%s%d" % (prefix, "dc" if tc == 0 else "ac", th)] = (tc, bits, vals)

    take("annexk", jpegsynth.encode(64, 48, cases.S420, seed=1))
    assert len(out) == 4
    for name, data in cases.matrix().items():
        take(name, data)
    assert any(k.startswith("opt_tables_420") for k in out) and any(k.startswith("four_comp_opt") for k in out)
    take("crafted", crafted.long_magnitude_case())
    assert "crafted_ac0" in out
    return out


def _check_entries(name, low, idxs, multi, fill):
    """The multi entries `multi` at the indices `idxs` against walks over the single entries `low` of the windows
    idx | fill (fill: the 53 bits behind the index of a 64-bit window), all indices at once. Returns the symbols each
    walk committed."""
    m_len, m_pre, m_adv = (multi & 31).astype(np.int64), ((multi >> 5) & 15).astype(np.int64), (multi >> 9).astype(np.int64)
    window = (idxs.astype(np.uint64) << np.uint64(53)) | np.uint64(fill)
    z = lambda: np.zeros(len(idxs), np.int64)
    bits, count, adv_sum, pre_sum, last_at, last_code = z(), z(), z(), z(), z(), z()
    prev_eob = np.zeros(len(idxs), bool)
    for _ in range(LB + 2):  # a symbol has at least one bit, and all but the last lie inside the index
        act = bits < m_len
        if not act.any():
            break
        e = low[((window >> (53 - bits).astype(np.uint64)) & np.uint64((1 << LB) - 1)).astype(np.int64)].astype(np.int64)
        ln, cat, adv = e & 31, (e >> 5) & 15, e >> 9
        assert not (act & (ln == 0)).any(), (name, "a claimed symbol has a code longer than the index")
        assert not (act & prev_eob).any(), (name, "an end of block in front of the last symbol")
        pre_sum = np.where(act, adv_sum, pre_sum)
        last_at = np.where(act, bits, last_at)
        last_code = np.where(act, ln - cat, last_code)
        prev_eob = np.where(act, adv == EOB_ADVANCE, prev_eob)
        adv_sum += np.where(act, adv, 0)
        bits += np.where(act, ln, 0)
        count += act
    bad = np.nonzero((bits != m_len) | (count < 2) | (pre_sum != m_pre) | (adv_sum != m_adv))[0]
    assert bad.size == 0, (name, "total bits / advance of all but the last / total advance", idxs[bad[:4]], fill)
    # every symbol but the last lies wholly inside the index, and the last one's code does
    assert (last_at <= LB).all() and (last_at + last_code <= LB).all(), name
    return count


def test_multi_entries_equal_single_walks(tables):
    rng = np.random.default_rng(2024)
    fills = [0, (1 << 53) - 1] + [int(x) for x in rng.integers(0, 1 << 53, FILLS, dtype=np.uint64)]
    multi_total = longest = behind = 0
    for name, (tc, bits, vals) in tables.items():
        wide = syncprobe.widen(bits, vals, is_dc=tc == 0)
        high, low = wide >> 16, wide & 0xFFFF
        if tc == 0:
            assert np.array_equal(high, low), (name, "DC tables hold single symbols only")
            continue
        idxs = np.nonzero(high != low)[0]
        if idxs.size == 0:
            continue
        counts = [_check_entries(name, low, idxs, high[idxs], f) for f in fills]
        assert all(np.array_equal(c, counts[0]) for c in counts), (name, "an entry depends on the bits behind the index")
        multi_total += idxs.size
        longest = max(longest, int((high[idxs] & 31).max()))
        behind += int(((high[idxs] & 31) > LB).sum())
        # against the strict rule (every symbol wholly inside the index): the same low halves; where it has a multi entry
        # the relaxed rule has one that is no shorter
        strict = syncprobe.widen(bits, vals, strict=True)
        assert np.array_equal(strict & 0xFFFF, low)
        s = strict >> 16
        had = s != low
        assert ((s[had] & 31) <= LB).all() and (high != low)[had].all() and ((s[had] & 31) <= (high[had] & 31)).all(), name
    assert multi_total > 0 and behind > 0 and 18 <= longest <= 26, (multi_total, behind, longest)


def test_crafted_file_has_entries_ending_in_long_magnitudes(tables):
    tc, bits, vals = tables["crafted_ac0"]
    wide = syncprobe.widen(bits, vals)
    low, high = wide & 0xFFFF, wide >> 16
    # (run 0, category 1) and (run 0, category 10) are the two shortest codes of the fitted table
    order = np.argsort(np.repeat(np.arange(1, 17), bits), kind="stable")
    assert {int(vals[order[0]]), int(vals[order[1]])} == {0x01, 0x0A}
    lens = (high & 31)[high != low]
    assert lens.max() >= 18, lens.max()
    # the file itself passes such entries: the loop's exit states equal decode_subsequence's, and steps took entries
    r = syncprobe.count_steps(crafted.long_magnitude_case(), 32)
    assert r.state_mismatches == 0 and r.longest_multi >= 18 and r.multi_steps > r.strict_multi_steps > 0


@pytest.mark.parametrize("which", ["cfg2_seed0", "photo"])
def test_symbols_per_step(which, photo_bytes):
    """Whole image, 256-byte subsequences (what a batch decodes at): the relaxed rule needs at least 6 % fewer steps than
    the strict one."""
    data = jpegsynth.config(2, seed=0) if which == "cfg2_seed0" else photo_bytes
    r = syncprobe.count_steps(data, 256)
    assert r.state_mismatches == 0 and r.subsequences > 10000
    print("\n%s: %d symbols in %d subsequences; strict rule %d steps (%.3f symbols/step), relaxed rule %d steps (%.3f), %.1f %% fewer; "
          "longest multi entry %d bits" % (which, r.symbols, r.subsequences, r.strict_steps, r.symbols / r.strict_steps, r.steps,
                                           r.symbols / r.steps, 100.0 * (1 - r.steps / r.strict_steps), r.longest_multi))
    assert r.steps <= 0.94 * r.strict_steps, (r.steps, r.strict_steps)
    assert r.longest_multi <= 26
