"""Small JPEGs built from explicit coefficient blocks that aim at the arithmetic and gather edges of the IDCT stage
(jg_idct.hip): the ISLOW transform's choice between its 32-bit and 64-bit pass 1, the entry counts at which the gathers
change path, escaped coefficients at the ends of the scaled kernel's load groups, and the range limit. Everything is
seeded; nothing here needs a GPU (tests/test_idct_cases_host.py proves the corpus is what it claims).

Every file but pass1_dcramp and kats16_* (a DC ramp cannot stand alone, since a unit's DC follows from its neighbour's;
the KAT groups are fixed blocks, all of them special: both hold setting (b) only) holds its SPECIAL units in two settings,
the other units being photo-like ("ordinary": a few small low-frequency coefficients whose dequantised values stay far
below 32,768):
  (a) alone among seven ordinary units of an aligned group of eight stream-consecutive units (the eight units a wave of
      idct_kernel works on in one iteration), special unit i of the file at position i % 8 of its group;
  (b) in groups of special units only.
A Case records, in stream order, which units are special, their setting and a label that says what each one is for.
"""
import functools
import os

import numpy as np

from tests import libjpeg_ref
from tests.scaled_ref import CONST_BITS, PASS1_BITS, descale, int32

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BLOCKS_X = 32  # grayscale files: 32 units per block row, so an aligned group of eight never straddles a row
S420 = ((2, 2), (1, 1), (1, 1))
# natural index of zig-zag position z (T.81 figure A.6)
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13,
                   6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45,
                   38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
ISLOW_PASS1_MAX = 32767  # kIslowPass1Max of jg_idct.hip: the largest input the 32-bit pass 1 is proven exact for
ORDINARY_MAX = 2000      # |dequantised| of an ordinary unit's coefficients stays below this
WORST_SIGNS = np.array([-1, -1, 1, 1, 1, -1, -1, -1])  # the signs of output 2's coefficients: sum |c_k| = 61,214


class Case:
    """One file: `data`; per component `blocks` int16 [blocks_y, blocks_x, 64] (natural order, DC absolute) and `qtabs`
    uint16 [64] (natural order); in stream order `stream` int16 [n, 64], `comp` (component of each unit), `special`
    (bool), `setting` ("a", "b", or "-" for ordinary units and for copies that are not group-aligned) and `label`."""

    def __init__(self, name, data, blocks, qtabs, stream, comp, special, setting, label, restart_interval=0, sampling=((1, 1),), notes=None):
        self.name, self.data, self.blocks, self.qtabs = name, data, blocks, [np.asarray(q, np.uint16) for q in qtabs]
        self.stream, self.comp, self.special = stream, np.asarray(comp), np.asarray(special, bool)
        self.setting, self.label = np.asarray(setting, object), np.asarray(label, object)
        self.restart_interval, self.sampling, self.notes = restart_interval, sampling, notes or {}

    @property
    def gray(self):
        return len(self.blocks) == 1

    def dequantised(self):
        """int64 [n, 8, 8] (row, column) of the stream's units."""
        q = np.stack([self.qtabs[c] for c in range(len(self.qtabs))]).astype(np.int64)
        return (self.stream.astype(np.int64) * q[self.comp]).reshape(-1, 8, 8)

    def special_mcus(self):
        """bool [mcus_y, mcus_x]: the MCUs that hold a special unit."""
        per = sum(h * v for h, v in self.sampling)
        mcus_x = self.blocks[0].shape[1] // self.sampling[0][0]
        return self.special.reshape(-1, per).any(axis=1).reshape(-1, mcus_x)


# ------------------------------------------------------------------------------------------------
# blocks
# ------------------------------------------------------------------------------------------------

def natural(zz):
    """[n, 64] in zig-zag order -> natural order."""
    out = np.zeros_like(zz)
    out[:, ZIGZAG] = zz
    return out


def ordinary(rng, n, q):
    """n photo-like units for quantisation table q: 1 to 11 coefficients among the first 20 zig-zag positions, Laplace
    distributed, clipped so that no dequantised value exceeds ORDINARY_MAX (zero where the quantiser is larger)."""
    k = rng.integers(1, 12, n)
    rank = rng.random((n, 20)).argsort(axis=1)
    vals = np.rint(rng.laplace(0, 30, (n, 20)))
    zz = np.zeros((n, 64), np.int64)
    zz[:, :20] = np.where(rank < k[:, None], vals, 0)
    lim = np.minimum(1023, ORDINARY_MAX // np.asarray(q, np.int64))
    return np.clip(natural(zz), -lim[None, :], lim[None, :]).astype(np.int16)


def entry_count(coef):
    """Symbol-stream entries of each unit (jg_defs.h): the DC, one per non-zero AC coefficient, one more (the escape) per
    AC coefficient of magnitude 512 and above."""
    ac = np.asarray(coef).reshape(-1, 64)[:, 1:].astype(np.int64)
    return 1 + (ac != 0).sum(axis=1) + (np.abs(ac) >= 512).sum(axis=1)


def has_escape(coef):
    return (np.abs(np.asarray(coef).reshape(-1, 64)[:, 1:].astype(np.int64)) >= 512).any(axis=1)


def entries_of(unit):
    """[(zig-zag position, is_escape)] of one unit's entries in stream order."""
    out = [(0, False)]
    for z in range(1, 64):
        v = int(unit[ZIGZAG[z]])
        if v:
            out.append((z, False))
            if abs(v) >= 512:
                out.append((z, True))
    return out


def arrange(specials, labels, rng, q, shuffle=False):
    """Stream-order units holding every special unit in setting (a) and in setting (b): (units, special, setting, label)."""
    specials = np.asarray(specials, np.int16).reshape(-1, 64)
    order = rng.permutation(len(specials)) if shuffle else np.arange(len(specials))
    specials, labels = specials[order], [labels[i] for i in order]
    n = len(specials)
    a = ordinary(rng, 8 * n, q).reshape(n, 8, 64)
    a[np.arange(n), np.arange(n) % 8] = specials
    sp_a = np.zeros((n, 8), bool)
    sp_a[np.arange(n), np.arange(n) % 8] = True
    lab_a = np.full((n, 8), "", object)
    lab_a[np.arange(n), np.arange(n) % 8] = labels
    pad = (-n) % 8
    b = np.concatenate([specials, specials[:pad]])
    lab_b = list(labels) + list(labels[:pad])
    units = np.concatenate([a.reshape(-1, 64), b])
    special = np.concatenate([sp_a.reshape(-1), np.ones(len(b), bool)])
    setting = np.where(special, np.concatenate([np.full(8 * n, "a", object), np.full(len(b), "b", object)]), "-")
    label = np.concatenate([lab_a.reshape(-1), np.array(lab_b, object)])
    return units, special, setting, label


def pad_rows(parts, rng, q, multiple=BLOCKS_X):
    """Concatenate (units, special, setting, label) parts and fill the last block row with ordinary units."""
    units = np.concatenate([p[0] for p in parts])
    special = np.concatenate([p[1] for p in parts])
    setting = np.concatenate([p[2] for p in parts])
    label = np.concatenate([p[3] for p in parts])
    pad = (-len(units)) % multiple
    if pad:
        units = np.concatenate([units, ordinary(rng, pad, q)])
        special = np.concatenate([special, np.zeros(pad, bool)])
        setting = np.concatenate([setting, np.full(pad, "-", object)])
        label = np.concatenate([label, np.full(pad, "", object)])
    return units, special, setting, label


# ------------------------------------------------------------------------------------------------
# files
# ------------------------------------------------------------------------------------------------

def with_qtables16(data, tables):
    """`data` with every table of its DQT segments rewritten as a 16-bit one (Pq = 1): tables[Tq] uint16 [64] in natural
    order, written in zig-zag order; a table that `tables` does not name keeps its values. The entropy-coded data is untouched, so the coefficients stay what they were."""
    out, i = bytearray(data[:2]), 2
    while i + 4 <= len(data) and data[i] == 0xFF:
        m, ln = data[i + 1], (data[i + 2] << 8) | data[i + 3]
        if m == 0xDB:
            seg, j = bytearray(), i + 4
            while j < i + 2 + ln:
                pq, tq = data[j] >> 4, data[j] & 15
                if tq in tables:
                    t = np.asarray(tables[tq], np.int64).reshape(64)[ZIGZAG]
                else:  # a table the caller does not name keeps its values
                    t = np.frombuffer(data, ">u2" if pq else np.uint8, 64, j + 1).astype(np.int64)
                assert 1 <= t.min() and t.max() <= 65535
                seg.append(0x10 | tq)
                seg += t.astype(">u2").tobytes()
                j += 1 + (128 if pq else 64)
            out += bytes([0xFF, 0xDB, (len(seg) + 2) >> 8, (len(seg) + 2) & 255]) + seg
        else:
            out += data[i:i + 2 + ln]
        i += 2 + ln
        if m == 0xDA:
            break
    return bytes(out + data[i:])


def gray_case(name, parts, q, restart_interval=0, notes=None):
    """A grayscale file of the units in `parts` with quantisation table q (8-bit if it fits, else a 16-bit rewrite)."""
    from tools import jpegsynth

    units, special, setting, label = parts
    q = np.asarray(q, np.int64).reshape(64)
    assert len(units) % BLOCKS_X == 0 and len(units) <= 6400, (name, len(units))
    if q.max() <= 255:
        data = jpegsynth.encode_blocks(units, BLOCKS_X, q.astype(np.uint8), restart_interval)
    else:
        data = with_qtables16(jpegsynth.encode_blocks(units, BLOCKS_X, np.ones(64, np.uint8), restart_interval), {0: q})
    return Case(name, data, [units.reshape(-1, BLOCKS_X, 64)], [q], units, np.zeros(len(units), int), special, setting, label,
                restart_interval, notes=notes)


def column_table(colq, others=None):
    """Quantisation table (natural order) whose column c holds colq[c] in every row; None: the row of `others`."""
    q = np.empty((8, 8), np.int64)
    for c in range(8):
        q[:, c] = colq[c] if colq[c] is not None else others[:, c]
    return q.reshape(64)


# column -> (quantiser, coefficient magnitude): 8-bit factorisations around the bound, and 1,023 * 255. A column at position
# 0 or 4 that wrongly took the 32-bit pass would not show (pass 2 multiplies those by 2^13, and the workspace's error is a
# multiple of 2^21: nothing below bit 32), so the values at and above the first inexact L sit in other columns.
EDGE8_COLUMNS = {0: (254, 129), 1: (151, 217), 2: (128, 256), 3: (99, 331), 4: (254, 129), 5: (128, 256), 6: (99, 331), 7: (255, 1023)}


def q16_columns():
    """The same for the two files with 16-bit tables: coefficient +-1, and +-1,023 for 1,023 * 65,535."""
    first_bad, last_good = pass1_thresholds()
    return ({1: (last_good, 1), 3: (first_bad, 1), 5: (40000, 1), 6: (65535, 1)},
            {0: (32768, 1), 2: (32769, 1), 4: (32767, 1), 7: (65535, 1023)})


@functools.lru_cache(maxsize=1)
def pass1_thresholds():
    """(first L at which a 32-bit pass 1 is inexact on a column of eight inputs of magnitude L with the worst signs, the
    largest L below it): from libjpeg_ref.islow_1d, by trying every L from 32,768 on."""
    L = np.arange(32768, 36000, dtype=np.int64)
    x = [WORST_SIGNS[k] * L for k in range(8)]
    bad = np.zeros(len(L), bool)
    for o in libjpeg_ref.islow_1d(x):
        bad |= pass1_32bit(o) != pass1_exact(o)
    assert bad.any() and not bad[0]
    first = int(L[np.argmax(bad)])
    return first, first - 1


def pass1_exact(out):
    """jidctint.c: DESCALE of a pass-1 output in 64 bits, kept in the int workspace."""
    return int32(descale(out, CONST_BITS - PASS1_BITS))


def pass1_32bit(out):
    """The same in wrapping 32-bit arithmetic, as idct_kernel's 32-bit pass 1 computes it."""
    return int32(int32(out) + (1 << (CONST_BITS - PASS1_BITS - 1))) >> np.int64(CONST_BITS - PASS1_BITS)


def sign_patterns(rng, extra=5):
    """[(name, signs[8])]: the worst pattern, its negative, all plus, and `extra` seeded ones."""
    out = [("worst", WORST_SIGNS), ("-worst", -WORST_SIGNS), ("plus", np.ones(8, int))]
    for k in range(extra):
        out.append(("seeded%d" % k, rng.integers(0, 2, 8) * 2 - 1))
    return out


def among_unit(rng, q, c):
    """An ordinary unit (8 x 8) whose columns other than c are not all empty."""
    u = ordinary(rng, 1, q).reshape(8, 8)
    if not np.delete(u, c, axis=1).any():
        row0 = np.asarray(q, np.int64).reshape(8, 8)[0].copy()
        row0[c] = 1 << 30
        assert row0.min() <= ORDINARY_MAX
        u[0, row0.argmin()] = 1
    return u


def column_specials(rng, q, columns):
    """Units with ONE column of eight coefficients of the same magnitude: columns = {column: (coefficient magnitude,
    what)}; for every sign pattern once in an otherwise empty unit ("lone") and once with ordinary content in the other
    columns ("among")."""
    units, labels = [], []
    for c, (mag, what) in columns.items():
        for pname, signs in sign_patterns(rng):
            for among in (False, True):
                u = among_unit(rng, q, c) if among else np.zeros((8, 8), np.int16)
                u[:, c] = signs * mag
                units.append(u.reshape(64))
                labels.append("%s/%s/col%d/%s" % (what, pname, c, "among" if among else "lone"))
    return units, labels


def pass1_cases():
    """The files that pin the ISLOW transform's pass selection and its 64-bit pass 1."""
    out = []
    # every sign pattern in every column position at L = 32,767 = 151 * 217: the 32-bit pass at its bound
    rng = np.random.default_rng(20261101)
    q = np.full(64, 151)
    u = np.arange(256)
    units = np.zeros((256, 8, 8), np.int16)
    for c in range(8):
        pattern = (u + 32 * c) % 256  # over the 256 units every pattern once per column
        for row in range(8):
            units[:, row, c] = np.where((pattern >> row) & 1, -217, 217)
    out.append(gray_case("pass1_bound", pad_rows([arrange(units.reshape(-1, 64), ["L32767/all-columns/%d" % i for i in u], rng, q)], rng, q), q,
                         notes={"large_columns": 0, "L": {32767}}))
    # 8-bit factorisations around the bound, one per column, and 1,023 * 255
    rng = np.random.default_rng(20261102)
    col = EDGE8_COLUMNS
    q = column_table([col[c][0] for c in range(8)])
    units, labels = column_specials(rng, q, {c: (m, "L%d" % (f * m)) for c, (f, m) in col.items()})
    n_large = sum(16 for f, m in col.values() if f * m > ISLOW_PASS1_MAX)
    # L = 32,768 in ONE row of a column whose other rows are small
    for c in (2, 5):
        for row in range(8):
            for among in (False, True):
                x = among_unit(rng, q, c) if among else np.zeros((8, 8), np.int16)
                x[:, c] = rng.integers(0, 2, 8) * 2 - 1
                x[row, c] = 256 if (row + c) & 1 else -256
                units.append(x.reshape(64))
                labels.append("L32768/one-row%d/col%d/%s" % (row, c, "among" if among else "lone"))
                n_large += 1
    out.append(gray_case("pass1_edge8", pad_rows([arrange(units, labels, rng, q)], rng, q), q,
                         notes={"large_columns": 2 * n_large, "L": {f * m for f, m in col.values()}}))
    # 16-bit tables, coefficient +-1 (and +-1,023 for 1,023 * 65,535) in four columns; the others keep small quantisers
    for name, seed, cols in (("pass1_q16a", 20261103, q16_columns()[0]), ("pass1_q16b", 20261104, q16_columns()[1])):
        rng = np.random.default_rng(seed)
        small = rng.integers(1, 17, (8, 8))
        q = column_table([cols[c][0] if c in cols else None for c in range(8)], small)
        units, labels = column_specials(rng, q, {c: (m, "L%d" % (f * m)) for c, (f, m) in cols.items()})
        n_large = sum(16 for f, m in cols.values() if f * m > ISLOW_PASS1_MAX)
        out.append(gray_case(name, pad_rows([arrange(units, labels, rng, q)], rng, q), q,
                             notes={"large_columns": 2 * n_large, "L": {f * m for f, m in cols.values()}}))
    # a DC ramp to +32,767 and -32,768 in steps of at most 2,047 with a 16-bit quantiser of 65,535: DC * 65,535 * 4 does not
    # fit the int workspace of pass 1. Every unit is special here (a unit's DC follows from its neighbour's).
    rng = np.random.default_rng(20261105)
    dc, v = [], 0
    for target in (32767, -32768, 0):
        while v != target:
            step = int(rng.integers(1, 2048))
            v = min(v + step, target) if target > v else max(v - step, target)
            dc.append(v)
    q = rng.integers(1, 17, 64)
    q[0] = 65535
    units = ordinary(rng, len(dc), q)
    units[::3, 1:] = 0  # a third of them DC only
    units[:, 0] = dc
    n = len(units)
    parts = pad_rows([(units, np.ones(n, bool), np.full(n, "b", object), np.array(["dc-ramp/%d" % d for d in dc], object))], rng, q)
    parts[0][n:, 0] = 0  # (the padding's DC: the table's clip already made it so)
    out.append(gray_case("pass1_dcramp", parts, q, notes={"large_columns": n - sum(1 for d in dc if abs(d * 65535) <= ISLOW_PASS1_MAX), "L": set()}))
    return out


def count_ladder(rng):
    """Units of exactly n entries without an escape, n = 1..64, on the first and on the last n - 1 zig-zag positions; and a
    one-hot unit for every zig-zag position and both signs."""
    units, labels = [], []
    for n in range(1, 65):
        for where in ("first", "last"):
            zz = np.zeros(64, np.int64)
            pos = np.arange(1, n) if where == "first" else np.arange(64 - (n - 1), 64)
            zz[pos] = rng.integers(1, 41, len(pos)) * (rng.integers(0, 2, len(pos)) * 2 - 1)
            zz[0] = rng.integers(-200, 201)
            units.append(natural(zz[None, :])[0])
            labels.append("count%d/%s" % (n, where))
    for z in range(64):
        for sign in (1, -1):
            zz = np.zeros(64, np.int64)
            zz[z] = sign * int(rng.integers(1, 512))
            units.append(natural(zz[None, :])[0])
            labels.append("one-hot/zz%d/%+d" % (z, sign))
    return units, labels


ESCAPE_ENTRIES = (8, 9, 16, 17)  # the ends of idct_scaled_kernel's groups of eight loads (and the ninth, look-ahead, load)


def escape_ladder(rng):
    """Units with escaped coefficients (|value| >= 512): 1 to 63 of them and nothing else (3 to 127 entries); an escape at
    zig-zag position 1 and at 63; an escape as entry 8, 9, 16 and 17 of the unit, as the unit's last entry and with
    entries behind it; an escaped one-hot unit for every AC position and both signs."""
    big = lambda k: rng.integers(512, 1024, k) * (rng.integers(0, 2, k) * 2 - 1)
    small = lambda k: rng.integers(1, 41, k) * (rng.integers(0, 2, k) * 2 - 1)
    units, labels = [], []
    for k in range(1, 64):
        zz = np.zeros(64, np.int64)
        pos = np.sort(rng.choice(np.arange(1, 64), k, replace=False)) if k < 63 else np.arange(1, 64)
        zz[pos] = big(k)
        zz[0] = rng.integers(-200, 201)
        units.append(natural(zz[None, :])[0])
        labels.append("escapes%d" % k)
    for e in ESCAPE_ENTRIES:  # entries: DC, e - 2 plain ones, the coefficient (entry e - 1), its escape (entry e)
        for tail in (0, 3):
            for spread in (False, True):
                zz = np.zeros(64, np.int64)
                pos = np.arange(1, e + tail) if not spread else np.sort(rng.choice(np.arange(1, 64), e - 1 + tail, replace=False))
                zz[pos] = small(len(pos))
                zz[pos[e - 2]] = big(1)[0]
                zz[0] = rng.integers(-200, 201)
                units.append(natural(zz[None, :])[0])
                labels.append("escape-entry%d/%s/%s" % (e, "last" if tail == 0 else "inner", "spread" if spread else "packed"))
    for z, what in ((1, "zz1"), (63, "zz63")):
        for plain in (0, 5):
            zz = np.zeros(64, np.int64)
            others = np.setdiff1d(np.arange(1, 64), [z])
            zz[rng.choice(others, plain, replace=False)] = small(plain)
            zz[z] = big(1)[0]
            units.append(natural(zz[None, :])[0])
            labels.append("escape-at/%s/plain%d" % (what, plain))
    for z in range(64):
        for sign in (1, -1):
            zz = np.zeros(64, np.int64)
            zz[z] = sign * int(rng.integers(512, 1024))
            units.append(natural(zz[None, :])[0])
            labels.append("one-hot-escaped/zz%d/%+d" % (z, sign))
    return units, labels


COUNTS_Q = np.clip(np.arange(64).reshape(8, 8).T // 5 + 2, 1, 13).reshape(64)  # a photo-like table: 1,023 * 13 < 32,768


def count_edge_units(units, labels):
    """Two more parts for the file of the plain ladder, from the ladder's own units. The units above 32 entries in the
    ladder's order: groups in which NO unit is covered by the words idct_kernel prefetches (setting (b); the shuffled
    ladder has none). And the units of 29 to 34 entries sixteen times each behind a short unit of 1, 2, 3 or 4 entries:
    where units are packed into a region, the short unit in front decides the parity of the long one's first entry
    (a unit of that length nearly fills a region of the smallest subsequence size, so little else stands in front)."""
    count = entry_count(np.asarray(units))
    long_ones = [i for i in range(len(units)) if count[i] > 32 and labels[i].startswith("count")]  # 33..64 entries: 64 units
    assert len(long_ones) % 8 == 0
    part = [(np.asarray([units[i] for i in long_ones], np.int16), np.ones(len(long_ones), bool), np.full(len(long_ones), "b", object),
             np.array([labels[i] for i in long_ones], object))]
    pairs, pair_labels, pair_special = [], [], []
    for n in range(29, 35):
        for rep in range(16):
            short = np.zeros(64, np.int16)
            short[0] = 5 * rep - 40
            short[ZIGZAG[1:1 + rep % 4]] = 1 + rep
            pairs += [short, units[2 * (n - 1) + (rep >> 2 & 1)]]
            pair_labels += ["", "parity/count%d/behind%d" % (n, 1 + rep % 4)]
            pair_special += [False, True]
    part.append((np.asarray(pairs, np.int16), np.array(pair_special), np.full(len(pairs), "-", object), np.array(pair_labels, object)))
    return tuple(np.concatenate([p[k] for p in part]) for k in range(4))


def escape_end_units(units, labels):
    """One more part for the file of the escape ladder: the units that hold an escape and END in a plain entry, each in front
    of a DC-only unit whose DC value has an index field (its low six bits) of 0 -- what a gather that looked for an escape
    behind a unit's last entry would take for one."""
    pairs, pair_labels, pair_special = [], [], []
    ends_plain = [i for i in range(len(units)) if labels[i].startswith(("escape-entry", "escape-at")) and not entries_of(units[i])[-1][1]]
    assert len(ends_plain) >= 8
    for k, i in enumerate(ends_plain * 2):
        follower = np.zeros(64, np.int16)
        follower[0] = (0, 64, -64, 128, -192, 320)[k % 6]
        pairs += [units[i], follower]
        pair_labels += ["escape-then-plain-end/" + labels[i], ""]
        pair_special += [True, False]
    return np.asarray(pairs, np.int16), np.array(pair_special), np.full(len(pairs), "-", object), np.array(pair_labels, object)


def counts_cases():
    """The ladders, each encoded as built and once more (in another seeded order) behind a single one-entry unit, with
    restart interval 0 (units packed into the regions of the symbol stream) and 1 (every unit starts a region)."""
    out = []
    for kind, ladder, seed in (("plain", count_ladder, 20261111), ("escape", escape_ladder, 20261112)):
        for ri, suffix in ((0, "packed"), (1, "restart")):
            rng = np.random.default_rng(seed)
            units, labels = ladder(rng)
            first = arrange(units, labels, rng, COUNTS_Q, shuffle=True)
            again = arrange(units, labels, rng, COUNTS_Q, shuffle=True)
            again = (again[0], again[1], np.where(again[1], "-", again[2]), again[3])  # behind the flip unit no group is aligned
            flip = (np.zeros((1, 64), np.int16), np.zeros(1, bool), np.full(1, "-", object), np.full(1, "flip", object))
            parts = [first, count_edge_units(units, labels) if kind == "plain" else escape_end_units(units, labels), flip, again]
            out.append(gray_case("counts_%s_%s" % (kind, suffix), pad_rows(parts, rng, COUNTS_Q), COUNTS_Q, ri))
    return out


LIMIT_EDGES = (-513, -512, -385, -384, -129, -128, 127, 128, 383, 384, 511, 512, -1024, 1023)


def limit_cases():
    """DC-only units with q[0] = 8 and every DC value -1024..1023: the value in front of the range limit is the DC value
    in every transform. Once more with a faint AC term (+-1 * 1 at zig-zag position 1 or 2), which no DC-only shortcut
    covers. Every unit of the sweep is special (setting (b)); the values at the range limit's edges are also held in
    setting (a)."""
    out = []
    for name, faint, seed in (("limit_dc", False, 20261121), ("limit_ac", True, 20261122)):
        rng = np.random.default_rng(seed)
        q = rng.integers(1, 9, 64)
        q[0], q[1], q[8] = 8, 1, 1
        sweep = np.zeros((2048, 64), np.int16)
        sweep[:, 0] = np.arange(-1024, 1024)
        if faint:
            sweep[np.arange(2048), np.where(np.arange(2048) & 2, 1, 8)] = np.where(np.arange(2048) & 1, 1, -1)
        labels = ["dc%d" % d for d in range(-1024, 1024)]
        edges = [i for i, d in enumerate(range(-1024, 1024)) if d in LIMIT_EDGES]
        a = arrange(sweep[edges], [labels[i] for i in edges], rng, q)
        keep = a[2] != "b"  # setting (b) is the sweep itself
        a = tuple(x[keep] for x in a)
        b = (sweep, np.ones(2048, bool), np.full(2048, "b", object), np.array(labels, object))
        out.append(gray_case(name, pad_rows([a, b], rng, q), q))
    return out


def kats16_cases():
    """The eight coefficient groups of tests/golden/idct_kats.npz with seeded 16-bit quantisers 1..65,535."""
    z = np.load(os.path.join(GOLDEN, "idct_kats.npz"))
    out = []
    for k, g in enumerate(sorted({f.split("/")[0] for f in z.files if "/" in f})):
        rng = np.random.default_rng(20261130 + k)
        q = rng.integers(1, 65536, 64)
        q[rng.integers(0, 64, 6)] = (1, 255, 256, 32767, 32768, 65535)
        coef = z[g + "/coef"].astype(np.int16)
        n = len(coef)
        parts = pad_rows([(coef, np.ones(n, bool), np.full(n, "b", object), np.full(n, g, object))], rng, q)
        out.append(gray_case("kats16_" + g, parts, q))
    return out


def ycc420_cases():
    """A 4:2:0 file whose luma AND chroma blocks are drawn from the special units of the files above, so that every size
    class of libjpeg's scale mode receives them (luma 4x4 / 2x2 / 1x1, chroma 8x8 ISLOW / 4x4 / 2x2 at 1/2, 1/4, 1/8), and
    a variant with 16-bit tables. Groups of eight stream-consecutive units cycle through settings (a), (b) and all
    ordinary (so that some MCUs hold no special unit)."""
    from tests.syncprobe import syncprobe
    from tools import jpegsynth

    out = []
    mx, my = 32, 20
    n = 6 * mx * my
    comp_of_k = np.array([0, 0, 0, 0, 1, 2])
    for name, seed in (("ycc420", 20261141), ("ycc420_q16", 20261142)):
        rng = np.random.default_rng(seed)
        if name == "ycc420":
            edge = EDGE8_COLUMNS
            qt = [np.where(np.arange(64) == 0, 8, COUNTS_Q), column_table([edge[c][0] for c in range(8)]), np.full(64, 151)]
        else:
            small = rng.integers(1, 17, (8, 8))
            ca, cb = q16_columns()
            edge = None
            qt = [column_table([ca[c][0] if c in ca else None for c in range(8)], small),
                  column_table([cb[c][0] if c in cb else None for c in range(8)], small), rng.integers(1, 65536, 64)]
        pools = []
        for c in range(3):
            units, labels = [], []
            u, l = count_ladder(rng)
            units += u[56:72] + u[128::9]  # counts 29..36 and some one-hot units
            labels += l[56:72] + l[128::9]
            u, l = escape_ladder(rng)
            units += u[::7] + u[63:63 + 16]
            labels += l[::7] + l[63:63 + 16]
            for d in LIMIT_EDGES:
                x = np.zeros(64, np.int16)
                x[0] = d
                units.append(x)
                labels.append("dc%d" % d)
            if name == "ycc420" and c == 1:
                u, l = column_specials(rng, qt[c], {k: (m, "L%d" % (f * m)) for k, (f, m) in edge.items()})
            elif name == "ycc420" and c == 2:
                u = [np.where(rng.integers(0, 2, 64) > 0, 217, -217).astype(np.int16) for _ in range(16)]
                l = ["L32767/all-columns"] * 16
            elif name == "ycc420_q16" and c < 2:
                cols = (ca, cb)[c]
                u, l = column_specials(rng, qt[c], {k: (m, "L%d" % (f * m)) for k, (f, m) in cols.items()})
            else:
                u, l = [], []
            pools.append((np.array(units + list(u), np.int16), labels + list(l)))
        stream = np.zeros((n, 64), np.int16)
        comp = np.tile(comp_of_k, n // 6)
        for c in range(3):
            stream[comp == c] = ordinary(rng, int((comp == c).sum()), qt[c])
        special = np.zeros(n, bool)
        setting = np.full(n, "-", object)
        label = np.full(n, "", object)
        cycle = "aaabaaoo"
        taken = [0, 0, 0]
        for g in range(n // 8):
            kind = cycle[g % len(cycle)]
            slots = [8 * g + (g // len(cycle)) % 8] if kind == "a" else list(range(8 * g, 8 * g + 8)) if kind == "b" else []
            for s in slots:
                if 8 <= (s // 6) // mx <= 12 and 12 <= (s // 6) % mx <= 17:
                    continue  # a rectangle of 5 x 6 MCUs stays ordinary: room for a cropped window without special units
                c = comp[s]
                units, labels = pools[c]
                i = taken[c] % len(units)
                taken[c] += 1
                stream[s], special[s], setting[s], label[s] = units[i], True, kind, labels[i]
        s = stream.reshape(my, mx, 6, 64)
        luma = s[:, :, :4].reshape(my, mx, 2, 2, 64).transpose(0, 2, 1, 3, 4).reshape(2 * my, 2 * mx, 64)
        blocks = [np.ascontiguousarray(luma), np.ascontiguousarray(s[:, :, 4]), np.ascontiguousarray(s[:, :, 5])]
        # tables fitted to the file's own blocks (encode_blocks writes grayscale files only, so its tables are taken from
        # the file it writes); DC-only units behind them ask for every DC category 0..11, whatever the order of the units
        ask = np.zeros((BLOCKS_X, 64), np.int16)
        ask[1:23:2, 0] = [1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1023]
        ask[23, 0] = -1024
        fitted = syncprobe.dht_tables(jpegsynth.encode_blocks(np.concatenate([stream, ask]), BLOCKS_X, np.ones(64, np.uint8), optimize=True))
        dc = [(b, v) for tc, _, b, v in fitted if tc == 0]
        ac = [(b, v) for tc, _, b, v in fitted if tc == 1]
        eight = all(int(t.max()) <= 255 for t in qt)
        data = jpegsynth.encode_custom(16 * mx, 16 * my, S420, blocks, dc, ac, tables=[(0, 0)] * 3,
                                       qtables=[t.astype(np.uint8) for t in qt] if eight else [np.ones(64, np.uint8)] * 3)
        if not eight:
            data = with_qtables16(data, {k: qt[k] for k in range(3)})
        out.append(Case(name, data, blocks, qt, stream, comp, special, setting, label, 0, S420))
    return out


@functools.lru_cache(maxsize=1)
def corpus():
    """name -> Case, every file of the corpus."""
    cases = pass1_cases() + counts_cases() + limit_cases() + ycc420_cases() + kats16_cases()
    out = {c.name: c for c in cases}
    assert len(out) == len(cases)
    return out


# ------------------------------------------------------------------------------------------------
# where the write pass puts a packed file's units (for choosing the ladder's order; the GPU test reads the real table)
# ------------------------------------------------------------------------------------------------

def _code_sizes(bits, vals):
    size, k = {}, 0
    for length in range(1, 17):
        for _ in range(int(bits[length - 1])):
            size[int(vals[k])] = length
            k += 1
    return size


def _category(v):
    return int(abs(int(v))).bit_length()


def predicted_first_entries(case, subseq_bytes):
    """Model of the data-unit table of a grayscale file without restart markers: (region, index of the first entry in
    the region) per unit. A subsequence's region takes the units whose DC symbol ENDS in the subsequence (jg_defs.h), one
    behind the other."""
    from tests.syncprobe import syncprobe

    assert case.gray and case.restart_interval == 0
    tabs = syncprobe.dht_tables(case.data)
    dc = _code_sizes(*[(b, v) for tc, _, b, v in tabs if tc == 0][0])
    ac = _code_sizes(*[(b, v) for tc, _, b, v in tabs if tc == 1][0])
    bits_per = 8 * subseq_bytes
    pos, pred = 0, 0
    region = np.zeros(len(case.stream), np.int64)
    for i, unit in enumerate(case.stream):
        s = _category(int(unit[0]) - pred)
        pred = int(unit[0])
        pos += dc[s] + s
        region[i] = (pos + bits_per - 1) // bits_per - 1
        run = 0
        for z in range(1, 64):
            v = int(unit[ZIGZAG[z]])
            if v == 0:
                run += 1
                continue
            while run > 15:
                pos += ac[0xF0]
                run -= 16
            s = _category(v)
            pos += ac[run << 4 | s] + s
            run = 0
        if run:
            pos += ac[0]
    cnt = entry_count(case.stream)
    first = np.zeros(len(cnt), np.int64)
    for i in range(1, len(cnt)):
        first[i] = first[i - 1] + cnt[i - 1] if region[i] == region[i - 1] else 0
    return region, first
