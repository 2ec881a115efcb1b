"""Markers and stuffing at every lane, wave and window boundary of the byte grid (plain module: no GPU, no Pillow).

The grid. The device-side marker scan (jg_front.hip) and destuff_kernel (jg_kernels.hip) classify the entropy-coded bytes
on a fixed grid: a lane owns 16 bytes, a wave 1024, a workgroup one 4096-byte window (kDestuffWin). The grid starts at

    xfer_begin = (scan_begin - 1) & ~15        (jg_reader.cpp, read_sos; scan_begin: the first entropy-coded byte)

so `grid_offset(data, file_pos) = file_pos - xfer_begin`, and the scan's first byte lies at offset 1..16. A longer header
(`pad` payload bytes of a COM segment in front of SOS) therefore moves the scan's bytes against the grid only modulo 16.
Fill bytes move them against the wave and window grids: any number of FF in front of a restart marker is legal (T.81
B.1.1.2), and everything behind them moves by that many bytes without a pixel changing.

`placements(base)` puts one instance of every pattern at every position of every grid -- a CELL, named
"pattern/grid/position[/zone]":

    pattern     rst           restart marker FF Dn
                stuffed       stuffed pair FF 00
                stuffed_rst   a stuffed pair directly behind a restart marker (FF Dn FF 00: the pair is placed)
                eoi           end of image FF D9
                fill_rst      fill + marker FF FF Dn, a fill of exactly one byte
    grid        16, 1024, 4096
    position    of the pattern's first byte: straddle (B - 1), starts (0), ends (B - 2); fill_rst: b1 (B - 1), b2 (B - 2),
                b3 (B - 3), b0 (0)
    zone        rst on the 4096 grid only: near (the pattern lies in windows 0..3) and far (beyond window 8)

and "lead/<pad>" for pad 0..15: the scan's first byte at each of the grid offsets 1..16 (`lead` in classify()). For a cell
the instance is taken that needs the fewest fill bytes (then the earliest one, then the smallest pad); the fill goes in
front of the marker two markers ahead of the pattern, so the pattern's neighbourhood stays as encoded.

Where the two walks differ by design. The host walk ends a segment's byte range at the FIRST FF of a fill run
(walk_scan: emit(chunk_begin, qo)), the device at the LAST, the FF in front of the marker code (classify: mark = F & ~(NF |
NZ); front_plan: b1 = mk_pos[k]). Fill bytes are no data, so both destuff the same bytes; but of a segment's last chunk
`end` lies `fill` bytes further on the device, and the device's chunk list has one more chunk for every fill byte that
lies on a window's first byte (`extra_device_chunks`): the windows the fill run enters, counted from the byte in front of
it. Those chunks hold no data byte. The tail parts differ as well: the host cuts in front of a segment that starts 960
subsequences or more behind the last cut, the device in front of one whose first subsequence opens a new block of 960
(`tail_parts_host`, `tail_parts_device`); a part is a run of whole segments either way.
"""
import functools

import numpy as np

from tests import cases
from tools import jpegsynth

WIN = 4096
GRIDS = (16, 1024, WIN)
POSITIONS = {"straddle": -1, "starts": 0, "ends": -2}
FILL_POSITIONS = {"b1": -1, "b2": -2, "b3": -3, "b0": 0}
LONG_FILLS = (4095, 4096, 4113, 9000)
TAIL_PART_SUBSEQ = 960  # kTailPartSubseq (jg_defs.h)
COM_HEADER = 4


def base_files():
    """name -> bytes. A: 4:2:0 with restart markers, long codes and much stuffing, 18 windows. B: grey, one MCU per segment,
    almost empty blocks: several markers in one lane's 16 bytes, more segments than front_plan has lanes. C: A without
    restart markers (header pads only)."""
    e = jpegsynth.encode
    return {
        "A": e(256, 192, cases.S420, restart_interval=3, quality=100, noise=40, seed=77),
        "B": e(1024, 768, ((1, 1),), restart_interval=1, quality=5, noise=0, seed=78),
        "C": e(256, 192, cases.S420, restart_interval=0, quality=100, noise=40, seed=77),
    }


class Parsed:
    """What a sequential walk finds in a single-scan file: `sos` (its FF), `begin` (first entropy-coded byte), `rst`
    [(first FF of the fill run or of the marker, the marker's own FF)], `stuffed` [FF of each FF 00], `bad` [second FF of
    each FF FF 00], `end` (the terminating marker: first FF, own FF; None if the file has none)."""


def parse(data):
    p = Parsed()
    i = 2
    while data[i + 1] != 0xDA:  # marker segments in front of SOS
        assert data[i] == 0xFF
        i += 2 + int.from_bytes(data[i + 2:i + 4], "big")
    p.sos = i
    p.begin = i + 2 + int.from_bytes(data[i + 2:i + 4], "big")
    a = np.frombuffer(data, np.uint8)
    p.rst, p.stuffed, p.bad, p.end = [], [], [], None
    ff = np.flatnonzero(a[p.begin:] == 0xFF) + p.begin
    k, n = 0, len(ff)
    while k < n:
        i = j = int(ff[k])
        while j + 1 < len(data) and data[j + 1] == 0xFF:
            j += 1
        k += j - i + 1
        if j + 1 >= len(data):
            break
        code = data[j + 1]
        if code == 0:
            if j > i:
                p.bad.append(j)
            else:
                p.stuffed.append(i)
        elif 0xD0 <= code <= 0xD7:
            p.rst.append((i, j))
        else:
            p.end = (i, j)
            break
    return p


def variant(base, pad, fills):
    """`base` with a COM segment of `pad` payload bytes in front of SOS and fills[i] extra FF in front of restart marker i
    (in front of its fill run, if it has one). `fills`: {marker index: count}."""
    p = parse(base)
    out = [base[:p.sos], b"\xff\xfe" + (2 + pad).to_bytes(2, "big") + b"\x20" * pad]
    at = p.sos
    for i in sorted(fills):
        q = p.rst[i][0]
        out += [base[at:q], b"\xff" * fills[i]]
        at = q
    out.append(base[at:])
    return b"".join(out)


def moved(base_parsed, pad, fills, pos):
    """Where byte `pos` of the base lies in variant(base, pad, fills); a fill inserted AT `pos` lies behind the result."""
    return pos + COM_HEADER + pad + sum(n for i, n in fills.items() if base_parsed.rst[i][0] < pos)


def xfer_begin(data):
    return (parse(data).begin - 1) & ~15


def grid_offset(data, file_pos):
    """Offset of byte `file_pos` on the grid of the kernels (module docstring)."""
    return file_pos - xfer_begin(data)


class Case:
    """One variant: `cell`, `base` (name), `pad`, `fills`, `data`; `pos` the file position of the pattern's first byte in
    `data`, `grid` and `want` (its offset modulo the grid), `kind` (what lies there), `fill` (length of the fill run that
    moves it, 0 if the header pad was enough)."""

    def __init__(self, cell, base, base_bytes, pad, fills, pos=None, grid=None, want=None, kind=None, fill=0):
        self.cell, self.base, self.pad, self.fills = cell, base, pad, dict(fills)
        self.data = variant(base_bytes, pad, fills)
        self.pos, self.grid, self.want, self.kind, self.fill = pos, grid, want, kind, fill

    def __repr__(self):
        return "%s:%s" % (self.base, self.cell)


def _solve(p, inst, grid, target, zone=None):
    """The instance (index into `inst`: (position of the pattern's first byte in the base, markers in front of it)), pad and
    fill with the fewest fill bytes that put the pattern's first byte at `target` modulo `grid`. The fill goes in front of
    marker (markers in front) - 2; an instance with fewer than two markers in front of it is moved by the pad alone.
    Returns (instance index, pad, fill) or None."""
    if not inst:
        return None
    rel = np.array([q - p.begin for q, _ in inst], np.int64)[:, None]
    ahead = np.array([m for _, m in inst], np.int64)[:, None]
    pads = np.arange(16, dtype=np.int64)[None, :]
    lead = ((p.begin + COM_HEADER + pads - 1) & 15) + 1  # grid offset of the scan's first byte
    fill = (target - rel - lead) % grid
    ok = (fill == 0) | (ahead >= 2)
    off = rel + lead + fill
    if zone == "near":
        ok &= off // WIN < 4
    elif zone == "far":
        # more fill moves a pattern on by whole windows, but a cell takes what the file has beyond window 8
        ok &= off // WIN > 8
    if not ok.any():
        return None
    cost = np.where(ok, fill, 1 << 40)
    k = int(np.argmin(cost))  # row-major: fewest fill bytes, then the earliest instance, then the smallest pad
    i, pad = divmod(k, 16)
    return i, pad, int(fill[i, pad])


def cells(with_lead=True):
    """Every cell name, in order."""
    out = []
    for pat in ("rst", "stuffed", "stuffed_rst", "eoi"):
        for g in GRIDS:
            for pos in POSITIONS:
                if pat == "rst" and g == WIN:
                    out += ["%s/%d/%s/%s" % (pat, g, pos, z) for z in ("near", "far")]
                else:
                    out.append("%s/%d/%s" % (pat, g, pos))
    out += ["fill_rst/%d/%s" % (g, pos) for g in GRIDS for pos in FILL_POSITIONS]
    if with_lead:
        out += ["lead/%d" % pad for pad in range(16)]
    return out


# cells that cannot exist: no restart marker of A is followed by a stuffed pair, and B's blocks are almost empty, so its
# scan holds no stuffed pair at all
IMPOSSIBLE = {
    "A": [c for c in cells() if c.startswith("stuffed_rst/")],
    "B": [c for c in cells() if c.startswith("stuffed")],
}


def _instances(p, pat):
    firsts = np.array([q for q, _ in p.rst], np.int64)
    ahead = lambda pos: int(np.searchsorted(firsts, pos))  # markers that begin in front of `pos`
    if pat in ("rst", "fill_rst"):
        return [(j if pat == "rst" else q, m) for m, (q, j) in enumerate(p.rst)]
    if pat == "stuffed":
        return [(s, ahead(s)) for s in p.stuffed]
    if pat == "stuffed_rst":
        behind = {j + 2 for _, j in p.rst}
        return [(s, ahead(s)) for s in p.stuffed if s in behind]
    if pat == "eoi":
        return [(p.end[1], len(p.rst))] if p.end is not None else []
    raise ValueError(pat)


def placements(name, base):
    """(cases, skipped): a Case for every cell of cells() that `base` can fill, and the names of those it cannot."""
    p = parse(base)
    assert not p.bad and p.end is not None and all(q == j for q, j in p.rst), "base files carry no fill bytes"
    out, skipped = [], []
    for cell in cells(with_lead=False):
        parts = cell.split("/")
        pat, grid, posname = parts[0], int(parts[1]), parts[2]
        zone = parts[3] if len(parts) > 3 else None
        target = (FILL_POSITIONS if pat == "fill_rst" else POSITIONS)[posname] % grid
        inst = _instances(p, pat)
        got = _solve(p, inst, grid, target, zone)
        if got is None:
            skipped.append(cell)
            continue
        i, pad, fill = got
        pos, ahead = inst[i]
        fills = {ahead - 2: fill} if fill else {}
        if pat == "fill_rst":
            fills[ahead] = 1  # `ahead` is the marker's own index: its fill byte is the pattern's first byte
        out.append(Case(cell, name, base, pad, fills, moved(p, pad, fills, pos), grid, target, pat, fill))
    return out + header_pads(name, base), skipped


def header_pads(name, base):
    """The sixteen header pads alone (file C: a scan without restart markers takes no fill)."""
    p = parse(base)
    return [Case("lead/%d" % pad, name, base, pad, {}, p.begin + COM_HEADER + pad, 16, ((p.begin + COM_HEADER + pad - 1) & 15) + 1, "lead")
            for pad in range(16)]


def long_fills(name, base):
    """Runs of 4095, 4096, 4113 and 9000 FF in front of one marker: a window, or two, holds nothing but FF."""
    p = parse(base)
    m = len(p.rst) // 3
    return [Case("long_fill/%d" % n, name, base, n % 16, {m: n}, moved(p, n % 16, {}, p.rst[m][0]), None, None, "long_fill", n) for n in LONG_FILLS]


def kind_at(data, pos):
    """What a fresh walk of `data` finds at file position `pos` (the first byte of a pattern), for the tests' cross-check."""
    p = parse(data)
    out = set()
    if pos == p.begin:
        out.add("lead")
    for q, j in p.rst:
        if pos == j and q == j:
            out.add("rst")
        if pos == q and j == q + 1:
            out.add("fill_rst")
        if pos == q and j > q + 1:
            out.add("long_fill")
    if pos in p.stuffed:
        out.add("stuffed")
        if any(j + 2 == pos for _, j in p.rst):
            out.add("stuffed_rst")
    if p.end is not None and pos == p.end[1] and data[pos + 1] == 0xD9:
        out.add("eoi")
    if pos in [j - 1 for j in p.bad]:
        out.add("ffff00")
    return out


def fill_runs(data):
    """[(first FF, the marker's own FF)] of every restart marker, by segment: the fill run of segment k's closing marker is
    [first, own)."""
    return parse(data).rst


def extra_device_chunks(data):
    """Chunks the device's work list has beyond the host's: one for every fill byte on a window's first byte (module
    docstring)."""
    xb = xfer_begin(data)
    return sum(len(range(q - xb + (-(q - xb)) % WIN, j - xb, WIN)) for q, j in parse(data).rst)


def tail_parts_host(seg_offsets):
    """Number of tail parts walk_scan cuts for segments that start at these subsequences."""
    cuts = [0]
    for o in seg_offsets:
        if o - cuts[-1] >= TAIL_PART_SUBSEQ:
            cuts.append(int(o))
    return len(cuts)


def tail_parts_device(seg_offsets):
    """Number of tail parts front_plan cuts for the same segments."""
    o = np.asarray(seg_offsets, np.int64) // TAIL_PART_SUBSEQ
    return 1 + int(np.count_nonzero(o[1:] != o[:-1]))


class Refusal:
    """A file both walks must refuse (`accepted`: one they must take, equal to the base), with the grid position it was
    built for: the first byte of its pattern lies at `want` modulo `grid`."""

    def __init__(self, name, data, accepted=False, pos=None, grid=None, want=None):
        self.name, self.data, self.accepted, self.pos, self.grid, self.want = name, data, accepted, pos, grid, want

    def __repr__(self):
        return self.name


def refusals(name, base):
    """FF FF 00 inside the scan with its first FF on the last and on the last but one byte of a lane, a wave and a window; the
    same three bytes behind EOI, which is legal; a file cut behind an FF that is a window's last byte; two restart markers
    back to back across a window edge (cases.empty_segment_case, shifted: the segment count still matches the geometry)."""
    p = parse(base)
    out = []
    rst_inst = _instances(p, "rst")
    for grid in GRIDS:
        for posname, target in (("b1", grid - 1), ("b2", grid - 2)):
            i, pad, fill = _solve(p, rst_inst, grid, target)
            pos, m = rst_inst[i]
            fills = {m - 2: fill} if fill else {}
            v = variant(base, pad, fills)
            at = moved(p, pad, fills, pos)
            out.append(Refusal("ffff00/%d/%s" % (grid, posname), v[:at] + b"\xff\xff\x00" + v[at:], False, at, grid, target))
    # behind the end of the image, from a window's first byte on: not the scan's business
    i, pad, fill = _solve(p, _instances(p, "eoi"), WIN, WIN - 2)
    fills = {len(p.rst) - 2: fill}
    v = variant(base, pad, fills)
    assert v[-2:] == b"\xff\xd9"
    out.append(Refusal("ffff00_behind_eoi", v + b"\xff\xff\x00" + bytes(100), True, len(v), WIN, 0))
    # the file ends with the FF of a restart marker, a window's last byte
    i, pad, fill = _solve(p, rst_inst, WIN, WIN - 1)
    pos, m = rst_inst[i]
    fills = {m - 2: fill} if fill else {}
    at = moved(p, pad, fills, pos)
    out.append(Refusal("cut_behind_ff", variant(base, pad, fills)[:at + 1], False, at, WIN, WIN - 1))
    # marker a taken out and put back right behind marker a + 1: FF Db FF Da, an empty segment
    a = len(p.rst) // 2
    (qa, _), (qb, _) = p.rst[a], p.rst[a + 1]
    empty = base[:qa] + base[qa + 2:qb + 2] + base[qa:qa + 2] + base[qb + 2:]
    pe = parse(empty)
    assert len(pe.rst) == len(p.rst) and pe.rst[a + 1][0] == pe.rst[a][0] + 2
    for posname, target in (("b1", WIN - 1), ("b2", WIN - 2), ("b3", WIN - 3)):
        i, pad, fill = _solve(pe, [(pe.rst[a][0], a)], WIN, target)
        fills = {a - 2: fill} if fill else {}
        out.append(Refusal("empty_segment/%s" % posname, variant(empty, pad, fills), False, moved(pe, pad, fills, pe.rst[a][0]), WIN, target))
    return out


def cells_hit(data):
    """The wave- and window-grid cells that the patterns of `data` lie on as they are (file C: its stuffed pairs meet those
    edges where the seed puts them)."""
    p = parse(data)
    xb = (p.begin - 1) & ~15
    hit = set()
    for pat, where in (("rst", [j for q, j in p.rst if q == j]), ("stuffed", p.stuffed), ("eoi", [p.end[1]] if p.end else [])):
        for g in GRIDS[1:]:
            for posname, t in POSITIONS.items():
                if any((w - xb) % g == t % g for w in where):
                    hit.add("%s/%d/%s" % (pat, g, posname))
    return hit


# what the sixteen header pads of file C reach on the wave and window grids (tests/test_marker_align_ref.py recomputes it)
C_CELLS = ("stuffed/1024/ends", "stuffed/1024/starts", "stuffed/1024/straddle", "stuffed/4096/ends", "stuffed/4096/starts",
           "stuffed/4096/straddle")


@functools.lru_cache(maxsize=None)
def everything():
    """All of the above, built once per process: {"bases", "cases": {name: [Case]}, "skipped": {name: [cell]}, "long":
    {name: [Case]}, "refusals": [Refusal], "crops": [(Case, rect)]}. Read-only."""
    bases = base_files()
    out = {"bases": bases, "cases": {}, "skipped": {}, "long": {}}
    for name in ("A", "B"):
        out["cases"][name], out["skipped"][name] = placements(name, bases[name])
        out["long"][name] = long_fills(name, bases[name])
    out["cases"]["C"], out["skipped"]["C"], out["long"]["C"] = header_pads("C", bases["C"]), [], []
    out["refusals"] = refusals("A", bases["A"])
    out["crops"] = crop_cases("A", bases["A"], 256, 16, 3)
    return out


def variants(name):
    """Every decodable variant of a base file: its cells and its long fills."""
    e = everything()
    return e["cases"][name] + e["long"][name]


def crop_cases(name, base, width, mcu, restart_interval):
    """For Reader::cut_segments (the chunk list of a crop is shifted by whole windows): variants in which a restart segment
    begins on a window's first byte and on a window's last byte, each with a crop rectangle whose first MCU is that
    segment's first. -> [(Case, (x, y, w, h))]"""
    p = parse(base)
    out = []
    mcus_x = -(-width // mcu)
    for posname, target in (("seg_at_0", WIN - 2), ("seg_at_last", WIN - 3)):
        # a marker in the first four windows whose segment starts a little way into an MCU row
        inst = [(j, m) for m, (_, j) in enumerate(p.rst) if ((m + 1) * restart_interval) % mcus_x <= mcus_x - 3]
        i, pad, fill = _solve(p, inst, WIN, target, "near")
        pos, m = inst[i]
        fills = {m - 2: fill} if fill else {}
        c = Case("crop/%s" % posname, name, base, pad, fills, moved(p, pad, fills, pos), WIN, target, "rst", fill)
        m0 = (m + 1) * restart_interval
        # (two pixels into the MCU: the one-sample halo of the upsamplers stays inside it for luma and chroma)
        out.append((c, ((m0 % mcus_x) * mcu + 2, (m0 // mcus_x) * mcu + 2, 2 * mcu + 5, mcu + 7)))
    return out
