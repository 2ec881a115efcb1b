"""CPU restatement of encoding with optimised Huffman tables (Image.save(f, "JPEG", optimize=True) on libjpeg-turbo), on top
of tests/encode_ref.py: jchuff.c's statistics pass and jpeg_gen_optimal_table in Python, and the same entropy coder with
the tables they give (tests/golden/encode_opt_pins.npz holds Pillow's files; tests/test_encode_opt_ref.py compares).

    gen_optimal_table(counts) -> (bits[16], values, status)   status 0, OVERFLOW or EMPTY; bits and values None unless 0
    symbol_counts(co, restart_interval) -> int64[2 tables][2: DC, AC][256]
    tables(img, ...) -> the (bits, values) pairs of DC0, AC0, DC1, AC1 (None for a table the scan does not use)
    encode(img, quality, subsampling, restart_interval, optimize=True) -> bytes
"""
import numpy as np

from tests import encode_ref as E

OK, OVERFLOW, EMPTY = 0, 2, 3  # JPEGGPU_EXT_ENCODE_OK, _TABLE_OVERFLOW, _EMPTY_TABLE
MAX_CLEN = 32
FREQ_LIMIT = 1000000000  # where libjpeg's search for the least count starts


class TableOverflow(ValueError):
    """A code length above 32 before limiting: libjpeg's JERR_HUFF_CLEN_OVERFLOW."""


def gen_optimal_table(counts):
    """jpeg_gen_optimal_table on 256 symbol counts. The two least counts of each merge are found as libjpeg finds them: the
    LAST index among equal counts (its loops take `<=`), c2 the same without c1."""
    freq = [int(v) for v in counts] + [1]  # the pseudo-symbol 256 keeps the all-ones code unused
    assert len(freq) == 257 and min(freq) >= 0
    if sum(freq) - 1 == 0 or sum(freq) - 1 >= FREQ_LIMIT or max(freq) >= 1 << 28:  # the library's limits: below them no sum passes FREQ_LIMIT
        return None, None, EMPTY
    codesize, others = [0] * 257, [-1] * 257
    while True:
        c1, v = -1, FREQ_LIMIT
        for i in range(257):
            if freq[i] and freq[i] <= v:
                v, c1 = freq[i], i
        c2, v = -1, FREQ_LIMIT
        for i in range(257):
            if freq[i] and freq[i] <= v and i != c1:
                v, c2 = freq[i], i
        if c2 < 0:
            break
        freq[c1] += freq[c2]
        freq[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    if max(codesize) > MAX_CLEN:
        return None, None, OVERFLOW
    bits = [0] * (MAX_CLEN + 1)
    for s in codesize:
        if s:
            bits[s] += 1
    for i in range(MAX_CLEN, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1  # the pseudo-symbol
    values = [j for i in range(1, MAX_CLEN + 1) for j in range(256) if codesize[j] == i]
    assert sum(bits[1:17]) == len(values)
    return bits[1:17], values, OK


def depth_before_limiting(counts):
    """The longest code before limiting (above 16: the table is limited, above 32: refused), by Huffman's algorithm on whole
    trees with libjpeg's choice of the two least -- written apart from gen_optimal_table's chains."""
    freq = {i: int(v) for i, v in enumerate(counts) if v}
    freq[256] = 1
    depth = dict.fromkeys(freq, 0)
    members = {i: [i] for i in freq}
    while len(freq) > 1:
        c1 = min(freq, key=lambda i: (freq[i], -i))
        c2 = min((i for i in freq if i != c1), key=lambda i: (freq[i], -i))
        freq[c1] += freq.pop(c2)
        members[c1] += members.pop(c2)
        for i in members[c1]:
            depth[i] += 1
    return max(depth.values())


def symbol_counts(co, restart_interval):
    """What jchuff.c's htest_one_block counts over a scan: counts[table][0] the DC categories, counts[table][1] the AC symbols
    (run << 4 | size, 0xF0 per 16 zeros of a longer run, 0x00 where a block ends in zeros). `co`: E.coefficients(...)."""
    coefs = co["coefs"].astype(np.int64)
    n = coefs.shape[0]
    comp, mcu = co["comp"], co["mcu"]
    seg = mcu // restart_interval if restart_interval else np.zeros(n, np.int64)
    tbl = (comp > 0).astype(np.int64)
    diff = coefs[:, 0].copy()
    for c in range(co["ncomp"]):
        idx = np.nonzero(comp == c)[0]
        prev = np.concatenate([[0], coefs[idx[:-1], 0]])
        prev[np.concatenate([[True], seg[idx[1:]] != seg[idx[:-1]]])] = 0
        diff[idx] -= prev
    out = np.zeros((2, 2, 256), np.int64)
    np.add.at(out, (tbl, 0, E._bitlen(np.abs(diff))), 1)
    b, k = np.nonzero(coefs[:, 1:])
    k = k + 1
    prev_k = np.concatenate([[0], k[:-1]])
    prev_k[np.concatenate([[True], b[1:] != b[:-1]])] = 0
    run = k - prev_k - 1
    np.add.at(out, (tbl[b], 1, (run & 15) << 4 | E._bitlen(np.abs(coefs[b, k]))), 1)
    np.add.at(out, (tbl[b], 1, 0xF0), run >> 4)
    last = np.zeros(n, np.int64)
    np.maximum.at(last, b, k)
    np.add.at(out, (tbl[last < 63], 1, 0), 1)
    return out


def tables_of_counts(counts, ncomp):
    """DC0, AC0, DC1, AC1 as (bits, values), None for the chroma tables of a grey scan."""
    out = []
    for t in range(1 if ncomp == 1 else 2):
        for cls in (0, 1):
            bits, values, status = gen_optimal_table(counts[t, cls])
            if status == OVERFLOW:
                raise TableOverflow("table %d class %d" % (t, cls))
            assert status == OK
            out.append((bits, values))
    return out + [None] * (4 - len(out))


def tables(img, quality=75, subsampling="4:2:0", restart_interval=0):
    hs, vs = E.SUBSAMPLINGS[subsampling]
    co = E.coefficients(img, hs, vs, quality)
    return tables_of_counts(symbol_counts(co, restart_interval), co["ncomp"])


def encode(img, quality=75, subsampling="4:2:0", restart_interval=0, optimize=True):
    """The whole file. With optimize=False it is E.encode's."""
    if not optimize:
        return E.encode(img, quality, subsampling, restart_interval)
    dc0, ac0, dc1, ac1 = tables(img, quality, subsampling, restart_interval)
    saved = E.DC_LUMA, E.AC_LUMA, E.DC_CHROMA, E.AC_CHROMA
    try:  # E.header and E.entropy_code read the module's tables when they are called
        E.DC_LUMA, E.AC_LUMA = dc0, ac0
        if dc1 is not None:
            E.DC_CHROMA, E.AC_CHROMA = dc1, ac1
        return E.encode(img, quality, subsampling, restart_interval)
    finally:
        E.DC_LUMA, E.AC_LUMA, E.DC_CHROMA, E.AC_CHROMA = saved


def fib_counts(n):
    """1, 2, 3, 5, .. over the first n symbols: a code as deep as a table of n symbols can get."""
    out, a, b = np.zeros(256, np.int64), 1, 2
    for i in range(n):
        out[i] = a
        a, b = b, a + b
    return out


FIB_SIDE = 664


def fibonacci_image():
    """83 x 83 blocks of flat 128; class k = 1..17 appears fib(k) times (1, 2, 3, 5, ..: 6763 blocks) at seeded places and
    adds one basis function, the one at zigzag position 1 + (k - 1) % 15, with amplitude 100 (12 above k = 15). At quality
    50, 4:4:4, its AC table has 18 symbols and lengths up to 18 before limiting."""
    side = FIB_SIDE // 8
    img = np.full((FIB_SIDE, FIB_SIDE), 128.0)
    classes = np.zeros(side * side, np.int64)
    fib, a, b = [], 1, 2
    for _ in range(17):
        fib.append(a)
        a, b = b, a + b
    labels = np.concatenate([np.full(f, k + 1) for k, f in enumerate(fib)])
    classes[:len(labels)] = labels
    np.random.default_rng(4242).shuffle(classes)
    x = np.arange(8)
    for at in np.nonzero(classes)[0]:
        k = int(classes[at])
        v, u = divmod(E.ZIGZAG[1 + (k - 1) % 15], 8)  # natural index = row (vertical frequency) * 8 + column
        amp = 100.0 if k <= 15 else 12.0
        f = amp * np.cos((2 * x[None, :] + 1) * u * np.pi / 16) * np.cos((2 * x[:, None] + 1) * v * np.pi / 16)
        by, bx = divmod(int(at), side)
        img[8 * by:8 * by + 8, 8 * bx:8 * bx + 8] += f
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def edge_cases():
    """The smallest inputs that reach each path of the table kernels: (case dict, image) pairs. The case dicts have
    encode_cases' keys; the images are built here."""
    from tests import encode_cases as K

    rng = np.random.default_rng(777)
    out = [
        (K._case("opt_flat_16x16_rgb", 16, 16, False, "opt_edge", 75, "4:2:0", 0), np.full((16, 16, 3), 128, np.uint8)),  # every table one symbol: all DC differences 0
        (K._case("opt_zero_8x8_grey", 8, 8, True, "opt_edge", 75, "4:4:4", 0), np.zeros((8, 8), np.uint8)),  # the pseudo-symbol and one code
        (K._case("opt_two_tiles_136x136_grey_r3", 136, 136, True, "opt_edge", 90, "4:4:4", 3), rng.integers(0, 256, (136, 136), dtype=np.uint8)),
        (K._case("opt_33x17_rgb_420_r1", 33, 17, False, "opt_edge", 85, "4:2:0", 1), rng.integers(0, 256, (33, 17, 3), dtype=np.uint8)),
        (K._case("opt_fibonacci_664_grey", FIB_SIDE, FIB_SIDE, True, "opt_edge", 50, "4:4:4", 0), fibonacci_image()),
    ]
    return out


_pins = None


def pins():
    """{name: dict(length, sha256, data or None)} and the recorded versions, from tests/golden/encode_opt_pins.npz."""
    global _pins
    if _pins is None:
        import json
        import os

        z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encode_opt_pins.npz"))
        meta = json.loads(z["meta"].tobytes().decode())
        table = {e["name"]: dict(length=e["length"], sha256=e["sha256"], data=z["file_" + e["name"]].tobytes() if e["whole"] else None) for e in meta["cases"]}
        _pins = (table, {k: v for k, v in meta.items() if k != "cases"})
    return _pins


def equals_pin(name, data):
    import hashlib

    pin = pins()[0][name]
    if pin["data"] is not None:
        return data == pin["data"]
    return len(data) == pin["length"] and hashlib.sha256(data).hexdigest() == pin["sha256"]
