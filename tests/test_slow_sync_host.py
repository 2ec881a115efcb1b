"""The slow-synchronising corpus (tests/cases.slow_sync) on the host: its streams really do not resynchronise (a plain
numpy measurement of the sync distance against the oracle's states), the emulation twin of the device pipeline is exact
on them at every cap of the sequence kernel's loop and with the multi-hypothesis tables, and the files are what Pillow
decodes (tests/golden/slow_sync_pins.json, written by tools/make_slow_sync_pins.py)."""
import hashlib
import json
import os

import numpy as np
import pytest

from oracle import oracle
from tests import cases, libjpeg_ref
from tests.conftest import GOLDEN
from tests.emu import emu

SIZES = (32, 64, 128, 256)


@pytest.fixture(scope="module")
def corpus():
    return cases.slow_sync()


def scan_tables(data, scan_idx):
    """(DC (BITS, HUFFVAL), AC (BITS, HUFFVAL)) per data unit of the MCU of scan `scan_idx` (T.81 B.2, A.2)."""
    i, dht, comps, nscan = 2, {}, {}, 0
    while True:
        assert data[i] == 0xFF
        m, n = data[i + 1], int.from_bytes(data[i + 2:i + 4], "big")
        seg = data[i + 4:i + 2 + n]
        if m == 0xC4:
            k = 0
            while k < len(seg):
                bits = list(seg[k + 1:k + 17])
                dht[seg[k] >> 4, seg[k] & 15] = (bits, list(seg[k + 17:k + 17 + sum(bits)]))
                k += 17 + sum(bits)
        elif m == 0xC0:
            for c in range(seg[5]):
                comps[seg[6 + 3 * c]] = seg[7 + 3 * c]  # id -> h << 4 | v
        elif m == 0xDA:
            if nscan == scan_idx:
                ns = seg[0]
                out = []
                for k in range(ns):
                    cid, t = seg[1 + 2 * k], seg[2 + 2 * k]
                    units = (comps[cid] >> 4) * (comps[cid] & 15) if ns > 1 else 1
                    out += [(dht[0, t >> 4], dht[1, t & 15])] * units
                return out
            nscan += 1
            i += 2 + n
            while not (data[i] == 0xFF and data[i + 1] not in (0x00, *range(0xD0, 0xD8))):  # entropy-coded data
                i += 1
            continue
        i += 2 + n


def _lut(table):
    """16-bit window -> (code length, symbol); length 0: no code."""
    bits, vals = table
    ln = np.zeros(1 << 16, np.int64)
    sy = np.zeros(1 << 16, np.int64)
    code, k = 0, 0
    for l in range(1, 17):
        for _ in range(bits[l - 1]):
            lo = code << (16 - l)
            ln[lo:lo + (1 << (16 - l))] = l
            sy[lo:lo + (1 << (16 - l))] = vals[k]
            code += 1
            k += 1
        code <<= 1
    return ln, sy


class _Decoder:
    """Symbol lengths and (c, z) steps of the sequential decoder, nothing else: enough to follow a flow's state."""

    def __init__(self, units):
        self.units = units
        self.luts = [(_lut(dc), _lut(ac)) for dc, ac in units]
        # the MCU as the all-zero bits decode it: every symbol's start and end bit and the state it starts in
        st, en, pc, pz = [], [], [], []
        pos = 0
        for c in range(len(units)):
            z = 0
            while z < 64:
                l, s, z2 = self.step(0, c, z)
                assert l > 0, "the all-zero code of a table must exist"
                st.append(pos), en.append(pos + l), pc.append(c), pz.append(z)
                pos, z = pos + l, z2
        self.st, self.en, self.pc, self.pz = (np.array(a, np.int64) for a in (st, en, pc, pz))
        self.mcu_bits = pos
        self.index = np.full(len(units) * 64, -1, np.int64)
        self.index[self.pc * 64 + self.pz] = np.arange(len(st))

    def step(self, win, c, z):
        """(bits taken, symbol, z after it) of the symbol in the 16-bit window `win`; 0 bits: no code."""
        (dl, ds), (al, as_) = self.luts[c]
        if z == 0:
            l, s = dl[win], ds[win]
            return (l + (s & 15) if l else 0), s, 1
        l, s = al[win], as_[win]
        if not l:
            return 0, s, z
        r, ss = s >> 4, s & 15
        return l + ss, s, (z + 16 if r == 15 else 64) if ss == 0 else z + r + 1

    def advance(self, win16, pos, c, z, bound):
        """One flow, symbol by symbol: the state of the first symbol that ends behind bit `bound`; None: no code."""
        n = len(self.units)
        while True:
            l, _, z2 = self.step(int(win16[pos]), c, z)
            if not l:
                return None
            if pos + l > bound:
                return pos, c, z
            pos, z = pos + l, z2
            if z >= 64:
                c, z = (c + 1) % n, 0


def sync_distance(data, scan_idx, subseq_bytes, window):
    """The longest run of subsequences a flow has to cover, measured: for every subsequence start s a decode from
    (c, z) = (0, 0) at s, followed until its state at a subsequence end equals the oracle's (oracle.scan_stages) -- from
    there on it is the true path. A subsequence's entry state is known once a flow from some s at or before it has met
    the true path before it; the distance is the largest gap between a subsequence and the latest such s. Flows are
    followed for `window` subsequences, so the result is exact up to `window` and `window` above it. Zero runs are
    stepped over whole MCUs at once, the rest symbol by symbol."""
    tw = oracle.scan_stages(data, scan_idx, subseq_bytes)
    dec = _Decoder(scan_tables(data, scan_idx))
    B = 8 * subseq_bytes
    L = dec.mcu_bits
    worst = 0
    for g in range(tw.num_segments):
        off, n = int(tw.seg_offset[g]), int(tw.seg_count[g])
        bits = np.unpackbits(tw.destuffed[off * subseq_bytes:(off + n) * subseq_bytes]).astype(np.int64)
        pad = np.concatenate([bits, np.zeros(32, np.int64)])
        win16 = np.zeros(len(bits) + 1, np.int64)
        for k in range(16):
            win16 = win16 << 1 | pad[k:k + len(bits) + 1]
        ones = np.concatenate([[0], np.cumsum(bits)])
        p, cz = tw.p[off:off + n], tw.cz[off:off + n]
        met = np.full(n, np.iinfo(np.int64).max)  # subsequence whose end the flow from s meets the true path at
        met[0] = -1
        pos = np.zeros(0, np.int64)
        c = np.zeros(0, np.int64)
        z = np.zeros(0, np.int64)
        start = np.zeros(0, np.int64)
        for j in range(n):
            if p[j] < 0:  # the segment's last subsequence: its end is the data's end
                break
            if j > 0:  # the flow from j, unless j already starts on the true path
                if p[j - 1] == j * B and cz[j - 1] == 0:
                    met[j] = j - 1
                else:
                    pos, c, z, start = (np.append(a, v) for a, v in ((pos, j * B), (c, 0), (z, 0), (start, j)))
            bound = (j + 1) * B
            k = dec.index[c * 64 + z]
            base = pos - dec.st[np.maximum(k, 0)]
            o = bound - base
            m = o // L
            idx = np.searchsorted(dec.en, o - m * L, side="right")
            wrap = idx == len(dec.en)
            idx = np.where(wrap, 0, idx)
            ex = base + (m + wrap) * L + dec.st[idx]
            fast = (k >= 0) & (ones[np.minimum(ex, len(bits))] == ones[np.minimum(pos, len(bits))])
            npos, nc, nz = np.where(fast, ex, pos), np.where(fast, dec.pc[idx], c), np.where(fast, dec.pz[idx], z)
            alive = np.ones(len(pos), bool)
            for i in np.flatnonzero(~fast):
                r = dec.advance(win16, int(pos[i]), int(c[i]), int(z[i]), bound)
                if r is None:
                    alive[i] = False
                else:
                    npos[i], nc[i], nz[i] = r
            hit = alive & (npos == p[j]) & ((nc | nz << 8) == cz[j])
            met[start[hit]] = j
            keep = alive & ~hit & (j + 1 - start < window)
            pos, c, z, start = npos[keep], nc[keep], nz[keep], start[keep]
        # entry of subsequence e is known from the latest s <= e whose flow met the true path before e
        known_from = np.full(n + 1, -1)
        for s in np.flatnonzero(met < n):
            known_from[met[s] + 1] = max(known_from[met[s] + 1], s)
        latest = np.maximum.accumulate(known_from[:n])
        worst = max(worst, int((np.arange(n) - latest).max()))
    return min(worst, window)


@pytest.mark.parametrize("subseq_bytes", SIZES)
def test_measured_sync_distance_reaches_the_stated_minimum(corpus, subseq_bytes):
    """The corpus cannot quietly become easy: each file's flows run at least its stated distance."""
    for name, case in corpus.items():
        scan = oracle.decode(case.data).nscans - 1  # the slow scan is the last one
        tw = oracle.scan_stages(case.data, scan, subseq_bytes)
        longest = int(tw.seg_count.max())
        want = min(case.min_distance, longest - 8)
        got = sync_distance(case.data, scan, subseq_bytes, want + 8)
        assert got >= want, (name, subseq_bytes, got, want)
        if case.mcu_bits is not None:
            assert _Decoder(scan_tables(case.data, scan)).mcu_bits == case.mcu_bits, name


def test_sync_distance_of_a_matrix_file_is_short():
    """The measurement against files that resynchronise at once: a few subsequences."""
    m = cases.matrix()
    for name in ("multi_seq_nodri", "cfg2_small", "gray"):
        assert sync_distance(m[name], 0, 64, 64) <= 16, name


@pytest.mark.parametrize("subseq_bytes", SIZES)
def test_emulated_pipeline_is_exact(corpus, subseq_bytes):
    """tests/emu against oracle.scan_stages with the sequence kernel's loop cut after 1, 2, 255 and 256 iterations (the
    unfinished flows go on in the tail pass), and with the multi-hypothesis tables."""
    for name, case in corpus.items():
        data = case.data
        for s in range(oracle.decode(data).nscans):
            tw = oracle.scan_stages(data, s, subseq_bytes)
            ok = tw.p >= 0
            for cap, mh in ((1, False), (2, False), (255, False), (256, False), (256, True)):
                rc, r = emu.decode_scan(data, s, subseq_bytes, cap, multi_hypothesis=mh)
                what = (name, s, subseq_bytes, cap, mh)
                assert rc == 0, what
                assert np.array_equal(r.destuffed, tw.destuffed) and np.array_equal(r.seg_index, tw.seg_index), what
                assert np.array_equal(r.p[ok], tw.p[ok]) and np.array_equal(r.n[ok], tw.n[ok]), what
                assert np.array_equal(r.cz[ok], tw.cz[ok]), what
                for k in range(4):
                    assert np.array_equal(r.dc[k][ok].astype(np.int16), tw.dc[k][ok].astype(np.int16)), what
                assert np.array_equal(r.coef, tw.stream_coef), what
                last = s == oracle.decode(data).nscans - 1
                if cap == 256 and not mh and last and case.min_distance >= 120:
                    # the sequence kernel's flows run to the end of the sequence (240 subsequences of a lone decode)
                    assert r.max_flow_iters >= min(200, tw.num_subseq - 16), (what, r.max_flow_iters)


def _pins():
    with open(os.path.join(GOLDEN, "slow_sync_pins.json")) as f:
        return json.load(f)


def _sha(b):
    return hashlib.sha256(np.ascontiguousarray(b).tobytes() if isinstance(b, np.ndarray) else b).hexdigest()


def test_corpus_is_pinned_and_equals_pillow(corpus):
    """The files are the pinned ones, and what Pillow (libjpeg-turbo) decoded from them at authoring time is what the
    numpy restatement of libjpeg (tests/libjpeg_ref.py) gives from the oracle's coefficients: RGB of the one- and
    three-component files; the four-component file's planes at full resolution (Image.draft, no colour conversion)."""
    pins = _pins()
    assert sorted(pins) == sorted(corpus)
    for name, case in corpus.items():
        pin = pins[name]
        assert _sha(case.data) == pin["jpeg_sha256"], name
        dec = oracle.decode(case.data)
        if "rgb_sha256" in pin:
            assert _sha(libjpeg_ref.libjpeg_rgb_of(dec)) == pin["rgb_sha256"], name
        if "planes_sha256" in pin:
            got = libjpeg_ref.islow_planes_of(dec)
            assert [_sha(p) for p in got] == pin["planes_sha256"], name


def test_marks_show_in_every_plane(corpus):
    """In the marked files a data unit put in the wrong place changes the planes: every component has marked blocks
    (brighter by the DC quantiser / 8) besides the plain ones, at the MCUs _zero_stream marked."""
    from oracle import oracle as o

    marked = [n for n in corpus if n.startswith("s420_763_")]
    assert len(marked) == 3
    for name in marked:
        dec = o.decode(corpus[name].data)
        for c in range(dec.ncomp):
            blocks = dec.coef[c].reshape(-1, 64)
            dcs = np.unique(blocks[:, 0])
            assert list(dcs) == [0, 1], (name, c, dcs)
            p = dec.planes[c]
            tiles = p[:p.shape[0] // 8 * 8, :p.shape[1] // 8 * 8].reshape(p.shape[0] // 8, 8, -1, 8).transpose(0, 2, 1, 3)
            assert len(np.unique(tiles.reshape(-1, 64), axis=0)) >= 2, (name, c)

