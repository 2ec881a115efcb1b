"""Shared matrix of synthetic inputs (reference coverage: test/test.sh:31-43 sampling variants and
grayscale; plus what it never tests)."""
import numpy as np

from tools import jpegsynth

S420 = ((2, 2), (1, 1), (1, 1))
S444 = ((1, 1), (1, 1), (1, 1))


def dense_escape_case(groups=96, seed=5):
    """The most entries per bit a code table allows (jg_defs.h, sym_region_entries): a grayscale file whose fitted
    tables give the DC symbol and the AC symbol (0, 1) one-bit codes, in groups of four data units of 63 coefficients
    +-1 (64 entries in 127 bits each) followed by one unit of 63 coefficients of magnitude >= 512 (127 entries: every
    one takes an escape). A subsequence that commits four dense units and the DC symbol of the escaped one emits
    4.03 B + 127 entries."""
    import numpy as np

    rng = np.random.default_rng(seed)
    n = 5 * groups
    coef = np.zeros((n, 64), np.int16)
    sign = lambda shape: rng.integers(0, 2, shape).astype(np.int16) * 2 - 1
    coef[:, 1:] = sign((n, 63))
    coef[4::5, 1:] = sign((groups, 63)) * rng.integers(512, 1024, (groups, 63)).astype(np.int16)
    return jpegsynth.encode_blocks(coef, 24, np.ones(64, np.uint8), optimize=True)


def empty_segment_case():
    """A 4:2:0 file with restart markers in which one restart marker was taken out and put back right behind the next
    one: the number of segments still matches the geometry, but one segment holds no byte at all (the chain
    walk of huff_mh_resolve had no first subsequence to start from). Both walks refuse it."""
    good = jpegsynth.encode(240, 168, S420, restart_interval=7, seed=9)
    sos = good.index(b"\xff\xda")
    marks = [i for i in range(sos, len(good) - 1) if good[i] == 0xFF and 0xD0 <= good[i + 1] <= 0xD7]
    assert len(marks) >= 4
    a, b = marks[1], marks[2]
    # segment 1 and 2 become one (their marker is gone), an empty one follows the next marker
    return good[:a] + good[a + 2:b + 2] + good[a:a + 2] + good[b + 2:]


def big_last_scan_case(restart_interval=0, seed=41):
    """Two non-interleaved scans of which the LAST one holds most of the bytes (component 1 has four times the samples of
    component 0): the shape of file whose last scan the device-side marker scan takes over (jpeggpu_ext_set_device_scan)."""
    return jpegsynth.encode(232, 176, ((1, 1), (2, 2)), interleaved=False, restart_interval=restart_interval, quality=90, noise=12, seed=seed)


def matrix():
    """name -> bytes. Small enough for the oracle to finish in well under a second each."""
    e = jpegsynth.encode
    cases = {
        # the reference's own variant matrix (test/test.sh): 1x1, 2x1, 2x2, 1x2, 4x1, grayscale
        "ss_1x1": e(200, 152, S444, seed=1),
        "ss_2x1": e(200, 152, ((2, 1), (1, 1), (1, 1)), seed=2),
        "ss_2x2": e(200, 152, S420, seed=3),
        "ss_1x2": e(200, 152, ((1, 2), (1, 1), (1, 1)), seed=4),
        "ss_4x1": e(200, 152, ((4, 1), (1, 1), (1, 1)), seed=5),
        "gray": e(200, 152, ((1, 1),), seed=6),
        "gray_hdr_2x2": e(120, 88, ((2, 2),), seed=7),  # single component: factors are ignored
        # restart intervals
        "dri_1": e(160, 96, S420, restart_interval=1, seed=8),
        "dri_7": e(240, 168, S420, restart_interval=7, seed=9),
        "dri_row": e(496, 360, S420, restart_interval=31, seed=10),
        "dri_nondiv": e(248, 200, S420, restart_interval=11, seed=11),
        "dri_fill": e(248, 200, S420, restart_interval=5, fill_bytes=2, seed=12),
        # odd sizes
        "odd_1x1px": e(1, 1, S420, seed=13),
        "odd_17x9": e(17, 9, S420, seed=14),
        "odd_partial_mcu": e(333, 251, S420, seed=15),
        # non-interleaved
        "ni_444": e(232, 176, S444, interleaved=False, seed=16),
        "ni_420": e(232, 176, S420, interleaved=False, seed=17),
        "ni_420_dri": e(233, 171, S420, interleaved=False, restart_interval=9, seed=18),
        "ni_big_last": big_last_scan_case(),
        "ni_big_last_dri": big_last_scan_case(restart_interval=5, seed=42),
        # components and tables
        "two_comp": e(160, 120, ((2, 1), (1, 1)), seed=19),
        "four_comp_opt": e(264, 200, ((2, 1), (1, 1), (1, 1), (2, 1)), optimize=True, seed=20),
        "four_comp_444": e(136, 104, ((1, 1),) * 4, seed=21),
        "opt_tables_420": e(320, 240, S420, optimize=True, seed=22),
        # entropy extremes
        "q100_noisy": e(160, 128, S420, quality=100, noise=40, seed=23),   # long codes, long blocks
        "q5_flat": e(640, 480, S420, quality=5, noise=0, seed=24),         # almost all EOB
        "dense_escapes": dense_escape_case(),  # worst-case entries per subsequence of the write pass
        "q16_tables": e(328, 248, S420, restart_interval=7, quality=3, noise=30, seed=31, qmax=65535),  # 16-bit DQT (Pq = 1)
        # more than one sequence without restart markers (inter-sequence flows), ~150 KB of scan
        "multi_seq_nodri": e(1024, 768, S420, quality=92, noise=12, seed=25),
        "multi_seq_dri": e(1024, 768, S420, quality=92, noise=12, restart_interval=64, seed=26),
        # BASELINE.json configs at reduced size
        "cfg2_small": jpegsynth.config(2, small=True),
        "cfg4_small": jpegsynth.config(4, small=True),
        "cfg5_small": jpegsynth.config(5, small=True),
    }
    return cases


class SlowSync:
    """An entropy-coded stream that does not resynchronise by itself (slow_sync below): the file, the bit length of a
    data unit of each component and of an MCU when the data are zeros, the restart interval, and how far a flow must
    run at least (`min_distance`, in subsequences, measured by tests/test_slow_sync_host.py)."""

    def __init__(self, data, unit_bits, mcu_bits, restart_interval, min_distance):
        self.data, self.unit_bits, self.mcu_bits = data, unit_bits, mcu_bits
        self.restart_interval, self.min_distance = restart_interval, min_distance


DC_Q = 64  # DC quantiser of the slow-sync files


def _zero_tables(d, a):
    """A DC table whose category 0 has the d-bit code 0...0 (category 1 the (d + 1)-bit code 10...0) and an AC table
    whose symbol (0, 1) has the a-bit code 0...0 (end of block 10...0). On all-zero bits a data unit whose 63 AC
    coefficients are -1 (value bit 0) and whose DC difference is 0 is then d + 63 (a + 1) bits long. (No code is all
    ones: libjpeg refuses a table without room for one.)"""
    dc = [0] * 16
    dc[d - 1], dc[d] = 1, 1
    ac = [0] * 16
    ac[a - 1], ac[a] = 1, 1
    return (dc, [0, 1]), (ac, [0x01, 0x00])


def _minus_one_blocks(by, bx):
    b = np.full((by, bx, 64), -1, np.int16)
    b[:, :, 0] = 0
    return b


def _zero_stream(width, height, sampling, dc_bits, interleaved=True, restart_interval=0, watermark=0):
    """Every component codes DC difference 0 and 63 AC coefficients -1 with the zero codes of _zero_tables (dc_bits[c],
    a = 1), so the entropy-coded data are zero bits only. `watermark` K > 0: in every K-th MCU the first data unit of
    each component instead has DC 1 (difference +1, and -1 in the component's next data unit: category 1). The DC
    quantiser is DC_Q, so a marked block is DC_Q / 8 levels brighter than the others and the planes show where each
    marked data unit was placed; the AC quantisers are 1."""
    hmax = max(h for h, _ in sampling)
    vmax = max(v for _, v in sampling)
    mx, my = -(-width // (8 * hmax)), -(-height // (8 * vmax))
    blocks = []
    for h, v in sampling:
        if interleaved and len(sampling) > 1:
            by, bx = my * v, mx * h
        else:
            by, bx = -(-(-(-height * v // vmax)) // 8), -(-(-(-width * h // hmax)) // 8)
        blocks.append(_minus_one_blocks(by, bx))
    if watermark:
        mcu = np.arange(mx * my)
        marked = mcu[mcu % watermark == watermark - 1]
        for c, (h, v) in enumerate(sampling):
            blocks[c][(marked // mx) * v, (marked % mx) * h, 0] = 1
    tabs = [_zero_tables(d, 1) for d in dc_bits]
    q = np.ones(64, np.uint8)
    q[0] = DC_Q
    return jpegsynth.encode_custom(width, height, sampling, blocks, [t[0] for t in tabs], [t[1] for t in tabs],
                                   qtables=[q] * len(sampling), interleaved=interleaved, restart_interval=restart_interval)


def slow_sync():
    """name -> SlowSync: streams on which a speculative decode that starts at a wrong bit offset does not meet the true
    path for hundreds of subsequences (flows across sequences, through one tail part of over a thousand subsequences
    and across multi-hypothesis blocks; a tail part is cut only at a segment start, so no flow leaves one). A decode that
    starts from (c, z) = (0, 0) at a subsequence start parses the zero bits as valid data units on a grid of its own;
    it is on the true path only where that grid is the true MCU grid, i.e. where the subsequence start is a multiple of
    the (odd) MCU bit length: once every mcu_bits subsequences."""
    S420 = ((2, 2), (1, 1), (1, 1))
    u = lambda d: d + 126
    out = {}
    # grayscale, L = 127, ~0.5 MP (130 KB of zero bytes)
    out["gray_127"] = SlowSync(_zero_stream(1024, 512, ((1, 1),), (1,)), [127], 127, 0, 120)
    # 4:2:0, Cr's DC code one bit longer: MCU of 4 * 127 + 127 + 128 = 763 bits, ~1 MP
    l420 = 6 * 126 + 4 + 1 + 2
    out["s420_763"] = SlowSync(_zero_stream(1024, 1024, S420, (1, 1, 2)), [u(1), u(1), u(2)], l420, 0, 700)
    # restart segments longer than the distance (4 segments) and much shorter (48 MCUs, ~36 kbit each): there the
    # restart markers end the flows. These two and the next file carry marks every 1000th MCU (_zero_stream): misplaced
    # data units show in their planes, and the marks' one bits leave flows of several hundred subsequences
    mk = dict(watermark=1000)
    out["s420_763_dri1024"] = SlowSync(_zero_stream(1024, 1024, S420, (1, 1, 2), restart_interval=1024, **mk), [u(1), u(1), u(2)], l420, 1024, 300)
    out["s420_763_dri48"] = SlowSync(_zero_stream(1024, 1024, S420, (1, 1, 2), restart_interval=48, **mk), [u(1), u(1), u(2)], l420, 48, 60)
    out["s420_763_mark1000"] = SlowSync(_zero_stream(1024, 1024, S420, (1, 1, 2), **mk), [u(1), u(1), u(2)], l420, 0, 300)
    # 4 components, 8 data units per MCU (2x2, 2x1, 1x1, 1x1): 8 * 126 + 4 + 2 + 1 + 2 = 1017 bits, no restart markers;
    # 2 304 MCUs, no marks: the scan is over 1 100 subsequences long even at 256 bytes, so at every size the distance
    # exceeds 960 subsequences (the size kTailPartSubseq would give a part if the scan had restart markers) and the
    # scan is one tail part and, at 32 to 128 bytes, more than one multi-hypothesis block
    l4 = 8 * 126 + 4 * 1 + 2 * 1 + 1 + 2
    out["four_1017"] = SlowSync(_zero_stream(768, 768, ((2, 2), (2, 1), (1, 1), (1, 1)), (1, 1, 1, 2)), [u(1), u(1), u(1), u(2)], l4, 0, 970)
    # three scans of one component each; the last (4x the samples of each other, L = 127) is the slow one, the others
    # (L = 128) resynchronise at once
    out["ni_last_127"] = SlowSync(_zero_stream(1024, 512, ((1, 1), (1, 1), (2, 2)), (2, 2, 1), interleaved=False), [u(2), u(2), u(1)], None, 0, 120)
    return out


# Sampling layouts of tests/cases.sampling_sweep(): name -> (h, v) per component. Every luma factor with h v <= 8 over
# 1x1 chroma, then chroma factors above 1, a chroma plane larger than luma (luma itself upsampled), Cb and Cr with
# different factors, and 2-D ratios. All have integral ratios h_max / h_c, v_max / v_c.
SWEEP_LAYOUTS = {"y%dx%d" % (h, v): ((h, v), (1, 1), (1, 1)) for h in range(1, 5) for v in range(1, 5) if h * v <= 8}
SWEEP_LAYOUTS.update({
    "y2x2_c1x2": ((2, 2), (1, 2), (1, 2)),
    "y2x2_c2x1": ((2, 2), (2, 1), (2, 1)),
    "y4x1_c2x1": ((4, 1), (2, 1), (2, 1)),
    "y1x4_c1x2": ((1, 4), (1, 2), (1, 2)),
    "y1x1_cb2x2": ((1, 1), (2, 2), (1, 1)),
    "y2x2_cr2x1": ((2, 2), (1, 1), (2, 1)),
    "y1x1_c2x1": ((1, 1), (2, 1), (2, 1)),
    "y2x1_cb1x2": ((2, 1), (1, 2), (1, 1)),
    "y1x2_cb2x1": ((1, 2), (2, 1), (1, 1)),
    "y2x2_cb2x2": ((2, 2), (2, 2), (1, 1)),  # 9 units: every MCU size from 3 to 10
})
# layouts that also get a non-interleaved and a restart-marker variant: the 10-unit MCUs, the ratios of 3 and the
# layouts in which luma is upsampled
SWEEP_VARIANTS = ("y4x2", "y2x4", "y3x1", "y1x3", "y3x2", "y2x3", "y1x1_cb2x2", "y1x1_c2x1", "y2x1_cb1x2", "y1x2_cb2x1")
# layouts with vmax 3 or 4 that also get a restart interval of one MCU row (what a segment shard cuts into bands)
SWEEP_ROW_DRI = ("y1x3", "y2x3", "y1x4", "y2x4", "y1x4_c1x2")
# layouts that also get a tiny size at which a chroma plane (or luma, where it is upsampled) is at most 2 samples wide
SWEEP_TINY = ("y2x1", "y2x2", "y4x1_c2x1", "y2x2_c1x2", "y1x1_cb2x2", "y1x1_c2x1", "y2x1_cb1x2", "y1x2_cb2x1", "y4x2")


def sweep_size(hmax, vmax, kind):
    """Width and height of a sweep file: the last MCU column and row are partial and (for a factor above 1) hold wholly
    invisible blocks. "a": one pixel into the last MCU, so h_max - 1 blocks of it are invisible; "b": the partial block
    is the MCU's last but one (5 pixels of it visible, h_max >= 3), its first (h_max = 2) or its only one."""
    def edge(f, mcus, kind):
        return 8 * f * mcus + (1 if kind == "a" else 8 * (f - 1) - 3 if f > 1 else 5)
    if kind == "a":
        return edge(hmax, max(2, 72 // (8 * hmax)), "a"), edge(vmax, max(2, 48 // (8 * vmax)), "a")
    return edge(hmax, max(1, 40 // (8 * hmax)), "b"), edge(vmax, max(1, 32 // (8 * vmax)), "b")


def sweep_restart_interval(mcus_x):
    """The smallest interval >= 2 that does not divide the MCU row: segments start in the middle of MCU rows."""
    ri = 2
    while mcus_x % ri == 0:
        ri += 1
    return ri


def sweep_is_planes_only(name):
    """Files of the sweep that the RGB calls refuse (a non-integral ratio, 2 or 4 components): checked as planes only."""
    return name.startswith("po_")


def sweep_is_refused(name):
    """Files of the sweep that parse_header refuses (JPEGGPU_INVALID_JPEG)."""
    return name.startswith("refuse_")


def sampling_sweep():
    """name -> bytes: every legal sampling layout of baseline JPEG that the matrix lacks (T.81 A.1.1: factors 1..4, at
    most 10 data units per MCU), each at two sizes (sweep_size), some at a tiny size, and, for SWEEP_VARIANTS, as
    one scan per component ("_ni") and with restart markers that cut MCU rows ("_dri"); row-interval restart files
    ("_rowdri") for SWEEP_ROW_DRI. Names with "po_" are files whose planes are checked but that have no RGB (a
    non-integral ratio, 2 or 4 components); "refuse_" an 11-unit MCU parse_header must refuse. Kept apart from matrix()
    so that the matrix loops do not grow; every file decodes on the oracle in a few milliseconds."""
    e = jpegsynth.encode
    out = {}
    seed = 300
    for name, samp in SWEEP_LAYOUTS.items():
        hmax, vmax = max(h for h, _ in samp), max(v for _, v in samp)
        for kind in ("a", "b"):
            w, h = sweep_size(hmax, vmax, kind)
            seed += 1
            out["%s_%s" % (name, kind)] = e(w, h, samp, seed=seed)
        if name in SWEEP_TINY:
            seed += 1
            out[name + "_tiny"] = e(3, 5, samp, seed=seed)
        w, h = sweep_size(hmax, vmax, "a")
        mcus_x = -(-w // (8 * hmax))
        if name in SWEEP_VARIANTS:
            seed += 1
            out[name + "_ni"] = e(w, h, samp, interleaved=False, seed=seed)
            seed += 1
            out[name + "_dri"] = e(w, h, samp, restart_interval=sweep_restart_interval(mcus_x), seed=seed)
        if name in SWEEP_ROW_DRI:
            seed += 1
            out[name + "_rowdri"] = e(w, h, samp, restart_interval=mcus_x, seed=seed)
    # planes only: a non-integral ratio (3 over 2), a second component larger than the first (10 units per MCU), four
    # components in 8 units per MCU
    out["po_y3x1_cb2x1"] = e(77, 45, ((3, 1), (2, 1), (1, 1)), seed=401)
    out["po_y3x1_cb2x1_dri"] = e(77, 45, ((3, 1), (2, 1), (1, 1)), restart_interval=2, seed=402)
    out["po_two_1x1_3x3"] = e(61, 53, ((1, 1), (3, 3)), seed=403)
    out["po_four_8du"] = e(69, 37, ((2, 2), (2, 1), (1, 1), (1, 1)), seed=404)
    # 9 + 1 + 1 = 11 data units per MCU: not a legal interleaved scan (T.81 B.2.3)
    out["refuse_11du"] = e(48, 48, ((3, 3), (1, 1), (1, 1)), seed=405)
    return out
