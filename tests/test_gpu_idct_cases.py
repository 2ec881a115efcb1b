"""The crafted IDCT corpus (tests/idct_cases.py) through every transform of the IDCT stage on the GPU, bit-exact against
the CPU references, into guarded planes: lone decodes at two subsequence sizes with the host's and the device's marker
scan, the symbol stream read back, crops, and batch calls of seven compositions (COMPOSITIONS) over every file. Every
comparison is array_equal; every stream is valid. tests/test_idct_cases_host.py proves on the CPU what the files contain.

Which file pins which branch of jg_idct.hip:
  pass1_q16a, pass1_q16b, pass1_edge8, ycc420*, kats16_*  the 64-bit pass 1 of idct_kernel<IslowJobs<..>> behind __ballot(!small);
                           a threshold raised to 40,000 fails test_lone_decode[islow-*] on pass1_q16a (L = 35,082 and 40,000
                           in setting (a), where no other unit of the group sends the wave to the 64-bit pass)
  pass1_bound              the 32-bit pass 1 at its bound, every sign pattern in every column
  pass1_dcramp             the int workspace wrapping in pass 1
  counts_plain_*           the gather of idct_kernel at 29..34 entries with either parity of the first entry: a `!plain` tail
                           loop that starts one entry early or late fails test_lone_decode and test_symbol_stream_and_gather_coverage
  counts_escape_*          idct_kernel's per-entry path in mixed groups; idct_scaled_kernel's e[j + 1] look-ahead: an escape as
                           entry 8, 9, 16, 17 and as the last entry (test_lone_decode[scale2-*], [scale4-*])
  counts_*, one-hot units  the rows and columns jpeg_idct_4x4 / jpeg_idct_2x2 must ignore (a column 4 that is not skipped fails
                           test_lone_decode[scale2-*] on the one-hot units of column 4)
  limit_*                  the range limit on both sides of every edge and of its wrap, in every transform
  ycc420, ycc420_q16       all of it in the size classes of libjpeg's scale mode (DraftJobs), luma and chroma
"""
import numpy as np
import pytest

from tests import cases, draft_ref, gpu_util, idct_cases, libjpeg_ref, scaled_ref
from tests.test_gpu_scaled import Guarded, _assert_planes, _tmp

pytestmark = pytest.mark.gpu

KINDS = {"reference": ("reference", 1, "uniform"), "islow": ("islow", 1, "uniform"), "scale2": ("reference", 2, "uniform"),
         "scale4": ("reference", 4, "uniform"), "scale8": ("reference", 8, "uniform"), "draft2": ("reference", 2, "libjpeg"),
         "draft4": ("reference", 4, "libjpeg"), "draft8": ("reference", 8, "libjpeg")}
LONE = [(32, False), (32, True), (256, False), (256, True)]


@pytest.fixture(scope="module")
def torch_cuda(gpu_lib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def corpus():
    return idct_cases.corpus()


class References:
    """The CPU references of every file, each computed once and never changed."""

    def __init__(self, files):
        self.files, self.decoded, self.planes = files, {}, {}

    def of(self, name, kind):
        from oracle import oracle

        if (name, kind) not in self.planes:
            if name not in self.decoded:
                self.decoded[name] = oracle.decode(self.files[name])
            dec = self.decoded[name]
            method, d, mode = KINDS[kind]
            if d == 1:
                p = libjpeg_ref.islow_planes_of(dec) if method == "islow" else [x.copy() for x in dec.planes]
            else:
                p = draft_ref.draft_planes_of(dec, d) if mode == "libjpeg" else scaled_ref.scaled_planes_of(dec, d)
            for x in p:
                x.setflags(write=False)
            self.planes[(name, kind)] = p
        return self.planes[(name, kind)]


@pytest.fixture(scope="module")
def refs(corpus):
    files = {name: c.data for name, c in corpus.items()}
    m = cases.matrix()
    files["matrix:ni_420_dri"], files["matrix:q100_noisy"] = m["ni_420_dri"], m["q100_noisy"]
    return References(files)


def kinds_of(case):
    """The transforms a file is decoded with: libjpeg's scale mode where the components differ in size."""
    return [k for k in KINDS if case.gray is False or not k.startswith("draft")]


def configure(dec, kind, device_scan=False, crop=None):
    method, d, mode = KINDS[kind]
    dec.set_scale(d)
    dec.set_scale_mode(mode)
    dec.set_idct(method)
    dec.set_device_scan(device_scan)
    if crop is not None:
        dec.set_crop(*crop)


def decode(torch, data, kind, subseq_bytes=None, device_scan=False, crop=None):
    """One lone decode into guarded planes: (planes, info, crop_info, scale_info, tmp, base, layout)."""
    import jpeggpu_amd

    dec = jpeggpu_amd.Decoder(subseq_bytes)
    try:
        configure(dec, kind, device_scan, crop)
        info = dec.parse_header(data)
        n = dec.get_buffer_size()
        tmp, base = _tmp(torch, n)
        g = Guarded(torch, info)
        dec.transfer(base, n, 0)
        dec.decode(g.ptrs, g.pitches, base, n, 0)
        torch.cuda.synchronize()
        if device_scan:
            assert dec.device_status(base, 0) == jpeggpu_amd.Status.SUCCESS
        return g.planes(), info, dec.crop_info(), dec.scale_info(), tmp, base, dec.layout()
    finally:
        dec.cleanup()


def window_of(planes, ci, info):
    return [p[ci.origin_y[c]:ci.origin_y[c] + info.sizes_y[c], ci.origin_x[c]:ci.origin_x[c] + info.sizes_x[c]] for c, p in enumerate(planes)]


@pytest.mark.parametrize("subseq_bytes,device_scan", LONE)
@pytest.mark.parametrize("kind", list(KINDS))
def test_lone_decode(torch_cuda, corpus, refs, kind, subseq_bytes, device_scan):
    n = 0
    for name, c in corpus.items():
        if kind not in kinds_of(c):
            continue
        got = decode(torch_cuda, c.data, kind, subseq_bytes, device_scan)[0]
        _assert_planes(got, refs.of(name, kind), (name, kind, subseq_bytes, device_scan))
        n += 1
    assert n == (2 if kind.startswith("draft") else len(corpus))


def du_table(torch, tmp, base, sl):
    """(physical index of the first entry, entries, escape flag) per data unit, as the write pass left them."""
    tab = gpu_util.tmp_view(torch, tmp, base, sl.off_du_table, sl.num_data_units * 2, torch.int32).view(np.uint32).reshape(-1, 2)
    return tab[:, 0].astype(np.int64), (tab[:, 1] & 127).astype(np.int64), (tab[:, 1] & 128) != 0


@pytest.mark.parametrize("subseq_bytes,device_scan", LONE)
def test_symbol_stream_and_gather_coverage(torch_cuda, corpus, subseq_bytes, device_scan):
    """The coefficients rebuilt from the symbol stream equal the blocks (so a plane that differs in test_lone_decode is the
    transform's doing, not the write pass's), the data-unit table holds the counts and escape flags the host worked out,
    and -- as a condition, not a hope -- the packed ladder meets idct_kernel's gather at its edge in every way: units
    of 31, 32 and 33 entries with an even AND an odd first entry (with an odd one the 32nd entry lies behind the two
    prefetched words), and every sector offset 0..15 of the first entry among units of 17 entries and more (`over` in
    `prefetch`)."""
    torch = torch_cuda
    for name, c in corpus.items():
        _, _, _, _, tmp, base, lay = decode(torch, c.data, "reference", subseq_bytes, device_scan)
        assert lay.num_scans == 1
        sl = lay.scans[0]
        S = None
        if sl.device_scan:
            words = gpu_util.tmp_view(torch, tmp, base, sl.off_device_status, 5, torch.int32)
            assert words[0] == 0
            S = int(words[1])
        coef = gpu_util.stream_coefficients(torch, tmp, base, sl, S)
        bad = np.flatnonzero((coef != c.stream).any(axis=1))
        assert len(bad) == 0, (name, len(bad), bad[:5], c.label[bad[:5]])
        first, cnt, esc = du_table(torch, tmp, base, sl)
        assert np.array_equal(cnt, idct_cases.entry_count(c.stream)) and np.array_equal(esc, idct_cases.has_escape(c.stream)), name
        if name == "counts_plain_packed":
            missing = [(n, parity) for n in (31, 32, 33) for parity in (0, 1) if not ((cnt == n) & ((first & 1) == parity)).any()]
            assert not missing, (subseq_bytes, "no unit of (entries, parity of the first entry)", missing)
            offsets = set(first[cnt >= 17] & 15)
            assert offsets == set(range(16)), (subseq_bytes, "sector offsets without a unit of 17 entries and more", sorted(set(range(16)) - offsets))
            # units whose entries behind the prefetched words only the tail loop of the `!plain` path places. (This file
            # holds no escape; elsewhere a unit beside an escaped one in its group takes the per-entry path instead.)
            assert not esc.any()
            tail = cnt > 32 - (first & 1)
            print("\n%s subseq_bytes=%d device_scan=%s: units of 31/32/33 entries, even first entry %s, odd first entry %s; units the tail loop "
                  "serves %d, of them at 32 or 33 entries %d" % (name, subseq_bytes, device_scan,
                                                                 [int(((cnt == n) & (first & 1 == 0)).sum()) for n in (31, 32, 33)],
                                                                 [int(((cnt == n) & (first & 1 == 1)).sum()) for n in (31, 32, 33)],
                                                                 int(tail.sum()), int((tail & (cnt <= 33)).sum())))
        if name == "counts_plain_restart":  # every unit starts a region: every first entry even, the 32nd entry always prefetched
            assert (first & 15 == 0).all(), name


def mcu_window(case, info, ci, si, kind):
    """(mx0, my0, mx1, my1), inclusive: the MCUs whose units a cropped decode transformed, from the windows it reports."""
    d = KINDS[kind][1]
    x0 = y0 = 1 << 30
    x1 = y1 = -1
    for c in range(info.num_components):
        bs = si.block_size[c] if KINDS[kind][2] == "libjpeg" and d > 1 else 8 // d
        h, v = case.sampling[c]
        x0, y0 = min(x0, ci.origin_x[c] // (h * bs)), min(y0, ci.origin_y[c] // (v * bs))
        x1, y1 = max(x1, (ci.origin_x[c] + info.sizes_x[c] - 1) // (h * bs)), max(y1, (ci.origin_y[c] + info.sizes_y[c] - 1) // (v * bs))
    return x0, y0, x1, y1


def crop_rectangles(case, kind):
    """Two rectangles in pixels of the image at the kind's scale: (1) its MCU window has special units on its first and
    last MCU column and row; (2) its MCU window holds no special unit but has some next to it -- None where the file has
    no such place (files that are special throughout). A margin keeps the one-sample halo of every component inside the
    chosen MCUs: one pixel, three where chroma is subsampled (its halo sample is two pixels wide and starts at an even one;
    in libjpeg's scale mode the chroma blocks of a 4:2:0 file are twice the size and no subsampling is left)."""
    S = case.special_mcus()
    rows, cols = S.shape
    mcu = 8 * case.sampling[0][0] // KINDS[kind][1]  # MCU side in pixels at the scale (4:2:0 and grayscale: square)
    margin = 1 if case.gray or kind.startswith("draft") else 3

    def pixels(c0, r0, c1, r1):
        x, y = c0 * mcu + margin, r0 * mcu + margin
        return x, y, (c1 + 1) * mcu - margin - x, (r1 + 1) * mcu - margin - y

    need = -(-(2 * margin + 1) // mcu)  # MCUs a side needs for the rectangle to hold a pixel
    return pixels(*edged_window(S, max(need, 4))), next((pixels(*w) for w in quiet_windows(S, need)), None)


def edged_window(S, side):
    """(c0, r0, c1, r1): the first window of side x side MCUs or more, away from the frame's edge, whose first and last row
    and column all hold a special MCU."""
    rows, cols = S.shape
    side = min(side, rows - 2)  # (the shortest file has five block rows)
    for r0 in range(1, rows - side):
        for c0 in range(1, cols - side):
            for r1 in range(r0 + side - 1, min(r0 + side + 3, rows - 1)):
                for c1 in range(c0 + side - 1, min(c0 + side + 24, cols - 1)):
                    if S[r0, c0:c1 + 1].any() and S[r1, c0:c1 + 1].any() and S[r0:r1 + 1, c0].any() and S[r0:r1 + 1, c1].any():
                        return c0, r0, c1, r1
    raise AssertionError("no window with special MCUs on all four edges")


def quiet_windows(S, need):
    """(c0, r0, c1, r1) of the windows without a special MCU that have two or more next to them, low and wide ones first."""
    rows, cols = S.shape
    for h in range(need, need + 3):
        for w in range(need + 4, need - 1, -1):
            for r in range(rows - h + 1):
                for c in range(cols - w + 1):
                    if not S[r:r + h, c:c + w].any() and S[max(r - 1, 0):r + h + 1, max(c - 1, 0):c + w + 1].sum() >= 2:
                        yield c, r, c + w - 1, r + h - 1


@pytest.mark.parametrize("kind", list(KINDS))
def test_crops(torch_cuda, corpus, refs, kind):
    """Two windows per file: special units on the window's edges, and a window without them whose neighbours they are.
    The window planes equal the same windows of the uncropped reference."""
    n = quiet = inside = 0
    for k, (name, c) in enumerate(corpus.items()):
        if kind not in kinds_of(c):
            continue
        full = refs.of(name, kind)
        S = c.special_mcus()
        for which, rect in enumerate(crop_rectangles(c, kind)):
            if rect is None:
                assert not (c.setting == "a").any(), (name, "a file with ordinary units has a window without special ones")
                continue
            got, info, ci, si, _, _, _ = decode(torch_cuda, c.data, kind, (32, 256)[(k + which) % 2], bool((k + which) & 2), crop=rect)
            _assert_planes(got, window_of(full, ci, info), (name, kind, rect))
            x0, y0, x1, y1 = mcu_window(c, info, ci, si, kind)
            inside += int(S[y0:y1 + 1, x0:x1 + 1].sum() and c.special.reshape(S.shape + (-1,))[y0:y1 + 1, x0:x1 + 1].sum())
            if which == 0:
                assert S[y0, x0:x1 + 1].any() and S[y1, x0:x1 + 1].any() and S[y0:y1 + 1, x0].any() and S[y0:y1 + 1, x1].any(), (name, kind, rect)
            else:
                assert not S[y0:y1 + 1, x0:x1 + 1].any() and S[max(y0 - 1, 0):y1 + 2, max(x0 - 1, 0):x1 + 2].any(), (name, kind, rect)
                quiet += 1
            n += 1
    print("\n%s: %d cropped decodes, %d of them without a special unit, %d special units inside the others' windows" % (kind, n, quiet, inside))
    assert quiet >= (2 if kind.startswith("draft") else 11) and n >= quiet + (2 if kind.startswith("draft") else len(corpus))


def batch_decode(torch, items, hint):
    """items: [(bytes, kind, crop or None)] through ONE jpeggpu_ext_decode_batch call: [(planes, info, crop_info)]."""
    import jpeggpu_amd

    keep, entries, total = [], [], 0
    for k, (data, kind, crop) in enumerate(items):
        dec = jpeggpu_amd.Decoder()
        dec.set_batch_hint(hint)
        configure(dec, kind, k % 3 == 1, crop)
        info = dec.parse_header(data)
        n = dec.get_buffer_size()
        tmp, base = _tmp(torch, n)
        g = Guarded(torch, info)
        dec.transfer(base, n, 0)
        total += dec.layout().num_scans
        keep.append((dec, tmp, g, base, info))
        entries.append((dec, g.ptrs, g.pitches, base, n))
    batch = jpeggpu_amd.Batch(total)
    scratch = torch.empty(batch.scratch_size, dtype=torch.uint8, device="cuda:0")
    batch.set_items(entries)
    batch.decode(scratch.data_ptr(), 0)
    torch.cuda.synchronize()
    out = []
    for dec, _t, g, base, info in keep:
        assert dec.device_status(base, 0) == jpeggpu_amd.Status.SUCCESS
        out.append((g.planes(), info, dec.crop_info()))
        dec.cleanup()
    batch.destroy()
    return out


# What one batch call holds decides which instantiations launch_idct picks for ALL of its items (jg_idct.hip): a single
# cropped item makes every launch a CropJobs one; full-size items of both methods, or ISLOW ones beside scaled ones, take
# JobArrayFullSizeOf<m>; reference items beside scaled ones and no ISLOW item take JobArrayFullSize. So several calls.
COMPOSITIONS = {
    # CropJobs<JobArrayFullSizeOf<m>>, IslowJobs<CropJobs<..>>, idct_scaled_kernel<CropJobs<JobArray>, lg>, DraftJobs<JobArray> with windows
    "with_crops": (list(KINDS), True),
    # the same without a window: JobArrayFullSizeOf<kIdctReference>, IslowJobs<JobArrayFullSizeOf<kIdctIslow>>,
    # idct_scaled_kernel<JobArray, lg>, DraftJobs<JobArray>
    "all": (list(KINDS), False),
    # full size only, both methods: the two JobArrayFullSizeOf<m> launches and nothing else
    "methods_only": (["reference", "islow"], False),
    # no ISLOW item: idct_kernel<JobArrayFullSize> beside idct_scaled_kernel<JobArray, lg>
    "reference_and_scaled": (["reference", "scale2", "scale4", "scale8"], False),
    # no reference item: IslowJobs<JobArrayFullSizeOf<kIdctIslow>> alone beside the scaled kernels
    "islow_and_scaled": (["islow", "scale2", "scale4", "scale8"], False),
    # one method, one scale: idct_kernel<JobArray> and IslowJobs<JobArray>, the plain batch sources
    "reference_only": (["reference"], False),
    "islow_only": (["islow"], False),
}


@pytest.mark.parametrize("full_batch_kernels", [False, True])
@pytest.mark.parametrize("composition", list(COMPOSITIONS))
def test_one_batch_holds_every_file(torch_cuda, corpus, refs, monkeypatch, composition, full_batch_kernels):
    """Every file, as every kind of item the composition allows (COMPOSITIONS: which job sources of jg_idct.hip the call
    then launches), beside two ordinary matrix files; "with_crops" adds two cropped items per file. Once with the kernels
    small calls get and once with the full-batch plan. Every item equals its lone reference."""
    monkeypatch.setenv("JPEGGPU_EXP_KEEP_FLOWS_BELOW", "0" if full_batch_kernels else "1000000000")  # read at jpeggpu_ext_batch_create
    import jpeggpu_amd

    kinds, crops = COMPOSITIONS[composition]
    items, what = [], []
    for k, (name, c) in enumerate(corpus.items()):
        mine = [kind for kind in kinds_of(c) if kind in kinds]
        for kind in mine:
            items.append((c.data, kind, None))
            what.append((name, kind, None))
        crop_kinds = [kd for kd in mine if kd != "reference"]
        for j in range(2 if crops else 0):
            kind = crop_kinds[(k + 3 * j) % len(crop_kinds)]
            first, second = crop_rectangles(c, kind)
            rect = second if j and second is not None else first
            items.append((c.data, kind, rect))
            what.append((name, kind, rect))
    for j, name in enumerate(("matrix:ni_420_dri", "matrix:q100_noisy")):
        for kind in kinds[::2]:
            at = (j * 4 + len(what) // 3) % len(what)
            items.insert(at, (refs.files[name], kind, None))
            what.insert(at, (name, kind, None))
    assert {w[1] for w in what} == set(kinds) and sum(w[2] is not None for w in what) == (2 * len(corpus) if crops else 0)
    for (planes, info, ci), (name, kind, rect) in zip(batch_decode(torch_cuda, items, 64 if full_batch_kernels else 0), what):
        want = refs.of(name, kind)
        _assert_planes(planes, window_of(want, ci, info) if rect else want, (name, kind, rect, composition, full_batch_kernels))
    assert jpeggpu_amd.fused_tail_timeouts() == 0
