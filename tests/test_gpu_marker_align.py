"""Markers and stuffing at every lane, wave and window boundary, on the GPU (tests/marker_align_cases.py; its CPU half is
tests/test_marker_align_ref.py): every variant through the device-side marker scan (jg_front.hip) and through the host walk,
in batches and alone, planes against the oracle's decode of the BASE file, and the tables the device builds against the
host walk's. The subsequence size is pinned to 32 and 128 everywhere: the per-image choice depends on the file length,
which the fill bytes change.

What "equal tables" means (read from the code, marker_align_cases' docstring has the derivation): the segment tables are
equal byte for byte. The chunk tables are equal except where a variant has fill bytes: the host walk ends a segment's
bytes at the first FF of the fill run, the device at the last, so the `end` of that segment's last chunk lies `fill`
bytes further on the device, and the device has one more chunk for every fill byte on a window's first byte. Both are
right -- a fill byte is no data byte, the destuffed bytes are the same -- so neither walk was changed; the tests assert
the device's table to be the host's with exactly that difference, and its chunk COUNT where the lists differ in length.
The layout does not expose the host walk's tail parts; the device's count is held against front_plan's rule applied to
the host's segment table."""
import numpy as np
import pytest

import jpeggpu_amd
from jpeggpu_amd import JpegGpuError, Status
from oracle import oracle
from tests import marker_align_cases as M
from tests.gpu_util import tmp_view

pytestmark = pytest.mark.gpu

BATCH = 128
SUBSEQ = (32, 128)


@pytest.fixture(scope="module")
def torch_cuda(gpu_lib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def E():
    return M.everything()


@pytest.fixture(scope="module")
def ref(E):
    """name -> the oracle's planes of the base file, computed once and shared (read-only)."""
    out = {}
    for name, data in E["bases"].items():
        out[name] = oracle.decode(data).planes
        for p in out[name]:
            p.setflags(write=False)
    return out


class Item:
    """What one item of a batch left behind: status, planes, and the tables of its scan read back from its tmp buffer."""

    def __init__(self, torch, dec, tmp, planes):
        base = (tmp.data_ptr() + 255) // 256 * 256
        lay = dec.layout()
        sc = lay.scans[lay.num_scans - 1]
        self.status = dec.device_status(base, 0)
        self.planes = [p.cpu().numpy() for p in planes]
        self.device = bool(sc.device_scan)
        view = lambda off, n: tmp_view(torch, tmp, base, off, n, torch.int32)
        self.words = None
        if self.device:
            self.words = [int(x) for x in view(sc.off_device_status, 8).view(np.uint32)[:5]]
            self.num_subseq, nseg, nchunks, self.parts = self.words[1:5]
        else:
            self.num_subseq, nseg, nchunks, self.parts = sc.num_subsequences, sc.num_segments, sc.num_chunks, None
        self.segments = view(sc.off_segments, 2 * nseg).reshape(nseg, 2)
        # {win_off, begin, end, dst_off, pad_end, seg, first, reserved} (DestuffChunk, jg_defs.h)
        self.chunks = view(sc.off_chunks, 8 * nchunks).reshape(nchunks, 8)


def decode_items(torch, datas, device_scan, subseq_bytes, hint=None, prefill=None):
    out = []
    for k in range(0, len(datas), BATCH):
        dev = device_scan[k:k + BATCH] if isinstance(device_scan, list) else device_scan
        with jpeggpu_amd.BatchDecode(datas[k:k + BATCH], idct="reference", device_scan=dev, subseq_bytes=subseq_bytes, hint=hint) as bd:
            if prefill is not None:
                for planes in bd.planes:
                    for p in planes:
                        p.fill_(prefill)
            bd.decode()
            torch.cuda.synchronize()
            out += [Item(torch, dec, tmp, planes) for dec, tmp, planes in zip(bd.decoders, bd.tmps, bd.planes)]
    return out


def assert_planes(item, want, what):
    assert item.status == Status.SUCCESS, (what, item.status)
    assert len(item.planes) == len(want), what
    for k, (got, w) in enumerate(zip(item.planes, want)):
        assert np.array_equal(got, w), (what, k)


def device_chunks_from_host(host_chunks, data):
    """The host walk's chunk table as the device builds it when no fill byte lies on a window's first byte: the last chunk of
    a segment (the one with pad_end) ends `fill` bytes later."""
    out = host_chunks.copy()
    runs = M.fill_runs(data)
    for row in out:
        k = int(row[5])
        if row[4] != 0 and k < len(runs):
            row[2] += runs[k][1] - runs[k][0]
    return out


@pytest.mark.parametrize("subseq_bytes", SUBSEQ)
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_batch_both_walks(torch_cuda, E, ref, name, subseq_bytes):
    """Every variant of a file in batches of at most 128 items, once with the device-side scan per item (FrontMany) and once
    with the host walk; reference IDCT. Planes equal the oracle's decode of the base file; the device's counts and tables
    equal the host walk's, with the one difference the module docstring derives."""
    torch = torch_cuda
    vs = M.variants(name)
    datas = [c.data for c in vs]
    host = decode_items(torch, datas, False, subseq_bytes)
    dev = decode_items(torch, datas, True, subseq_bytes)
    crossing = 0
    for c, h, d in zip(vs, host, dev):
        assert not h.device and d.device, c
        assert_planes(h, ref[name], (c, "host walk"))
        assert_planes(d, ref[name], (c, "device scan"))
        assert d.words[0] == 0, (c, d.words)
        assert d.num_subseq == h.num_subseq and len(d.segments) == len(h.segments), (c, d.words, h.num_subseq, len(h.segments))
        assert d.segments.tobytes() == h.segments.tobytes(), (c, "segment table")
        assert d.parts == M.tail_parts_device(h.segments[:, 0]), (c, d.words)
        extra = M.extra_device_chunks(c.data)
        assert len(d.chunks) == len(h.chunks) + extra, (c, len(d.chunks), len(h.chunks), extra)
        if extra == 0:
            want = device_chunks_from_host(h.chunks, c.data)
            assert np.array_equal(d.chunks, want), (c, "chunk table", np.flatnonzero((d.chunks != want).any(axis=1))[:4])
            if not any(c.fills.values()):
                assert d.chunks.tobytes() == h.chunks.tobytes(), (c, "chunk table")
        else:
            crossing += 1
    if name != "C":
        assert crossing >= 4  # the long fills at least


@pytest.mark.parametrize("subseq_bytes", SUBSEQ)
@pytest.mark.parametrize("name", ["A", "C"])
def test_lone_decode(torch_cuda, E, ref, name, subseq_bytes):
    """jpeggpu_decoder_decode with the device-side scan (FrontOneJob; for C, a scan without restart markers, the blocks of the
    multi-hypothesis chain walk are built on the device too)."""
    for c in M.variants(name):
        planes, _ = jpeggpu_amd.decode_to_planes(c.data, subseq_bytes=subseq_bytes, device_scan=True)
        for k, w in enumerate(ref[name]):
            assert np.array_equal(planes[k].cpu().numpy(), w), (c, k)


@pytest.mark.parametrize("subseq_bytes", SUBSEQ)
def test_full_batch_plan(torch_cuda, E, ref, monkeypatch, subseq_bytes):
    """The plan and the kernels of a call that fills the chip (one flow iteration, the fused tail and write pass), which a
    call this small gets when it is told so: the wave- and window-grid variants, device-scanned and host-walked items
    mixed in one call."""
    monkeypatch.setenv("JPEGGPU_EXP_KEEP_FLOWS_BELOW", "0")  # read at jpeggpu_ext_batch_create
    torch = torch_cuda
    vs = [c for name in ("A", "B") for c in M.variants(name) if c.grid != 16]
    assert len(vs) > 50
    for flip in (0, 1):
        dev = [bool((i + flip) & 1) for i in range(len(vs))]
        items = decode_items(torch, [c.data for c in vs], dev, subseq_bytes, hint=64)
        for c, want_dev, it in zip(vs, dev, items):
            assert it.device == want_dev
            assert_planes(it, ref[c.base], (c, want_dev))
    assert jpeggpu_amd.fused_tail_timeouts() == 0


def test_refusals_alone(torch_cuda, E, ref):
    """Each refusal case: INVALID_JPEG from the host walk at parse time and from the device's status, the planes (pre-filled
    with 0x5A) untouched; the FF FF 00 behind EOI decodes."""
    from tests.test_gpu_api import _decode_device_scan

    torch = torch_cuda
    for r in E["refusals"]:
        want = Status.SUCCESS if r.accepted else Status.INVALID_JPEG
        for sb in SUBSEQ:
            host = jpeggpu_amd.Decoder(sb)
            try:
                host.parse_header(r.data)
                host_status = Status.SUCCESS
            except JpegGpuError as e:
                host_status = e.status
            host.cleanup()
            assert host_status == want, (r, sb, host_status)
            status, planes, lay, words = _decode_device_scan(torch, jpeggpu_amd, r.data, sb)
            assert lay.scans[0].device_scan and status == want, (r, sb, status, words)
            if r.accepted:
                for k, w in enumerate(ref["A"]):
                    assert np.array_equal(planes[k], w), (r, sb, k)
            else:
                assert all((p == 0x5A).all() for p in planes), (r, sb)


@pytest.mark.parametrize("subseq_bytes", SUBSEQ)
def test_refusals_in_a_batch(torch_cuda, E, ref, subseq_bytes):
    """The refused items in one call between good variants: they report their status and leave their planes alone, the good
    ones decode exactly."""
    torch = torch_cuda
    good = [c for c in M.variants("A") if c.grid == M.WIN or c.grid is None]
    entries = []
    for i, r in enumerate(E["refusals"]):
        entries += [good[i % len(good)], r]
    entries.append(good[-1])
    items = decode_items(torch, [e.data for e in entries], True, subseq_bytes, prefill=0x5A)
    for e, it in zip(entries, items):
        assert it.device, e
        if isinstance(e, M.Refusal) and not e.accepted:
            assert it.status == Status.INVALID_JPEG, (e, it.status, it.words)
            assert all((p == 0x5A).all() for p in it.planes), e
        else:
            assert_planes(it, ref["A"], e)


@pytest.mark.parametrize("subseq_bytes", SUBSEQ)
def test_crops_that_begin_at_a_window_edge(torch_cuda, E, subseq_bytes):
    """Reader::cut_segments shifts a crop's chunk list by whole windows (win_shift): a crop whose first kept segment begins on
    a window's first byte, and one whose first segment begins on a window's last byte (host walk)."""
    torch = torch_cuda
    cs = E["crops"]
    datas, rects = [c.data for c, _ in cs], [r for _, r in cs]
    whole = [t.cpu().numpy() for t in jpeggpu_amd.decode_batch_to_rgb(datas, subseq_bytes=subseq_bytes)]
    assert np.array_equal(whole[0], whole[1])
    got = jpeggpu_amd.decode_batch_to_rgb(datas, crops=rects, subseq_bytes=subseq_bytes)
    for (c, (x, y, w, h)), g, full in zip(cs, got, whole):
        assert np.array_equal(g.cpu().numpy(), full[y:y + h, x:x + w]), c
    # the cut did begin where the case says: the first chunk of the kept segments, in the shifted list
    with jpeggpu_amd.BatchDecode(datas, crops=rects, subseq_bytes=subseq_bytes) as bd:
        torch.cuda.synchronize()
        for (c, _), dec, tmp in zip(cs, bd.decoders, bd.tmps):
            sc = dec.layout().scans[0]
            first = tmp_view(torch, tmp, (tmp.data_ptr() + 255) // 256 * 256, sc.off_chunks, 8, torch.int32)
            total = len(M.parse(c.data).rst) + 1
            assert 0 < sc.num_segments < total and first[0] == 0 and first[6] == 1, (c, first)
            assert first[1] == (c.want + 2) % M.WIN, (c, first)
