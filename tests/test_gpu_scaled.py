"""Scaled decoding on the GPU (jpeggpu_ext_set_scale): every entry point at 1/2, 1/4 and 1/8 size against the numpy
restatement of libjpeg-turbo's reduced IDCTs (tests/scaled_ref.py), with guard bytes around every plane."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from tests import cases, scaled_ref

pytestmark = pytest.mark.gpu

GUARD = 0x5A


@pytest.fixture(scope="module")
def torch_cuda(gpu_lib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def matrix():
    return cases.matrix()


class Guarded:
    """Planes of `info` inside larger buffers: two guard rows above and below, 8 guard bytes in front of every row and a
    padded pitch behind it. A kernel that used full-size geometry, or any wrong placement, writes into the guards."""

    def __init__(self, torch, info):
        self.bufs, self.ptrs, self.pitches, self.shape = [], [], [], []
        for c in range(info.num_components):
            w, h = info.sizes_x[c], info.sizes_y[c]
            buf = torch.full((h + 4, w + 8 + 21), GUARD, dtype=torch.uint8, device="cuda:0")
            self.bufs.append(buf)
            self.ptrs.append(buf[2:, 8:].data_ptr())
            self.pitches.append(buf.stride(0))
            self.shape.append((h, w))

    def planes(self):
        out = []
        for buf, (h, w) in zip(self.bufs, self.shape):
            a = buf.cpu().numpy()
            inner = a[2:2 + h, 8:8 + w].copy()
            a[2:2 + h, 8:8 + w] = GUARD
            assert (a == GUARD).all(), "a guard byte around the plane was written"
            out.append(inner)
        return out


def _tmp(torch, n):
    tmp = torch.empty(n + 256, dtype=torch.uint8, device="cuda:0")
    return tmp, (tmp.data_ptr() + 255) // 256 * 256


def decode_scaled(torch, data, d, subseq_bytes=None, device_scan=False):
    import jpeggpu_amd

    dec = jpeggpu_amd.Decoder(subseq_bytes)
    try:
        dec.set_scale(d)
        dec.set_device_scan(device_scan)
        info = dec.parse_header(data)
        n = dec.get_buffer_size()
        tmp, base = _tmp(torch, n)
        g = Guarded(torch, info)
        dec.transfer(base, n, 0)
        dec.decode(g.ptrs, g.pitches, base, n, 0)
        torch.cuda.synchronize()
        if device_scan:
            assert dec.device_status(base, 0) == jpeggpu_amd.Status.SUCCESS
        return g.planes(), info
    finally:
        dec.cleanup()


def _assert_planes(got, want, what):
    assert len(got) == len(want), what
    for c, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape, (what, c, a.shape, b.shape)
        if not np.array_equal(a, b):
            bad = np.argwhere(a != b)
            raise AssertionError("%s component %d: %d samples differ, first at %s" % (what, c, len(bad), bad[0]))


@pytest.mark.parametrize("subseq_bytes,device_scan", [(32, False), (32, True), (256, False), (256, True)])
def test_matrix_at_every_scale(torch_cuda, matrix, subseq_bytes, device_scan):
    from oracle import oracle

    for name, data in matrix.items():
        dec = oracle.decode(data)
        for d in (2, 4, 8):
            got, info = decode_scaled(torch_cuda, data, d, subseq_bytes, device_scan)
            _assert_planes(got, scaled_ref.scaled_planes_of(dec, d), (name, d, subseq_bytes, device_scan))


def test_reference_photo_at_every_scale(torch_cuda, photo_bytes):
    from oracle import oracle

    dec = oracle.decode(photo_bytes)
    for d in (1, 2, 4, 8):
        for device_scan in (False, True):
            got, _ = decode_scaled(torch_cuda, photo_bytes, d, device_scan=device_scan)
            _assert_planes(got, scaled_ref.scaled_planes_of(dec, d), ("IMG_6510", d, device_scan))


@pytest.mark.parametrize("cfg", [2, 4, 5])
def test_baseline_configs_full_size_at_one_eighth(torch_cuda, cfg):
    from oracle import oracle
    from tools import jpegsynth

    data = jpegsynth.config(cfg, seed=5)
    want = scaled_ref.scaled_planes_of(oracle.decode(data), 8)
    for device_scan in (False, True):
        got, _ = decode_scaled(torch_cuda, data, 8, device_scan=device_scan)
        _assert_planes(got, want, (cfg, device_scan))


def _batch_decode(torch, items, batched_hint):
    """items: [(bytes, d)] through one jpeggpu_ext_decode_batch call; returns (planes per item, infos)."""
    import jpeggpu_amd

    keep, entries, infos, total = [], [], [], 0
    for k, (data, d) in enumerate(items):
        dec = jpeggpu_amd.Decoder()
        dec.set_batch_hint(batched_hint)
        dec.set_scale(d)
        dec.set_device_scan(k % 3 == 1)
        info = dec.parse_header(data)
        n = dec.get_buffer_size()
        tmp, base = _tmp(torch, n)
        g = Guarded(torch, info)
        dec.transfer(base, n, 0)
        total += dec.layout().num_scans
        keep.append((dec, tmp, g, base))
        entries.append((dec, g.ptrs, g.pitches, base, n))
        infos.append(info)
    batch = jpeggpu_amd.Batch(total)
    scratch = torch.empty(batch.scratch_size, dtype=torch.uint8, device="cuda:0")
    batch.set_items(entries)
    batch.decode(scratch.data_ptr(), 0)
    torch.cuda.synchronize()
    out = []
    for dec, _tmp_, g, base in keep:
        assert dec.device_status(base, 0) == jpeggpu_amd.Status.SUCCESS
        out.append(g.planes())
        dec.cleanup()
    batch.destroy()
    return out, infos


def test_batch_mixes_scales(torch_cuda, matrix):
    import jpeggpu_amd
    from oracle import oracle

    names = ["multi_seq_dri", "ni_420_dri", "four_comp_opt", "gray", "odd_1x1px", "cfg4_small", "dri_1", "odd_partial_mcu",
             "ss_4x1", "q16_tables", "dense_escapes", "ni_big_last"]
    items = [(matrix[name], (1, 2, 4, 8)[k % 4]) for k, name in enumerate(names + names[::-1])]
    for hint in (0, 64):
        got, _ = _batch_decode(torch_cuda, items, hint)
        for (data, d), planes, name in zip(items, got, names + names[::-1]):
            ref = oracle.decode(data)
            want = ref.planes if d == 1 else scaled_ref.scaled_planes_of(ref, d)
            _assert_planes(planes, want, (name, d, hint))
    assert jpeggpu_amd.fused_tail_timeouts() == 0


@pytest.mark.parametrize("d", [8, 2])
def test_full_batch_of_64_twelve_megapixel_images_scaled(torch_cuda, d):
    """BASELINE.json configs[2] (64 x 12 MP 4:2:0) in one call at 1/d: the fused huff_tail_write launch, then the scaled
    IDCT; plane hashes against the restatement."""
    import jpeggpu_amd
    from oracle import oracle
    from tools import jpegsynth

    datas = [jpegsynth.config(2, seed=100 + s) for s in range(4)]
    want = [[hashlib.sha256(p.tobytes()).hexdigest() for p in scaled_ref.scaled_planes_of(oracle.decode(x), d)] for x in datas]
    got, _ = _batch_decode(torch_cuda, [(datas[i % 4], d) for i in range(64)], 64)
    bad = [i for i, planes in enumerate(got) if [hashlib.sha256(p.tobytes()).hexdigest() for p in planes] != want[i % 4]]
    assert not bad, bad
    assert jpeggpu_amd.fused_tail_timeouts() == 0


def test_segment_shard_bands_at_scale(torch_cuda, matrix):
    import jpeggpu_amd
    from oracle import oracle
    from tools import jpegsynth

    torch = torch_cuda
    inputs = {"dri_row": matrix["dri_row"], "gray_rows": jpegsynth.encode(200, 152, ((1, 1),), restart_interval=50, seed=77),
              "two_rows": jpegsynth.encode(333, 251, cases.S420, restart_interval=42, seed=78)}
    for name, data in inputs.items():
        ref = oracle.decode(data)
        for d in (2, 8):
            want = scaled_ref.scaled_planes_of(ref, d)
            for world in (2, 3):
                planes = [torch.full(p.shape, 0xAB, dtype=torch.uint8, device="cuda:0") for p in want]
                for rank in range(world):
                    dec = jpeggpu_amd.Decoder(32 if rank % 2 else 64)
                    dec.set_scale(d)
                    dec.set_segment_shard(rank, world)
                    info = dec.parse_header(data)
                    assert [(info.sizes_y[c], info.sizes_x[c]) for c in range(info.num_components)] == [p.shape for p in want]
                    n = dec.get_buffer_size()
                    tmp, base = _tmp(torch, n)
                    before = [p.clone() for p in planes]
                    dec.transfer(base, n, 0)
                    dec.decode([p.data_ptr() for p in planes], [p.stride(0) for p in planes], base, n, 0)
                    torch.cuda.synchronize()
                    for c in range(info.num_components):
                        a, cnt = dec.shard_rows(c)
                        assert torch.equal(planes[c][:a], before[c][:a]) and torch.equal(planes[c][a + cnt:], before[c][a + cnt:]), (name, d, world, rank, c)
                        assert np.array_equal(planes[c][a:a + cnt].cpu().numpy(), want[c][a:a + cnt]), (name, d, world, rank, c)
                    dec.cleanup()
                for c in range(len(want)):
                    assert np.array_equal(planes[c].cpu().numpy(), want[c]), (name, d, world, c)


def test_planes_to_rgbi_on_scaled_420(torch_cuda, matrix):
    import jpeggpu_amd
    from jpeggpu_amd.api import Img, lib
    from oracle import oracle

    torch = torch_cuda
    for name in ("ss_2x2", "odd_partial_mcu", "odd_17x9"):
        data = matrix[name]
        ref = oracle.decode(data)
        for d in (2, 4, 8):
            planes, info = jpeggpu_amd.decode_to_planes(data, scale=d)
            W, H = info.sizes_x[0], info.sizes_y[0]  # luma has the maximum factors in these files
            assert (W, H) == (-(-ref.width // d), -(-ref.height // d))
            src = Img()
            for c in range(3):
                src.image[c], src.pitch[c] = planes[c].data_ptr(), planes[c].stride(0)
            pitch = 3 * W + 5
            out = torch.full((H, pitch), GUARD, dtype=torch.uint8, device="cuda:0")
            assert lib().jpeggpu_ext_planes_to_rgbi(C.byref(info), C.byref(src), out.data_ptr(), pitch, W, H, None) == 0
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            assert (got[:, 3 * W:] == GUARD).all(), (name, d)
            got = got[:, :3 * W].reshape(H, W, 3).astype(np.int32)
            want = oracle.planes_to_rgbi(scaled_ref.scaled_planes_of(ref, d), list(info.subsampling.x), list(info.subsampling.y), W, H)
            diff = np.abs(got - want.astype(np.int32))
            assert diff.max() <= 1 and (diff == 0).mean() > 0.99, (name, d, int(diff.max()))


def test_corrupt_entropy_data_at_one_eighth_is_memory_safe(torch_cuda, matrix):
    """Random damage inside the entropy-coded segment, decoded at 1/8 alone and as a batch item: every decode completes,
    stays inside d_tmp and the planes' guards, and the device decodes correctly afterwards."""
    import jpeggpu_amd
    from oracle import oracle

    torch = torch_cuda
    rng = np.random.default_rng(4321)
    for name in ("multi_seq_dri", "multi_seq_nodri", "four_comp_opt", "ni_420_dri"):
        good = matrix[name]
        lo, hi = oracle.scan_info(good, 0, 128).scan_begin, oracle.scan_info(good, 0, 128).scan_end
        for trial in range(4):
            bad = bytearray(good)
            for pos in rng.integers(lo + 4, hi - 4, size=int(rng.integers(1, 40))):
                if bad[pos] != 0xFF and bad[pos - 1] != 0xFF:
                    bad[pos] = int(rng.integers(0, 255))
            for batched in (False, True):
                dec = jpeggpu_amd.Decoder(int(rng.choice([32, 64, 128])))
                dec.set_scale(8)
                dec.set_device_scan(bool(trial & 1))
                if batched:
                    dec.set_batch_hint(64)
                try:
                    info = dec.parse_header(bytes(bad))
                except jpeggpu_amd.JpegGpuError:
                    dec.cleanup()
                    continue
                n = dec.get_buffer_size()
                guard = 4096
                tmp = torch.full((n + 256 + 2 * guard,), GUARD, dtype=torch.uint8, device="cuda:0")
                base = (tmp.data_ptr() + guard + 255) // 256 * 256
                g = Guarded(torch, info)
                dec.transfer(base, n, 0)
                if batched:
                    batch = jpeggpu_amd.Batch(dec.layout().num_scans)
                    scratch = torch.empty(batch.scratch_size, dtype=torch.uint8, device="cuda:0")
                    batch.set_items([(dec, g.ptrs, g.pitches, base, n)])
                    batch.decode(scratch.data_ptr(), 0)
                else:
                    dec.decode(g.ptrs, g.pitches, base, n, 0)
                torch.cuda.synchronize()
                off = base - tmp.data_ptr()
                assert (tmp[:off] == GUARD).all() and (tmp[off + n:] == GUARD).all(), (name, trial, batched, "tmp overrun")
                g.planes()  # raises if a guard byte was written
                if batched:
                    batch.destroy()
                dec.cleanup()
        got, _ = decode_scaled(torch, good, 8)
        _assert_planes(got, scaled_ref.scaled_planes(good, 8), (name, "after damage"))
    assert jpeggpu_amd.fused_tail_timeouts() == 0
