"""Runs of subsequences per lane in the batched sequence kernel (huff_sync_intra_batch<W, JS, R>, jg_sync_runs.h) on the
GPU: batched calls on the full batch's path (forced: these items alone do not fill the chip) with runs of 2 and 4, the
tail kernel fused with the write pass and not, at 128- and 256-byte subsequences. The planes equal the CPU oracle's and
those of the same items decoded with runs of 1; every item's state arrays and symbol stream are checked against the CPU
twin as well. Inputs: tests/syncruns/inputs.py (segments of 1, 2, 3 and R + 1 subsequences, scans of fewer than R, of
exactly 255 R and 255 R + 1 subsequences, with and without restart markers, interleaved, three scans, four components),
a stream that synchronises slowly and the long-magnitude file. A few seconds per case."""
import numpy as np
import pytest

from tests import cases
from tests.syncprobe import crafted
from tests.syncruns import inputs
from tests.test_gpu_scaled import Guarded, _tmp
from tests.test_gpu_slow_sync import _assert_planes, check_stages

pytestmark = pytest.mark.gpu

CANARY = 0x5A


@pytest.fixture(scope="module")
def torch_cuda(gpu_lib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def full_batches():
    """Every batch of this module takes the kernels of a call that fills the chip (read at jpeggpu_ext_batch_create)."""
    mp = pytest.MonkeyPatch()
    mp.setenv("JPEGGPU_EXP_KEEP_FLOWS_BELOW", "0")
    mp.delenv("JPEGGPU_SYNC_RUN", raising=False)
    yield
    mp.undo()


_refs = {}


def _ref(data):
    from oracle import oracle

    if data not in _refs:
        _refs[data] = oracle.decode(data).planes
    return _refs[data]


def _files(r, subseq_bytes):
    out = inputs.files(r, subseq_bytes)
    out["slow_dri48"] = cases.slow_sync()["s420_763_dri48"].data
    out["long_magnitudes"] = crafted.long_magnitude_case()
    return out


def _decode(torch, datas, sizes, r, fused, stages=True):
    """One jpeggpu_ext_decode_batch call with runs of r: (planes per item, device status per item). `sizes`: the
    subsequence size of every item. The tmp buffers lie between canaries, the planes in guarded buffers."""
    import jpeggpu_amd

    keep, entries, total, guard = [], [], 0, 4096
    for data, size in zip(datas, sizes):
        dec = jpeggpu_amd.Decoder(size)
        dec.set_batch_hint(64)
        info = dec.parse_header(data)
        n = dec.get_buffer_size()
        tmp = torch.full((n + 256 + 2 * guard,), CANARY, dtype=torch.uint8, device="cuda:0")
        base = (tmp.data_ptr() + guard + 255) // 256 * 256
        g = Guarded(torch, info)
        dec.transfer(base, n, 0)
        total += dec.layout().num_scans
        keep.append((dec, tmp, g, base, n))
        entries.append((dec, g.ptrs, g.pitches, base, n))
    batch = jpeggpu_amd.Batch(total)
    try:
        scratch = torch.empty(batch.scratch_size, dtype=torch.uint8, device="cuda:0")
        batch.set_items(entries)
        batch.set_sync_run(r)
        batch.set_fused_tail(fused)
        batch.decode(scratch.data_ptr(), 0)
        torch.cuda.synchronize()
        planes, status = [], []
        for k, (dec, tmp, g, base, n) in enumerate(keep):
            off = base - tmp.data_ptr()
            assert (tmp[:off] == CANARY).all() and (tmp[off + n:] == CANARY).all(), ("tmp overrun", k, r, fused)
            status.append(dec.device_status(base, 0))
            lay = dec.layout()
            assert lay.subsequences_per_sequence == 255 and lay.subsequence_bytes == sizes[k], (k, r, fused)
            if stages:
                check_stages(torch, datas[k], tmp, base, lay, sizes[k], ("item", k, "runs of", r, "fused", fused))
            planes.append(g.planes())
        return planes, status
    finally:
        batch.destroy()
        for dec, *_ in keep:
            dec.cleanup()


@pytest.mark.parametrize("subseq_bytes", [128, 256])
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("r", [2, 4])
def test_runs_equal_oracle_and_single_subsequences(torch_cuda, full_batches, r, fused, subseq_bytes):
    import jpeggpu_amd

    files = _files(r, subseq_bytes)
    names, datas = list(files), list(files.values())
    sizes = [subseq_bytes] * len(datas)
    got, status = _decode(torch_cuda, datas, sizes, r, fused)
    one, status_one = _decode(torch_cuda, datas, sizes, 1, fused, stages=False)
    assert status == status_one == [jpeggpu_amd.Status.SUCCESS] * len(datas)
    for name, data, a, b in zip(names, datas, got, one):
        _assert_planes(a, _ref(data), (name, r, fused, subseq_bytes, "against the oracle"))
        _assert_planes(a, b, (name, r, fused, subseq_bytes, "against runs of 1"))
    assert jpeggpu_amd.fused_tail_timeouts() == 0


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("r", [2, 4])
def test_one_call_with_both_subsequence_sizes(torch_cuda, full_batches, r, fused):
    import jpeggpu_amd

    datas, sizes = [], []
    for size in (128, 256):
        f = _files(r, size)
        for name in ("segments_of_3", "255r_plus_1", "420_dri", "three_scans", "slow_dri48", "fewer_than_r"):
            datas.append(f[name])
            sizes.append(size)
    order = np.random.default_rng(r).permutation(len(datas))  # the call sorts its items by size: hand them over mixed
    datas, sizes = [datas[i] for i in order], [sizes[i] for i in order]
    got, status = _decode(torch_cuda, datas, sizes, r, fused)
    one, _ = _decode(torch_cuda, datas, sizes, 1, fused, stages=False)
    assert status == [jpeggpu_amd.Status.SUCCESS] * len(datas)
    for k, (data, a, b) in enumerate(zip(datas, got, one)):
        _assert_planes(a, _ref(data), (k, sizes[k], r, fused, "against the oracle"))
        _assert_planes(a, b, (k, sizes[k], r, fused, "against runs of 1"))
    assert jpeggpu_amd.fused_tail_timeouts() == 0


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("r", [2, 4])
def test_damaged_item_among_good_ones(torch_cuda, full_batches, r, fused):
    """One item whose entropy data is damaged (bytes replaced, the marker structure intact: its planes are garbage by
    definition) between good ones: the call returns what it returns with runs of 1, every buffer's canaries survive, and
    the good items stay bit-exact. (It damages bytes and checks memory; nothing here provokes a fault.)"""
    import jpeggpu_amd
    from oracle import oracle

    f = _files(r, 128)
    good = [f["420_dri"], f["segments_of_3"], f["255r_plus_1"], f["no_restart"]]
    victim = f["slow_dri48"]
    lo, hi = oracle.scan_info(victim, 0, 128).scan_begin, oracle.scan_info(victim, 0, 128).scan_end
    rng = np.random.default_rng(99)
    bad = bytearray(victim)
    for pos in rng.integers(lo + 4, hi - 4, size=60):
        if bad[pos] != 0xFF and bad[pos - 1] != 0xFF and bad[pos + 1] != 0xFF:
            bad[pos] = int(rng.integers(0, 255))  # never 0xFF
    datas = good[:2] + [bytes(bad)] + good[2:]
    sizes = [128] * len(datas)
    got, status = _decode(torch_cuda, datas, sizes, r, fused, stages=False)
    one, status_one = _decode(torch_cuda, datas, sizes, 1, fused, stages=False)
    assert status == status_one
    for k, (data, a, b) in enumerate(zip(datas, got, one)):
        if k != 2:
            _assert_planes(a, _ref(data), (k, r, fused, "good item beside a damaged one"))
            _assert_planes(a, b, (k, r, fused, "against runs of 1"))
    assert jpeggpu_amd.fused_tail_timeouts() == 0
    # the device still decodes correctly afterwards
    planes, _ = jpeggpu_amd.decode_to_planes(good[0])
    _assert_planes([p.cpu().numpy() for p in planes], _ref(good[0]), "after the damaged call")


def test_setter_accepts_1_2_4_only(torch_cuda):
    import jpeggpu_amd

    batch = jpeggpu_amd.Batch(4)
    try:
        for r in (1, 2, 4):
            batch.set_sync_run(r)
        for r in (0, 3, 8, -1):
            with pytest.raises(jpeggpu_amd.JpegGpuError):
                batch.set_sync_run(r)
    finally:
        batch.destroy()
