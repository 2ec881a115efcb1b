"""Sync-pack multi-symbol entries whose last symbol ends behind the index bits (jg_defs.h), on the GPU: a crafted file
whose entries end in 10-bit magnitudes (tests/syncprobe/crafted.py), the densest file a code table allows and a file
with one restart interval per MCU row, through every state-only kernel -- the lone decode's speculation, flows and tail
at 32 and 256 bytes, and the full batch's huff_sync_intra_batch and tail kernel, fused with the write pass and not.
Bit-exact against the CPU oracle: planes, synchronised states, DC sums, symbol stream."""
import pytest

from tests import cases
from tests.syncprobe import crafted
from tests.test_gpu_slow_sync import _assert_planes, _batch, check_stages

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda(gpu_lib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def inputs():
    return {"long_magnitudes": crafted.long_magnitude_case(), "dense_escapes": cases.dense_escape_case(),
            "dri_row": cases.matrix()["dri_row"]}


@pytest.fixture(scope="module")
def refs(inputs):
    from oracle import oracle

    return {k: oracle.decode(d) for k, d in inputs.items()}


@pytest.mark.parametrize("subseq_bytes", [32, 256])
def test_lone_decode_states_and_planes(torch_cuda, inputs, refs, subseq_bytes):
    import jpeggpu_amd

    for name, data in inputs.items():
        planes, info, tmp, base, lay = jpeggpu_amd.decode_to_planes(data, subseq_bytes=subseq_bytes, return_tmp=True)
        what = (name, subseq_bytes)
        check_stages(torch_cuda, data, tmp, base, lay, subseq_bytes, what)  # st_p / st_n / st_cz / dc01 / dc23, symbol stream
        _assert_planes([p.cpu().numpy() for p in planes], refs[name].planes, what)


@pytest.mark.parametrize("fused", [True, False])
def test_full_batch_plan(torch_cuda, inputs, refs, fused, monkeypatch):
    """Four copies of every input in ONE batched call on the full batch's path (forced: these items alone do not fill the
    chip): huff_sync_intra_batch after one flow iteration, the rest in the tail kernel, fused with the write pass or a
    launch of its own."""
    import jpeggpu_amd

    monkeypatch.setenv("JPEGGPU_EXP_KEEP_FLOWS_BELOW", "0")  # read at jpeggpu_ext_batch_create
    names = [n for n in inputs for _ in range(4)]
    before = jpeggpu_amd.fused_tail_timeouts()
    got, lays = _batch(torch_cuda, [inputs[n] for n in names], fused=fused)  # checks every item's stage buffers too
    assert all(l.subsequences_per_sequence == 255 for l in lays)
    for name, planes in zip(names, got):
        _assert_planes(planes, refs[name].planes, (name, fused))
    assert jpeggpu_amd.fused_tail_timeouts() == before == 0
