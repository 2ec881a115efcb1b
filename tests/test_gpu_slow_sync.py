"""Streams that do not resynchronise by themselves (tests/cases.slow_sync) on the GPU, bit-exact against the CPU oracle:
every stage buffer, guarded planes of lone and batched decodes (every flow path: the sequence kernel's long flows, the
tail kernel's parts and the fused tail + write launch, the multi-hypothesis tables), and the ISLOW, scaled and cropped
decodes on top of them. Their flows run for hundreds of subsequences, across sequences and multi-hypothesis blocks and
far into the tail kernel's parts: a wrong hand-off anywhere on that path shows here and nowhere in the matrix files,
which resynchronise within a few subsequences. Batch items are checked stage by stage in their own buffers, and the
marked files' planes show a misplaced data unit. The whole file takes about 17 s on one MI355X."""
import numpy as np
import pytest

from tests import cases, gpu_util, libjpeg_ref, scaled_ref
from tests.test_gpu_crop import assert_window, decode
from tests.test_gpu_scaled import Guarded, _tmp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda(gpu_lib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def corpus():
    return {k: v.data for k, v in cases.slow_sync().items()}


@pytest.fixture(scope="module")
def refs(corpus):
    from oracle import oracle

    return {k: oracle.decode(d) for k, d in corpus.items()}


def _assert_planes(got, want, what):
    assert len(got) == len(want), what
    for c, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape, (what, c, a.shape, b.shape)
        bad = np.argwhere(a != b)
        assert len(bad) == 0, "%s component %d: %d samples differ, first at %s" % (what, c, len(bad), bad[:4].tolist())


def check_stages(torch, data, tmp, base, lay, subseq_bytes, what):
    """Every intermediate buffer of a lone decode against its CPU twin (as tests/test_gpu_parity.test_stage_parity)."""
    from oracle import oracle

    view = gpu_util.tmp_view
    for s in range(lay.num_scans):
        sl = lay.scans[s]
        tw = oracle.scan_stages(data, s, subseq_bytes)
        S, G = sl.num_subsequences, sl.num_segments
        if sl.device_scan:
            words = view(torch, tmp, base, sl.off_device_status, 5, torch.int32)
            assert words[0] == 0 and S >= words[1], what
            S, G = int(words[1]), int(words[2])
            segs = view(torch, tmp, base, sl.off_segments, 2 * G, torch.int32).reshape(G, 2)
            assert np.array_equal(segs[:, 0], tw.seg_offset) and np.array_equal(segs[:, 1], tw.seg_count), (what, s, "segments")
        assert S == tw.num_subseq and G == tw.num_segments and sl.num_data_units == tw.num_du, (what, s)
        W = subseq_bytes // 4
        R = 16 if W >= 64 else 32
        tiles = (S + R - 1) // R
        tiled = view(torch, tmp, base, sl.off_destuffed, tiles * R * (subseq_bytes + 12), torch.uint8)
        rows = tiled.reshape(tiles, W + 3, R, 4)[..., ::-1].transpose(0, 2, 1, 3).reshape(tiles * R, W + 3, 4)[:S]
        assert np.array_equal(rows[:, 1:W + 1].reshape(-1), tw.destuffed), (what, s, "destuffed bytes")
        assert np.array_equal(view(torch, tmp, base, sl.off_segment_index, S, torch.int32), tw.seg_index), (what, s, "segment index")
        ok = tw.p >= 0
        for nm, off, ref in (("p", sl.off_state_p, tw.p), ("n", sl.off_state_n, tw.n), ("cz", sl.off_state_cz, tw.cz)):
            got = view(torch, tmp, base, off, S, torch.int32)
            bad = np.flatnonzero(got[ok] != ref[ok])
            assert len(bad) == 0, (what, s, "state " + nm, len(bad), np.flatnonzero(ok)[bad[:4]].tolist())
        d01 = view(torch, tmp, base, sl.off_state_dc01, S, torch.int32).view(np.uint32)
        d23 = view(torch, tmp, base, sl.off_state_dc23, S, torch.int32).view(np.uint32)
        halves = [d01 & 0xFFFF, d01 >> 16, d23 & 0xFFFF, d23 >> 16]
        for k in range(sl.num_components):
            assert np.array_equal(halves[k][ok], tw.dc[k][ok].astype(np.uint32) & 0xFFFF), (what, s, "dc sums %d" % k)
        coef = gpu_util.stream_coefficients(torch, tmp, base, sl, S)
        bad = np.flatnonzero((coef != tw.stream_coef).any(1))
        assert len(bad) == 0, (what, s, "coefficients", len(bad), bad[:4].tolist())


@pytest.mark.parametrize("subseq_bytes", [32, 64, 128, 256])
@pytest.mark.parametrize("device_scan", [False, True])
def test_stage_parity(torch_cuda, corpus, refs, subseq_bytes, device_scan):
    import jpeggpu_amd

    for name, data in corpus.items():
        planes, info, tmp, base, lay = jpeggpu_amd.decode_to_planes(data, subseq_bytes=subseq_bytes, return_tmp=True,
                                                                    device_scan=device_scan)
        what = (name, subseq_bytes, device_scan)
        check_stages(torch_cuda, data, tmp, base, lay, subseq_bytes, what)
        _assert_planes([p.cpu().numpy() for p in planes], refs[name].planes, what)


@pytest.mark.parametrize("subseq_bytes", [None, 32, 256])
def test_lone_decode_guarded_planes(torch_cuda, corpus, refs, subseq_bytes):
    """The lone decode with the library's plan (None: multi-hypothesis tables where the scan has several data units per
    MCU, walked block by block on scans of more than 1024 subsequences) and forced sizes, guard bytes around every plane."""
    for name, data in corpus.items():
        for device_scan in (False, True):
            got, _, _, _ = decode(torch_cuda, data, subseq_bytes=subseq_bytes, device_scan=device_scan)
            _assert_planes(got, refs[name].planes, (name, subseq_bytes, device_scan))


def _batch(torch, datas, hint=None, iters=None, fused=None, device_scan_every=0):
    """One jpeggpu_ext_decode_batch call into guarded planes: (planes per item, the layouts after the call). Every
    item's own buffer is also checked stage by stage (check_stages at the subsequence size the call used for it): the
    states and the symbol stream the tail kernel's parts and the fused writers left there."""
    import jpeggpu_amd

    keep, entries, total = [], [], 0
    for k, data in enumerate(datas):
        dec = jpeggpu_amd.Decoder()
        if hint is not None:
            dec.set_batch_hint(hint)
        if device_scan_every and k % device_scan_every == 1:
            dec.set_device_scan(True)
        info = dec.parse_header(data)
        n = dec.get_buffer_size()
        tmp, base = _tmp(torch, n)
        g = Guarded(torch, info)
        dec.transfer(base, n, 0)
        total += dec.layout().num_scans
        keep.append((dec, tmp, g, base))
        entries.append((dec, g.ptrs, g.pitches, base, n))
    batch = jpeggpu_amd.Batch(total)
    try:
        scratch = torch.empty(batch.scratch_size, dtype=torch.uint8, device="cuda:0")
        batch.set_items(entries)
        if iters is not None:
            batch.set_sync_iterations(iters)
        if fused is not None:
            batch.set_fused_tail(fused)
        batch.decode(scratch.data_ptr(), 0)
        torch.cuda.synchronize()
        out, lays = [], []
        for k, (dec, tmp, g, base) in enumerate(keep):
            assert dec.device_status(base, 0) == jpeggpu_amd.Status.SUCCESS
            lay = dec.layout()
            check_stages(torch, datas[k], tmp, base, lay, lay.subsequence_bytes, ("batch item", k, hint, iters, fused))
            out.append(g.planes())
            lays.append(lay)
        return out, lays
    finally:
        batch.destroy()
        for dec, _t, _g, _b in keep:
            dec.cleanup()


def _mixed(corpus):
    """The slow streams between normal matrix files: parts and sequences of both kinds in one call."""
    m = cases.matrix()
    normal = [m[k] for k in ("multi_seq_nodri", "dri_row", "cfg5_small", "ni_420_dri", "gray", "multi_seq_dri")]
    names, datas = [], []
    for k, (name, data) in enumerate(corpus.items()):
        names += [name, "normal%d" % k]
        datas += [data, normal[k % len(normal)]]
    return names, datas


@pytest.mark.parametrize("iters,fused", [(None, True), (None, False), (1, None), (3, None)])
def test_full_batch_guarded_planes(torch_cuda, corpus, refs, iters, fused, monkeypatch):
    """The full batch's plan (forced: these items alone would not fill the chip): huff_sync_intra_batch cut after one
    flow iteration, or after the caller's one or three, and the rest of every flow in the tail kernel's parts (cut at
    segment starts), which here run for hundreds of subsequences; with the library's cap the write pass is fused into
    the tail launch (its writers wait for the parts) or, switched off, a launch of its own. The planes and every item's
    stage buffers against the oracle."""
    import jpeggpu_amd
    from oracle import oracle

    monkeypatch.setenv("JPEGGPU_EXP_KEEP_FLOWS_BELOW", "0")  # read at jpeggpu_ext_batch_create
    names, datas = _mixed(corpus)
    before = jpeggpu_amd.fused_tail_timeouts()
    got, _ = _batch(torch_cuda, datas, iters=iters, fused=fused, device_scan_every=3)
    for name, data, planes in zip(names, datas, got):
        want = refs[name].planes if name in refs else oracle.decode(data).planes
        _assert_planes(planes, want, (name, iters, fused))
    assert jpeggpu_amd.fused_tail_timeouts() == before == 0


@pytest.mark.parametrize("images", [2, 8])
def test_small_batch_plans_guarded_planes(torch_cuda, corpus, refs, images, monkeypatch):
    """A small call (jpeggpu_ext_set_batch_hint) keeps its flows in the lone decode's huff_sync_intra; forced onto the full batch's
    path (JPEGGPU_EXP_KEEP_FLOWS_BELOW=0) the same items go through the fused huff_tail_write launch."""
    import jpeggpu_amd
    from oracle import oracle

    names, datas = _mixed(corpus)
    names, datas = names[:images], datas[:images]
    for mode in ("auto", "marks"):
        # read at jpeggpu_ext_batch_create; tools/soak_gpu.py (test_random_soak_short) leaves it set in the process
        monkeypatch.setenv("JPEGGPU_EXP_KEEP_FLOWS_BELOW", "0" if mode == "marks" else "220000")
        got, lays = _batch(torch_cuda, datas, hint=images)
        assert [l.subsequences_per_sequence for l in lays] == [240 if mode == "auto" else 255] * images, mode
        for name, data, planes in zip(names, datas, got):
            want = refs[name].planes if name in refs else oracle.decode(data).planes
            _assert_planes(planes, want, (name, images, mode))
    assert jpeggpu_amd.fused_tail_timeouts() == 0


def test_islow_scaled_and_cropped(torch_cuda, corpus, refs):
    """The features on top of the path: ISLOW at full size and the 1/8 scale against their numpy restatements, and a
    crop of the short-restart variant, whose rectangle skips most segments, against the uncropped planes sliced."""
    for name, data in corpus.items():
        got, _, _, _ = decode(torch_cuda, data, method="islow")
        _assert_planes(got, libjpeg_ref.islow_planes_of(refs[name]), (name, "islow"))
        got, _, _, _ = decode(torch_cuda, data, scale=8)
        _assert_planes(got, scaled_ref.scaled_planes_of(refs[name], 8), (name, "1/8"))
    data = corpus["s420_763_dri48"]
    full = refs["s420_763_dri48"].planes
    for rect in ((200, 440, 224, 160), (0, 1000, 1024, 24), (1001, 3, 23, 1021)):
        for device_scan in (False, True):
            planes, info, ci, _ = decode(torch_cuda, data, crop=rect, device_scan=device_scan)
            assert_window(planes, full, info, ci, (rect, device_scan))
