"""libjpeg-compatible full-size decoding on the GPU: the ISLOW IDCT mode (jpeggpu_ext_set_idct) and the fancy-upsampled
RGB output (jpeggpu_ext_planes_to_rgbi_fancy, decode_to_rgb) against the numpy restatement (tests/libjpeg_ref.py) and
Pillow's pinned output (tests/golden/libjpeg_pins.npz), with guard bytes around every plane."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import cases, libjpeg_ref, scaled_ref
from tests.conftest import GOLDEN, ROOT
from tests.test_gpu_scaled import GUARD, Guarded, _assert_planes, _tmp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda(gpu_lib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def matrix():
    return cases.matrix()


@pytest.fixture(scope="module")
def pins():
    return np.load(os.path.join(GOLDEN, "libjpeg_pins.npz"))


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def decode_islow(torch, data, subseq_bytes=None, device_scan=False):
    import jpeggpu_amd

    dec = jpeggpu_amd.Decoder(subseq_bytes)
    try:
        dec.set_idct("islow")
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


@pytest.mark.parametrize("subseq_bytes,device_scan", [(32, False), (64, True), (256, False), (256, True)])
def test_matrix_islow_full_size(torch_cuda, matrix, subseq_bytes, device_scan):
    """Every matrix file, q16_tables and dense_escapes included. None of them reaches the 64-bit pass 1: their largest
    |coefficient * quantiser| is 1,023 (dense_escapes; 534 in q16_tables), far below kIslowPass1Max. That pass is run by
    tests/test_gpu_idct_cases.py::test_lone_decode[islow-*] on the pass1_*, ycc420* and kats16_* files of tests/idct_cases.py."""
    from oracle import oracle

    for name, data in matrix.items():
        got, _ = decode_islow(torch_cuda, data, subseq_bytes, device_scan)
        _assert_planes(got, libjpeg_ref.islow_planes_of(oracle.decode(data)), (name, subseq_bytes, device_scan))


def test_islow_planes_equal_pillow_pins(torch_cuda, pins):
    n = 0
    for name, c, array, sha in libjpeg_ref.pinned_arrays(pins, "planes"):
        got, _ = decode_islow(torch_cuda, libjpeg_ref.pinned_jpeg(pins, name))
        assert libjpeg_ref.matches_pin(got[c], array, sha), (name, c)
        n += 1
    assert n >= 30


def test_decode_to_rgb_equals_pillow_pins(torch_cuda, pins):
    import jpeggpu_amd

    n = 0
    for name, _, array, sha in libjpeg_ref.pinned_arrays(pins, "rgb"):
        got = jpeggpu_amd.decode_to_rgb(libjpeg_ref.pinned_jpeg(pins, name)).cpu().numpy()
        assert libjpeg_ref.matches_pin(got, array, sha), name
        n += 1
    assert n >= 47


def test_decode_to_rgb_photo_equals_pillow(torch_cuda, pins, photo_bytes):
    import jpeggpu_amd

    for device_scan in (False, True):
        got = jpeggpu_amd.decode_to_rgb(photo_bytes, device_scan=device_scan).cpu().numpy()
        assert got.shape == (3024, 4032, 3)
        assert _sha(got) == str(pins["photo_rgb_sha256"]), device_scan


def test_fancy_kernel_on_reference_planes_with_guards(torch_cuda, matrix):
    """The kernel alone, on whatever planes it is given (here the reference IDCT's), rows padded and unaligned: equals the
    restatement of jdsample.c + jdcolor.c and writes nothing past a row."""
    import jpeggpu_amd
    from jpeggpu_amd.api import Img, lib

    torch = torch_cuda
    for name in ("ss_2x2", "ss_2x1", "ss_1x2", "ss_4x1", "ss_1x1", "gray", "odd_1x1px", "odd_17x9", "odd_partial_mcu", "dri_row"):
        planes, info = jpeggpu_amd.decode_to_planes(matrix[name])
        n = info.num_components
        hs, vs = list(info.subsampling.x[:n]), list(info.subsampling.y[:n])
        W = info.sizes_x[hs.index(max(hs))]
        H = info.sizes_y[vs.index(max(vs))]
        src = Img()
        for c in range(n):
            src.image[c], src.pitch[c] = planes[c].data_ptr(), planes[c].stride(0)
        pitch = 3 * W + 5
        out = torch.full((H + 1, pitch), GUARD, dtype=torch.uint8, device="cuda:0")
        assert lib().jpeggpu_ext_planes_to_rgbi_fancy(C.byref(info), C.byref(src), out.data_ptr(), pitch, W, H, None) == 0
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert (got[:, 3 * W:] == GUARD).all() and (got[H] == GUARD).all(), (name, "wrote past the image")
        want = libjpeg_ref.planes_to_rgb_fancy([p.cpu().numpy() for p in planes], hs, vs, W, H)
        assert np.array_equal(got[:H, :3 * W].reshape(H, W, 3), want), name


def test_fancy_kernel_refuses_what_it_does_not_support(torch_cuda, matrix):
    import jpeggpu_amd
    from jpeggpu_amd.api import Img, ImgInfo, lib

    torch = torch_cuda
    out = torch.zeros((8, 64), dtype=torch.uint8, device="cuda:0")
    for name in ("two_comp", "four_comp_444", "four_comp_opt"):  # 2 and 4 components, as jpeggpu_ext_planes_to_rgbi
        planes, info = jpeggpu_amd.decode_to_planes(matrix[name])
        src = Img()
        for c in range(info.num_components):
            src.image[c], src.pitch[c] = planes[c].data_ptr(), planes[c].stride(0)
        assert lib().jpeggpu_ext_planes_to_rgbi_fancy(C.byref(info), C.byref(src), out.data_ptr(), 64, 8, 8, None) == int(jpeggpu_amd.Status.NOT_SUPPORTED), name
    # a ratio that is not an integer (factors 3 and 2): libjpeg refuses it too
    info = ImgInfo()
    info.num_components = 3
    src = Img()
    for c, (h, w) in enumerate(((3, 1), (2, 1), (1, 1))):
        info.subsampling.x[c], info.subsampling.y[c] = h, w
        info.sizes_x[c], info.sizes_y[c] = 6 * h, 8
        src.image[c], src.pitch[c] = out.data_ptr(), 64
    assert lib().jpeggpu_ext_planes_to_rgbi_fancy(C.byref(info), C.byref(src), out.data_ptr(), 64, 18, 8, None) == int(jpeggpu_amd.Status.NOT_SUPPORTED)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0).all()


def _batch_decode(torch, items, batched_hint):
    """items: [(bytes, scale, method)] through one jpeggpu_ext_decode_batch call; returns the planes per item."""
    import jpeggpu_amd

    keep, entries, total = [], [], 0
    for k, (data, d, method) in enumerate(items):
        dec = jpeggpu_amd.Decoder()
        dec.set_batch_hint(batched_hint)
        dec.set_scale(d)
        dec.set_idct(method)
        dec.set_device_scan(k % 3 == 1)
        info = dec.parse_header(data)
        n = dec.get_buffer_size()
        tmp, base = _tmp(torch, n)
        g = Guarded(torch, info)
        dec.transfer(base, n, 0)
        total += dec.layout().num_scans
        keep.append((dec, tmp, g, base))
        entries.append((dec, g.ptrs, g.pitches, base, n))
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
    return out


def _want(ref, d, method):
    if d != 1:
        return scaled_ref.scaled_planes_of(ref, d)  # the method only affects scale 1
    return libjpeg_ref.islow_planes_of(ref) if method == "islow" else ref.planes


@pytest.mark.parametrize("kinds", ["all", "methods_only", "islow_and_scaled"])
def test_batch_mixes_methods_and_scales(torch_cuda, matrix, kinds):
    import jpeggpu_amd
    from oracle import oracle

    names = ["multi_seq_dri", "ni_420_dri", "four_comp_opt", "gray", "odd_1x1px", "cfg4_small", "dri_1", "odd_partial_mcu",
             "ss_4x1", "q16_tables", "dense_escapes", "ni_big_last"]
    pattern = {"all": [(1, "islow"), (1, "reference"), (2, "islow"), (8, "reference"), (4, "islow")],
               "methods_only": [(1, "islow"), (1, "reference")],
               "islow_and_scaled": [(1, "islow"), (8, "islow"), (2, "reference")]}[kinds]
    order = names + names[::-1]
    items = [(matrix[name], *pattern[k % len(pattern)]) for k, name in enumerate(order)]
    refs = {name: oracle.decode(matrix[name]) for name in names}
    for hint in (0, 64):
        got = _batch_decode(torch_cuda, items, hint)
        for (data, d, method), planes, name in zip(items, got, order):
            _assert_planes(planes, _want(refs[name], d, method), (name, d, method, hint))
            # and each item gives what it gives alone
            if d == 1:
                alone = decode_islow(torch_cuda, data)[0] if method == "islow" else [p.cpu().numpy() for p in jpeggpu_amd.decode_to_planes(data)[0]]
                _assert_planes(planes, alone, (name, method, "alone"))
    assert jpeggpu_amd.fused_tail_timeouts() == 0


def test_full_batch_of_64_twelve_megapixel_images_islow(torch_cuda):
    """BASELINE.json configs[2] (64 x 12 MP 4:2:0) in one call with the ISLOW IDCT: plane hashes against the restatement."""
    import jpeggpu_amd
    from oracle import oracle
    from tools import jpegsynth

    datas = [jpegsynth.config(2, seed=100 + s) for s in range(4)]
    want = [[hashlib.sha256(p.tobytes()).hexdigest() for p in libjpeg_ref.islow_planes_of(oracle.decode(x))] for x in datas]
    got = _batch_decode(torch_cuda, [(datas[i % 4], 1, "islow") for i in range(64)], 64)
    bad = [i for i, planes in enumerate(got) if [hashlib.sha256(p.tobytes()).hexdigest() for p in planes] != want[i % 4]]
    assert not bad, bad
    assert jpeggpu_amd.fused_tail_timeouts() == 0


def test_segment_shard_bands_islow(torch_cuda, matrix):
    import jpeggpu_amd
    from oracle import oracle
    from tools import jpegsynth

    torch = torch_cuda
    inputs = {"dri_row": matrix["dri_row"], "gray_rows": jpegsynth.encode(200, 152, ((1, 1),), restart_interval=50, seed=77),
              "two_rows": jpegsynth.encode(333, 251, cases.S420, restart_interval=42, seed=78)}
    for name, data in inputs.items():
        want = libjpeg_ref.islow_planes_of(oracle.decode(data))
        for world in (2, 3):
            planes = [torch.full(p.shape, 0xAB, dtype=torch.uint8, device="cuda:0") for p in want]
            for rank in range(world):
                dec = jpeggpu_amd.Decoder(32 if rank % 2 else 64)
                dec.set_idct("islow")
                dec.set_segment_shard(rank, world)
                info = dec.parse_header(data)
                n = dec.get_buffer_size()
                tmp, base = _tmp(torch, n)
                before = [p.clone() for p in planes]
                dec.transfer(base, n, 0)
                dec.decode([p.data_ptr() for p in planes], [p.stride(0) for p in planes], base, n, 0)
                torch.cuda.synchronize()
                for c in range(info.num_components):
                    a, cnt = dec.shard_rows(c)
                    assert torch.equal(planes[c][:a], before[c][:a]) and torch.equal(planes[c][a + cnt:], before[c][a + cnt:]), (name, world, rank, c)
                dec.cleanup()
            for c in range(len(want)):
                assert np.array_equal(planes[c].cpu().numpy(), want[c]), (name, world, c)


_CHILD = r"""
import hashlib, sys
sys.path.insert(0, sys.argv[1])
import jpeggpu_amd, torch
planes, _ = jpeggpu_amd.decode_to_planes(open(sys.argv[2], "rb").read())
torch.cuda.synchronize()
print(" ".join(hashlib.sha256(p.cpu().numpy().tobytes()).hexdigest() for p in planes))
"""


def test_environment_selects_islow_for_the_drop_in_api(torch_cuda, matrix, tmp_path):
    """JPEGGPU_IDCT=islow, read at jpeggpu_decoder_startup: a caller that never calls jpeggpu_ext_set_idct gets ISLOW
    planes; without it (or with "reference") the reference's. Each in a fresh child process."""
    from oracle import oracle

    data = matrix["dri_7"]
    path = tmp_path / "dri_7.jpg"
    path.write_bytes(data)
    ref = oracle.decode(data)
    want = {"islow": [hashlib.sha256(p.tobytes()).hexdigest() for p in libjpeg_ref.islow_planes_of(ref)],
            "reference": [hashlib.sha256(p.tobytes()).hexdigest() for p in ref.planes]}
    assert want["islow"] != want["reference"]
    for value, expect in (("islow", "islow"), ("reference", "reference"), (None, "reference")):
        env = dict(os.environ)
        env.pop("JPEGGPU_IDCT", None)
        if value is not None:
            env["JPEGGPU_IDCT"] = value
        r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(path)], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stdout.split() == want[expect], (value, r.stderr[-2000:])
