"""Progressive JPEGs on the GPU at the sizes and structures tests/test_gpu_progressive.py does not reach
(tests/progressive_cases.py: large(), structure(); what each input holds is asserted in
tests/test_progressive_large_host.py): end-of-band runs of every category and of 0x7FFF blocks on one lane, scans of
tens of KB with optimised tables, thousands of restart segments, work lists with idle items, 64 scans in one level, 14
levels, and a batch whose items differ widely in all of that. Every comparison is exact."""
import hashlib

import numpy as np
import pytest

from tests import progressive_cases as pc
from tests.test_gpu_progressive import batch_decode, decode_with_coefficients, same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda(gpu_lib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def large():
    return pc.large()


@pytest.fixture(scope="module")
def structure():
    return pc.structure()


@pytest.fixture(scope="module")
def oracle_of():
    """oracle.decode of a baseline file, computed once per file and shared (read-only)."""
    from oracle import oracle

    cache = {}

    def get(data):
        if data not in cache:
            cache[data] = oracle.decode(data)
        return cache[data]

    return get


def quantisers(data):
    """{table index: 64 values in natural order} of a file's 8-bit DQT segments."""
    from tests import progressive_ref as pr

    out, i = {}, 2
    while data[i + 1] != 0xDA:
        n = data[i + 2] << 8 | data[i + 3]
        if data[i + 1] == 0xDB:
            seg = data[i + 4:i + 2 + n]
            for k in range(0, len(seg), 65):
                assert seg[k] >> 4 == 0
                q = np.zeros(64, np.uint16)
                q[pr.ZIGZAG] = list(seg[k + 1:k + 65])
                out[seg[k] & 15] = q
        i += 2 + n
    return out


def planes_of(want, data):
    """The oracle's IDCT of the restatement's coefficients, cut to the planes' sizes."""
    from oracle import oracle

    q = quantisers(data)
    out = []
    for c, comp in enumerate(want.comps):
        vy, vx = want.visible[c]
        plane = np.zeros((vy * 8, vx * 8), np.uint8)
        for by in range(vy):
            for bx in range(vx):
                plane[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] = oracle.idct_block(want.coef[c][by, bx], q[comp["q"]])
        out.append(plane[:comp["ht"], :comp["w"]])
    return out


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest()


@pytest.mark.parametrize("name", ["eob_ladder", "eob_cap"])
def test_long_end_of_band_runs(torch_cuda, large, name):
    """Coefficient buffers equal to the restatement's, padded blocks included; planes equal to the oracle's IDCT of them."""
    prog = large[name].prog
    want, _ = pc.restated(prog)
    planes, info, coef, pi = decode_with_coefficients(torch_cuda, prog)
    assert info.num_components == 1 and (pi.num_scans, pi.num_levels) == (6, 2)
    same(coef[0], want.coef[0], (name, "coefficients"))
    same(planes[0], planes_of(want, prog)[0], (name, "planes"))


def check_against_source(torch, name, prog, base, oracle_of, padded=True):
    """Coefficients (the visible blocks) and planes against the oracle's decode of the baseline file with the same
    coefficients; with `padded` the whole buffer, padded blocks included, against the restatement."""
    o = oracle_of(base)
    planes, info, coef, pi = decode_with_coefficients(torch, prog)
    assert info.num_components == o.ncomp, name
    if padded:
        want, _ = pc.restated(prog)
        assert (pi.num_scans, pi.num_levels) == (len(want.scans), max(want.levels) + 1), name
    for c in range(o.ncomp):
        vy, vx = pi.visible_blocks_y[c], pi.visible_blocks_x[c]
        assert (vy, vx) == (-(-o.planes[c].shape[0] // 8), -(-o.planes[c].shape[1] // 8)), name
        same(coef[c][:vy, :vx], o.coef[c][:vy, :vx], (name, c, "coefficients"))
        if padded:
            same(coef[c], want.coef[c], (name, c, "coefficient buffer"))
        else:
            assert coef[c].shape[:2] == (vy, vx), (name, c)
        same(planes[c], o.planes[c], (name, c, "planes"))


@pytest.mark.parametrize("name", ["photo", "photo_rst"])
def test_photo_coefficients_and_planes(torch_cuda, large, oracle_of, name):
    """(Both sizes are whole MCUs: the buffers have no padded blocks, and the oracle's coefficients cover them.)"""
    check_against_source(torch_cuda, name, large[name].prog, large[name].twin, oracle_of, padded=False)


@pytest.mark.parametrize("name", ["photo", "photo_rst"])
def test_photo_to_rgb_equals_pillow_and_the_twin(torch_cuda, large, name):
    """decode_to_rgb at 1, 1/2, 1/4, 1/8 hashes to Pillow's pin and equals the twin's output; an odd-offset crop at full
    size is the slice of the twin's output. (Five decodes of the progressive file; the module decodes `photo` six times.)"""
    import jpeggpu_amd

    f = large[name]
    full = None
    for d in pc.SCALES:
        got = jpeggpu_amd.decode_to_rgb(f.prog, scale=d).cpu().numpy()
        digest, shape = f.rgb[d]
        assert got.shape == shape, (name, d)
        same(got, jpeggpu_amd.decode_to_rgb(f.twin, scale=d).cpu().numpy(), (name, d, "twin"))
        assert sha(got) == digest, (name, d, "Pillow's pin")
        if d == 1:
            full = got
    H, W = full.shape[:2]
    x, y, w, h = 37, 21, W - 37 - 11, H - 21 - 5
    crop = jpeggpu_amd.decode_to_rgb(f.prog, crop=(x, y, w, h)).cpu().numpy()
    same(crop, full[y:y + h, x:x + w], (name, "crop"))


def test_photo_rst_resized(torch_cuda, large):
    import jpeggpu_amd

    f = large["photo_rst"]
    out = jpeggpu_amd.decode_resized([f.prog, f.twin], 32, filt="bilinear", layout="NHWC").cpu().numpy()
    assert out.shape == (2, 32, 32, 3)
    same(out[0], out[1], "photo_rst resized against its twin")
    assert out[0].std() > 5  # (a picture, not a constant)


@pytest.mark.parametrize("name", ["two_large_444", "threshold_420", "threshold_420_below", "deep_levels"])
def test_structure_against_the_source(torch_cuda, structure, oracle_of, name):
    check_against_source(torch_cuda, name, structure[name][0], structure[name][1], oracle_of)


def test_sixty_four_scans(torch_cuda, structure, oracle_of):
    """64 scans in one level. The script never codes the chroma AC coefficients: luma and the DC values are the source
    file's, the buffers are the restatement's, the planes the oracle's IDCT of them (luma's: the source file's plane)."""
    prog, base = structure["sixty_four_scans"]
    o = oracle_of(base)
    want, _ = pc.restated(prog)
    planes, info, coef, pi = decode_with_coefficients(torch_cuda, prog)
    assert (pi.num_scans, pi.num_levels) == (64, 1)
    ref = planes_of(want, prog)
    for c in range(3):
        same(coef[c], want.coef[c], (c, "coefficient buffer"))
        same(planes[c], ref[c], (c, "planes"))
    vy, vx = pi.visible_blocks_y[0], pi.visible_blocks_x[0]
    same(coef[0][:vy, :vx], o.coef[0][:vy, :vx], "luma coefficients")
    same(planes[0], o.planes[0], "luma plane")


def test_mixed_batch(torch_cuda, large, structure):
    """One jpeggpu_ext_decode_batch call over items that differ widely in levels (1 to 14) and in items per level (1 to
    3 072 and more): the grid is sized by the largest item of each level, so most workgroups of most items return early --
    beyond their count, beyond their last level, on idle items. Every item equals its lone decode; again reversed."""
    import jpeggpu_amd

    pins = pc.pins()
    datas = [large["eob_ladder"].prog, pins["p420_odd"][0], large["photo_rst"].prog, pins["p420_rst1"][1],
             structure["deep_levels"][0], structure["sixty_four_scans"][0], structure["two_large_444"][0]]
    lone = [[p.cpu().numpy() for p in jpeggpu_amd.decode_to_planes(f, progressive=True)[0]] for f in datas]
    for order in (list(range(len(datas))), list(reversed(range(len(datas))))):
        got = batch_decode(torch_cuda, [datas[i] for i in order])
        for k, i in enumerate(order):
            assert len(got[k]) == len(lone[i])
            for c in range(len(lone[i])):
                same(got[k][c], lone[i][c], (i, c, "batch item against its lone decode"))


def test_one_decoder_large_small_large(torch_cuda, large):
    """One decoder and one d_tmp decode eob_ladder, p420_odd, eob_ladder: each equals a fresh decode. The 4 MB coefficient
    buffer is zeroed by every decode (refinement scans add to what is there, so what an earlier decode left would show)."""
    import jpeggpu_amd

    torch = torch_cuda
    stream = torch.cuda.current_stream().cuda_stream
    ladder, small = large["eob_ladder"].prog, pc.pins()["p420_odd"][0]
    fresh = {f: [p.cpu().numpy() for p in jpeggpu_amd.decode_to_planes(f, progressive=True)[0]] for f in (ladder, small)}
    dec = jpeggpu_amd.Decoder()
    try:
        dec.set_progressive(True)
        dec.parse_header(ladder)
        size = dec.get_buffer_size()
        tmp = torch.empty(size + 256, dtype=torch.uint8, device="cuda:0")
        base = (tmp.data_ptr() + 255) // 256 * 256
        for f in (ladder, small, ladder):
            info = dec.parse_header(f)
            n = dec.get_buffer_size()
            assert n <= size
            planes = [torch.zeros((info.sizes_y[c], info.sizes_x[c]), dtype=torch.uint8, device="cuda:0") for c in range(info.num_components)]
            dec.transfer(base, n, stream)
            dec.decode([p.data_ptr() for p in planes], [p.stride(0) for p in planes], base, n, stream)
            torch.cuda.synchronize()
            for c in range(info.num_components):
                same(planes[c].cpu().numpy(), fresh[f][c], (len(f), c))
    finally:
        dec.cleanup()
