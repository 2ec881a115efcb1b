"""Progressive JPEGs (SOF2) on the GPU: the scan kernels' coefficients and the planes behind the hand-over against the CPU
oracle's decode of a baseline file with the same coefficients; the Pillow-equal routes against Pillow's pinned RGB
(tests/golden/progressive_pins.npz) and against the baseline twins; batches that mix progressive and baseline items.
Every comparison is exact. Inputs: tests/progressive_cases.py (a few blocks each; corrupt streams are not run here)."""
import numpy as np
import pytest

from tests import progressive_cases as pc
from tests import progressive_ref as pr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda(gpu_lib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def pins():
    return pc.pins()


@pytest.fixture(scope="module")
def crafted():
    return pc.crafted()


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


def same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, len(bad), bad[:4].tolist())


def decode_with_coefficients(torch, data, **kw):
    """(planes as numpy, ImgInfo, coefficient buffers int16 [blocks_y, blocks_x, 64] read through progressive_info)."""
    import jpeggpu_amd
    from tests import gpu_util

    planes, info, tmp, base, lay, pi = jpeggpu_amd.decode_to_planes(data, progressive=True, return_tmp=True, **kw)
    assert pi.progressive == 1 and lay.num_scans == info.num_components
    coef = []
    for c in range(info.num_components):
        n = pi.blocks_x[c] * pi.blocks_y[c] * 64
        coef.append(gpu_util.tmp_view(torch, tmp, base, pi.off_coefficients[c], n, torch.int16).reshape(pi.blocks_y[c], pi.blocks_x[c], 64))
    return [p.cpu().numpy() for p in planes], info, coef, pi


def test_reference_idct_planes_and_coefficients(torch_cuda, pins, crafted, oracle_of):
    """Every pin and every crafted complete case: planes bit-exact with the oracle's decode of the baseline file, the
    coefficient buffer's visible blocks equal to the oracle's coefficients."""
    files = {n: (p, t) for n, (p, t, _) in pins.items()}
    files.update({n: crafted[n] for n in pc.COMPLETE})
    assert len(files) == 10 + 8
    for name, (prog, base) in files.items():
        o = oracle_of(base)
        planes, info, coef, pi = decode_with_coefficients(torch_cuda, prog)
        assert info.num_components == o.ncomp, name
        for c in range(o.ncomp):
            vy, vx = pi.visible_blocks_y[c], pi.visible_blocks_x[c]
            assert (vy, vx) == (-(-o.planes[c].shape[0] // 8), -(-o.planes[c].shape[1] // 8)), name
            same(coef[c][:vy, :vx], o.coef[c][:vy, :vx], (name, c, "coefficients"))
            same(planes[c], o.planes[c], (name, c, "planes"))


def test_script_that_stops_early(torch_cuda, crafted, oracle_of):
    """Unrefined bits stay 0 and a band no scan coded is 0: the restatement's coefficients, and the oracle's IDCT of them."""
    from oracle import oracle

    for name in ("early_stop_420", "early_stop_gray_rst"):
        prog, base = crafted[name]
        want = pr.decode(prog)
        o = oracle_of(base)
        planes, info, coef, pi = decode_with_coefficients(torch_cuda, prog)
        differs = False
        for c in range(o.ncomp):
            same(coef[c], want.coef[c], (name, c, "coefficients"))
            vy, vx = want.visible[c]
            differs |= not np.array_equal(coef[c][:vy, :vx], o.coef[c][:vy, :vx])
            h, w = o.planes[c].shape
            plane = np.zeros((vy * 8, vx * 8), np.uint8)
            for by in range(vy):
                for bx in range(vx):
                    plane[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] = oracle.idct_block(want.coef[c][by, bx], o.qtab[o.qidx[c]])
            same(planes[c], plane[:h, :w], (name, c, "planes"))
        assert differs, (name, "the script is meant to leave the coefficients incomplete")


def test_decode_to_rgb_equals_pillow_and_the_twin(torch_cuda, pins):
    import jpeggpu_amd

    for name, (prog, twin, rgb) in pins.items():
        for d in pc.SCALES:
            got = jpeggpu_amd.decode_to_rgb(prog, scale=d).cpu().numpy()
            same(got, rgb[d], (name, d, "Pillow's pin"))
            same(got, jpeggpu_amd.decode_to_rgb(twin, scale=d).cpu().numpy(), (name, d, "twin"))
        H, W = rgb[1].shape[:2]
        x, y = 3 if W > 8 else 1, 1
        w, h = W - x - 2, H - y - 2  # odd offsets, the far edges left out
        crop = jpeggpu_amd.decode_to_rgb(prog, crop=(x, y, w, h)).cpu().numpy()
        same(crop, rgb[1][y:y + h, x:x + w], (name, "crop"))
        H2, W2 = rgb[2].shape[:2]
        if W2 > 4 and H2 > 4:
            crop = jpeggpu_amd.decode_to_rgb(prog, crop=(1, 1, W2 - 2, H2 - 3), scale=2).cpu().numpy()
            same(crop, rgb[2][1:H2 - 2, 1:W2 - 1], (name, "crop at 1/2"))


def batch_decode(torch, datas, progressive=True):
    """One jpeggpu_ext_decode_batch call over `datas`; the planes of every item as numpy."""
    import jpeggpu_amd

    stream = torch.cuda.current_stream().cuda_stream
    decs, entries, planes_all, keep = [], [], [], []
    try:
        scans = 0
        for data in datas:
            dec = jpeggpu_amd.Decoder()
            decs.append(dec)
            dec.set_batch_hint(len(datas))
            dec.set_progressive(progressive)
            info = dec.parse_header(data)
            scans += dec.layout().num_scans
            n = dec.get_buffer_size()
            tmp = torch.empty(n + 256, dtype=torch.uint8, device="cuda:0")
            base = (tmp.data_ptr() + 255) // 256 * 256
            planes = [torch.zeros((info.sizes_y[c], info.sizes_x[c]), dtype=torch.uint8, device="cuda:0") for c in range(info.num_components)]
            dec.transfer(base, n, stream)
            keep.append(tmp)
            entries.append((dec, [p.data_ptr() for p in planes], [p.stride(0) for p in planes], base, n))
            planes_all.append(planes)
        batch = jpeggpu_amd.Batch(scans)
        scratch = torch.empty(batch.scratch_size, dtype=torch.uint8, device="cuda:0")
        batch.set_items(entries)
        batch.decode(scratch.data_ptr(), stream)
        torch.cuda.synchronize()
        batch.destroy()
        return [[p.cpu().numpy() for p in planes] for planes in planes_all]
    finally:
        for dec in decs:
            dec.cleanup()


def test_batch_of_progressive_and_baseline_items(torch_cuda, pins):
    """All pins in one call, progressive files and twins interleaved: every item equals its lone decode; again reversed."""
    import jpeggpu_amd

    datas = [f for _, (prog, twin, _) in sorted(pins.items()) for f in (prog, twin)]
    lone = [[p.cpu().numpy() for p in jpeggpu_amd.decode_to_planes(f, progressive=True)[0]] for f in datas]
    for order in (list(range(len(datas))), list(reversed(range(len(datas))))):
        got = batch_decode(torch_cuda, [datas[i] for i in order])
        for k, i in enumerate(order):
            assert len(got[k]) == len(lone[i])
            for c in range(len(lone[i])):
                same(got[k][c], lone[i][c], (i, c, "batch item against its lone decode"))
    for i in range(0, len(datas), 2):  # and a progressive file's planes are its twin's
        for c in range(len(lone[i])):
            same(lone[i][c], lone[i + 1][c], (i, c, "progressive against twin"))


def test_batch_of_progressive_items_only(torch_cuda, pins, crafted):
    datas = [pins[n][0] for n in ("p420_rst1", "pgray", "pcmyk")] + [crafted["three_refinements_rst"][0]]
    import jpeggpu_amd

    got = batch_decode(torch_cuda, datas)
    for k, f in enumerate(datas):
        lone = jpeggpu_amd.decode_to_planes(f, progressive=True)[0]
        for c in range(len(lone)):
            same(got[k][c], lone[c].cpu().numpy(), (k, c))


def test_decode_resized_mix(torch_cuda, pins):
    """decode_resized over progressive files and twins, to 32 x 32: a progressive file's output is its twin's; crops included."""
    import jpeggpu_amd

    names = sorted(pins)
    datas = [f for n in names for f in pins[n][:2]]
    crops = []
    for n in names:
        H, W = pins[n][2][1].shape[:2]
        c = None if len(crops) % 4 == 0 else (1, 1, W - 2, H - 3)
        crops += [c, c]
    for filt in ("bilinear", "bicubic"):
        for layout in ("NHWC", "NCHW"):
            out = jpeggpu_amd.decode_resized(datas, 32, crops=crops, filt=filt, layout=layout).cpu().numpy()
            assert out.shape == ((len(datas), 32, 32, 3) if layout == "NHWC" else (len(datas), 3, 32, 32))
            for i in range(0, len(datas), 2):
                same(out[i], out[i + 1], (names[i // 2], filt, layout))


def test_uniform_scales_and_islow(torch_cuda, pins):
    import jpeggpu_amd

    for name in ("p420", "pgray"):
        prog, twin, _ = pins[name]
        for kw in (dict(idct="islow"), dict(scale=2), dict(scale=4), dict(scale=8), dict(scale=2, scale_mode="libjpeg")):
            a = jpeggpu_amd.decode_to_planes(prog, progressive=True, **kw)[0]
            b = jpeggpu_amd.decode_to_planes(twin, **kw)[0]
            assert len(a) == len(b)
            for c in range(len(a)):
                same(a[c].cpu().numpy(), b[c].cpu().numpy(), (name, kw, c))


def test_one_decoder_baseline_progressive_baseline(torch_cuda, pins, oracle_of):
    """A decoder that parses baseline, progressive, baseline in turn decodes each as a fresh decoder does, and a second
    decode of the progressive file on the same d_tmp equals the first: the coefficient buffer is zeroed by every decode
    (refinement scans OR into it, so a buffer left from the decode before would show)."""
    import jpeggpu_amd

    torch = torch_cuda
    stream = torch.cuda.current_stream().cuda_stream
    prog, twin, _ = pins["p420_rst1"]
    other = pins["p444"][1]
    want = {f: [p for p in oracle_of(t).planes] for f, t in ((prog, twin), (twin, twin), (other, other))}
    dec = jpeggpu_amd.Decoder()
    try:
        dec.set_progressive(True)
        tmp = torch.empty(1 << 22, dtype=torch.uint8, device="cuda:0")
        base = (tmp.data_ptr() + 255) // 256 * 256
        for f in (twin, prog, prog, other, prog):
            info = dec.parse_header(f)
            n = dec.get_buffer_size()
            assert n + 256 <= tmp.numel()
            planes = [torch.zeros((info.sizes_y[c], info.sizes_x[c]), dtype=torch.uint8, device="cuda:0") for c in range(info.num_components)]
            dec.transfer(base, n, stream)
            for _ in range(2):  # the second decode runs on what the first left in d_tmp
                dec.decode([p.data_ptr() for p in planes], [p.stride(0) for p in planes], base, n, stream)
                torch.cuda.synchronize()
                for c in range(info.num_components):
                    same(planes[c].cpu().numpy(), want[f][c], (len(f), c))
    finally:
        dec.cleanup()


def test_default_decoder_refuses_and_switches_are_ignored(torch_cuda, pins, oracle_of):
    import jpeggpu_amd

    prog, twin, _ = pins["p422_rstrow"]
    with pytest.raises(jpeggpu_amd.JpegGpuError) as e:
        jpeggpu_amd.decode_to_planes(prog)
    assert e.value.status == jpeggpu_amd.Status.NOT_SUPPORTED
    # the device scan does not apply to a progressive image: the host walk is used, silently
    planes = jpeggpu_amd.decode_to_planes(prog, progressive=True, device_scan=True)[0]
    for c, want in enumerate(oracle_of(twin).planes):
        same(planes[c].cpu().numpy(), want, c)


def test_stage_timing_keeps_its_names(torch_cuda, pins):
    import jpeggpu_amd

    torch = torch_cuda
    stream = torch.cuda.current_stream().cuda_stream
    dec = jpeggpu_amd.Decoder()
    try:
        dec.set_progressive(True)
        dec.set_profiling(True)
        info = dec.parse_header(pins["p420_rst1"][0])
        n = dec.get_buffer_size()
        tmp = torch.empty(n + 256, dtype=torch.uint8, device="cuda:0")
        base = (tmp.data_ptr() + 255) // 256 * 256
        planes = [torch.zeros((info.sizes_y[c], info.sizes_x[c]), dtype=torch.uint8, device="cuda:0") for c in range(info.num_components)]
        dec.transfer(base, n, stream)
        dec.decode([p.data_ptr() for p in planes], [p.stride(0) for p in planes], base, n, stream)
        torch.cuda.synchronize()
        ms = dec.stage_ms()
        assert tuple(ms) == jpeggpu_amd.api.STAGES
        assert ms["write"] > 0 and ms["idct"] > 0  # the progressive launches are counted in the write stage's slot
    finally:
        dec.cleanup()
