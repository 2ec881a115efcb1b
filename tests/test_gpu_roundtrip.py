"""JPEG round trip on the device (jpeggpu_ext_roundtrip_batch, jpeg_roundtrip): every case of tests/roundtrip_ref.cases() equals
Pillow's pinned save-then-open (tests/golden/roundtrip_pins.npz) and the library's own encode_jpeg -> decode chain; mixed
calls, layouts, views, in-place outputs, refusals, calls in a row. Outputs lie in buffers pre-filled with 0xA5, and every
byte outside the images' rectangles is checked to still hold it."""
import ctypes as C
import os

import numpy as np
import pytest

import jpeggpu_amd
from jpeggpu_amd import Status
from jpeggpu_amd.api import IMAGE_LAYOUTS, SUBSAMPLINGS
from tests import roundtrip_ref as R

pytestmark = pytest.mark.gpu

GUARD = 0xA5
DEV = "cuda:0"
CASES = R.cases()
PINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "roundtrip_pins.npz")


@pytest.fixture(scope="module")
def torch(gpu_lib):
    import torch

    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def pins():
    return np.load(PINS)


_single = {}


def single_results(torch):
    """Every case through a jpeg_roundtrip call of its own, once per module: {case index: numpy array}."""
    if not _single:
        for i, case in enumerate(CASES):
            x = torch.from_numpy(R.case_input(case)).to(DEV)
            _single[i] = jpeggpu_amd.jpeg_roundtrip([x], quality=case[6], subsampling=case[5])[0].cpu().numpy()
    return _single


def test_every_case_equals_its_pin(torch, pins):
    got = single_results(torch)
    wrong = [CASES[i][0] for i in range(len(CASES)) if not R.matches_pin(pins, i, got[i])]
    assert not wrong, "%d of %d cases differ from Pillow: %s" % (len(wrong), len(CASES), wrong[:20])


def test_every_case_equals_the_encode_decode_chain(torch):
    """decode_batch_to_rgb(encode_jpeg(x)) -- grey: decode_batch_to_gray -- is what the library computed before this call
    existed: one encode and one decode call per size and kind."""
    got = single_results(torch)
    wrong = []
    for w, h in R.SIZES:
        for ch in (1, 3):
            idx = [i for i, c in enumerate(CASES) if (c[1], c[2], c[3]) == (w, h, ch)]
            xs = [torch.from_numpy(R.case_input(CASES[i])).to(DEV) for i in idx]
            files = jpeggpu_amd.encode_jpeg(xs, quality=[CASES[i][6] for i in idx], subsampling=[CASES[i][5] for i in idx])
            chain = jpeggpu_amd.decode_batch_to_rgb(files, DEV) if ch == 3 else jpeggpu_amd.decode_batch_to_gray(files, DEV)
            wrong += [CASES[i][0] for i, y in zip(idx, chain) if not np.array_equal(y.cpu().numpy(), got[i])]
    assert not wrong, "%d cases differ from the chain: %s" % (len(wrong), wrong[:20])


def test_range_limit_wraps_as_the_decoders(torch):
    """R.WRAP_BLOCK at quality 1 overshoots below -512: the sample is 255 by jidctint.c's table lookup, as the ISLOW decoder
    of the chain computes it, and 0 by a plain clamp. Alone, inside a larger grey image, and as every channel of an RGB one
    (4:4:4: luma is the block itself, chroma is constant)."""
    y0, x0 = R.WRAP_AT
    tiled = np.tile(R.WRAP_BLOCK, (3, 5))
    rgb = np.repeat(R.WRAP_BLOCK[:, :, None], 3, axis=2)
    for a, ss in ((R.WRAP_BLOCK, "4:4:4"), (tiled, "4:4:4"), (rgb, "4:4:4")):
        x = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        got = jpeggpu_amd.jpeg_roundtrip([x], quality=1, subsampling=ss)[0].cpu().numpy()
        files = jpeggpu_amd.encode_jpeg([x], quality=1, subsampling=ss)
        chain = (jpeggpu_amd.decode_batch_to_rgb(files, DEV) if a.ndim == 3 else jpeggpu_amd.decode_batch_to_gray(files, DEV))[0].cpu().numpy()
        assert np.array_equal(got, chain) and np.array_equal(got, R.roundtrip(a, 1, ss))
        assert (got[y0, x0] == 255).all() and (got[16 + y0, 32 + x0] == 255 if a is tiled else True)


def _mixed_inputs():
    """Grey items of exactly 1, 255, 256 and 257 blocks, RGB items of 6, 255 and 399 blocks in the three subsamplings, one of
    several tiles, and small ones with odd sides; qualities over the whole range."""
    rng = np.random.default_rng(77)
    shapes = [(8, 8, 1, "4:4:4"), (136, 120, 1, "4:4:4"), (128, 128, 1, "4:4:4"), (8, 2056, 1, "4:4:4"), (16, 16, 3, "4:2:0"), (40, 136, 3, "4:4:4"),
              (136, 120, 3, "4:2:0"), (128, 88, 3, "4:2:2"), (250, 131, 3, "4:4:4"), (17, 33, 3, "4:2:0"), (3, 2, 3, "4:2:2"), (1, 1, 3, "4:2:0"),
              (9, 17, 1, "4:4:4"), (33, 6, 3, "4:2:2")]
    qualities = [1, 100, 50, 75, 2, 99, 10, 90, 25, 49, 51, 95, 33, 66]
    images = [rng.integers(0, 256, (h, w) if ch == 1 else (h, w, 3), dtype=np.uint8) for w, h, ch, _ in shapes]
    images[2][:] = ((np.indices((128, 128)).sum(0) & 1) * 255).astype(np.uint8)  # a checkerboard: the range limit wraps
    return images, qualities, [s[3] for s in shapes]


def test_one_call_holds_everything(torch):
    images, qualities, ss = _mixed_inputs()
    blocks = [-(-a.shape[1] // 8) * -(-a.shape[0] // 8) for a in images[:4]]
    assert blocks == [1, 255, 256, 257]
    want = [R.roundtrip(a, q, s) for a, q, s in zip(images, qualities, ss)]
    xs = [torch.from_numpy(a).to(DEV) for a in images]
    alone = [jpeggpu_amd.jpeg_roundtrip([x], quality=q, subsampling=s)[0].cpu().numpy() for x, q, s in zip(xs, qualities, ss)]
    for i, (a, b) in enumerate(zip(alone, want)):
        assert np.array_equal(a, b), "item %d alone differs from the CPU restatement" % i
    for order in (list(range(len(xs))), list(reversed(range(len(xs))))):
        got = jpeggpu_amd.jpeg_roundtrip([xs[i] for i in order], quality=[qualities[i] for i in order], subsampling=[ss[i] for i in order])
        for i, y in zip(order, got):
            assert np.array_equal(y.cpu().numpy(), alone[i]), "item %d in a mixed call differs from its own call" % i


def _guarded(torch, shape):
    return torch.full(shape, GUARD, dtype=torch.uint8, device=DEV)


def test_layouts_and_views(torch):
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    want = R.roundtrip(a, 60, "4:2:0")
    hwc = torch.from_numpy(a).to(DEV)
    chw = hwc.permute(2, 0, 1).contiguous()
    big = _guarded(torch, (60, 70, 3))
    big[10:47, 5:58] = hwc
    window = big[10:47, 5:58]  # row pitch 210 > 3 * 53
    assert not window.is_contiguous() and window.stride(0) > 3 * 53
    for name, x, layout in (("hwc", hwc, "HWC"), ("chw", chw, "CHW"), ("window", window, "HWC"), ("channels-last view of chw", chw.permute(1, 2, 0), "HWC"),
                            ("chw view of hwc", hwc.permute(2, 0, 1), "CHW")):
        y = jpeggpu_amd.jpeg_roundtrip([x], quality=60, subsampling="4:2:0", layout=layout)[0]
        assert y.shape == x.shape
        y = y.cpu().numpy()
        assert np.array_equal(y if layout == "HWC" else y.transpose(1, 2, 0), want), name
    # out= with padded pitches: HWC rows of 3 * 53 + 11 bytes, CHW rows of 64 in planes of 40 rows, grey rows of 61
    buf = _guarded(torch, (37, 3 * 53 + 11))
    out = buf.as_strided((37, 53, 3), (3 * 53 + 11, 3, 1))
    assert jpeggpu_amd.jpeg_roundtrip([hwc], 60, "4:2:0", out=[out])[0] is out
    host = buf.cpu().numpy()
    assert np.array_equal(host[:, :3 * 53].reshape(37, 53, 3), want) and (host[:, 3 * 53:] == GUARD).all()
    buf = _guarded(torch, (3, 40, 64))
    jpeggpu_amd.jpeg_roundtrip([chw], 60, "4:2:0", layout="CHW", out=[buf[:, :37, :53]])
    host = buf.cpu().numpy()
    assert np.array_equal(host[:, :37, :53].transpose(1, 2, 0), want) and (host[:, 37:] == GUARD).all() and (host[:, :, 53:] == GUARD).all()
    g = np.ascontiguousarray(a[:, :, 1])
    buf = _guarded(torch, (40, 61))
    jpeggpu_amd.jpeg_roundtrip([torch.from_numpy(g).to(DEV)], 35, out=[buf[:37, :53]])
    host = buf.cpu().numpy()
    assert np.array_equal(host[:37, :53], R.roundtrip(g, 35)) and (host[37:] == GUARD).all() and (host[:, 53:] == GUARD).all()
    # a grey input with a pixel stride of 3, and a window whose pixels around it stay what they were
    y = jpeggpu_amd.jpeg_roundtrip([hwc[:, :, 1]], 35)[0]
    assert np.array_equal(y.cpu().numpy(), R.roundtrip(g, 35))
    # in place: out is the input
    for x, layout in ((hwc.clone(), "HWC"), (chw.clone(), "CHW"), (window, "HWC")):
        jpeggpu_amd.jpeg_roundtrip([x], 60, "4:2:0", layout=layout, out=[x])
        y = x.cpu().numpy()
        assert np.array_equal(y if layout == "HWC" else y.transpose(1, 2, 0), want), layout
    host = big.cpu().numpy()
    host[10:47, 5:58] = GUARD
    assert (host == GUARD).all(), "bytes around the window were written"
    x = torch.from_numpy(g).to(DEV)
    jpeggpu_amd.jpeg_roundtrip([x], 35, out=[x])
    assert np.array_equal(x.cpu().numpy(), R.roundtrip(g, 35))


def _item(x, dst, quality=75, subsampling="4:2:0", layout="HWC"):
    """A struct jpeggpu_ext_roundtrip_item of contiguous tensors: H x W grey, or HWC / CHW."""
    it = jpeggpu_amd.api.RoundtripItem()
    assert x.is_contiguous() and dst.is_contiguous() and dst.shape == x.shape
    if x.dim() == 2:
        (h, w), ch = x.shape, 1
        strides, pitch, plane = (w, 1, 0), w, 0
    elif layout == "HWC":
        h, w, ch = x.shape
        strides, pitch, plane = (3 * w, 3, 1), 3 * w, 0
    else:
        ch, h, w = x.shape
        strides, pitch, plane = (w, 1, h * w), w, h * w
    it.data, it.width, it.height, it.channels = x.data_ptr(), w, h, ch
    it.row_pitch, it.pixel_stride, it.channel_stride = strides
    it.quality, it.subsampling = quality, SUBSAMPLINGS[subsampling]
    it.dst, it.dst_pitch, it.plane_stride = dst.data_ptr(), pitch, plane
    return it


def _call(torch, items, layout="HWC", scratch=None, size=None):
    L = jpeggpu_amd.lib()
    arr = (jpeggpu_amd.api.RoundtripItem * len(items))(*items)
    need = L.jpeggpu_ext_roundtrip_scratch_size(arr, len(items))
    if scratch is None:
        scratch = torch.empty(max(need, 1), dtype=torch.uint8, device=DEV)
    return L.jpeggpu_ext_roundtrip_batch(arr, len(items), IMAGE_LAYOUTS[layout], scratch.data_ptr(), need if size is None else size,
                                         torch.cuda.current_stream().cuda_stream), need


def test_refusals_write_nothing(torch):
    L = jpeggpu_amd.lib()
    x = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (20, 24, 3), dtype=np.uint8)).to(DEV)
    g = x[:, :, 0].contiguous()
    dst, gdst = _guarded(torch, (20, 24, 3)), _guarded(torch, (20, 24))
    INV, NS = Status.INVALID_ARGUMENT, Status.NOT_SUPPORTED
    good = lambda: _item(x, dst)  # noqa: E731
    assert _call(torch, [good()], size=0)[0] == INV  # scratch too small
    need = _call(torch, [good()], size=0)[1]
    assert need > 0 and _call(torch, [good()], size=need - 1)[0] == INV
    arr = (jpeggpu_amd.api.RoundtripItem * 1)(good())
    stream = torch.cuda.current_stream().cuda_stream
    scratch = torch.empty(need, dtype=torch.uint8, device=DEV)
    assert L.jpeggpu_ext_roundtrip_batch(None, 1, 0, scratch.data_ptr(), need, stream) == INV
    assert L.jpeggpu_ext_roundtrip_batch(arr, 1, 0, None, need, stream) == INV
    for n in (0, -1, 65536):
        assert L.jpeggpu_ext_roundtrip_batch(arr, n, 0, scratch.data_ptr(), 1 << 40, stream) == INV
        assert L.jpeggpu_ext_roundtrip_scratch_size(arr, n) == 0
    for layout in (-1, 2):
        assert L.jpeggpu_ext_roundtrip_batch(arr, 1, layout, scratch.data_ptr(), need, stream) == INV

    def refused(change, item=good, layout="HWC", status=INV):
        it = item()
        change(it)
        arr1 = (jpeggpu_amd.api.RoundtripItem * 2)(item(), it)  # the bad item behind a good one: nothing of either is written
        st = L.jpeggpu_ext_roundtrip_batch(arr1, 2, IMAGE_LAYOUTS[layout], scratch.data_ptr(), 1 << 40, stream)
        assert st == status, (st, status)

    refused(lambda it: setattr(it, "data", None))
    refused(lambda it: setattr(it, "dst", None))
    for v in (0, -1, 65536):
        refused(lambda it: setattr(it, "width", v))
        refused(lambda it: setattr(it, "height", v))
    for v in (0, 2, 4):
        refused(lambda it: setattr(it, "channels", v))
    for v in (0, -1, 101):
        refused(lambda it: setattr(it, "quality", v))
        refused(lambda it: setattr(it, "quality", v), item=lambda: _item(g, gdst))
    for v in (-1, 3):
        refused(lambda it: setattr(it, "subsampling", v))
    refused(lambda it: setattr(it, "dst_pitch", 3 * 24 - 1))
    refused(lambda it: setattr(it, "dst_pitch", 23), item=lambda: _item(g, gdst))
    planar = x.permute(2, 0, 1).contiguous()
    chw = lambda: _item(planar, dst.view(3, 20, 24), layout="CHW")  # noqa: E731
    refused(lambda it: setattr(it, "dst_pitch", 23), item=chw, layout="CHW")
    refused(lambda it: setattr(it, "plane_stride", 20 * 24 - 1), item=chw, layout="CHW")
    # a call of 2^31 blocks: 32 grey items of 65535 x 65535 (nothing is dereferenced before the refusal); 31 such items pass
    # the plan and are refused for their scratch size only when it is too small
    huge = _item(g, gdst)
    huge.width = huge.height = huge.dst_pitch = 65535
    huge.row_pitch = 65535
    arr32 = (jpeggpu_amd.api.RoundtripItem * 32)(*[huge] * 32)
    assert L.jpeggpu_ext_roundtrip_batch(arr32, 32, 0, scratch.data_ptr(), 1 << 40, stream) == NS
    assert L.jpeggpu_ext_roundtrip_scratch_size(arr32, 32) == 0 and L.jpeggpu_ext_roundtrip_scratch_size(arr32, 31) > 0
    assert L.jpeggpu_ext_roundtrip_batch(arr32, 31, 0, scratch.data_ptr(), 64, stream) == INV
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == GUARD).all() and (gdst.cpu().numpy() == GUARD).all()
    # and the same items, unchanged, are taken
    assert _call(torch, [good(), _item(g, gdst, 40)])[0] == Status.SUCCESS
    want = R.roundtrip(x.cpu().numpy(), 75, "4:2:0")
    assert np.array_equal(dst.cpu().numpy(), want) and np.array_equal(gdst.cpu().numpy(), R.roundtrip(g.cpu().numpy(), 40))
    dst.fill_(GUARD)
    assert _call(torch, [chw()], layout="CHW")[0] == Status.SUCCESS
    assert np.array_equal(dst.view(3, 20, 24).cpu().numpy().transpose(1, 2, 0), want)


def test_calls_in_a_row_share_a_scratch_buffer(torch, pins):
    """Two calls and then five (the staging ring holds four) on one stream with ONE scratch buffer, nothing waited for in
    between: each call's descriptors and planes replace the call's before, in stream order."""
    picks = [i for i, c in enumerate(CASES) if (c[1], c[2]) in ((17, 33), (64, 48), (250, 131)) and c[4] == "noise" and c[6] in (10, 95)]
    assert len(picks) == 3 * 4 * 2
    groups = [picks[k::7] for k in range(7)]
    xs = {i: torch.from_numpy(R.case_input(CASES[i])).to(DEV) for i in picks}
    outs = {i: _guarded(torch, tuple(xs[i].shape)) for i in picks}
    arrays = [[_item(xs[i], outs[i], CASES[i][6], CASES[i][5]) for i in g] for g in groups]
    need = max(_call(torch, a, size=0)[1] for a in arrays)
    scratch = torch.empty(need, dtype=torch.uint8, device=DEV)
    for a in arrays[:2]:
        assert _call(torch, a, scratch=scratch, size=need)[0] == Status.SUCCESS
    torch.cuda.synchronize()
    for a in arrays[2:]:
        assert _call(torch, a, scratch=scratch, size=need)[0] == Status.SUCCESS
    torch.cuda.synchronize()
    wrong = [CASES[i][0] for i in picks if not R.matches_pin(pins, i, outs[i].cpu().numpy())]
    assert not wrong, wrong
