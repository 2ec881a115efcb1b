"""The batched resize as a model's input on the GPU (jpeggpu_ext_resize_to_tensor, resize_to_tensor, decode_resized with
dtype / mean / std / flips). The expected value is always built from the EXISTING uint8 call on the same items
(resize_to_rgb, which other tests pin to Pillow) and torch on the CPU: u.to(float32).div(255), sub and div by float32 mean
and std tensors, .to(dtype) for the halves, torch.flip over the width -- code this feature does not touch. Bit patterns are
compared; equality is exact. Guard bytes (0xA5, 64 and more on each side) surround every output."""
import numpy as np
import pytest

from tests import cases, exif_ref
from tests import pillow_resample_ref as R

pytestmark = pytest.mark.gpu

GUARD = 0xA5
PAD = 64
IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
FILTERS = ("bilinear", "bicubic")
LAYOUT_NAMES = ("NHWC", "NCHW")
# (w, h): one tile; odd sizes with a short last lane; (260, 6): two column tiles, a last lane of fewer than four pixels
# and two row tiles; the smallest output
SIZES = ((8, 8), (7, 5), (13, 9), (260, 6), (1, 1))


@pytest.fixture(scope="module")
def torch_cuda(gpu_lib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


class Batch:
    """Decoded items (planes, infos, crop infos, colours) and the uint8 results of the existing call on them, each computed
    once and shared (read-only, on the CPU)."""

    def __init__(self, torch, picks):
        import jpeggpu_amd

        matrix = cases.matrix()
        self.torch = torch
        self.planes, self.infos, self.cis, self.colors = [], [], [], []
        for name, rect, color in picks:
            planes, info, ci = jpeggpu_amd.decode_to_planes(matrix[name], idct="islow", crop=rect)
            self.planes.append(planes), self.infos.append(info), self.cis.append(ci), self.colors.append(color)
        self.n = len(picks)
        self.cache = {}

    def u8(self, w, h, filt, layout, orientations=None):
        """resize_to_rgb of the items: the parent's route."""
        import jpeggpu_amd

        key = (w, h, filt, layout, tuple(orientations) if orientations else None)
        if key not in self.cache:
            out = jpeggpu_amd.resize_to_rgb(self.planes, self.infos, (h, w), self.cis, filt, layout, colors=self.colors, orientations=orientations)
            self.torch.cuda.synchronize()
            assert out.dtype == self.torch.uint8
            self.cache[key] = out.cpu()
        return self.cache[key]


@pytest.fixture(scope="module")
def mixed(torch_cuda):
    """A grey item, 4:2:0, 4:4:4 and a CMYK one (the horizontal pass that knows every model), each with a crop."""
    import jpeggpu_amd

    CS = jpeggpu_amd.ColorSpace
    return Batch(torch_cuda, [("gray", (11, 7, 90, 60), CS.GRAY), ("ss_2x2", (33, 21, 77, 99), CS.YCBCR), ("ss_1x1", (5, 5, 100, 80), CS.YCBCR),
                              ("four_comp_444", (9, 13, 70, 64), CS.CMYK)])


@pytest.fixture(scope="module")
def plain(torch_cuda):
    """Grey and YCbCr items alone (the three-tile horizontal pass): grey, 4:2:0, 4:2:2, 4:4:4 and an odd small file."""
    import jpeggpu_amd

    CS = jpeggpu_amd.ColorSpace
    return Batch(torch_cuda, [("gray", (1, 2, 30, 20), CS.GRAY), ("ss_2x2", (40, 30, 120, 100), CS.YCBCR), ("ss_2x1", (10, 5, 120, 70), CS.YCBCR),
                              ("ss_1x1", (0, 0, 200, 152), CS.YCBCR), ("odd_17x9", (1, 1, 15, 7), CS.YCBCR)])


def expected(torch, u8, layout, dtype, mean=None, std=None, flips=None):
    """ToTensor + Normalize + the cast + the flips of a uint8 result, by torch on the CPU."""
    x = u8
    if dtype != torch.uint8:
        shape = (1, 1, 1, 3) if layout == "NHWC" else (1, 3, 1, 1)
        m = torch.tensor(mean if mean is not None else (0.0, 0.0, 0.0), dtype=torch.float32).view(shape)
        s = torch.tensor(std if std is not None else (1.0, 1.0, 1.0), dtype=torch.float32).view(shape)
        x = u8.to(torch.float32).div(255).sub(m).div(s)
        assert x.dtype == torch.float32
        if dtype != torch.float32:
            x = x.to(dtype)
    if flips is not None:
        x = x.clone()
        for i, f in enumerate(flips):
            if f:
                x[i] = torch.flip(x[i], [1 if layout == "NHWC" else 2])
    return x


def bits(torch, x):
    return x if x.dtype == torch.uint8 else x.view(torch.int32 if x.element_size() == 4 else torch.int16)


def run(torch, batch, w, h, filt, layout, dtype, mean=None, std=None, flips=None, orientations=None, offset=0, stream=None, refused=False):
    """resize_to_tensor of the batch into a guarded output that starts `offset` elements behind a 256-byte boundary; the
    result on the CPU. `refused`: the call must raise INVALID_ARGUMENT and leave every byte as it was."""
    import jpeggpu_amd

    S = torch.empty(0, dtype=dtype).element_size()
    shape = (batch.n, h, w, 3) if layout == "NHWC" else (batch.n, 3, h, w)
    size = batch.n * h * w * 3 * S
    buf = torch.full((size + 2 * PAD + 512,), GUARD, dtype=torch.uint8, device="cuda:0")
    start = (-(buf.data_ptr() + PAD)) % 256 + PAD + offset * S
    out = buf[start:start + size].view(dtype).view(shape)
    assert out.data_ptr() == buf.data_ptr() + start and (out.data_ptr() - offset * S) % 256 == 0
    torch.cuda.synchronize()

    def call():
        return jpeggpu_amd.resize_to_tensor(batch.planes, batch.infos, (h, w), batch.cis, filt, layout, colors=batch.colors,
                                            orientations=orientations, dtype=dtype, mean=mean, std=std, flips=flips, out=out)

    if refused:
        with pytest.raises(jpeggpu_amd.JpegGpuError) as e:
            call()
        assert e.value.status == jpeggpu_amd.Status.INVALID_ARGUMENT
        torch.cuda.synchronize()
        assert bool((buf == GUARD).all()), "a refused call wrote something"
        return None
    if stream is not None:
        with torch.cuda.stream(stream):
            got = call()
        stream.synchronize()
    else:
        got = call()
    assert got is out and got.dtype == dtype and tuple(got.shape) == shape
    torch.cuda.synchronize()
    a = buf.cpu()
    assert bool((a[:start] == GUARD).all()) and bool((a[start + size:] == GUARD).all()), "a guard byte around the output was written"
    return a[start:start + size].view(dtype).view(shape)


def same(torch, got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    g, w = bits(torch, got), bits(torch, want)
    if not torch.equal(g, w):
        bad = (g != w).nonzero()
        first = tuple(bad[0].tolist())
        assert False, (what, len(bad), first, got[first].item(), want[first].item())


@pytest.mark.parametrize("size", SIZES)
def test_uint8_without_flips_is_the_uint8_call(torch_cuda, plain, mixed, size):
    torch = torch_cuda
    w, h = size
    for batch in (plain, mixed):
        for layout in LAYOUT_NAMES:
            for filt in FILTERS:
                got = run(torch, batch, w, h, filt, layout, torch.uint8)
                same(torch, got, batch.u8(w, h, filt, layout), ("u8", batch.n, size, layout, filt))


@pytest.mark.parametrize("norm", (IMAGENET, (None, None)), ids=("imagenet", "totensor"))
@pytest.mark.parametrize("size", SIZES)
def test_float32_is_totensor_and_normalize(torch_cuda, mixed, size, norm):
    torch = torch_cuda
    w, h = size
    mean, std = norm
    for layout in LAYOUT_NAMES:
        for filt in FILTERS:
            got = run(torch, mixed, w, h, filt, layout, torch.float32, mean, std)
            want = expected(torch, mixed.u8(w, h, filt, layout), layout, torch.float32, mean, std)
            same(torch, got, want, ("f32", size, layout, filt, mean))


@pytest.mark.parametrize("dtype_name", ("float16", "bfloat16"))
def test_halves_are_the_float32_value_converted_once(torch_cuda, mixed, dtype_name):
    torch = torch_cuda
    dtype = getattr(torch, dtype_name)
    mean, std = IMAGENET
    for w, h in ((8, 8), (13, 9)):
        for layout in LAYOUT_NAMES:
            got = run(torch, mixed, w, h, "bilinear", layout, dtype, mean, std)
            want = expected(torch, mixed.u8(w, h, "bilinear", layout), layout, dtype, mean, std)
            same(torch, got, want, (dtype_name, w, h, layout))


@pytest.mark.parametrize("size", ((8, 8), (260, 6), (7, 5), (13, 9)))  # the first two take the aligned mirrored loads, the others bytes
@pytest.mark.parametrize("oriented", (False, True), ids=("stored", "oriented"))
def test_flips_are_torch_flip_of_the_resized_item(torch_cuda, mixed, size, oriented):
    torch = torch_cuda
    w, h = size
    mean, std = IMAGENET
    orientations = [1, 3, 6, 8] if oriented else None
    for flips in ([1, 0, 1, 0], [0, 1, 1, 1]):
        for layout in LAYOUT_NAMES:
            u8 = mixed.u8(w, h, "bilinear", layout, orientations)
            got = run(torch, mixed, w, h, "bilinear", layout, torch.uint8, flips=flips, orientations=orientations)
            want = expected(torch, u8, layout, torch.uint8, flips=flips)
            same(torch, got, want, ("u8 flips", size, layout, flips, orientations))
            for i, f in enumerate(flips):  # said once more, item by item: unflipped items are untouched
                assert f or torch.equal(got[i], u8[i])
            got = run(torch, mixed, w, h, "bilinear", layout, torch.float32, mean, std, flips=flips, orientations=orientations)
            want = expected(torch, u8, layout, torch.float32, mean, std, flips)
            same(torch, got, want, ("f32 flips", size, layout, flips, orientations))


def test_bicubic_flips_and_the_halves(torch_cuda, plain):
    """The other filter and the 2-byte stores under a flip, on the batch of grey and YCbCr items."""
    torch = torch_cuda
    mean, std = IMAGENET
    flips = [1, 1, 0, 1, 0]
    for w, h in ((8, 8), (13, 9)):
        for layout in LAYOUT_NAMES:
            got = run(torch, plain, w, h, "bicubic", layout, torch.bfloat16, mean, std, flips=flips)
            want = expected(torch, plain.u8(w, h, "bicubic", layout), layout, torch.bfloat16, mean, std, flips)
            same(torch, got, want, ("bf16 bicubic flips", w, h, layout))


@pytest.mark.parametrize("case", (("float32", "NCHW"), ("float16", "NHWC")), ids=("f32_nchw", "f16_nhwc"))
def test_unaligned_destination(torch_cuda, mixed, case):
    """dst one element behind a 256-byte boundary: no store wider than the element's alignment allows."""
    torch = torch_cuda
    dtype, layout = getattr(torch, case[0]), case[1]
    mean, std = IMAGENET
    flips = [0, 1, 0, 1]
    got = run(torch, mixed, 8, 8, "bilinear", layout, dtype, mean, std, flips=flips, offset=1)
    want = expected(torch, mixed.u8(8, 8, "bilinear", layout), layout, dtype, mean, std, flips)
    same(torch, got, want, ("offset 1", case))


def test_a_refused_call_writes_nothing(torch_cuda, mixed):
    run(torch_cuda, mixed, 8, 8, "bilinear", "NHWC", torch_cuda.float32, IMAGENET[0], (0.229, 0.0, 0.225), refused=True)


def test_non_default_stream(torch_cuda, mixed):
    torch = torch_cuda
    mean, std = IMAGENET
    flips = [1, 0, 0, 1]
    got = run(torch, mixed, 13, 9, "bilinear", "NCHW", torch.float32, mean, std, flips=flips, stream=torch.cuda.Stream())
    want = expected(torch, mixed.u8(13, 9, "bilinear", "NCHW"), "NCHW", torch.float32, mean, std, flips)
    same(torch, got, want, "stream")


def test_decode_resized_is_the_whole_train_transform(torch_cuda):
    """decode_resized with dtype, mean, std and flips against decode_resized without them followed by the CPU steps; four
    files with EXIF orientations and displayed crops."""
    import jpeggpu_amd

    torch = torch_cuda
    matrix = cases.matrix()
    picks = (("ss_2x2", 1, (33, 21, 77, 99)), ("ss_1x1", 3, (5, 5, 100, 80)), ("gray", 6, (7, 11, 60, 90)), ("ss_2x1", 8, (10, 5, 70, 120)))
    datas = [exif_ref.with_orientation(matrix[name], o) for name, o, _ in picks]
    crops = [rect for _, _, rect in picks]
    mean, std = IMAGENET
    flips = [1, 0, 1, 1]
    kw = dict(crops=crops, layout="NCHW", exif_transpose=True)
    u8 = jpeggpu_amd.decode_resized(datas, (9, 13), **kw)
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == (4, 3, 9, 13)
    u8 = u8.cpu()
    got = jpeggpu_amd.decode_resized(datas, (9, 13), dtype=torch.float16, mean=mean, std=std, flips=flips, **kw)
    same(torch, got.cpu(), expected(torch, u8, "NCHW", torch.float16, mean, std, flips), "decode_resized f16")
    # only flips: bytes; only mean / std: float32
    got = jpeggpu_amd.decode_resized(datas, (9, 13), flips=flips, **kw)
    same(torch, got.cpu(), expected(torch, u8, "NCHW", torch.uint8, flips=flips), "decode_resized flips")
    got = jpeggpu_amd.decode_resized(datas, (9, 13), mean=mean, std=std, **kw)
    same(torch, got.cpu(), expected(torch, u8, "NCHW", torch.float32, mean, std), "decode_resized f32")
    # none of the new arguments: the parent's route -- Pillow's resize of the displayed crop, image by image
    for i, (data, rect) in enumerate(zip(datas, crops)):
        rgb = jpeggpu_amd.decode_to_rgb(data, crop=rect, exif_transpose=True).cpu().numpy()
        assert np.array_equal(u8[i].permute(1, 2, 0).numpy(), R.resize(rgb, 13, 9, "bilinear")), i
