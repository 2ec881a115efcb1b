"""RGB-, CMYK- and YCCK-coded JPEGs on the GPU (jpeggpu_ext_get_color_space, the jpeggpu_ext_*_cs calls, decode_to_rgb,
decode_resized): every result equals the numpy restatement of Pillow's convert("RGB") (tests/color_ref.py), and Pillow's own
pinned outputs where they are pinned (tests/golden/color_pins.npz). Every comparison is exact."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

from tests import color_ref, draft_ref
from tests import pillow_resample_ref as R
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

GUARD = 0x5A
NOT_SUPPORTED = 4


@pytest.fixture(scope="module")
def torch_cuda(gpu_lib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def files():
    return color_ref.cases()


@pytest.fixture(scope="module")
def pins():
    return np.load(os.path.join(GOLDEN, "color_pins.npz"))


class Reference:
    """The restated RGB of every case and scale, computed once and shared (read-only)."""

    def __init__(self, files):
        from oracle import oracle

        self.files = files
        self.dec = {name: oracle.decode(data) for name, (data, _) in files.items()}
        self.cache = {}

    def rgb(self, name, d=1):
        if (name, d) not in self.cache:
            a = color_ref.color_rgb_of(self.dec[name], self.files[name][1], d)
            a.setflags(write=False)
            self.cache[name, d] = a
        return self.cache[name, d]

    def size(self, name, d=1):
        return draft_ref.ceil_div(self.dec[name].width, d), draft_ref.ceil_div(self.dec[name].height, d)

    def scales(self, name):
        """The 3 x 5 files are compared at full size only: draft() does not return their 1 / d image."""
        return (1,) if (self.dec[name].width, self.dec[name].height) == (3, 5) else color_ref.SCALES


@pytest.fixture(scope="module")
def ref(files):
    return Reference(files)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, len(bad), bad[:4].tolist())


def test_the_files_are_the_pinned_ones(files, pins):
    assert {k.partition("/")[2] for k in pins.files if k.startswith("jpeg_sha256/")} == set(files)
    for name, (data, model) in files.items():
        assert hashlib.sha256(data).hexdigest() == str(pins["jpeg_sha256/" + name]), (name, "input differs from the pinned one")
        assert int(pins["model/" + name]) == model, name


def test_decode_to_rgb_whole_at_every_scale(torch_cuda, files, ref, pins):
    import jpeggpu_amd

    n = pinned = replicated = 0
    for k, (name, (data, model)) in enumerate(files.items()):
        for d in ref.scales(name):
            got = jpeggpu_amd.decode_to_rgb(data, scale=d, device_scan=bool((k + d) & 1)).cpu().numpy()
            same(got, ref.rgb(name, d), (name, d))
            key = "%s/%d" % (name, d)
            if "rgb/" + key in pins.files:
                same(got, pins["rgb/" + key], (key, "Pillow's pin"))
            else:
                assert sha(got) == str(pins["rgb_sha256/" + key]), (key, "Pillow's pin")
            pinned += 1
            replicated += d == 8 and draft_ref.needs_replication(ref.dec[name], 8)
            n += 1
    assert n == 26 * 4 + 6
    assert pinned == sum(k.startswith(("rgb/", "rgb_sha256/")) for k in pins.files) - 6  # the 3 x 5 files' pins at 1/2
    assert replicated >= 4  # 1/8 with subsampling left: the replicating call, the fourth component included


def rectangles(W, H):
    """Rectangles that touch each edge and each corner, and an interior one that crosses the 256-pixel tile seam of a
    wide image (in the image's and in its own coordinates)."""
    w, h = max(1, (2 * W) // 3), max(1, (2 * H) // 3)
    out = [(0, 0, w, h), (W - w, 0, w, h), (0, H - h, w, h), (W - w, H - h, w, h), (0, H // 2, W, 1), (W // 2, 0, 1, H)]
    if W > 4 and H > 4:
        out.append((1, 2, W - 3, H - 4) if W < 262 else (3, 1, 259, H - 3))
    return out


def test_decode_to_rgb_crops(torch_cuda, files, ref):
    import jpeggpu_amd

    n = 0
    for k, (name, (data, model)) in enumerate(files.items()):
        for d in ref.scales(name) if k % 4 == 0 else (1,):
            W, H = ref.size(name, d)
            for x, y, w, h in rectangles(W, H):
                got = jpeggpu_amd.decode_to_rgb(data, scale=d, crop=(x, y, w, h)).cpu().numpy()
                same(got, ref.rgb(name, d)[y:y + h, x:x + w], (name, d, (x, y, w, h)))
                n += 1
    assert n > 32 * 6


def guarded_rgb(torch, W, H):
    """(buffer, pitch, pointer to pixel (0, 0)): a guard row above and below, guard bytes behind every row."""
    pitch = 3 * W + 7
    buf = torch.full((H + 2, pitch), GUARD, dtype=torch.uint8, device="cuda:0")
    return buf, pitch, buf[1:].data_ptr()


def read_guarded(torch, buf, W, H, what):
    torch.cuda.synchronize()
    a = buf.cpu().numpy()
    assert (a[0] == GUARD).all() and (a[-1] == GUARD).all() and (a[1:-1, 3 * W:] == GUARD).all(), (what, "wrote outside the image")
    return a[1:-1, :3 * W].reshape(H, W, 3)


def img_of(planes):
    from jpeggpu_amd.api import Img

    src = Img()
    for c, p in enumerate(planes):
        src.image[c], src.pitch[c] = p.data_ptr(), p.stride(0)
    return src


def test_c_calls_write_inside_their_buffers(torch_cuda, files, ref):
    """The four jpeggpu_ext_*_cs conversions into padded, guarded buffers: whole planes and a window, fancy and (at 1/8)
    replicating."""
    import jpeggpu_amd

    torch, L = torch_cuda, jpeggpu_amd.lib()
    n = differs = 0
    for name, (data, model) in files.items():
        for d in (1, 8) if len(ref.scales(name)) > 1 else (1,):
            kw = dict(scale=d, idct="islow", scale_mode="libjpeg")
            replicate = d == 8
            W, H = ref.size(name, d)
            planes, info = jpeggpu_amd.decode_to_planes(data, **kw)
            buf, pitch, ptr = guarded_rgb(torch, W, H)
            call = L.jpeggpu_ext_planes_to_rgbi_replicate_cs if replicate else L.jpeggpu_ext_planes_to_rgbi_fancy_cs
            src = img_of(planes)
            assert call(C.byref(info), model, C.byref(src), ptr, pitch, W, H, None) == 0, (name, d)
            same(read_guarded(torch, buf, W, H, (name, d)), ref.rgb(name, d), (name, d, "planes"))
            if replicate and draft_ref.needs_replication(ref.dec[name], 8):  # and it is not the fancy call's output
                buf, pitch, ptr = guarded_rgb(torch, W, H)
                assert L.jpeggpu_ext_planes_to_rgbi_fancy_cs(C.byref(info), model, C.byref(src), ptr, pitch, W, H, None) == 0
                differs += not np.array_equal(read_guarded(torch, buf, W, H, name), ref.rgb(name, d))
            x, y, w, h = rectangles(W, H)[-1]
            planes, info, ci = jpeggpu_amd.decode_to_planes(data, crop=(x, y, w, h), **kw)
            buf, pitch, ptr = guarded_rgb(torch, w, h)
            call = L.jpeggpu_ext_crop_to_rgbi_replicate_cs if replicate else L.jpeggpu_ext_crop_to_rgbi_fancy_cs
            src = img_of(planes)
            assert call(C.byref(info), model, C.byref(ci), C.byref(src), ptr, pitch, None) == 0, (name, d)
            same(read_guarded(torch, buf, w, h, (name, d)), ref.rgb(name, d)[y:y + h, x:x + w], (name, d, "crop"))
            n += 1
    assert n == 26 * 2 + 6 and differs >= 3


def test_the_entry_points_without_a_model_are_unchanged(torch_cuda, files, ref):
    """Three components are YCbCr there whatever the file says, and four are refused."""
    import jpeggpu_amd

    torch, L = torch_cuda, jpeggpu_amd.lib()
    for name in ("s444_adobe0", "s420_ids", "s420_seam_adobe1"):
        planes, info = jpeggpu_amd.decode_to_planes(files[name][0], idct="islow")
        got = jpeggpu_amd.planes_to_rgb(planes, info).cpu().numpy()
        same(got, color_ref.color_rgb_of(ref.dec[name], color_ref.YCBCR), name)
        same(jpeggpu_amd.planes_to_rgb(planes, info, color=jpeggpu_amd.ColorSpace.YCBCR).cpu().numpy(), got, name)
    planes, info = jpeggpu_amd.decode_to_planes(files["c444_adobe2"][0], idct="islow")
    W, H = ref.size("c444_adobe2")
    buf, pitch, ptr = guarded_rgb(torch, W, H)
    src = img_of(planes)
    for call in (L.jpeggpu_ext_planes_to_rgbi_fancy, L.jpeggpu_ext_planes_to_rgbi_replicate):
        assert call(C.byref(info), C.byref(src), ptr, pitch, W, H, None) == NOT_SUPPORTED
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == GUARD).all()


@pytest.mark.parametrize("layout", ("NHWC", "NCHW"))
@pytest.mark.parametrize("filt", R.FILTERS)
def test_one_resize_batch_mixes_the_models(torch_cuda, files, ref, layout, filt):
    """Grey, YCbCr, RGB, CMYK and YCCK items, cropped and whole, at scales 1 and 2, through decode_resized."""
    import jpeggpu_amd
    from oracle import oracle
    from tools import jpegsynth

    gray = jpegsynth.encode(150, 90, ((1, 1),), seed=9)
    plain = jpegsynth.encode(150, 90, color_ref.S420, seed=10)
    extra = {"gray": (gray, color_ref.GRAY), "plain": (plain, color_ref.YCBCR)}
    names = ["gray", "c22_adobe2", "s420_seam_adobe0", "plain", "c21_plain", "s420_ids", "ycck_dri", "c22_k1_adobe0", "s420_adobe1",
             "c444_adobe2", "ycck_ni", "c22_21_plain", "s444_ids", "c21_adobe2"]
    datas, crops, scales, want, models = [], [], [], [], set()
    for k, name in enumerate(names):
        data, model = extra[name] if name in extra else files[name]
        dec = oracle.decode(data) if name in extra else ref.dec[name]
        d = (1, 2)[(k // 2) % 2]
        W, H = draft_ref.ceil_div(dec.width, d), draft_ref.ceil_div(dec.height, d)
        rect = (W // 5, H // 7, max(1, (3 * W) // 5), max(1, (2 * H) // 3)) if k % 2 else None
        rgb = color_ref.color_rgb_of(dec, model, d) if name in extra else ref.rgb(name, d)
        if rect is not None:
            x, y, w, h = rect
            rgb = rgb[y:y + h, x:x + w]
        datas.append(data), crops.append(rect), scales.append(d), want.append(R.resize(rgb, 40, 32, filt))
        models.add((model, rect is None, d))
    assert {m for m, _, _ in models} == {color_ref.GRAY, color_ref.YCBCR, color_ref.RGB, color_ref.CMYK, color_ref.YCCK}
    got = jpeggpu_amd.decode_resized(datas, (32, 40), crops=crops, scales=scales, filt=filt, layout=layout).cpu().numpy()
    assert got.shape == ((len(names), 32, 40, 3) if layout == "NHWC" else (len(names), 3, 32, 40))
    for i, name in enumerate(names):
        same(got[i] if layout == "NHWC" else got[i].transpose(1, 2, 0), want[i], (name, scales[i], crops[i]))


def test_resize_of_wide_crops_and_refusal_of_replication(torch_cuda, files, ref):
    """A four-component item wider than one chunk of the horizontal pass, not resized in x; and decode_resized keeps
    refusing what libjpeg replicates."""
    import jpeggpu_amd

    data, _ = files["c22_adobe2"]
    W, H = ref.size("c22_adobe2")
    got = jpeggpu_amd.decode_resized([data, files["s420_adobe0"][0]], (60, W)).cpu().numpy()
    same(got[0], R.resize(ref.rgb("c22_adobe2"), W, 60, "bilinear"), "c22_adobe2")
    same(got[1], R.resize(ref.rgb("s420_adobe0"), W, 60, "bilinear"), "s420_adobe0")
    with pytest.raises(ValueError, match="replicates"):
        jpeggpu_amd.decode_resized([files["c21_adobe2"][0]], 16, scales=[8])
    jpeggpu_amd.decode_resized([files["c444_adobe2"][0]], 16, scales=[8])


def test_refusals_write_nothing(torch_cuda, files, ref):
    """A model that does not fit the component count, UNKNOWN, and non-integral ratios: NOT_SUPPORTED from every _cs call."""
    import jpeggpu_amd
    from jpeggpu_amd.api import FILTERS, LAYOUTS, ImgInfo, _resize_items
    from tools import jpegsynth

    torch, L = torch_cuda, jpeggpu_amd.lib()
    CS = jpeggpu_amd.ColorSpace
    inputs = {1: jpegsynth.encode(40, 24, ((1, 1),), seed=1), 2: jpegsynth.encode(40, 24, ((1, 1),) * 2, seed=2),
              3: files["s444_adobe0"][0], 4: files["c444_adobe2"][0]}
    fits = {1: (CS.GRAY,), 2: (), 3: (CS.YCBCR, CS.RGB), 4: (CS.CMYK, CS.YCCK)}
    good = jpeggpu_amd.decode_to_planes(inputs[3], idct="islow")
    tried = 0

    def refused(planes, info, ci, color, W, H):
        buf, pitch, ptr = guarded_rgb(torch, W, H)
        src = img_of(planes)
        if ci is None:
            for call in (L.jpeggpu_ext_planes_to_rgbi_fancy_cs, L.jpeggpu_ext_planes_to_rgbi_replicate_cs):
                assert call(C.byref(info), int(color), C.byref(src), ptr, pitch, W, H, None) == NOT_SUPPORTED, (info.num_components, color)
        else:
            for call in (L.jpeggpu_ext_crop_to_rgbi_fancy_cs, L.jpeggpu_ext_crop_to_rgbi_replicate_cs):
                assert call(C.byref(info), int(color), C.byref(ci), C.byref(src), ptr, pitch, None) == NOT_SUPPORTED, (info.num_components, color)
        # as the second item of a resize, behind one that is fine
        items, _keep = _resize_items([good[0], planes], [good[1], info], [None, ci])
        colors = (C.c_int * 2)(int(CS.YCBCR), int(color))
        assert L.jpeggpu_ext_resize_scratch_size_cs(items, colors, 2, 16, 12, FILTERS["bilinear"]) == 0
        out = torch.full((2 * 12 * 16 * 3,), GUARD, dtype=torch.uint8, device="cuda:0")
        scratch = torch.empty(1 << 20, dtype=torch.uint8, device="cuda:0")
        st = L.jpeggpu_ext_resize_to_rgb_cs(items, colors, 2, 16, 12, FILTERS["bilinear"], LAYOUTS["NHWC"], out.data_ptr(), scratch.data_ptr(), 1 << 20, None)
        assert st == NOT_SUPPORTED, (info.num_components, color)
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == GUARD).all() and (out.cpu().numpy() == GUARD).all(), "a refused call wrote"

    for nc, data in inputs.items():
        planes, info = jpeggpu_amd.decode_to_planes(data, idct="islow")
        cplanes, cinfo, ci = jpeggpu_amd.decode_to_planes(data, idct="islow", crop=(5, 3, 20, 11))
        for color in CS:
            if color in fits[nc]:
                continue
            refused(planes, info, None, color, planes[0].shape[1], planes[0].shape[0])
            refused(cplanes, cinfo, ci, color, 20, 11)
            tried += 1
    assert tried == 5 + 6 + 4 + 4
    # factors 3 and 2: a ratio that is not an integer, with a model that fits
    for nc, color in ((3, CS.RGB), (4, CS.CMYK), (4, CS.YCCK)):
        info = ImgInfo()
        info.num_components = nc
        planes = [torch.zeros((8, 64), dtype=torch.uint8, device="cuda:0") for _ in range(nc)]
        for c, h in enumerate((3, 2, 1, 1)[:nc]):
            info.subsampling.x[c], info.subsampling.y[c] = h, 1
            info.sizes_x[c], info.sizes_y[c] = 6 * h, 8
        refused(planes, info, None, color, 18, 8)
    # a NULL colour array
    items, _keep = _resize_items([good[0]], [good[1]], [None])
    assert L.jpeggpu_ext_resize_scratch_size_cs(items, None, 1, 16, 12, 0) == 0
    out = torch.full((12 * 16 * 3,), GUARD, dtype=torch.uint8, device="cuda:0")
    scratch = torch.empty(1 << 20, dtype=torch.uint8, device="cuda:0")
    assert L.jpeggpu_ext_resize_to_rgb_cs(items, None, 1, 16, 12, 0, 0, out.data_ptr(), scratch.data_ptr(), 1 << 20, None) == int(jpeggpu_amd.Status.INVALID_ARGUMENT)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == GUARD).all()
    # and the Python wrappers pass the status on
    with pytest.raises(jpeggpu_amd.JpegGpuError) as e:
        jpeggpu_amd.planes_to_rgb(good[0], good[1], color=CS.CMYK)
    assert e.value.status == jpeggpu_amd.Status.NOT_SUPPORTED
    with pytest.raises(jpeggpu_amd.JpegGpuError) as e:
        jpeggpu_amd.decode_to_rgb(inputs[2])
    assert e.value.status == jpeggpu_amd.Status.NOT_SUPPORTED
