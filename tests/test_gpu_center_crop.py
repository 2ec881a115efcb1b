"""Resize + CenterCrop on the GPU (jpeggpu_ext_resize_view_to_tensor, decode_center_cropped): every result equals the numpy
restatement (tests/center_crop_ref.py on tests/pillow_resample_ref.py) applied to the GPU's own full RGB of the item, and
Pillow's own outputs where they are pinned (tests/golden/center_crop_pins.npz); guard bytes around every output."""
import hashlib
import os

import numpy as np
import pytest

from tests import cases
from tests import center_crop_ref as CC
from tests import exif_ref
from tests import pillow_resample_ref as R
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

GUARD = 0xA5
PAD = 64
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


@pytest.fixture(scope="module")
def torch_cuda(gpu_lib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def matrix():
    return cases.matrix()


@pytest.fixture(scope="module")
def decoded(torch_cuda):
    """(data, d, stored crop or None) -> (planes, info, crop_info or None, color, replicate): decoded once, shared."""
    import jpeggpu_amd
    from jpeggpu_amd.api import _needs_replication

    cache = {}

    def get(data, d=1, crop=None):
        key = (data, d, crop)
        if key not in cache:
            kw = dict(idct="islow", scale=d, scale_mode="libjpeg", progressive=True, return_color=True)
            if crop is None:
                planes, info, color = jpeggpu_amd.decode_to_planes(data, **kw)
                ci = None
            else:
                planes, info, ci, color = jpeggpu_amd.decode_to_planes(data, crop=crop, **kw)
            cache[key] = (planes, info, ci, color, _needs_replication(info, d))
        return cache[key]

    return get


_RGB = {}


def stored_rgb(entry):
    """The whole item's RGB in stored order, by the calls that know no view: (h, w, 3) numpy. Computed once per entry."""
    import jpeggpu_amd

    planes, info, ci, color, rep = entry
    assert ci is None
    if id(planes) not in _RGB:
        _RGB[id(planes)] = (planes, jpeggpu_amd.planes_to_rgb(planes, info, replicate=rep, color=color).cpu().numpy())
    return _RGB[id(planes)][1]


def stored_size(entry):
    from jpeggpu_amd.api import _frame_size

    planes, info, ci = entry[:3]
    return (ci.full_x[0], ci.full_y[0]) if ci is not None else _frame_size(info)  # component 0 has the largest factors in every file here


def view_of(entry, resize, crop, o=1):
    """(resized_w, resized_h, x, y) of Resize(resize) + CenterCrop(crop) on the entry's displayed image, by the contract."""
    ch, cw = (crop, crop) if isinstance(crop, int) else crop
    dw, dh = exif_ref.orient_size(o, *stored_size(entry))
    rw, rh = CC.resized_size(dw, dh, resize)
    return (rw, rh) + CC.center_crop_window(rw, rh, cw, ch)


def run(torch, entries, views, crop, filt="bilinear", layout="NHWC", orients=None, dtype=None, mean=None, std=None, flips=None):
    """jpeggpu_ext_resize_view_to_tensor of the entries into a guarded output; the result as a CPU tensor, NHWC or NCHW."""
    import jpeggpu_amd

    ch, cw = (crop, crop) if isinstance(crop, int) else crop
    dtype = torch.uint8 if dtype is None else dtype
    n = len(entries)
    es = torch.empty((), dtype=dtype).element_size()
    size = n * ch * cw * 3 * es
    buf = torch.full((size + 2 * PAD,), GUARD, dtype=torch.uint8, device="cuda:0")
    shape = (n, ch, cw, 3) if layout == "NHWC" else (n, 3, ch, cw)
    out = buf[PAD:PAD + size].view(dtype).view(shape)
    torch.cuda.synchronize()
    got = jpeggpu_amd.resize_views_to_tensor([e[0] for e in entries], [e[1] for e in entries], views, (ch, cw), [e[2] for e in entries], filt, layout,
                                             colors=[e[3] for e in entries], orientations=orients, replicates=[e[4] for e in entries],
                                             dtype=dtype, mean=mean, std=std, flips=flips, out=out)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    a = buf.cpu()
    assert bool((a[:PAD] == GUARD).all()) and bool((a[PAD + size:] == GUARD).all()), "a guard byte around the output was written"
    return a[PAD:PAD + size].view(dtype).view(shape)


def nhwc(a, layout):
    a = a.numpy()
    return a if layout == "NHWC" else a.transpose(0, 2, 3, 1)


def want(entry, view, crop, filt, o=1, flip=False):
    """The restatement on the GPU's own full RGB of the item, displayed."""
    ch, cw = (crop, crop) if isinstance(crop, int) else crop
    shown = np.ascontiguousarray(exif_ref.apply(stored_rgb(entry), o))
    out = CC.resize_view(shown, view[0], view[1], view[2], view[3], cw, ch, filt)
    return out[:, ::-1] if flip else out


def assert_items(got, wants, what):
    for i, exp in enumerate(wants):
        bad = np.argwhere(got[i] != exp)
        assert len(bad) == 0, (what, i, len(bad), bad[:4].tolist())


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def normalised(torch, u8_nhwc):
    """ToTensor + Normalize of NHWC bytes by torch on the CPU, float32."""
    return torch.from_numpy(np.ascontiguousarray(u8_nhwc)).to(torch.float32).div(255).sub(torch.tensor(MEAN)).div(torch.tensor(STD))


# (resize, crop): a second, partial 32-column tile and an odd offset; a lane with fewer than 4 pixels
EVERY_FILE = ((48, 40), (64, 37))
# on the 200 x 152 files: an upscale (231 x 176); both directions unchanged (200 x 152)
ON_200x152 = ((176, 150), (152, 120))


@pytest.mark.parametrize("filt", R.FILTERS)
def test_whole_planes_of_every_file(torch_cuda, matrix, decoded, filt):
    from jpeggpu_amd.api import _frame_size

    entries = [decoded(data) for data in matrix.values()]
    entries = [e for e in entries if e[1].num_components in (1, 3)]
    assert len(entries) >= 26
    big = [e for e in entries if _frame_size(e[1]) == (200, 152)]
    assert len(big) >= 6
    for group, todo in ((entries, EVERY_FILE), (big, ON_200x152)):
        for resize, crop in todo:
            views = [view_of(e, resize, crop) for e in group]
            if (resize, crop) == (176, 150):
                assert views[0][:2] == (231, 176)
            if (resize, crop) == (152, 120):
                assert views[0] == (200, 152, 40, 16)
            wants = [want(e, v, crop, filt) for e, v in zip(group, views)]
            for layout in ("NHWC", "NCHW"):
                got = nhwc(run(torch_cuda, group, views, crop, filt, layout), layout)
                assert_items(got, wants, (resize, crop, filt, layout))


@pytest.mark.parametrize("filt", R.FILTERS)
def test_cropped_decode_equals_whole_planes(torch_cuda, matrix, decoded, filt):
    import jpeggpu_amd

    names = ("dri_7", "dri_row", "odd_partial_mcu", "ni_420_dri")
    for resize, crop in EVERY_FILE + ((300, 224),):
        whole = [decoded(matrix[n]) for n in names]
        views = [view_of(e, resize, crop) for e in whole]
        rects = [jpeggpu_amd.resize_view_rect(*stored_size(e), v, crop, filt) for e, v in zip(whole, views)]
        cropped = [decoded(matrix[n], 1, r) for n, r in zip(names, rects)]
        for e, c, r in zip(whole, cropped, rects):
            assert (c[2].x, c[2].y, c[2].width, c[2].height) == r
        w, h = stored_size(whole[1])
        assert rects[1][2] * rects[1][3] < w * h, "dri_row: the rectangle is the whole image"
        a = run(torch_cuda, whole, views, crop, filt)
        b = run(torch_cuda, cropped, views, crop, filt)
        assert torch_cuda.equal(a, b), (resize, crop, filt)
        assert_items(a.numpy(), [want(e, v, crop, filt) for e, v in zip(whole, views)], (resize, crop, filt))


@pytest.mark.parametrize("filt", R.FILTERS)
def test_padding(torch_cuda, matrix, decoded, filt):
    """Images smaller than the crop: zeros around the resized image, normalised like any byte for a float type."""
    a, b = decoded(matrix["ss_2x2"]), decoded(matrix["odd_17x9"])
    va, vb = view_of(a, 32, 40), view_of(b, (9, 17), 24)
    assert va == (42, 32, 1, -4)     # rows only: 4 above, 4 below
    assert vb == (17, 9, -3, -7)     # both, odd differences: 3 left and 4 right, 7 above and 8 below
    for entry, view, crop in ((a, va, 40), (b, vb, 24)):
        exp = want(entry, view, crop, filt)
        assert not exp[:max(-view[3], 0)].any() and not exp[:, :max(-view[2], 0)].any()
        for layout in ("NHWC", "NCHW"):
            got = nhwc(run(torch_cuda, [entry], [view], crop, filt, layout), layout)
            assert_items(got, [exp], ("u8", view, layout))
            f = run(torch_cuda, [entry], [view], crop, filt, layout, dtype=torch_cuda.float32, mean=MEAN, std=STD)
            f = f if layout == "NHWC" else f.permute(0, 2, 3, 1).contiguous()
            assert torch_cuda.equal(f.view(torch_cuda.int32), normalised(torch_cuda, exp[None]).view(torch_cuda.int32)), (view, layout)
    # both in one call
    got = run(torch_cuda, [a, b], [view_of(a, 32, 24), vb], 24, filt).numpy()
    assert_items(got, [want(a, view_of(a, 32, 24), 24, filt), want(b, vb, 24, filt)], "two")


@pytest.mark.parametrize("filt", R.FILTERS)
def test_orientations(torch_cuda, decoded, filt):
    """Views are in displayed pixels: all eight values on a 4:2:0 and a 4:2:2 file in one call, whole planes and the
    cropped decode of resize_view_rect; one padded case at orientation 6."""
    import jpeggpu_amd

    files = exif_ref.gpu_files()
    crop = (20, 28)
    entries, orients = [], []
    for name in ("s420", "s422"):
        for o in range(1, 9):
            entries.append(decoded(files[name][0]))
            orients.append(o)
    views = [view_of(e, 30, crop, o) for e, o in zip(entries, orients)]
    wants = [want(e, v, crop, filt, o) for e, v, o in zip(entries, views, orients)]
    for layout in ("NHWC", "NCHW"):
        assert_items(nhwc(run(torch_cuda, entries, views, crop, filt, layout, orients=orients), layout), wants, ("whole", filt, layout))
    rects = [jpeggpu_amd.resize_view_rect(*stored_size(e), v, crop, filt, o) for e, v, o in zip(entries, views, orients)]
    assert any(r[2] * r[3] < 53 * 37 for r in rects)
    cropped = [decoded(files[name][0], 1, r) for name, r in zip(["s420"] * 8 + ["s422"] * 8, rects)]
    assert_items(run(torch_cuda, cropped, views, crop, filt, orients=orients).numpy(), wants, ("cropped", filt))
    e = decoded(files["s422"][0])
    v = view_of(e, 16, 24, 6)
    assert v[2] < 0 or v[3] < 0
    assert_items(run(torch_cuda, [e], [v], 24, filt, orients=[6]).numpy(), [want(e, v, 24, filt, 6)], ("padded at 6", filt))


def mixed(matrix, decoded):
    """[(entry, orientation, resize, flip)]: sizes 17 x 9 to 496 x 360; grey, YCbCr and CMYK; scales 1, 2 and 8 (8 on the
    4:2:2 file: replicated chroma); orientations 6 and 3; a padded item; a flip; one cropped decode."""
    import jpeggpu_amd

    rows = [(decoded(matrix["gray"]), 1, 48, False),
            (decoded(matrix["ss_2x2"], 2), 1, 48, False),
            (decoded(matrix["ss_2x1"], 8), 1, 48, False),
            (decoded(matrix["four_comp_444"]), 1, 48, False),
            (decoded(matrix["ss_1x2"]), 6, 48, False),
            (decoded(matrix["dri_7"]), 3, 56, True),
            (decoded(matrix["odd_17x9"]), 1, 20, False),
            (decoded(matrix["odd_partial_mcu"]), 1, 64, True)]
    e = decoded(matrix["dri_row"])
    rect = jpeggpu_amd.resize_view_rect(*stored_size(e), view_of(e, 48, 40), 40, "bicubic")  # the larger of the two filters' rectangles
    rows.append((decoded(matrix["dri_row"], 1, rect), 1, 48, False))
    return rows


@pytest.mark.parametrize("filt", R.FILTERS)
def test_one_mixed_call(torch_cuda, matrix, decoded, filt):
    from jpeggpu_amd import ColorSpace

    rows = mixed(matrix, decoded)
    entries, orients, flips = [r[0] for r in rows], [r[1] for r in rows], [r[3] for r in rows]
    assert entries[2][4] and [e[3] for e in entries[:4]] == [ColorSpace.GRAY, ColorSpace.YCBCR, ColorSpace.YCBCR, ColorSpace.CMYK]
    views = [view_of(e, r[2], 40, r[1]) for e, r in zip(entries, rows)]
    assert views[6][2] < 0 and views[6][3] < 0
    got = run(torch_cuda, entries, views, 40, filt, orients=orients, flips=flips)
    for i in range(len(rows)):  # the same items one call each
        one = run(torch_cuda, [entries[i]], [views[i]], 40, filt, orients=[orients[i]], flips=[flips[i]])
        assert torch_cuda.equal(one[0], got[i]), (i, filt)
    whole = entries[:-1] + [decoded(matrix["dri_row"])]
    assert_items(got.numpy(), [want(e, v, 40, filt, o, f) for e, v, o, f in zip(whole, views, orients, flips)], ("mixed", filt))
    pins = np.load(os.path.join(GOLDEN, "center_crop_pins.npz"))
    assert views[2][:2] == (63, 48)
    assert sha(got[2].numpy()) == str(pins["out_sha256/ss_2x1/8/48/40x40/" + filt])  # Pillow after draft(): replicated chroma
    f16 = run(torch_cuda, entries, views, 40, filt, "NCHW", orients=orients, flips=flips, dtype=torch_cuda.float16, mean=MEAN, std=STD)
    exp = normalised(torch_cuda, got.numpy()).to(torch_cuda.float16).permute(0, 3, 1, 2).contiguous()
    assert torch_cuda.equal(f16.view(torch_cuda.int16), exp.view(torch_cuda.int16))


@pytest.mark.parametrize("filt", R.FILTERS)
def test_identity_view_is_resize_to_tensor(torch_cuda, matrix, decoded, filt):
    """{resized = out, x = y = 0} on whole items: jpeggpu_ext_resize_to_tensor byte for byte."""
    import jpeggpu_amd

    entries = [decoded(matrix[n]) for n in ("gray", "ss_2x1", "ss_2x2", "ss_4x1", "odd_partial_mcu", "four_comp_444", "odd_17x9")]
    orients = [1, 2, 5, 8, 3, 1, 6]
    flips = [False, True, False, True, False, False, True]
    args = ([e[0] for e in entries], [e[1] for e in entries])
    for (h, w), layout, dtype in (((90, 120), "NHWC", torch_cuda.uint8), ((152, 200), "NCHW", torch_cuda.float16), ((37, 9), "NCHW", torch_cuda.float32)):
        kw = dict(colors=[e[3] for e in entries], orientations=orients, dtype=dtype, flips=flips)
        if dtype != torch_cuda.uint8:
            kw.update(mean=MEAN, std=STD)
        exp = jpeggpu_amd.resize_to_tensor(*args, (h, w), None, filt, layout, **kw).cpu()
        got = run(torch_cuda, entries, [(w, h, 0, 0)] * len(entries), (h, w), filt, layout, orients=orients, dtype=dtype, mean=kw.get("mean"),
                  std=kw.get("std"), flips=flips)
        bits = {1: torch_cuda.uint8, 2: torch_cuda.int16, 4: torch_cuda.int32}[got.element_size()]
        assert torch_cuda.equal(got.view(bits), exp.view(bits)), (h, w, layout, dtype)


def test_pillow_pins(torch_cuda, matrix, photo_bytes):
    """Pillow's Image.open(f)[.draft()].convert("RGB").resize(...).crop(...), pinned: decode_center_cropped gives exactly
    that -- the small Pillow-encoded files, the 4:2:2 matrix file, and the photo at scale 1 and 8 to (256, 224)."""
    import jpeggpu_amd

    pins = np.load(os.path.join(GOLDEN, "center_crop_pins.npz"))
    lib_pins = np.load(os.path.join(GOLDEN, "libjpeg_pins.npz"))
    groups = {}
    for key in pins.files:
        kind, name, d, resize, crop, filt = key.split("/")
        groups.setdefault((d, resize, crop, filt), []).append((name, key))
    n = photos = 0
    for (d, resize, crop, filt), rows in groups.items():
        datas = [photo_bytes if name == "photo" else matrix[name] if name in matrix else lib_pins["jpeg/" + name].tobytes() for name, _ in rows]
        ch, cw = (int(v) for v in crop.split("x"))
        got = jpeggpu_amd.decode_center_cropped(datas, int(resize), (ch, cw), filt, scales=[int(d)] * len(datas)).cpu().numpy()
        for (name, key), g in zip(rows, got):
            if key.startswith("out/"):
                assert np.array_equal(g, pins[key]), key
            else:
                assert sha(g) == str(pins[key]), key
            n += 1
            photos += name == "photo"
    assert n == len(pins.files) >= 170 and photos == 4


@pytest.mark.parametrize("filt", R.FILTERS)
def test_decode_center_cropped_equals_the_per_image_route(torch_cuda, matrix, filt):
    """ONE batch decode and ONE view call against the route there was before: per image, decode_resized at that image's
    own (rh, rw) and a slice. Scales 1, 2 and 4, EXIF orientations, grey, CMYK and a progressive file."""
    import jpeggpu_amd

    files = exif_ref.gpu_files()
    rows = [(matrix["gray"], 1), (matrix["ss_1x1"], 1), (matrix["ss_2x1"], 2), (matrix["ss_2x2"], 4), (matrix["dri_row"], 1),
            (exif_ref.with_orientation(matrix["ss_1x2"], 6), 1), (exif_ref.with_orientation(matrix["dri_7"], 4), 2), (matrix["four_comp_444"], 1),
            (exif_ref.with_orientation(files["prog"][0], 7), 1), (matrix["odd_partial_mcu"], 1)]
    datas, scales = [r[0] for r in rows], [r[1] for r in rows]
    resize, crop = 36, (30, 34)
    for layout, kw in (("NHWC", {}), ("NCHW", dict(dtype=torch_cuda.float16, mean=MEAN, std=STD))):
        got = jpeggpu_amd.decode_center_cropped(datas, resize, crop, filt, layout, scales=scales, exif_transpose=True, **kw).cpu()
        assert tuple(got.shape) == ((10, 30, 34, 3) if layout == "NHWC" else (10, 3, 30, 34))
        for i, (data, d) in enumerate(rows):
            dec = jpeggpu_amd.Decoder()
            try:
                dec.set_progressive(True)
                if d != 1:
                    dec.set_scale(d)
                    dec.set_scale_mode("libjpeg")
                from jpeggpu_amd.api import _frame_size
                w, h = _frame_size(dec.parse_header(data))
                w, h = jpeggpu_amd.orient_size(dec.orientation(), w, h)
            finally:
                dec.cleanup()
            rw, rh = jpeggpu_amd.resized_size(w, h, resize)
            x, y = jpeggpu_amd.center_crop_window(rw, rh, crop)
            assert x >= 0 and y >= 0
            one = jpeggpu_amd.decode_resized([data], (rh, rw), filt=filt, layout=layout, scales=[d], exif_transpose=True, **kw).cpu()[0]
            exp = one[y:y + 30, x:x + 34] if layout == "NHWC" else one[:, y:y + 30, x:x + 34]
            bits = torch_cuda.uint8 if layout == "NHWC" else torch_cuda.int16
            assert torch_cuda.equal(got[i].contiguous().view(bits), exp.contiguous().view(bits)), (i, layout, filt)
