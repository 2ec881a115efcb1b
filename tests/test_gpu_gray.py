"""Grey output on the GPU: luma-only decoding (jpeggpu_ext_set_luma_only) and the grey output stage (decode_to_gray,
decode_batch_to_gray, mode="L" of decode_resized and decode_center_cropped), exactly equal to the restatement
(tests/gray_ref.py) and to Pillow's pinned draft("L") outputs (tests/golden/gray_pins.npz). The files are gray_ref.files():
83 x 61 in every sampling, 1 x 1 .. 80 x 64 in 4:2:0 and 4:2:2, grey, RGB-coded, restart intervals, non-interleaved,
progressive, luma smaller than chroma."""
import numpy as np
import pytest

from tests import draft_ref, exif_ref, gray_ref

pytestmark = pytest.mark.gpu

POISON, GUARD = 0x5A, 0xA5
FILES = gray_ref.files()
NAMES = gray_ref.names(FILES)
YCC = [n for n in NAMES if n not in ("gray", "rgb", "rgb420")]


@pytest.fixture(scope="module")
def torch_cuda(gpu_lib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def pins():
    return gray_ref.load_pins()


@pytest.fixture(scope="module")
def ref():
    """(name, d) -> the restated grey of the stored image, computed once and shared (read-only)."""
    cache = {}

    def get(name, d=1):
        if (name, d) not in cache:
            a = gray_ref.gray(gray_ref.twin(FILES, name), d)
            a.setflags(write=False)
            cache[(name, d)] = a
        return cache[(name, d)]

    return get


def decode_luma(torch, data, d=1, libjpeg=True, crop=None, chroma="null", luma_only=True):
    """One lone decode through the Decoder: plane 0 (numpy), and the chroma buffers where they were passed (with a guard
    row above and below each)."""
    import jpeggpu_amd

    dec = jpeggpu_amd.Decoder()
    try:
        dec.set_luma_only(luma_only)
        dec.set_progressive(True)
        if libjpeg:
            dec.set_idct("islow")
            dec.set_scale_mode("libjpeg")
        dec.set_scale(d)
        if crop is not None:
            dec.set_crop(*crop)
        info = dec.parse_header(data)
        n = dec.get_buffer_size()
        tmp = torch.empty(n + 256, dtype=torch.uint8, device="cuda:0")
        base = (tmp.data_ptr() + 255) // 256 * 256
        bufs = [torch.full((info.sizes_y[c] + 2, info.sizes_x[c]), POISON, dtype=torch.uint8, device="cuda:0") for c in range(info.num_components)]
        ptrs = [b[1:-1].data_ptr() for b in bufs]
        if chroma == "null":
            ptrs[1:] = [0] * (len(ptrs) - 1)
        dec.transfer(base, n, 0)
        dec.decode(ptrs, [b.stride(0) for b in bufs], base, n, 0)
        torch.cuda.synchronize()
        return [b.cpu().numpy() for b in bufs], info
    finally:
        dec.cleanup()


@pytest.mark.parametrize("name", YCC)
def test_luma_only_planes_libjpeg_mode(torch_cuda, name):
    """ISLOW and the reduced IDCTs with per-component block sizes: plane 0 is the restatement's, scales 1..8; the chroma
    planes, passed and poisoned, are untouched, and so are the guard rows of all three."""
    from oracle import oracle

    dec = oracle.decode(gray_ref.twin(FILES, name))
    for d in gray_ref.SCALES:
        bufs, info = decode_luma(torch_cuda, FILES[name], d, chroma="poison")
        want = draft_ref.draft_planes_of(dec, d)[0]
        assert np.array_equal(bufs[0][1:-1], want), (name, d)
        assert (bufs[0][0] == POISON).all() and (bufs[0][-1] == POISON).all(), (name, d, "guard rows of plane 0")
        for b in bufs[1:]:
            assert (b == POISON).all(), (name, d, "a chroma plane was written")


@pytest.mark.parametrize("name", ("s420", "s411", "luma_small", "dri1", "ni", "prog", "s420_1x1", "s422_17x33"))
def test_luma_only_planes_default_mode(torch_cuda, name):
    """The reference transform and the uniform scale mode: plane 0 is the ordinary decode's, with NULL chroma pointers."""
    for d in gray_ref.SCALES:
        got, _ = decode_luma(torch_cuda, FILES[name], d, libjpeg=False)
        want, _ = decode_luma(torch_cuda, FILES[name], d, libjpeg=False, luma_only=False, chroma="poison")
        assert np.array_equal(got[0], want[0]), (name, d)
        assert (got[1] == POISON).all() and (got[2] == POISON).all()


@pytest.mark.parametrize("crop", ((3, 5, 41, 29), (0, 0, 83, 61), (17, 31, 1, 1), (64, 47, 19, 14)))
def test_luma_only_cropped_planes(torch_cuda, crop):
    """With jpeggpu_ext_set_crop the window of plane 0 is the ordinary cropped decode's, in both modes and at a scale."""
    for libjpeg, d in ((True, 1), (False, 1), (True, 2)):
        c = crop if d == 1 else (crop[0] // 2, crop[1] // 2, max(crop[2] // 2, 1), max(crop[3] // 2, 1))
        got, _ = decode_luma(torch_cuda, FILES["s420"], d, libjpeg, crop=c)
        want, _ = decode_luma(torch_cuda, FILES["s420"], d, libjpeg, crop=c, luma_only=False, chroma="poison")
        assert np.array_equal(got[0], want[0]), (crop, libjpeg, d)


@pytest.mark.parametrize("name", NAMES)
def test_decode_to_gray_is_the_restatement_and_pillow(torch_cuda, pins, ref, name):
    import jpeggpu_amd

    for d in gray_ref.SCALES:
        got = jpeggpu_amd.decode_to_gray(FILES[name], scale=d).cpu().numpy()
        assert np.array_equal(got, ref(name, d)), (name, d)
        key = "L/%s/%d" % (name, d)
        if key in pins.files:
            assert gray_ref.matches_pin(got, pins[key]), key


def test_cmyk_and_ycck_are_refused(torch_cuda):
    import jpeggpu_amd

    for name in ("ycck",):
        with pytest.raises(jpeggpu_amd.JpegGpuError) as e:
            jpeggpu_amd.decode_to_gray(exif_ref.gpu_files()[name][0])
        assert e.value.status == jpeggpu_amd.Status.NOT_SUPPORTED


@pytest.mark.parametrize("o", range(1, 9))
def test_orientations_with_a_crop(torch_cuda, pins, ref, o):
    """exif_transpose: the displayed image (Pillow's pinned exif_transpose of the "L" draft), and a crop in displayed pixels
    with an odd origin and size."""
    import jpeggpu_amd

    d = gray_ref.ORIENT_SCALE
    data = exif_ref.with_orientation(FILES[gray_ref.ORIENT_FILE], o)
    whole = jpeggpu_amd.decode_to_gray(data, scale=d, exif_transpose=True).cpu().numpy()
    assert np.array_equal(whole, exif_ref.apply(ref(gray_ref.ORIENT_FILE, d), o))
    assert gray_ref.matches_pin(whole, pins["exif/%d" % o])
    for name in ("s420", "s422", "luma_small", "rgb"):
        shown = exif_ref.apply(ref(name, 1), o)
        crop = (3, 5, min(41, shown.shape[1] - 3), min(29, shown.shape[0] - 5))
        got = jpeggpu_amd.decode_to_gray(exif_ref.with_orientation(FILES[name], o), crop=crop, exif_transpose=True).cpu().numpy()
        assert np.array_equal(got, shown[5:5 + crop[3], 3:3 + crop[2]]), (name, o)


def test_mixed_batch_in_one_call(torch_cuda, ref):
    """One jpeggpu_ext_decode_batch call of a luma-only decoder, an ordinary one, a cropped and a scaled luma-only one (and the
    same with the reference transform): every item is right, and the ordinary item's planes are those of a call without
    grey items."""
    from jpeggpu_amd.api import BatchDecode
    from oracle import oracle

    datas = [FILES["s420"], FILES["s422"], FILES["s420"], FILES["s411"], FILES["ni"], FILES["prog"]]
    luma = [True, False, True, True, True, True]
    crops = [None, None, (3, 5, 41, 29), None, None, None]
    scales = [1, 1, 1, 2, 4, 1]
    for idct in ("islow", "reference"):
        with BatchDecode(datas, scales=scales, crops=crops, luma_only=luma, idct=idct) as bd, BatchDecode([datas[1]] * 4, idct=idct) as plain:
            bd.decode()
            plain.decode()
            torch_cuda.cuda.synchronize()
            assert [len(p) for p in bd.planes] == [1, 3, 1, 1, 1, 1]
            for c in range(3):
                assert torch_cuda.equal(bd.planes[1][c], plain.planes[0][c]), (idct, c)
            if idct == "islow":
                names = ("s420", None, "s420", "s411", "ni", "prog")
                for i, name in enumerate(names):
                    if name is None:
                        continue
                    want = draft_ref.draft_planes_of(oracle.decode(gray_ref.twin(FILES, name)), scales[i])[0]
                    got = bd.planes[i][0].cpu().numpy()
                    if crops[i] is not None:
                        ci = bd.crop_infos[i]
                        want = want[ci.origin_y[0]:ci.origin_y[0] + got.shape[0], ci.origin_x[0]:ci.origin_x[0] + got.shape[1]]
                    assert np.array_equal(got, want), (idct, i)
            else:  # the reference transform at full size: the ordinary decode's plane 0
                with BatchDecode([datas[0]] * 4, idct=idct) as full:
                    full.decode()
                    torch_cuda.cuda.synchronize()
                    assert torch_cuda.equal(bd.planes[0][0], full.planes[0][0])


def test_decode_batch_to_gray_mixed_list(torch_cuda, ref):
    import jpeggpu_amd

    names = ["s420", "rgb", "gray", "prog", "luma_small", "s411", "s420_1x1", "rgb420", "s440", "s422_80x64"]
    scales = [1, 2, 1, 4, 1, 8, 1, 1, 2, 1]
    crops = [(3, 5, 41, 29), None, (1, 1, 80, 59), None, (7, 3, 33, 41), None, None, (2, 3, 11, 21), None, None]
    outs = jpeggpu_amd.decode_batch_to_gray([FILES[n] for n in names], crops=crops, scales=scales)
    for got, name, d, crop in zip(outs, names, scales, crops):
        want = ref(name, d)
        if crop is not None:
            want = want[crop[1]:crop[1] + crop[3], crop[0]:crop[0] + crop[2]]
        assert np.array_equal(got.cpu().numpy(), want), (name, d, crop)
    # every orientation in one call, displayed crops
    datas = [exif_ref.with_orientation(FILES["s422"], o) for o in range(1, 9)]
    outs = jpeggpu_amd.decode_batch_to_gray(datas, crops=[(3, 5, 41, 29)] * 8, exif_transpose=True)
    for o, got in zip(range(1, 9), outs):
        assert np.array_equal(got.cpu().numpy(), exif_ref.apply(ref("s422", 1), o)[5:34, 3:44]), o


def test_batch_to_gray_guards(torch_cuda, ref):
    """jpeggpu_ext_batch_to_gray into one guarded buffer with padded pitches and unaligned starts: the copy path (orientation
    1, luma at full resolution), the staged path and the transposing one write their rectangles and nothing else."""
    import jpeggpu_amd
    from jpeggpu_amd.api import BatchDecode, RgbItem, _resize_items

    torch = torch_cuda
    names, orients = ["s420", "s420", "luma_small", "s420", "rgb", "s422_80x64"], [1, 3, 1, 6, 8, 1]
    with BatchDecode([FILES[n] for n in names], luma_only=True) as bd:
        bd.decode()
        items, _keep = _resize_items(bd.planes, bd.infos, None)
        it = (RgbItem * len(names))()
        shapes, offs, total = [], [], 1
        for i, n in enumerate(names):
            h, w = exif_ref.apply(ref(n, 1), orients[i]).shape
            pitch = w + 5
            shapes.append((h, w, pitch))
            offs.append(total)
            total += h * pitch + 3
        buf = torch.full((total,), GUARD, dtype=torch.uint8, device="cuda:0")
        for i in range(len(names)):
            it[i].info, it[i].crop, it[i].src = items[i].info, items[i].crop, items[i].src
            it[i].color, it[i].orientation, it[i].replicate = int(bd.colors[i]), orients[i], 0
            it[i].dst, it[i].dst_pitch = buf.data_ptr() + offs[i], shapes[i][2]
        need = jpeggpu_amd.lib().jpeggpu_ext_batch_gray_scratch_size(len(names))
        scratch = torch.empty(need, dtype=torch.uint8, device="cuda:0")
        st = jpeggpu_amd.lib().jpeggpu_ext_batch_to_gray(it, len(names), scratch.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
        assert st == 0
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        mask = np.ones(total, bool)
        for i, n in enumerate(names):
            h, w, pitch = shapes[i]
            rows = host[offs[i]:offs[i] + h * pitch].reshape(h, pitch)
            assert np.array_equal(rows[:, :w], exif_ref.apply(ref(n, 1), orients[i])), (n, orients[i])
            m = mask[offs[i]:offs[i] + h * pitch].reshape(h, pitch)
            m[:, :w] = False
        assert (host[mask] == GUARD).all(), "bytes outside the rectangles were written"


@pytest.mark.parametrize("filt", gray_ref.FILTERS)
def test_resize_is_pillow(torch_cuda, pins, ref, filt):
    """mode="L" of decode_resized (views == NULL): 83 x 61 to 24 x 17, 5 x 3 and 224 x 224, both layouts, against Pillow's
    pinned resize of the "L" image; then a mixed list with crops against the restatement."""
    import jpeggpu_amd

    for ow, oh in gray_ref.RESIZES:
        for layout in ("NHWC", "NCHW"):
            out = jpeggpu_amd.decode_resized([FILES[gray_ref.RESIZE_FILE]], (oh, ow), filt=filt, layout=layout, mode="L")
            assert tuple(out.shape) == ((1, oh, ow, 1) if layout == "NHWC" else (1, 1, oh, ow)) and out.dtype == torch_cuda.uint8
            got = out.cpu().numpy().reshape(oh, ow)
            assert gray_ref.matches_pin(got, pins["resize/%s/%dx%d" % (filt, ow, oh)]), (ow, oh, layout)
            assert np.array_equal(got, gray_ref.resize(ref(gray_ref.RESIZE_FILE), ow, oh, filt))
    names = ["s444", "rgb", "gray", "prog", "luma_small", "s420_9x7"]
    crops = [(3, 5, 41, 29), None, (1, 1, 80, 59), None, (7, 3, 33, 41), None]
    out = jpeggpu_amd.decode_resized([FILES[n] for n in names], (17, 24), crops=crops, filt=filt, mode="L").cpu().numpy()
    for i, (name, crop) in enumerate(zip(names, crops)):
        a = ref(name)
        if crop is not None:
            a = a[crop[1]:crop[1] + crop[3], crop[0]:crop[0] + crop[2]]
        assert np.array_equal(out[i, :, :, 0], gray_ref.resize(a, 24, 17, filt)), (name, crop)


def test_resize_orientations_flips_and_types(torch_cuda, ref):
    """Every orientation with displayed crops in one call; per-item flips; the four element types with one mean and std."""
    import jpeggpu_amd

    torch = torch_cuda
    datas = [exif_ref.with_orientation(FILES["s422"], o) for o in range(1, 9)]
    crop = (3, 5, 41, 29)
    flips = [bool(o & 1) for o in range(8)]
    want = np.stack([gray_ref.resize(exif_ref.apply(ref("s422"), o)[5:34, 3:44], 24, 17, "bilinear") for o in range(1, 9)])
    plain = jpeggpu_amd.decode_resized(datas, (17, 24), crops=[crop] * 8, exif_transpose=True, mode="L").cpu().numpy()[..., 0]
    assert np.array_equal(plain, want)
    flipped = np.stack([w[:, ::-1] if f else w for w, f in zip(want, flips)])
    u8 = jpeggpu_amd.decode_resized(datas, (17, 24), crops=[crop] * 8, exif_transpose=True, mode="L", flips=flips)
    assert u8.dtype == torch.uint8 and np.array_equal(u8.cpu().numpy()[..., 0], flipped)
    mean, std = 0.449, 0.226
    x = torch.from_numpy(np.ascontiguousarray(flipped)).to(torch.float32)
    f32 = ((x / 255.0) - torch.tensor(mean, dtype=torch.float32)) / torch.tensor(std, dtype=torch.float32)  # ToTensor + Normalize on the CPU
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        for layout in ("NHWC", "NCHW"):
            out = jpeggpu_amd.decode_resized(datas, (17, 24), crops=[crop] * 8, exif_transpose=True, mode="L", flips=flips, dtype=dtype,
                                             mean=mean, std=(std,), layout=layout)
            assert out.dtype == dtype and tuple(out.shape) == ((8, 17, 24, 1) if layout == "NHWC" else (8, 1, 17, 24))
            assert torch.equal(out.cpu().reshape(8, 17, 24), f32.to(dtype)), (dtype, layout)
    # a width that is no multiple of 4: flipped items read bytes
    odd = jpeggpu_amd.decode_resized(datas[:2], (5, 7), mode="L", flips=[True, False]).cpu().numpy()[..., 0]
    assert np.array_equal(odd[0], gray_ref.resize(ref("s422"), 7, 5, "bilinear")[:, ::-1])
    with pytest.raises(ValueError):
        jpeggpu_amd.decode_resized(datas[:1], 8, mode="L", mean=(0.5, 0.5, 0.5))


def test_center_crop_with_padding(torch_cuda, ref):
    """mode="L" of decode_center_cropped: a window inside the resized image, and one that needs zero padding."""
    import jpeggpu_amd

    names = ["s420", "rgb", "s420_17x33", "luma_small"]
    for resize, crop in ((48, 32), (24, (40, 36))):
        for filt in gray_ref.FILTERS:
            out = jpeggpu_amd.decode_center_cropped([FILES[n] for n in names], resize=resize, crop=crop, filt=filt, mode="L").cpu().numpy()
            for i, n in enumerate(names):
                assert np.array_equal(out[i, :, :, 0], gray_ref.resize_center_crop(ref(n), resize, crop, filt)), (n, resize, crop, filt)


def test_corrupt_entropy_data_is_memory_safe(torch_cuda):
    """Random damage inside the entropy-coded segment of luma-only decodes: plane 0's content is unspecified; its guard rows
    and the poisoned chroma planes are untouched, and the decoder stays usable."""
    from oracle import oracle

    rng = np.random.default_rng(4321)
    for name in ("s420", "drirow", "ni"):
        good = FILES[name]
        si = oracle.scan_info(good, 0, 128)
        for trial in range(4):
            bad = bytearray(good)
            for pos in rng.integers(si.scan_begin + 4, si.scan_end - 4, size=int(rng.integers(1, 30))):
                if bad[pos] != 0xFF and bad[pos - 1] != 0xFF:
                    bad[pos] = int(rng.integers(0, 255))
            try:
                bufs, _ = decode_luma(torch_cuda, bytes(bad), (1, 2)[trial & 1], libjpeg=bool(trial & 2), chroma="poison")
            except Exception as e:  # a header the damage made invalid
                import jpeggpu_amd

                assert isinstance(e, jpeggpu_amd.JpegGpuError)
                continue
            assert (bufs[0][0] == POISON).all() and (bufs[0][-1] == POISON).all(), (name, trial)
            assert all((b == POISON).all() for b in bufs[1:]), (name, trial)
    got, _ = decode_luma(torch_cuda, FILES["s420"])
    assert np.array_equal(got[0][1:-1], gray_ref.gray(FILES["s420"]))
