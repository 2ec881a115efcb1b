"""Thumbnails on the GPU (jpeggpu_ext_thumbnail_to_rgb, decode_thumbnails, thumbnail_jpeg): every case of
tests/thumbnail_cases.py equals Pillow's pinned Image.thumbnail (tests/golden/thumbnail_pins.npz) and the numpy restatement
(tests/thumbnail_ref.py) applied to the GPU's own decode at the plan's scale; zeros around every thumbnail in its canvas
slot and guard bytes around the canvas; refusals write nothing; thumbnail_jpeg's files equal Pillow's byte for byte."""
import hashlib

import numpy as np
import pytest

from tests import exif_ref
from tests import thumbnail_cases as TC
from tests import thumbnail_ref as T

pytestmark = pytest.mark.gpu

GUARD = 0xA5
PAD = 64
BY_NAME = {c[0]: c for c in TC.CASES}


@pytest.fixture(scope="module")
def torch_cuda(gpu_lib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def pins():
    return TC.load_pins()


_RGB = {}


def gpu_decode(data):
    """decode(scale) for thumbnail_ref.thumbnail: the GPU's own RGB of the file at that scale (one channel of a grey
    file), by the calls that know no thumbnail. Computed once per file and scale."""
    import jpeggpu_amd

    def decode(s):
        if (data, s) not in _RGB:
            a = jpeggpu_amd.decode_to_rgb(data, scale=s).cpu().numpy()
            _RGB[data, s] = a[:, :, 0] if components_of(data) == 1 else a
        return _RGB[data, s]

    return decode


def components_of(data):
    i = 2
    while data[i + 1] not in (0xC0, 0xC1, 0xC2):
        i += 2 + (data[i + 2] << 8 | data[i + 3])
    return data[i + 9]


def run(torch, datas, reqs, gaps, filt, margin=(3, 5), plans=None):
    """One BatchDecode at the plans' scales and one jpeggpu_ext_thumbnail_to_rgb into a guarded canvas that is `margin`
    (rows, columns) larger than the largest thumbnail. Checks the guards and the zeros around every thumbnail; returns
    (the thumbnails as numpy arrays -- (h, w) for a grey file, whose three channels must agree --, the plans)."""
    import jpeggpu_amd

    n = len(datas)
    if plans is None:
        plans = [jpeggpu_amd.thumbnail_plan(*exif_ref.frame_size(d), r, filt, g) for d, r, g in zip(datas, reqs, gaps)]
    ch, cw = max(p.out_h for p in plans) + margin[0], max(p.out_w for p in plans) + margin[1]
    size = n * ch * cw * 3
    buf = torch.full((size + 2 * PAD,), GUARD, dtype=torch.uint8, device="cuda:0")
    out = buf[PAD:PAD + size].view(n, ch, cw, 3)
    with jpeggpu_amd.BatchDecode(datas, scales=[p.scale for p in plans]) as bd:
        for p, rep in zip(plans, bd.replicates):
            p.replicate = int(bool(rep))
        bd.decode()
        got = jpeggpu_amd.thumbnails_to_rgb(bd.planes, bd.infos, plans, (ch, cw), filt, bd.colors, out=out)
        assert got.data_ptr() == out.data_ptr()
        torch.cuda.synchronize()
        grey = [info.num_components == 1 for info in bd.infos]
    a = buf.cpu().numpy()
    assert (a[:PAD] == GUARD).all() and (a[PAD + size:] == GUARD).all(), "a guard byte around the canvas was written"
    canvas = a[PAD:PAD + size].reshape(n, ch, cw, 3)
    thumbs = []
    for i, p in enumerate(plans):
        assert not canvas[i, p.out_h:].any() and not canvas[i, :, p.out_w:].any(), "item %d: its slot is not zero around the thumbnail" % i
        t = canvas[i, :p.out_h, :p.out_w]
        if grey[i]:
            assert np.array_equal(t[:, :, 0], t[:, :, 1]) and np.array_equal(t[:, :, 0], t[:, :, 2])
            t = t[:, :, 0]
        thumbs.append(t)
    return thumbs, plans


def equals_pin(pins, case, filt, got):
    k = TC.key(case, filt)
    if "out/" + k in pins.files:
        want = pins["out/" + k]
        assert got.shape == want.shape, (case, filt, got.shape, want.shape)
        assert np.array_equal(got, want), (case, filt, int((got != want).sum()), "bytes differ from Pillow")
    else:
        assert (got.shape[1], got.shape[0]) == tuple(pins["size/" + k]), (case, filt, got.shape)
        assert hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest() == str(pins["out_sha256/" + k]), (case, filt)


@pytest.mark.parametrize("filt", TC.FILTERS)
@pytest.mark.parametrize("case", [c[0] for c in TC.CASES])
def test_case_equals_pillow_and_the_restatement(torch_cuda, pins, case, filt):
    _, src, req, gap = BY_NAME[case]
    data = TC.source(pins, src)
    (got,), (p,) = run(torch_cuda, [data], [req], [gap], filt)
    w, h = exif_ref.frame_size(data)
    assert p.astuple() == T.plan(w, h, req[0], req[1], gap).astuple()
    want, _ = T.thumbnail(gpu_decode(data), w, h, req[0], req[1], filt, gap)
    assert got.shape == want.shape and np.array_equal(got, want), (case, filt, "differs from the restatement")
    equals_pin(pins, case, filt, got)


@pytest.mark.parametrize("filt", TC.FILTERS)
@pytest.mark.parametrize("order", ("forward", "backward"))
def test_mixed_batch(torch_cuda, pins, filt, order):
    """Every case in ONE call: items that reduce and items that do not, grey and RGB-coded ones beside YCbCr, identity
    tables beside real ones, each with its own size in the common canvas."""
    cases = TC.CASES if order == "forward" else TC.CASES[::-1]
    thumbs, plans = run(torch_cuda, [TC.source(pins, c[1]) for c in cases], [c[2] for c in cases], [c[3] for c in cases], filt, margin=(0, 0))
    assert any(p.fx > 1 or p.fy > 1 for p in plans) and any(p.identity for p in plans) and any(p.replicate for p in plans)
    for c, got in zip(cases, thumbs):
        equals_pin(pins, c[0], filt, got)


def test_decode_thumbnails_of_a_list(torch_cuda, pins):
    """The public call on files of one request: views of one canvas, (h, w, 3) or (h, w) for a grey file."""
    import jpeggpu_amd

    names = [c for c in TC.CASES if c[2] == (10, 10) and c[3] == 2.0]
    assert len(names) >= 6
    for filt in TC.FILTERS:
        views = jpeggpu_amd.decode_thumbnails([TC.source(pins, c[1]) for c in names], (10, 10), filt, 2.0)
        assert len({v.untyped_storage().data_ptr() for v in views}) == 1
        for c, v in zip(names, views):
            assert v.dtype == torch_cuda.uint8 and v.dim() == (2 if c[1] == "g641" else 3)
            equals_pin(pins, c[0], filt, v.cpu().numpy())
    with pytest.raises(ValueError):
        jpeggpu_amd.decode_thumbnails([], (10, 10))
    with pytest.raises(ValueError):
        jpeggpu_amd.decode_thumbnails([TC.source(pins, "small")], (10, 10), "lanczos")


@pytest.mark.parametrize("filt", TC.FILTERS)
def test_exif_transpose_of_the_eight_orientations(torch_cuda, pins, filt):
    import jpeggpu_amd

    base = TC.source(pins, TC.EXIF_SOURCE)
    datas = [exif_ref.with_orientation(base, o) for o in range(1, 9)]
    views = jpeggpu_amd.decode_thumbnails(datas, TC.EXIF_REQUEST, filt, TC.EXIF_GAP, exif_transpose=True)
    plain = jpeggpu_amd.decode_thumbnails(datas[4:5], TC.EXIF_REQUEST, filt, TC.EXIF_GAP)[0].cpu().numpy()
    for o, v in zip(range(1, 9), views):
        want = pins["exif/%d/%s" % (o, filt)]
        got = v.cpu().numpy()
        assert got.shape == want.shape and np.array_equal(got, want), (o, filt)
        assert np.array_equal(got, exif_ref.apply(plain, o)), (o, filt)  # the thumbnail first, then the turn


def test_refused_items_leave_the_canvas_alone(torch_cuda, pins):
    import jpeggpu_amd
    from jpeggpu_amd import JpegGpuError, Status
    from jpeggpu_amd.api import Thumbnail
    from tests import color_ref
    from tools import jpegsynth

    cmyk, model = color_ref.cases()["c444_adobe0"]
    assert model == color_ref.CMYK
    good = TC.source(pins, "c444")

    def refused(datas, plans):
        with pytest.raises(JpegGpuError) as e:
            run(torch_cuda, datas, None, None, "bicubic", plans=plans)
        assert e.value.status == Status.NOT_SUPPORTED
        buf = torch_cuda.full((len(datas) * 16 * 16 * 3,), GUARD, dtype=torch_cuda.uint8, device="cuda:0")
        with jpeggpu_amd.BatchDecode(datas, scales=[p.scale for p in plans]) as bd:
            bd.decode()
            with pytest.raises(JpegGpuError):
                jpeggpu_amd.thumbnails_to_rgb(bd.planes, bd.infos, plans, (16, 16), "bicubic", bd.colors, out=buf.view(len(datas), 16, 16, 3))
            torch_cuda.cuda.synchronize()
        assert bool((buf == GUARD).all()), "a refused call wrote to the canvas"

    plan = lambda d, gap=2.0: jpeggpu_amd.thumbnail_plan(*exif_ref.frame_size(d), (10, 10), "bicubic", gap)  # noqa: E731
    refused([good, cmyk], [plan(good), plan(cmyk)])  # behind an item that would have been reduced
    with pytest.raises(JpegGpuError) as e:
        jpeggpu_amd.decode_thumbnails([good, cmyk], (10, 10))
    assert e.value.status == Status.NOT_SUPPORTED
    tall = jpegsynth.encode(4, 500, TC.S444, quality=60, noise=6, seed=77)
    with pytest.raises(JpegGpuError) as e:  # more than 100 times taller than wide at the resize: the plan refuses it
        plan(tall, None)
    assert e.value.status == Status.NOT_SUPPORTED
    with pytest.raises(JpegGpuError):
        jpeggpu_amd.decode_thumbnails([tall], (10, 10), reducing_gap=None)
    by_hand = Thumbnail(1, 4, 500, 1, 1, 4, 500, 4.0, 500.0, 1, 10, 0, 0)
    refused([good, tall], [plan(good), by_hand])  # and so does the call, for a plan made by hand
    assert plan(tall).fy > 1 and plan(tall).identity == 0  # with the gap it is reduced first and is no longer tall
    (got,), _ = run(torch_cuda, [tall], [(10, 10)], [2.0], "bicubic")
    want, _ = T.thumbnail(gpu_decode(tall), 4, 500, 10, 10, "bicubic", 2.0)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("case,filt,save", TC.JPEG_CASES, ids=[c[0] for c in TC.JPEG_CASES])
def test_thumbnail_jpeg_equals_pillow_s_file(torch_cuda, pins, case, filt, save):
    import jpeggpu_amd

    _, src, req, gap = BY_NAME[case]
    data = TC.source(pins, src)
    for mode, extra in TC.JPEG_MODES.items():
        (got,) = jpeggpu_amd.thumbnail_jpeg([data], req, filt, gap, **save, **extra)
        want = pins["jpeg/%s/%s" % (TC.key(case, filt), mode)].tobytes()
        assert got == want, (case, filt, mode, len(got), len(want))
