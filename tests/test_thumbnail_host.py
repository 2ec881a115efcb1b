"""Thumbnails on the host (jpeggpu_ext_thumbnail_plan, jpeggpu_ext_resize_box_weights, the checks of
jpeggpu_ext_thumbnail_to_rgb and its scratch size): the library against the numpy restatement of Pillow's chain
(tests/thumbnail_ref.py). No GPU needed: every device call below is refused before anything is enqueued."""
import ctypes as C

import numpy as np
import pytest

import jpeggpu_amd
from jpeggpu_amd import JpegGpuError, Status
from jpeggpu_amd import build as jbuild
from jpeggpu_amd.api import CropInfo, Img, ImgInfo, ResizeItem, Thumbnail
from tests import pillow_resample_ref as R
from tests import thumbnail_ref as T

BILINEAR, BICUBIC = 0, 1
GAPS = (None, 1.0, 2.0, 3.0)


@pytest.fixture(scope="module")
def L():
    jbuild.build()
    return jpeggpu_amd.lib()


def plan_grid():
    """(w, h, rw, rh): requests of 1, rw >= W only, rh >= H only, requests that hold the image, ties in round_aspect
    (y * aspect or x / aspect ending in .5, and ratios at the same distance from floor and ceil), extreme shapes, and a
    seeded random part."""
    sizes = [(640, 480), (480, 640), (641, 479), (500, 375), (4032, 3024), (333, 251), (64, 64), (65, 33), (1, 1), (1, 500), (500, 1),
             (3, 2), (2, 3), (7, 5), (5000, 40), (40, 3999), (40, 4001), (17, 9), (65535, 65535), (65535, 1)]
    reqs = [(1, 1), (1, 100), (100, 1), (10, 10), (64, 64), (128, 128), (48, 48), (96, 4), (4, 96), (3, 3), (5, 5), (7, 7), (2, 1), (1, 2),
            (640, 10), (10, 640), (700, 100), (100, 700), (640, 480), (5000, 5000), (33, 17), (80, 60), (81, 60), (320, 240), (321, 241)]
    grid = [(w, h, rw, rh) for w, h in sizes for rw, rh in reqs]
    grid += [(3, 2, 1, 5), (2, 3, 5, 1), (6, 4, 1, 9), (10, 4, 5, 1), (4, 10, 1, 5), (100, 8, 25, 1), (8, 100, 1, 25), (15, 10, 5, 3), (10, 15, 3, 5)]
    # the draft hits the final size (with gap 1.0): sizes that divide, requested at 1/2, 1/4 and 1/8
    grid += [(w, h, w // s, h // s) for w, h in ((640, 480), (320, 240), (800, 600), (64, 64), (160, 120), (1024, 768)) for s in (2, 4, 8)]
    rng = np.random.default_rng(17)
    for _ in range(600):
        w, h = int(rng.integers(1, 5000)), int(rng.integers(1, 5000))
        grid.append((w, h, int(rng.integers(1, 400)), int(rng.integers(1, 400))))
    return grid


def test_plan_equals_the_restatement(L):
    seen = {"noop": 0, "identity": 0, "draft": 0, "reduce": 0, "fx_ne_fy": 0, "refused": 0, "one": 0, "ragged": 0}
    for w, h, rw, rh in plan_grid():
        for gap in GAPS:
            try:
                want = T.plan(w, h, rw, rh, gap)
            except T.Refused:
                with pytest.raises(JpegGpuError) as e:
                    jpeggpu_amd.thumbnail_plan(w, h, (rw, rh), "bicubic", gap)
                assert e.value.status == Status.NOT_SUPPORTED, (w, h, rw, rh, gap)
                seen["refused"] += 1
                continue
            got = jpeggpu_amd.thumbnail_plan(w, h, (rw, rh), "bilinear" if (w + rw) % 2 else "bicubic", gap)
            assert got.astuple() == want.astuple(), (w, h, rw, rh, gap)
            assert got.replicate == 0
            seen["noop"] += rw >= w and rh >= h
            seen["identity"] += bool(want.identity) and not (rw >= w and rh >= h)
            seen["draft"] += want.scale > 1
            seen["reduce"] += want.fx > 1 or want.fy > 1
            seen["fx_ne_fy"] += want.fx != want.fy
            seen["one"] += want.out_w == 1 or want.out_h == 1
            seen["ragged"] += (want.fx > 1 and want.dec_w % want.fx != 0) or (want.fy > 1 and want.dec_h % want.fy != 0)
    assert all(v >= 10 for v in seen.values()), seen


def test_plan_names_the_issue_s_example(L):
    p = jpeggpu_amd.thumbnail_plan(640, 480, (10, 10), "bicubic", 2.0)
    assert (p.scale, p.dec_w, p.dec_h, p.fx, p.fy, p.red_w, p.red_h, p.out_w, p.out_h) == (8, 80, 60, 4, 3, 20, 20, 10, 8)
    p = jpeggpu_amd.thumbnail_plan(4032, 3024, (48, 48))
    assert (p.scale, p.dec_w, p.dec_h, p.fx, p.fy, p.red_w, p.red_h, p.out_w, p.out_h) == (8, 504, 378, 5, 5, 101, 76, 48, 36)
    p = jpeggpu_amd.thumbnail_plan(640, 480, (10, 10), "bicubic", None)
    assert (p.scale, p.fx, p.fy, p.dec_w, p.out_w, p.out_h, p.identity) == (1, 1, 1, 640, 10, 8, 0)


def test_plan_arguments(L):
    p = Thumbnail()
    f = L.jpeggpu_ext_thumbnail_plan
    assert f(640, 480, 10, 10, BICUBIC, 2.0, C.byref(p)) == Status.SUCCESS
    assert f(640, 480, 10, 10, BICUBIC, 2.0, None) == Status.INVALID_ARGUMENT
    for w, h, rw, rh in ((0, 480, 10, 10), (640, 0, 10, 10), (640, 480, 0, 10), (640, 480, 10, 0), (65536, 480, 10, 10), (640, 65536, 10, 10)):
        assert f(w, h, rw, rh, BICUBIC, 2.0, C.byref(p)) == Status.INVALID_ARGUMENT, (w, h, rw, rh)
    assert f(640, 480, 10, 10, BICUBIC, 0.5, C.byref(p)) == Status.INVALID_ARGUMENT
    assert f(640, 480, 10, 10, BICUBIC, float("nan"), C.byref(p)) == Status.INVALID_ARGUMENT
    assert f(640, 480, 10, 10, 2, 2.0, C.byref(p)) == Status.NOT_SUPPORTED
    assert f(640, 480, 10, 10, BICUBIC, -1.0, C.byref(p)) == Status.SUCCESS and p.scale == 1  # None
    assert f(40, 4001, 10, 10, BICUBIC, 0.0, C.byref(p)) == Status.NOT_SUPPORTED  # step 6: 4001 > 100 * 40, and it gets shorter
    assert f(40, 4000, 10, 10, BICUBIC, 0.0, C.byref(p)) == Status.SUCCESS
    with pytest.raises(ValueError):
        jpeggpu_amd.thumbnail_plan(640, 480, (0.5, 10))
    with pytest.raises(ValueError):
        jpeggpu_amd.thumbnail_plan(640, 480, (10, 10), "lanczos")
    assert jpeggpu_amd.thumbnail_plan(640, 480, (10.9, 10.2)).astuple() == jpeggpu_amd.thumbnail_plan(640, 480, (10, 10)).astuple()


def box_cases():
    """(in, extent, out): extents that are no binary32 values (rounded on the way in, as Pillow's box is), fractional
    boxes of drafts and reductions, extents beyond and below the size, and the integer extent."""
    cases = [(77, 460 / 6, 10), (20, 80 / 4, 10), (20, 60 / 3, 8), (63, 500 / 8, 24), (47, 375 / 8, 18), (101, 504 / 5, 48), (76, 378 / 5, 36),
             (13, 100 / 8, 5), (13, 100 / 8, 13), (13, 12.5, 1), (1, 0.125, 1), (2, 1.125, 1), (9, 8.875, 30), (100, 99.5, 100), (100, 100.0, 100),
             (7, 6.3, 7)]
    rng = np.random.default_rng(23)
    for _ in range(150):
        n = int(rng.integers(1, 700))
        cases.append((n, float(n - rng.random()), int(rng.integers(1, 200))))
    return cases


@pytest.mark.parametrize("filt", R.FILTERS)
def test_box_weights_equal_the_restatement(L, filt):
    for n, extent, out in box_cases():
        e32 = np.float32(extent)
        first, count, w = jpeggpu_amd.resize_box_weights(n, extent, out, filt)
        if out == n and float(e32) == n:
            assert np.array_equal(first, np.arange(out)) and (count == 1).all() and (w[:, 0] == 1 << 22).all()
            continue
        rf, rc, rw = T.box_weights(n, e32, out, filt)
        assert w.shape == rw.shape, (n, extent, out)
        assert np.array_equal(first, rf) and np.array_equal(count, rc) and np.array_equal(w, rw), (n, extent, out, filt)
        assert np.abs(w).max() < 1 << 23
        assert (first + count <= n).all() and (first >= 0).all()


@pytest.mark.parametrize("filt", R.FILTERS)
def test_box_weights_of_the_integer_extent_are_resize_weights(L, filt):
    rng = np.random.default_rng(29)
    pairs = [(1, 1), (1, 9), (9, 1), (224, 224), (640, 10), (10, 640)] + [(int(a), int(b)) for a, b in zip(rng.integers(1, 3000, 120), rng.integers(1, 400, 120))]
    for n, out in pairs:
        a, b = jpeggpu_amd.resize_box_weights(n, float(n), out, filt), jpeggpu_amd.resize_weights(n, out, filt)
        for x, y in zip(a, b):
            assert x.shape == y.shape and np.array_equal(x, y), (n, out, filt)


def test_box_weights_arguments(L):
    f, c, w = (C.c_int * 8)(), (C.c_int * 8)(), (C.c_int * 64)()
    g = L.jpeggpu_ext_resize_box_weights
    assert g(8, 7.5, 4, BILINEAR, f, c, w, 5) == Status.SUCCESS  # 2 ceil(1.875) + 1
    assert g(8, 7.5, 4, BILINEAR, f, c, w, 4) == Status.INVALID_ARGUMENT
    assert g(8, 7.5, 4, BICUBIC, f, c, w, 8) == Status.INVALID_ARGUMENT  # needs 9
    assert g(8, 7.5, 4, 2, f, c, w, 64) == Status.NOT_SUPPORTED
    assert g(0, 7.5, 4, BILINEAR, f, c, w, 64) == Status.INVALID_ARGUMENT
    assert g(8, 7.5, 0, BILINEAR, f, c, w, 64) == Status.INVALID_ARGUMENT
    assert g(8, 0.0, 4, BILINEAR, f, c, w, 64) == Status.INVALID_ARGUMENT
    assert g(8, float("inf"), 4, BILINEAR, f, c, w, 64) == Status.INVALID_ARGUMENT
    assert g(8, 7.5, 4, BILINEAR, None, c, w, 64) == Status.INVALID_ARGUMENT
    assert g(8, 7.5, 4, BILINEAR, f, c, None, 64) == Status.INVALID_ARGUMENT


FAKE = 1 << 40  # a device address that is never dereferenced: every call below is refused before anything is enqueued
GRAY, YCBCR, RGB, CMYK, YCCK = 1, 2, 3, 4, 5


def item(size, sampling=((2, 2), (1, 1), (1, 1)), crop=False):
    """(ResizeItem, objects to keep) of a made-up decoded image of `size` pixels with fake plane addresses."""
    info, src = ImgInfo(), Img()
    n = len(sampling)
    info.num_components = n
    hmax, vmax = max(s[0] for s in sampling), max(s[1] for s in sampling)
    for c, (h, v) in enumerate(sampling):
        info.subsampling.x[c], info.subsampling.y[c] = h, v
        info.sizes_x[c] = -(-size[0] * h // hmax)
        info.sizes_y[c] = -(-size[1] * v // vmax)
        src.image[c], src.pitch[c] = FAKE + c * (1 << 24), info.sizes_x[c]
    it = ResizeItem()
    it.info, it.src = C.pointer(info), C.pointer(src)
    ci = None
    if crop:
        ci = CropInfo()
        ci.x, ci.y, ci.width, ci.height = 0, 0, size[0], size[1]
        for c in range(n):
            ci.full_x[c], ci.full_y[c] = info.sizes_x[c], info.sizes_y[c]
        it.crop = C.pointer(ci)
    return it, (info, src, ci)


def arrays(its, plans, colors=None):
    a = (ResizeItem * len(its))()
    for i, (it, _) in enumerate(its):
        a[i] = it
    cs = (C.c_int * len(its))(*colors) if colors is not None else None
    return a, cs, (Thumbnail * len(plans))(*plans)


def planned(w, h, req, gap=2.0, sampling=((2, 2), (1, 1), (1, 1))):
    p = jpeggpu_amd.thumbnail_plan(w, h, req, "bicubic", gap)
    return item((p.dec_w, p.dec_h), sampling), p


def size_and_call(L, its, plans, canvas=(96, 96), colors=None, filt=BICUBIC, n=None, scratch=FAKE, dst=FAKE, size=None):
    a, cs, ps = arrays(its, plans, colors)
    n = len(its) if n is None else n
    need = L.jpeggpu_ext_thumbnail_scratch_size(a, cs, ps, n, canvas[0], canvas[1], filt)
    st = L.jpeggpu_ext_thumbnail_to_rgb(a, cs, ps, n, canvas[0], canvas[1], filt, dst, scratch, need if size is None else size, None)
    return need, st


def copy_of(p, **kw):
    q = Thumbnail.from_buffer_copy(p)
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def test_every_refusal(L):
    it, p = planned(640, 480, (10, 10))  # scale 8, factors 4 and 3
    assert (p.fx, p.fy) == (4, 3)
    # what is refused only for the missing memory: the size call accepts it
    need, st = size_and_call(L, [it], [p], dst=None)
    assert need > 0 and st == Status.INVALID_ARGUMENT
    assert size_and_call(L, [it], [p], scratch=None)[1] == Status.INVALID_ARGUMENT
    assert size_and_call(L, [it], [p], size=need - 1)[1] == Status.INVALID_ARGUMENT

    def refused(status, its, plans, **kw):
        need, st = size_and_call(L, its, plans, **kw)
        assert need == 0 and st == status, (need, st, kw)

    refused(Status.INVALID_ARGUMENT, [it], [p], n=0)
    refused(Status.INVALID_ARGUMENT, [it], [p], canvas=(0, 96))
    refused(Status.INVALID_ARGUMENT, [it], [p], canvas=(96, 0))
    refused(Status.INVALID_ARGUMENT, [it], [p], canvas=(9, 96))  # out_w = 10 does not fit
    refused(Status.INVALID_ARGUMENT, [it], [p], canvas=(96, 7))  # out_h = 8 does not fit
    refused(Status.NOT_SUPPORTED, [it], [p], filt=2)
    a, cs, ps = arrays([it], [p])
    assert L.jpeggpu_ext_thumbnail_scratch_size(None, cs, ps, 1, 96, 96, BICUBIC) == 0
    assert L.jpeggpu_ext_thumbnail_scratch_size(a, cs, None, 1, 96, 96, BICUBIC) == 0
    assert L.jpeggpu_ext_thumbnail_to_rgb(None, cs, ps, 1, 96, 96, BICUBIC, FAKE, FAKE, 1 << 30, None) == Status.INVALID_ARGUMENT
    assert L.jpeggpu_ext_thumbnail_to_rgb(a, cs, None, 1, 96, 96, BICUBIC, FAKE, FAKE, 1 << 30, None) == Status.INVALID_ARGUMENT
    # the colour models Pillow keeps as CMYK, and models that do not fit
    four = item((80, 60), ((1, 1),) * 4)
    refused(Status.NOT_SUPPORTED, [four], [p], colors=[CMYK])
    refused(Status.NOT_SUPPORTED, [four], [p], colors=[YCCK])
    refused(Status.NOT_SUPPORTED, [four], [p])  # four components without a model
    refused(Status.NOT_SUPPORTED, [it], [p], colors=[GRAY])
    refused(Status.NOT_SUPPORTED, [item((80, 60), ((3, 1), (2, 1), (1, 1)))], [p])  # non-integral ratios
    # a cropped decode is no thumbnail source
    refused(Status.INVALID_ARGUMENT, [item((80, 60), crop=True)], [p])
    # plans that do not fit their item
    refused(Status.INVALID_ARGUMENT, [item((81, 60))], [p])
    for kw in (dict(fx=0), dict(fy=0), dict(red_w=21), dict(red_h=19), dict(out_w=0), dict(out_h=0), dict(box_w=0.0), dict(box_h=-1.0),
               dict(box_w=float("inf")), dict(box_h=float("nan")), dict(identity=1), dict(dec_w=79)):
        refused(Status.INVALID_ARGUMENT, [it], [copy_of(p, **kw)])
    it1, p1 = planned(80, 60, (500, 500))  # the decode is the thumbnail
    assert p1.identity == 1 and size_and_call(L, [it1], [p1], dst=None)[0] > 0
    refused(Status.INVALID_ARGUMENT, [it1], [copy_of(p1, out_w=79)])
    # tall at the resize: Pillow's other order
    tall = item((40, 4001))
    pt = copy_of(p, dec_w=40, dec_h=4001, fx=1, fy=1, red_w=40, red_h=4001, box_w=40.0, box_h=4001.0, out_w=1, out_h=96)
    refused(Status.NOT_SUPPORTED, [tall], [pt])
    assert size_and_call(L, [item((40, 4000))], [copy_of(pt, dec_h=4000, red_h=4000, box_h=4000.0)], dst=None)[0] > 0
    # a box whose sum would not fit 32 bits
    big = item((8192, 8192), ((1, 1),))
    refused(Status.NOT_SUPPORTED, [big], [copy_of(p, dec_w=8192, dec_h=8192, fx=4096, fy=4096, red_w=2, red_h=2, box_w=2.0, box_h=2.0, out_w=1, out_h=1)])
    # the first item that fails decides
    refused(Status.NOT_SUPPORTED, [it, four], [p, p], colors=[YCBCR, CMYK])


def test_scratch_size_is_monotone_in_n(L):
    mix = [planned(640, 480, (10, 10)), planned(333, 251, (64, 64)), planned(80, 60, (500, 500)), planned(500, 375, (96, 96), None),
           planned(641, 479, (48, 20), 3.0, ((1, 1),)), planned(200, 152, (20, 20), 2.0, ((2, 1), (1, 1), (1, 1)))]
    its, plans = [m[0] for m in mix] * 3, [m[1] for m in mix] * 3
    a, cs, ps = arrays(its, plans)
    last = 0
    for n in range(1, len(its) + 1):
        need = L.jpeggpu_ext_thumbnail_scratch_size(a, cs, ps, n, 96, 96, BICUBIC)
        assert need > last, n
        last = need
    # an item without a reduction needs what the view call needs for it, and the room to align the pointer again
    it, p = planned(500, 375, (96, 96), None)
    a, cs, ps = arrays([it], [p])
    from jpeggpu_amd.api import ResizeView

    view = (ResizeView * 1)(ResizeView(p.out_w, p.out_h, 0, 0, 0))
    assert L.jpeggpu_ext_thumbnail_scratch_size(a, cs, ps, 1, 96, 96, BICUBIC) == L.jpeggpu_ext_resize_view_scratch_size(a, cs, None, view, 1, 96, 96, BICUBIC) + 256
