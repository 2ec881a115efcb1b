"""Batched conversion to RGB on the GPU (jpeggpu_ext_batch_to_rgb, batch_to_rgb, decode_batch_to_rgb): every item of a call
equals the per-image call (jpeggpu_ext_planes_to_rgbi_oriented / jpeggpu_ext_crop_to_rgbi_oriented) and Pillow's pinned
ImageOps.exif_transpose output (tests/golden/exif_pins.npz), in both layouts. Every output lies in ONE guarded buffer per
call: guard bytes before and after it, between the items, between rows and, for CHW, between planes, all intact after the
call. The files are tests/exif_ref.gpu_files(): they cross both tile shapes (256 x 8 and 64 x 64) both ways."""
import hashlib
import os

import numpy as np
import pytest

from tests import exif_ref
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

GUARD = 0xA5
PAD = 64


@pytest.fixture(scope="module")
def torch_cuda(gpu_lib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def files():
    return exif_ref.gpu_files()


@pytest.fixture(scope="module")
def pins():
    return np.load(os.path.join(GOLDEN, "exif_pins.npz"))


@pytest.fixture(scope="module")
def decoded(torch_cuda, files):
    """(name, d, stored crop or None) -> (planes, info, crop_info or None, color, replicate): decoded once, shared."""
    import jpeggpu_amd
    from jpeggpu_amd.api import _needs_replication

    cache = {}

    def get(name, d=1, crop=None):
        key = (name, d, crop)
        if key not in cache:
            kw = dict(idct="islow", scale=d, scale_mode="libjpeg", progressive=True, return_color=True)
            if crop is None:
                planes, info, color = jpeggpu_amd.decode_to_planes(files[name][0], **kw)
                ci = None
            else:
                planes, info, ci, color = jpeggpu_amd.decode_to_planes(files[name][0], crop=crop, **kw)
            cache[key] = (planes, info, ci, color, _needs_replication(info, d))
        return cache[key]

    return get


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def size_of(entry):
    from jpeggpu_amd.api import _frame_size

    planes, info, ci = entry[:3]
    return (ci.width, ci.height) if ci is not None else _frame_size(info)


def shown_size(entry, o):
    w, h = size_of(entry)
    return (h, w) if o >= 5 else (w, h)


def per_image(torch, entry, o):
    """The per-image call of the parent library: the displayed image as (oh, ow, 3) numpy."""
    import jpeggpu_amd

    planes, info, ci, color, rep = entry
    fn = jpeggpu_amd.planes_to_rgb if ci is None else jpeggpu_amd.crop_to_rgb
    args = (planes, info) if ci is None else (planes, info, ci)
    out = fn(*args, replicate=rep, color=color, orientation=o)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def enqueue(torch, entries, orients, layout="HWC", pitch=None, plane=None, stream=None, expect=0, colors=None, scratch_short=0):
    """One jpeggpu_ext_batch_to_rgb call of `entries` into a guarded buffer, not waited for. `pitch(i, ow)`: item i's
    dst_pitch; `plane(i, pitch, oh)`: its plane stride (CHW). Returns what collect() needs."""
    import jpeggpu_amd
    from jpeggpu_amd.api import IMAGE_LAYOUTS, RgbItem, _resize_items

    L = jpeggpu_amd.lib()
    n = len(entries)
    pitch = pitch or ((lambda i, ow: 3 * ow) if layout == "HWC" else (lambda i, ow: ow))
    plane = plane or (lambda i, p, oh: p * oh)
    items, keep = _resize_items([e[0] for e in entries], [e[1] for e in entries], [e[2] for e in entries])
    metas, off = [], PAD
    for i, (e, o) in enumerate(zip(entries, orients)):
        ow, oh = shown_size(e, o if 1 <= o <= 8 else 1)
        p = pitch(i, ow)
        ps = plane(i, p, oh) if layout == "CHW" else 0
        size = max(oh * p if layout == "HWC" else 2 * ps + oh * p, 1)
        metas.append((off, ow, oh, p, ps, size))
        off += size + PAD
    buf = torch.full((off,), GUARD, dtype=torch.uint8, device="cuda:0")
    rgb = (RgbItem * n)()
    for i, (e, o) in enumerate(zip(entries, orients)):
        rgb[i].info, rgb[i].crop, rgb[i].src = items[i].info, items[i].crop, items[i].src
        rgb[i].color = int(e[3]) if colors is None else colors[i]
        rgb[i].orientation, rgb[i].replicate = o, int(e[4])
        rgb[i].dst = buf.data_ptr() + metas[i][0]
        rgb[i].dst_pitch, rgb[i].plane_stride = metas[i][3], metas[i][4]
    need = L.jpeggpu_ext_batch_rgb_scratch_size(n)
    assert need > 0
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda:0")
    if stream is None:
        torch.cuda.synchronize()
    else:  # the guard fill ran on the current stream: ordered in front of the call on the device, no host wait
        stream.wait_stream(torch.cuda.current_stream())
    st = L.jpeggpu_ext_batch_to_rgb(rgb, n, IMAGE_LAYOUTS[layout], scratch.data_ptr(), need - scratch_short, stream.cuda_stream if stream is not None else None)
    assert st == expect, jpeggpu_amd.status_string(st)
    return buf, metas, layout, expect, (scratch, keep, rgb)


def collect(torch, call):
    """The items of an enqueued call as (oh, ow, 3) numpy, after checking every guard byte of its buffer."""
    buf, metas, layout, expect, _keep = call
    torch.cuda.synchronize()
    a = buf.cpu().numpy()
    if expect != 0:
        assert (a == GUARD).all(), "a refused call wrote something"
        return None
    guard = np.ones(a.shape, bool)
    out = []
    for off, ow, oh, p, ps, size in metas:
        if layout == "HWC":
            guard[off:off + oh * p].reshape(oh, p)[:, :3 * ow] = False
            out.append(a[off:off + oh * p].reshape(oh, p)[:, :3 * ow].reshape(oh, ow, 3).copy())
        else:
            chans = []
            for c in range(3):
                guard[off + c * ps:off + c * ps + oh * p].reshape(oh, p)[:, :ow] = False
                chans.append(a[off + c * ps:off + c * ps + oh * p].reshape(oh, p)[:, :ow])
            out.append(np.stack(chans, axis=2))
    assert (a[guard] == GUARD).all(), "a guard byte around an output, between two rows or between two planes was written"
    return out


def run(torch, entries, orients, **kw):
    return collect(torch, enqueue(torch, entries, orients, **kw))


def assert_pin(pins, got, name, o, d):
    key = "%s/%d/%d" % (name, o, d)
    if "rgb/" + key in pins.files:
        assert np.array_equal(got, pins["rgb/" + key]), key
    else:
        assert sha(got) == str(pins["rgb_sha256/" + key]), key


def pinned(pins, name, o, d):
    return any(k in pins.files for k in ("rgb/%s/%d/%d" % (name, o, d), "rgb_sha256/%s/%d/%d" % (name, o, d)))


@pytest.fixture(scope="module")
def everything(torch_cuda, files, decoded):
    """All 14 files x 8 orientations as the items of one call: (names, orientations, entries), and the per-image results."""
    names = [name for name in files for _ in range(8)]
    orients = [o for _ in files for o in range(1, 9)]
    entries = [decoded(name) for name in names]
    assert len(entries) == 112
    want = [per_image(torch_cuda, e, o) for e, o in zip(entries, orients)]
    return names, orients, entries, want


def test_every_file_and_value_in_one_call(torch_cuda, pins, everything):
    """112 items, most rows not dword-aligned. The call holds grey, YCbCr and YCCK items: the all-models instantiations;
    the same call without the YCCK file takes the others and must give the same bytes."""
    names, orients, entries, want = everything
    got = run(torch_cuda, entries, orients, pitch=lambda i, ow: 3 * ow + (i % 3))
    assert {int(e[3]) for e in entries} == {1, 2, 5}
    n = 0
    for i, (name, o) in enumerate(zip(names, orients)):
        assert got[i].shape == want[i].shape and np.array_equal(got[i], want[i]), (name, o, "the per-image call")
        if pinned(pins, name, o, 1):
            assert_pin(pins, got[i], name, o, 1)
            n += 1
    assert n >= 8 * 14
    few = [i for i, e in enumerate(entries) if int(e[3]) in (1, 2)]
    assert len(few) == 8 * 13 and {int(entries[i][3]) for i in few} == {1, 2}
    again = run(torch_cuda, [entries[i] for i in few], [orients[i] for i in few], pitch=lambda i, ow: 3 * ow + (i % 3))
    for k, i in enumerate(few):
        assert np.array_equal(again[k], got[i]), (names[i], orients[i], "grey and YCbCr alone")


def test_chw(torch_cuda, everything):
    names, orients, entries, want = everything
    kw = dict(layout="CHW", pitch=lambda i, ow: ow + 5, plane=lambda i, p, oh: p * oh + 11)
    got = run(torch_cuda, entries, orients, **kw)
    for i, (name, o) in enumerate(zip(names, orients)):
        assert np.array_equal(got[i], want[i]), (name, o)
    few = [i for i, e in enumerate(entries) if int(e[3]) in (1, 2)]
    again = run(torch_cuda, [entries[i] for i in few], [orients[i] for i in few], **kw)
    for k, i in enumerate(few):
        assert np.array_equal(again[k], want[i]), (names[i], orients[i], "grey and YCbCr alone")
    tight = run(torch_cuda, entries, orients, layout="CHW")  # unpadded rows and planes: many start on a dword
    for i, (name, o) in enumerate(zip(names, orients)):
        assert np.array_equal(tight[i], want[i]), (name, o, "tight")


def displayed_rects(ow, oh):
    """Each corner, odd origins, 1 x 1, a full row and a full column of the displayed image (as tests/test_gpu_exif.py)."""
    out = [(0, 0, min(5, ow), min(3, oh)), (max(ow - 7, 0), 0, min(7, ow), min(4, oh)), (0, max(oh - 5, 0), min(6, ow), min(5, oh)),
           (max(ow - 9, 0), max(oh - 3, 0), min(9, ow), min(3, oh)), (ow // 2 | 1 if ow > 2 else 0, oh // 2 | 1 if oh > 2 else 0, 1, 1),
           (0, oh // 3, ow, 1), (ow // 3, 0, 1, oh)]
    if ow > 12 and oh > 12:
        out.append((3, 5, ow - 8, oh - 11))
    return out


@pytest.mark.parametrize("name", ("s420", "s422", "s440", "ycck", "wide", "tall", "t65x63", "prog"))
def test_crops(torch_cuda, decoded, name):
    """Rectangles given in displayed coordinates, decoded cropped, all eight orientations in ONE call per file: each
    result is that part of the displayed whole image."""
    import jpeggpu_amd

    full = decoded(name)
    w, h = size_of(full)
    entries, orients, want = [], [], []
    for o in range(1, 9):
        shown = per_image(torch_cuda, full, o)
        ow, oh = jpeggpu_amd.orient_size(o, w, h)
        for rect in displayed_rects(ow, oh):
            stored = jpeggpu_amd.orient_rect(o, w, h, rect)
            entry = decoded(name, 1, stored)
            assert size_of(entry) == stored[2:]
            x, y, rw, rh = rect
            entries.append(entry)
            orients.append(o)
            want.append((shown[y:y + rh, x:x + rw], o, rect))
    for layout in ("HWC", "CHW"):
        got = run(torch_cuda, entries, orients, layout=layout, pitch=lambda i, ow: (3 * ow if layout == "HWC" else ow) + (i % 3))
        for g, (wnt, o, rect) in zip(got, want):
            assert np.array_equal(g, wnt), (name, o, rect, layout)


def test_scales_and_replication(torch_cuda, pins, decoded):
    cases = [("s420", 2), ("s422", 8), ("s420", 8)]
    assert [bool(decoded(name, d)[4]) for name, d in cases] == [False, True, False]  # libjpeg replicates 4:2:2 at 1/8 only
    entries, orients, keys = [], [], []
    for name, d in cases:
        for o in (1, 3, 6, 8):
            entries.append(decoded(name, d))
            orients.append(o)
            keys.append((name, o, d))
    for layout in ("HWC", "CHW"):
        got = run(torch_cuda, entries, orients, layout=layout)
        for g, (name, o, d) in zip(got, keys):
            assert pinned(pins, name, o, d), (name, o, d)
            assert_pin(pins, g, name, o, d)


@pytest.mark.parametrize("layout", ("HWC", "CHW"))
def test_item_boundaries(torch_cuda, decoded, layout):
    for name, o in (("s420", 1), ("odd", 4), ("t63x65", 7)):  # n = 1
        e = decoded(name)
        assert np.array_equal(run(torch_cuda, [e], [o], layout=layout)[0], per_image(torch_cuda, e, o)), (name, o)
    # tile counts that differ, alternating between the two tile lists: 5 row tiles, 5 transposed, 1 row, 5 transposed
    names, orients = ("col", "wide", "row", "tall"), (1, 6, 2, 5)
    entries = [decoded(n) for n in names]
    want = [per_image(torch_cuda, e, o) for e, o in zip(entries, orients)]
    got = run(torch_cuda, entries, orients, layout=layout)
    back = run(torch_cuda, entries[::-1], orients[::-1], layout=layout)[::-1]
    for i in range(4):
        assert np.array_equal(got[i], want[i]), (names[i], orients[i])
        assert np.array_equal(back[i], want[i]), (names[i], orients[i], "reversed")
    # items of one list only, in front of and behind each other
    for os_ in ((5, 8, 6, 7), (4, 1, 3, 2)):
        got = run(torch_cuda, entries, os_, layout=layout)
        for e, o, g in zip(entries, os_, got):
            assert np.array_equal(g, per_image(torch_cuda, e, o)), (os_, o)


def test_refused_calls_write_nothing(torch_cuda, decoded):
    entries = [decoded("s420"), decoded("wide"), decoded("gray")]
    assert run(torch_cuda, entries, [1, 6, 9], expect=1) is None
    assert run(torch_cuda, entries, [1, 6, 0], expect=1) is None
    assert run(torch_cuda, entries, [1, 6, 2], pitch=lambda i, ow: 3 * ow - (i == 2), expect=1) is None
    assert run(torch_cuda, entries, [1, 6, 5], pitch=lambda i, ow: 3 * ow - (i == 2), expect=1) is None
    assert run(torch_cuda, entries, [1, 6, 2], layout="CHW", plane=lambda i, p, oh: p * oh - (i == 2), expect=1) is None
    assert run(torch_cuda, entries, [1, 6, 2], colors=[2, 2, 4], expect=4) is None  # CMYK of one component: NOT_SUPPORTED
    assert run(torch_cuda, entries, [1, 6, 2], scratch_short=1, expect=1) is None


def test_another_stream_and_the_staging_ring(torch_cuda, decoded):
    """Six calls in a row on a stream of their own, nothing waited for in between: more than the staging ring of four."""
    s = torch_cuda.cuda.Stream()
    sets = []
    for k in range(6):
        names = ("s420", "wide", "ycck", "tall", "gray", "t65x63", "prog", "row")[k % 3:][:5 + k % 2]
        orients = [(k + 3 * i) % 8 + 1 for i in range(len(names))]
        sets.append(([decoded(n) for n in names], orients, "CHW" if k % 2 else "HWC"))
    want = [[per_image(torch_cuda, e, o) for e, o in zip(entries, orients)] for entries, orients, _ in sets]
    torch_cuda.cuda.synchronize()
    calls = [enqueue(torch_cuda, entries, orients, layout=layout, stream=s) for entries, orients, layout in sets]
    for call, w in zip(calls, want):
        got = collect(torch_cuda, call)
        for g, x in zip(got, w):
            assert np.array_equal(g, x)


# ------------------------------------------------------------------------------------------------
# Python: batch_to_rgb, decode_batch_to_rgb
# ------------------------------------------------------------------------------------------------

def test_decode_batch_to_rgb_with_displayed_crops(torch_cuda, files):
    import jpeggpu_amd

    cases = exif_ref.batch_cases()
    datas = [exif_ref.with_orientation(files[name][0], o) for name, o, _ in cases]
    crops = [box for _, _, box in cases]
    want = [jpeggpu_amd.decode_to_rgb(d, crop=c, exif_transpose=True) for d, c in zip(datas, crops)]
    got = jpeggpu_amd.decode_batch_to_rgb(datas, crops=crops, exif_transpose=True)
    chw = jpeggpu_amd.decode_batch_to_rgb(datas, crops=crops, exif_transpose=True, layout="CHW")
    assert len(got) == len(chw) == 8
    for g, c, w, (name, o, box) in zip(got, chw, want, cases):
        assert g.dtype == torch_cuda.uint8 and tuple(g.shape) == (box[3], box[2], 3) and tuple(c.shape) == (3, box[3], box[2])
        assert torch_cuda.equal(g, w), (name, o, box)
        assert torch_cuda.equal(c, w.permute(2, 0, 1)), (name, o, box, "CHW")
    # without the flag the tag is ignored and the crops are stored rectangles, as decode_to_rgb has it
    stored = [(1, 0, 9, 1)] * 8
    plain = jpeggpu_amd.decode_batch_to_rgb(datas, crops=stored)
    for g, d in zip(plain, datas):
        assert torch_cuda.equal(g, jpeggpu_amd.decode_to_rgb(d, crop=stored[0]))


def test_decode_batch_to_rgb_equals_the_pins(torch_cuda, files, pins):
    import jpeggpu_amd

    cases = exif_ref.batch_cases()
    datas = [exif_ref.with_orientation(files[name][0], o) for name, o, _ in cases]
    got = jpeggpu_amd.decode_batch_to_rgb(datas, exif_transpose=True)
    for g, (name, o, _) in zip(got, cases):
        assert_pin(pins, g.cpu().numpy(), name, o, 1)
    # one allocation: every result is a view of it, starts on a multiple of 256 bytes and has unpadded rows
    assert len({g.untyped_storage().data_ptr() for g in got}) == 1
    assert all(g.data_ptr() % 256 == 0 and g.is_contiguous() for g in got)
    chw = jpeggpu_amd.decode_batch_to_rgb(datas, exif_transpose=True, layout="CHW")
    assert len({g.untyped_storage().data_ptr() for g in chw}) == 1
    assert all(g.data_ptr() % 256 == 0 and g.is_contiguous() for g in chw)


def test_decode_batch_to_rgb_takes_what_libjpeg_replicates(torch_cuda, files, pins):
    import jpeggpu_amd

    datas = [files["s422"][0], files["s420"][0], exif_ref.with_orientation(files["s422"][0], 6), files["s440"][0]]
    scales = [8, 8, 8, 2]
    got = jpeggpu_amd.decode_batch_to_rgb(datas, scales=scales, exif_transpose=True)
    for g, d, s in zip(got, datas, scales):
        assert torch_cuda.equal(g, jpeggpu_amd.decode_to_rgb(d, scale=s, exif_transpose=True)), s
    assert_pin(pins, got[0].cpu().numpy(), "s422", 1, 8)
    assert_pin(pins, got[2].cpu().numpy(), "s422", 6, 8)
    with pytest.raises(ValueError):  # the batched resize still refuses it
        jpeggpu_amd.decode_resized(datas[:1], 8, scales=[8])


def test_decode_batch_to_rgb_arguments(torch_cuda, files):
    import jpeggpu_amd

    assert jpeggpu_amd.decode_batch_to_rgb([]) == []
    assert jpeggpu_amd.batch_to_rgb([], []) == []
    data = files["s420"][0]
    with pytest.raises(ValueError):
        jpeggpu_amd.decode_batch_to_rgb([data], crops=[None, None])
    with pytest.raises(ValueError):
        jpeggpu_amd.decode_batch_to_rgb([data], scales=[3])
    with pytest.raises(ValueError):
        jpeggpu_amd.decode_batch_to_rgb([data, data], scales=[1])
    with pytest.raises(ValueError):
        jpeggpu_amd.decode_batch_to_rgb([data], layout="NHWC")
