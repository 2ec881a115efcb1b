"""DCT-domain access on the device (jpeggpu_amd.read_coefficients / write_coefficients; read_blocks and gather_blocks<true> of
jg_encode.hip behind a batched decode that stops in front of the IDCT). Every comparison is exact.

Reading: every source of tests/coefficients_ref.sources() -- one block in one tile; 8 x 8, 9 x 9 and 17 x 9 in five
samplings (dummy blocks to the right, below and both; chroma grids of one block); 825 luma blocks (4 tiles, the last ragged);
a component's own scans and the progressive file of the same coefficients; restart intervals of 1, 2 and 3 MCUs, with the
device scan and without; escapes at every position, AC of +-1023, a unit of 63 coefficients; CMYK, two components, 16-bit
tables -- and Pillow's pins, each alone and all in ONE call, as int16, float32 and float16, against the reference's arrays.
Writing: the round trip against the reference's bytes, Pillow's own files and transcode_jpeg(frame="source"); after two
changes made on the device; from scratch; an uncodable item between two good ones. Behind every tensor and every output slot
lie guard bytes. Every source is at most 264 x 200 pixels."""
import ctypes as C
import io

import numpy as np
import pytest

import jpeggpu_amd
from jpeggpu_amd import ColorSpace, JpegGpuError, Status, api
from tests import coefficients_ref as K

pytestmark = pytest.mark.gpu

GUARD, G = 0xA5, 64
DEV = "cuda:0"
UNCODABLE = 4  # JPEGGPU_EXT_ENCODE_UNCODABLE
KINDS = {"plain": dict(), "optimize": dict(optimize=True), "progressive": dict(progressive=True), "restart": dict(restart_interval=2),
         "optimize_restart": dict(optimize=True, restart_interval=5)}


@pytest.fixture(scope="module")
def torch(gpu_lib):
    import torch

    assert torch.cuda.is_available()
    assert hasattr(jpeggpu_amd.lib(), "jpeggpu_ext_read_coefficients_batch"), "the library lacks jpeggpu_ext_read_coefficients_batch"
    return torch


@pytest.fixture(scope="module")
def everything():
    """name -> (file, the reference's read of it), computed once and not changed: the sources and Pillow's plain pins."""
    out = {k: v for k, v in K.sources().items()}
    out.update({"pin_" + k: f["A"] for k, f in K.pins()[0].items()})
    return {k: (v, K.read(v)) for k, v in out.items()}


def read_guarded(torch, datas, dtype=None, dequantize=False, **decode):
    """One batched decode and ONE jpeggpu_ext_read_coefficients_batch call into tensors that lie between guard bytes.
    Returns per file the host arrays [blocks_y, blocks_x, 64]; asserts that nothing outside them was written."""
    dtype = dtype or torch.int16
    esize = torch.empty(0, dtype=dtype).element_size()
    with jpeggpu_amd.BatchDecode(datas, DEV, **decode) as bd:
        bd.decode()
        infos = [d.coefficient_info() for d in bd.decoders]
        spans, total = [], G
        for ci in infos:
            for c in range(ci.num_components):
                total = (total + 15) // 16 * 16
                spans.append((total, ci.blocks_y[c] * ci.blocks_x[c] * 64 * esize))
                total += spans[-1][1] + G
        buf = torch.full((total + 16,), GUARD, dtype=torch.uint8, device=DEV)
        shift = -buf.data_ptr() % 16
        items, k = (api.CoefficientReadItem * len(datas))(), 0
        for i, (ci, (dec, _, _, base, _)) in enumerate(zip(infos, bd._entries)):
            items[i].decoder, items[i].d_tmp = dec._h, base
            for c in range(ci.num_components):
                items[i].dst[c] = buf.data_ptr() + shift + spans[k][0]
                k += 1
        spec = api.CoefficientSpec(api.COEFFICIENT_TYPE_NAMES[str(dtype).split(".")[1]], int(dequantize))
        need = jpeggpu_amd.lib().jpeggpu_ext_read_coefficients_scratch_size(len(datas))
        scratch = torch.empty(need, dtype=torch.uint8, device=DEV)
        st = jpeggpu_amd.lib().jpeggpu_ext_read_coefficients_batch(items, len(datas), C.byref(spec), scratch.data_ptr(), need,
                                                                   torch.cuda.current_stream().cuda_stream)
        assert st == 0, st
        host = buf.cpu().numpy()
    untouched = np.ones(host.size, bool)
    out, k = [], 0
    for ci in infos:
        comps = []
        for c in range(ci.num_components):
            at, size = spans[k]
            untouched[shift + at:shift + at + size] = False
            comps.append(host[shift + at:shift + at + size].view(str(dtype).split(".")[1]).reshape(ci.blocks_y[c], ci.blocks_x[c], 64))
            k += 1
        out.append(comps)
    assert (host[untouched] == GUARD).all(), "bytes outside the tensors were written"
    return out


def same(got, ref):
    return len(got) == len(ref.coef) and all(g.shape == r.shape and np.array_equal(g, r) for g, r in zip(got, ref.coef))


def dequantised(ref, half=False):
    """coef.astype(float32) * q in float32; for float16 that cast once with numpy."""
    out = [c.astype(np.float32) * q.astype(np.float32)[None, None, :] for c, q in zip(ref.coef, ref.qtables)]
    assert all(o.dtype == np.float32 for o in out)
    with np.errstate(over="ignore"):
        return [o.astype(np.float16) for o in out] if half else out


def bits_equal(got, want):
    return all(g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g.view(np.uint8), w.view(np.uint8)) for g, w in zip(got, want))


# ------------------------------------------------------------------------------------------------
# reading
# ------------------------------------------------------------------------------------------------

def test_read_each_source_alone(torch, everything):
    """Each file in a call of its own: 1 x 1 grey runs one tile with a single busy lane, 264 x 200 four luma tiles."""
    bad = [name for name, (data, ref) in everything.items() if not name.startswith("pin_") and not same(read_guarded(torch, [data], coefficients_only=True)[0], ref)]
    assert bad == []
    luma = everything["264x200_420"][1].coef[0]
    assert luma.shape[0] * luma.shape[1] == 825 and 825 % K.READ_TILE == 57  # more than one tile, and the last one ragged
    crafted = everything["crafted"][1].coef[0]
    assert crafted.max() == 1023 and crafted.min() == -1023 and (crafted.reshape(-1, 64)[:, 1:] != 0).sum(1).max() == 63


@pytest.mark.parametrize("coefficients_only", [True, False])
def test_read_everything_in_one_call(torch, everything, coefficients_only):
    """Items of every size, component count and coding share the launch; the decode may have run its IDCT stage or not."""
    names = sorted(everything)
    got = read_guarded(torch, [everything[n][0] for n in names], coefficients_only=coefficients_only)
    assert [n for n, g in zip(names, got) if not same(g, everything[n][1])] == []


def test_read_pins_by_their_hashes(torch):
    """Pillow's three files of a case hold the same coefficients: every one reads as the pinned tensors."""
    files = K.pins()[0]
    names = sorted(files)
    for kind in "ABC":
        got = read_guarded(torch, [files[n][kind] for n in names], coefficients_only=True)
        assert [n for n, g in zip(names, got) if [K.sha(c) for c in g] != files[n]["sha"]] == [], kind


def test_read_progressive_equals_baseline(torch, everything):
    a, b = read_guarded(torch, [everything["ni_420"][0], everything["prog_of_ni_420"][0]], coefficients_only=True)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and same(a, everything["ni_420"][1])


@pytest.mark.parametrize("device_scan", [False, True])
def test_read_restart_intervals(torch, everything, device_scan):
    """The DC stays absolute across the resets, whoever found the markers."""
    names = ["dri1_420", "dri3_422", "q16"]
    got = read_guarded(torch, [everything[n][0] for n in names], coefficients_only=True, device_scan=device_scan)
    assert [n for n, g in zip(names, got) if not same(g, everything[n][1])] == []
    assert [everything[n][1].restart for n in names] == [1, 3, 2]


@pytest.mark.parametrize("half", [False, True])
def test_read_dequantised(torch, everything, half):
    names = sorted(everything)
    dtype = torch.float16 if half else torch.float32
    got = read_guarded(torch, [everything[n][0] for n in names], dtype, True, coefficients_only=True)
    assert [n for n, g in zip(names, got) if not bits_equal(g, dequantised(everything[n][1], half))] == []
    # without `dequantize` the float types hold the values themselves
    got = read_guarded(torch, [everything[n][0] for n in names[:6]], dtype, False, coefficients_only=True)
    for n, g in zip(names, got):
        assert bits_equal(g, [c.astype(np.float16 if half else np.float32) for c in everything[n][1].coef]), n
    # what the comparison above covered: products that float32 rounds, and ones beyond the half range, which become
    # infinities as numpy's cast makes them
    exact = everything["crafted_q16"][1].coef[0].astype(np.int64) * everything["crafted_q16"][1].qtables[0].astype(np.int64)
    assert (dequantised(everything["crafted_q16"][1])[0].astype(np.int64) != exact).any()
    if half:
        assert np.isinf(dequantised(everything["crafted_q16"][1], True)[0]).any()


def test_read_coefficients_python(torch, everything):
    """The public call: one allocation for all tensors, each a 256-byte aligned view [by, bx, 8, 8]; tables, factors and
    colour models; dequantised int16 refused."""
    names = ["17x9_411", "cmyk", "q16", "prog_of_ni_420", "grey_1x1", "two_comp"]
    cs = jpeggpu_amd.read_coefficients([everything[n][0] for n in names], device=DEV)
    storages = {t.untyped_storage().data_ptr() for x in cs for t in x.coefficients}
    assert len(storages) == 1
    for n, x in zip(names, cs):
        ref = everything[n][1]
        assert (x.width, x.height, x.sampling, int(x.color_space), x.progressive) == (ref.w, ref.h, ref.sampling, ref.color, ref.progressive)
        for t, r, q, rq in zip(x.coefficients, ref.coef, x.qtables, ref.qtables):
            assert t.dtype == torch.int16 and t.is_contiguous() and t.data_ptr() % 256 == 0 and tuple(t.shape) == r.shape[:2] + (8, 8)
            assert np.array_equal(t.cpu().numpy().reshape(r.shape), r)
            assert q.dtype == np.uint16 and q.shape == (8, 8) and np.array_equal(q.reshape(64), rq)
    f32 = jpeggpu_amd.read_coefficients([everything["q16"][0]], device=DEV, dtype=torch.float32, dequantize=True)[0]
    assert bits_equal([t.cpu().numpy().reshape(t.shape[0], t.shape[1], 64) for t in f32.coefficients], dequantised(everything["q16"][1]))
    with pytest.raises(JpegGpuError) as e:
        jpeggpu_amd.read_coefficients([everything["q16"][0]], device=DEV, dequantize=True)
    assert e.value.status == Status.INVALID_ARGUMENT
    assert jpeggpu_amd.read_coefficients([]) == []


# ------------------------------------------------------------------------------------------------
# writing
# ------------------------------------------------------------------------------------------------

def as_item(torch, ref, coef=None):
    """A reference Coef as the object write_coefficients takes, its tensors on the device."""
    coef = ref.coef if coef is None else coef
    return jpeggpu_amd.Coefficients([torch.from_numpy(np.ascontiguousarray(c)).to(DEV).view(c.shape[0], c.shape[1], 8, 8) for c in coef],
                                    [q.reshape(8, 8) for q in ref.qtables], ref.w, ref.h, ref.sampling, ref.color)


def write_guarded(torch, cs, capacities=None, **options):
    """One jpeggpu_ext_write_coefficients_batch call into guarded slots: (files, sizes, status), files[i] None where status
    is not 0. Asserts that nothing outside the files was written."""
    capacities = [4096 + 4 * sum(t.numel() for t in x.coefficients) for x in cs] if capacities is None else capacities  # 32 bits a coefficient
    offsets, total = [], G
    for cap in capacities:
        offsets.append(total)
        total += cap + G
    buf = torch.full((total,), GUARD, dtype=torch.uint8, device=DEV)
    sizes, status = jpeggpu_amd.write_coefficients_into(cs, [buf[o:o + cap] for o, cap in zip(offsets, capacities)], **options)
    sizes, status = sizes.cpu().tolist(), status.cpu().tolist()
    host = buf.cpu().numpy()
    untouched = np.ones(total, bool)
    files = []
    for o, size, st in zip(offsets, sizes, status):
        if st == 0:
            untouched[o:o + size] = False
        files.append(host[o:o + size].tobytes() if st == 0 else None)
    assert (host[untouched] == GUARD).all(), "bytes outside the files were written"
    return files, sizes, status


@pytest.mark.parametrize("kind", list(KINDS))
def test_round_trip_against_the_reference(torch, everything, kind):
    """write_coefficients(read_coefficients(files)) in one call over every source and pin: the reference's bytes."""
    names = sorted(everything)
    cs = jpeggpu_amd.read_coefficients([everything[n][0] for n in names], device=DEV)
    files, _, status = write_guarded(torch, cs, **KINDS[kind])
    assert status == [0] * len(names)
    assert [n for n, f in zip(names, files) if f != K.write(everything[n][1], **KINDS[kind])] == []


def test_round_trip_of_pillows_files(torch):
    """For a source Pillow wrote the file is Pillow's own -- plain, optimised, progressive, from any of the three -- and the
    one transcode_jpeg(frame="source") makes."""
    pins = K.pins()[0]
    names = sorted(pins)
    for src in "AC":
        cs = jpeggpu_amd.read_coefficients([pins[n][src] for n in names], device=DEV)
        for kind, options in K.KINDS.items():
            files = jpeggpu_amd.write_coefficients(cs, **options)
            assert [n for n, f in zip(names, files) if f != pins[n][kind]] == [], (src, kind)
            if src == "A":
                assert files == jpeggpu_amd.transcode_jpeg([pins[n]["A"] for n in names], frame="source", restart_interval=0, **options), kind


CHANGES = {
    "lowpass": lambda t: t * ((torch_arange(t, 8).view(8, 1) + torch_arange(t, 8).view(1, 8)) <= 3),  # zero every coefficient with u + v > 3
    "mirror": lambda t: t * (1 - 2 * (torch_arange(t, 8) % 2)).view(1, 8),                              # negate the odd-u ones
}
CHANGES_REF = {
    "lowpass": lambda c: c * ((np.arange(8)[:, None] + np.arange(8)[None, :]) <= 3).reshape(64).astype(np.int16),
    "mirror": lambda c: c * np.tile(1 - 2 * (np.arange(8) % 2), 8).astype(np.int16),
}


def torch_arange(t, n):
    import torch

    return torch.arange(n, device=t.device, dtype=t.dtype)


@pytest.mark.parametrize("change", list(CHANGES))
def test_write_after_a_change_on_the_device(torch, everything, change):
    """A few tensor ops between the two calls: the file is the reference's for the changed arrays, and Pillow decodes it to
    what libjpeg's IDCT, upsampling and colour conversion make of them."""
    from PIL import Image

    names = ["pin_75x53_420_q75", "pin_75x53_422_q95", "pin_17x9_444_q30", "pin_75x53_grey_q75", "264x200_420", "17x9_440", "cmyk"]
    cs = jpeggpu_amd.read_coefficients([everything[n][0] for n in names], device=DEV)
    for x in cs:
        x.coefficients = [CHANGES[change](t).contiguous() for t in x.coefficients]
        assert all(t.dtype == torch.int16 for t in x.coefficients)
    for options in (dict(), dict(optimize=True, restart_interval=3), dict(progressive=True)):
        files, _, status = write_guarded(torch, cs, **options)
        assert status == [0] * len(names)
        for n, f in zip(names, files):
            ref = everything[n][1].copy()
            ref.coef = [CHANGES_REF[change](c) for c in ref.coef]
            assert f == K.write(ref, **options), (n, options)
            if n.startswith("pin_") or n == "264x200_420":
                assert np.array_equal(np.asarray(Image.open(io.BytesIO(f)).convert("RGB")), K.rgb(ref)), n


def test_write_from_scratch(torch):
    """A DC-only 4:2:0 image built with torch.full: Pillow decodes the flat colour libjpeg's arithmetic predicts."""
    from PIL import Image

    w, h, q = 40, 24, np.full((8, 8), 4, np.uint16)
    sampling = [(2, 2), (1, 1), (1, 1)]
    grids = jpeggpu_amd.coefficient_grid(w, h, sampling)
    assert grids == [(3, 5), (2, 3), (2, 3)]
    coefs = []
    for (by, bx), dc in zip(grids, (60, -45, 70)):
        t = torch.zeros((by, bx, 8, 8), dtype=torch.int16, device=DEV)
        t[:, :, 0, 0] = torch.full((by, bx), dc, dtype=torch.int16, device=DEV)
        coefs.append(t)
    item = jpeggpu_amd.Coefficients(coefs, [q, q, q], w, h, sampling, ColorSpace.YCBCR)
    ref = K.Coef([t.cpu().numpy().reshape(t.shape[0], t.shape[1], 64) for t in coefs], [q.reshape(64)] * 3, w, h, sampling, K.COLORS.index("ycbcr"))
    for options in (dict(), dict(optimize=True), dict(progressive=True), dict(restart_interval=1)):
        data = jpeggpu_amd.write_coefficients([item], **options)[0]
        assert data == K.write(ref, **options)
        rgb = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        assert rgb.shape == (h, w, 3) and np.array_equal(rgb, K.rgb(ref)) and (rgb == rgb[0, 0]).all()
    back = jpeggpu_amd.read_coefficients([data], device=DEV)[0]
    assert all(torch.equal(a, b) for a, b in zip(back.coefficients, coefs))


@pytest.mark.parametrize("what", ["ac", "dc"])
@pytest.mark.parametrize("kind", ["plain", "optimize", "progressive"])
def test_uncodable_item_between_two_good_ones(torch, everything, what, kind):
    """An AC of 1024, or a DC step of 2048 in the file's prediction order: that item alone is UNCODABLE with size 0 and an
    untouched slot (write_guarded's guard test covers it), and its neighbours' bytes are what they are without it."""
    refs = [everything[n][1] for n in ("pin_75x53_420_q75", "17x9_420", "pin_17x9_422_q95")]
    good = [as_item(torch, r) for r in refs]
    alone, _, status = write_guarded(torch, good, **KINDS[kind])
    assert status == [0, 0, 0]
    bad = refs[1].copy()
    if what == "ac":
        bad.coef[0][1, 2, 63] = 1024
    else:  # the second luma block of the first MCU against the first
        bad.coef[0][0, 0, 0], bad.coef[0][0, 1, 0] = -1024, 1024
    with pytest.raises(K.Unsupported):
        K.write(bad, **KINDS[kind])
    files, sizes, status = write_guarded(torch, [good[0], as_item(torch, bad), good[2]], **KINDS[kind])
    assert status == [0, UNCODABLE, 0] and sizes[1] == 0
    assert files[0] == alone[0] and files[2] == alone[2]
    with pytest.raises(JpegGpuError) as e:
        jpeggpu_amd.write_coefficients([as_item(torch, bad)], **KINDS[kind])
    assert e.value.status == Status.NOT_SUPPORTED
    # one less is codable
    edge = refs[1].copy()
    if what == "ac":
        edge.coef[0][1, 2, 63] = -1023
    else:
        edge.coef[0][0, 0, 0], edge.coef[0][0, 1, 0] = -1024, 1023
    assert jpeggpu_amd.write_coefficients([as_item(torch, edge)], **KINDS[kind])[0] == K.write(edge, **KINDS[kind])


def test_slots_that_are_too_small(torch, everything):
    """Status 1 and the size the slot needs, nothing written; the public call then tries again with that size."""
    refs = [everything[n][1] for n in ("pin_75x53_444_q95", "cmyk")]
    items = [as_item(torch, r) for r in refs]
    want = [K.write(r) for r in refs]
    files, sizes, status = write_guarded(torch, items, capacities=[len(want[0]) - 1, len(want[1])])
    assert status == [1, 0] and sizes == [len(want[0]), len(want[1])] and files[1] == want[1]
    buf, offsets, sizes = jpeggpu_amd.write_coefficients_to_device(items, capacities=[16, 16])
    assert [buf[o:o + s].cpu().numpy().tobytes() for o, s in zip(offsets, sizes)] == want


def test_python_refuses_what_does_not_fit(torch, everything):
    ref = everything["17x9_420"][1]
    ok = as_item(torch, ref)
    for spoil in (lambda x: setattr(x, "coefficients", [x.coefficients[0][:, :2]] + x.coefficients[1:]),           # a grid that does not fit the frame
                  lambda x: setattr(x, "coefficients", [x.coefficients[0].transpose(2, 3)] + x.coefficients[1:]),  # not contiguous
                  lambda x: setattr(x, "coefficients", [x.coefficients[0].to(torch.int32)] + x.coefficients[1:]),
                  lambda x: setattr(x, "qtables", [np.zeros((8, 8), np.uint16)] + x.qtables[1:]),
                  lambda x: setattr(x, "sampling", [(5, 1), (1, 1), (1, 1)])):
        x = as_item(torch, ref)
        spoil(x)
        with pytest.raises(JpegGpuError) as e:
            jpeggpu_amd.write_coefficients([x])
        assert e.value.status == Status.INVALID_ARGUMENT
    misaligned = torch.zeros(ref.coef[0].size + 4, dtype=torch.int16, device=DEV)[4:].view(ok.coefficients[0].shape)
    assert misaligned.data_ptr() % 16 == 8
    x = as_item(torch, ref)
    x.coefficients[0] = misaligned
    with pytest.raises(JpegGpuError) as e:
        jpeggpu_amd.write_coefficients([x])
    assert e.value.status == Status.INVALID_ARGUMENT
    assert jpeggpu_amd.write_coefficients([ok])[0] == K.write(ref)
