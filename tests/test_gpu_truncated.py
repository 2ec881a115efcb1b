"""Truncated files on the GPU (jpeggpu_ext_set_truncated, the `truncated=True` of the Python wrappers): every result equals the
CPU restatement of libjpeg's rule (tests/truncated_ref.py, which tests/test_truncated_ref.py holds against Pillow with
ImageFile.LOAD_TRUNCATED_IMAGES at every cut) and, at the pinned cuts, the digests of Pillow's own RGB
(tests/golden/truncated_pins.npz). The cuts are decoded in batches, never one call each, except where the lone decode is
what is tested. Every test here fails without the feature: parse_header refuses a file that ends early."""
import numpy as np
import pytest

import jpeggpu_amd
from jpeggpu_amd import JpegGpuError, Status
from tests import center_crop_ref, color_ref, exif_ref, gray_ref, pillow_resample_ref, thumbnail_ref
from tests import truncated_ref as T

pytestmark = pytest.mark.gpu

FILES = T.pinned_files()
NAMES = sorted(FILES)
BATCH = 128


@pytest.fixture(scope="module")
def torch_cuda(gpu_lib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def ref():
    """(file bytes, cut) -> the restated RGB, computed once and shared (read-only)."""
    cache = {}

    def get(data, cut):
        key = (T.sha(np.frombuffer(data, np.uint8)), cut)
        if key not in cache:
            a = T.rgb(data[:cut])
            a.setflags(write=False)
            cache[key] = a
        return cache[key]

    return get


def batch_rgb(datas, **kw):
    out = []
    for k in range(0, len(datas), BATCH):
        out += [t.cpu().numpy() for t in jpeggpu_amd.decode_batch_to_rgb(datas[k:k + BATCH], truncated=True, **kw)]
    return out


def assert_cuts(data, cuts, ref, **kw):
    got = batch_rgb([data[:c] for c in cuts], **kw)
    for c, g in zip(cuts, got):
        want = ref(data, c)
        assert g.shape == want.shape and np.array_equal(g, want), (c, len(data), T.decode(data[:c]).cut_mcu, kw)


# ------------------------------------------------------------------------------------------------
# small files: every cut
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_every_cut_of_a_small_file(torch_cuda, ref, name):
    data, pin_cuts, pin_shas = T.pinned()[name]
    assert len(data) - T.scan_begin(data) <= 2048
    cuts = list(T.cuts(data))
    got = batch_rgb([data[:c] for c in cuts])
    pinned = dict(zip(pin_cuts, pin_shas))
    for c, g in zip(cuts, got):
        assert np.array_equal(g, ref(data, c)), (name, c, T.decode(data[:c]).cut_mcu)
        if c in pinned:
            assert T.sha(g) == pinned[c], (name, c, "Pillow's digest")
    assert len(pinned) >= 10


@pytest.mark.parametrize("name", ["s420_rst1", "s444_opt", "gray_rst5"])
def test_lone_decode_of_a_small_file(torch_cuda, ref, name):
    """The lone decode (jpeggpu_decoder_decode, multi-hypothesis speculation where the plan has it): every seventh cut."""
    data = FILES[name]
    for c in list(T.cuts(data))[::7]:
        g = jpeggpu_amd.decode_to_rgb(data[:c], truncated=True).cpu().numpy()
        assert np.array_equal(g, ref(data, c)), (name, c)


# ------------------------------------------------------------------------------------------------
# around subsequence and sequence boundaries
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("subseq_bytes", [32, 64, 128, 256])
@pytest.mark.parametrize("which", ["plain", "rstrow"])
def test_cuts_around_subsequence_boundaries(torch_cuda, ref, which, subseq_bytes):
    """512 x 384: the cuts whose last destuffed byte ends a subsequence or starts one, the two offsets to either side, a cut
    in the first subsequence of a segment and one in its last -- where a cut finder can go wrong."""
    data = T.large_files()[which]
    cuts = T.boundary_cuts(data, subseq_bytes, segments=(0,) if which == "plain" else (0, 3, 11))
    assert len(cuts) >= 12
    assert_cuts(data, cuts, ref, subseq_bytes=subseq_bytes)
    for c in cuts[2:5]:  # ... and through the lone decode
        planes, info, color = jpeggpu_amd.decode_to_planes(data[:c], subseq_bytes=subseq_bytes, idct="islow", return_color=True, truncated=True)
        g = jpeggpu_amd.planes_to_rgb(planes, info, fancy=True, color=color).cpu().numpy()
        assert np.array_equal(g, ref(data, c)), (which, subseq_bytes, c)


@pytest.mark.parametrize("which", ["plain", "rstrow"])
def test_full_batch_plan(torch_cuda, ref, monkeypatch, which):
    """The plan and the kernels of a batch that fills the chip -- one flow iteration, the fused tail and write pass --, which
    a call this small gets when it is told so (jpeggpu_ext_set_batch_hint; the batch's threshold from the environment)."""
    monkeypatch.setenv("JPEGGPU_EXP_KEEP_FLOWS_BELOW", "0")
    data = T.large_files()[which]
    b = T.scan_begin(data)
    cuts = [b + (len(data) - b) // 3, b + 2 * (len(data) - b) // 3 + 1, len(data)]
    assert_cuts(data, cuts, ref, hint=64)


def test_cut_at_a_sequence_boundary(torch_cuda, ref, monkeypatch):
    """The smallest file with two sequences at 32-byte subsequences: cuts whose MCU lies across the boundary between them, for
    the lone decode's sequences of 240 subsequences and the full batch's of 255."""
    data = T.large_files()["twoseq"]
    lone = T.boundary_cuts(data, 32, rows=(240,))
    assert len(lone) >= 6
    assert_cuts(data, lone, ref, subseq_bytes=32)
    for c in lone[1::2]:
        planes, info, color = jpeggpu_amd.decode_to_planes(data[:c], subseq_bytes=32, idct="islow", return_color=True, truncated=True)
        assert np.array_equal(jpeggpu_amd.planes_to_rgb(planes, info, fancy=True, color=color).cpu().numpy(), ref(data, c)), c
    monkeypatch.setenv("JPEGGPU_EXP_KEEP_FLOWS_BELOW", "0")
    assert_cuts(data, T.boundary_cuts(data, 32, rows=(255,)), ref, subseq_bytes=32, hint=64)


# ------------------------------------------------------------------------------------------------
# special ends
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["s420_stuffed", "s420_rst5", "gray_rst1", "s444_rstrow", "s422_plain"])
def test_special_ends(torch_cuda, ref, name):
    data = FILES[name]
    sp = T.special_cuts(data)
    keys = sorted(sp)
    got = dict(zip(keys, batch_rgb([data[:sp[k]] for k in keys])))
    whole = jpeggpu_amd.decode_batch_to_rgb([data])[0].cpu().numpy()  # without the flag
    for k in keys:
        assert np.array_equal(got[k], ref(data, sp[k])), (name, k)
    assert np.array_equal(got["no_eoi"], whole) and np.array_equal(got["eoi_ff"], whole)  # a file that lacks only its EOI: bit for bit
    if "interval_end" in sp:
        assert np.array_equal(got["interval_end"], got["in_rst"]) and np.array_equal(got["in_rst"], got["behind_rst"])
        assert not np.array_equal(got["interval_end"], whole)
    if "in_ff00" in sp:
        assert np.array_equal(got["in_ff00"], ref(data, sp["in_ff00"] - 1))


# ------------------------------------------------------------------------------------------------
# mixed batches, reused decoders
# ------------------------------------------------------------------------------------------------

def test_mixed_batch_both_orders(torch_cuda, ref):
    """Seven items, whole and truncated, of different layouts and subsequence sizes, in one call; then the other way round."""
    big = T.large_files()["rstrow"]
    items = [(FILES["s420_plain"], len(FILES["s420_plain"]), 32), (FILES["gray_rst1"], 400, 64), (big, len(big) // 2, 128), (FILES["s444_opt"], 500, 32),
             (big, len(big), 256), (FILES["s422_rst5"], 700, 64), (FILES["s420_stuffed"], 1421, 128)]
    for order in (items, items[::-1]):
        got = batch_rgb([d[:c] for d, c, _ in order], subseq_bytes=[b for _, _, b in order])
        for (d, c, b), g in zip(order, got):
            assert np.array_equal(g, ref(d, c)), (c, b)
    with jpeggpu_amd.BatchDecode([d[:c] for d, c, _ in items], truncated=True) as bd:
        assert bd.truncated == [False, True, True, True, False, True, True]


def test_one_decoder_and_tmp_truncated_whole_truncated(torch_cuda, ref):
    """No stale state: one decoder and one d_tmp take a truncated file, the whole file, and another cut of it; the whole
    decode equals a fresh decoder's, bit for bit."""
    torch = torch_cuda
    data = T.large_files()["rstrow"]
    b = T.scan_begin(data)
    sequence = [b + 3000, len(data), b + 900, len(data), b + 12000]
    dec = jpeggpu_amd.Decoder()
    try:
        dec.set_truncated(True)
        dec.set_idct("islow")
        sizes = []
        for c in sequence:
            dec.parse_header(data[:c])
            sizes.append(dec.get_buffer_size())
        tmp = torch.empty(max(sizes) + 256, dtype=torch.uint8, device="cuda:0")
        base = (tmp.data_ptr() + 255) // 256 * 256
        stream = torch.cuda.current_stream().cuda_stream
        fresh = jpeggpu_amd.decode_to_rgb(data).cpu().numpy()
        for c in sequence:
            info = dec.parse_header(data[:c])
            planes = [torch.full((info.sizes_y[k], info.sizes_x[k]), 0x5A, dtype=torch.uint8, device="cuda:0") for k in range(info.num_components)]
            dec.transfer(base, max(sizes), stream)
            dec.decode([p.data_ptr() for p in planes], [p.stride(0) for p in planes], base, max(sizes), stream)
            g = jpeggpu_amd.planes_to_rgb(planes, info, fancy=True, color=dec.color_space()).cpu().numpy()
            assert np.array_equal(g, ref(data, c)), c
            if c == len(data):
                assert np.array_equal(g, fresh) and dec.truncated().truncated == 0
            else:
                assert dec.truncated().truncated == 1
    finally:
        dec.cleanup()


# ------------------------------------------------------------------------------------------------
# routes
# ------------------------------------------------------------------------------------------------

ROUTE = ("s420_rst5", 900)      # a file with restart markers, cut in its lower half
ROUTE_PLAIN = ("s420_plain", 850)


def test_route_planes_reference_idct(torch_cuda):
    from oracle import oracle

    data, cut = FILES[ROUTE[0]], ROUTE[1]
    dec = T.decode(data[:cut])
    planes, info = jpeggpu_amd.decode_to_planes(data[:cut], truncated=True)
    for c in range(dec.ncomp):
        coef = dec.coef[c]
        want = np.stack([oracle.idct_block(blk, dec.qtab[dec.qidx[c]]).reshape(8, 8) for blk in coef.reshape(-1, 64)])
        want = want.reshape(coef.shape[0], coef.shape[1], 8, 8).transpose(0, 2, 1, 3).reshape(coef.shape[0] * 8, coef.shape[1] * 8)
        h, w = dec.planes[c].shape
        assert np.array_equal(planes[c].cpu().numpy(), want[:h, :w]), c


@pytest.mark.parametrize("name,cut", [ROUTE, ROUTE_PLAIN, ("gray_opt", 330)])
def test_route_gray(torch_cuda, name, cut):
    data = FILES[name]
    want = gray_ref.gray_of(T.decode(data[:cut]), T.model_of(data))
    assert np.array_equal(jpeggpu_amd.decode_to_gray(data[:cut], truncated=True).cpu().numpy(), want)
    assert np.array_equal(jpeggpu_amd.decode_batch_to_gray([data[:cut], data], truncated=True)[0].cpu().numpy(), want)


@pytest.mark.parametrize("scale", [2, 4, 8])
def test_route_draft_scales(torch_cuda, scale):
    for name, cut in (ROUTE, ROUTE_PLAIN, ("s444_rstrow", 800)):
        data = FILES[name]
        want = T.rgb(data[:cut], scale)
        assert np.array_equal(jpeggpu_amd.decode_to_rgb(data[:cut], scale=scale, truncated=True).cpu().numpy(), want), (name, scale)
        got = jpeggpu_amd.decode_batch_to_rgb([data[:cut]] * 2, scales=[scale, scale], truncated=True)
        assert np.array_equal(got[1].cpu().numpy(), want), (name, scale)


@pytest.mark.parametrize("name,cut", [ROUTE, ROUTE_PLAIN])
def test_route_crops_across_and_below_the_cut(torch_cuda, ref, name, cut):
    data = FILES[name]
    whole = ref(data, cut)
    mcu = T.decode(data[:cut]).cut_mcu[1]
    y_cut = (mcu // 4) * 16  # 64 pixels wide: four MCUs per row
    assert 16 <= y_cut <= 32
    rects = [(5, y_cut - 9, 41, 20), (17, y_cut + 17, 30, 47 - y_cut - 17), (0, 0, 64, 48)]
    got = jpeggpu_amd.decode_batch_to_rgb([data[:cut]] * len(rects), crops=rects, truncated=True)
    for (x, y, w, h), g in zip(rects, got):
        assert np.array_equal(g.cpu().numpy(), whole[y:y + h, x:x + w]), (name, (x, y, w, h))
    x, y, w, h = rects[0]
    assert np.array_equal(jpeggpu_amd.decode_to_rgb(data[:cut], crop=rects[0], truncated=True).cpu().numpy(), whole[y:y + h, x:x + w])
    assert (whole[y_cut + 20:] == 128).all()  # below the cut: grey


def test_route_exif_transpose(torch_cuda, ref):
    data, cut = FILES[ROUTE[0]], ROUTE[1]
    turned = exif_ref.with_orientation(data, 6)
    shift = len(turned) - len(data)
    want = exif_ref.apply(ref(data, cut), 6)
    assert np.array_equal(jpeggpu_amd.decode_to_rgb(turned[:cut + shift], exif_transpose=True, truncated=True).cpu().numpy(), want)
    got = jpeggpu_amd.decode_batch_to_rgb([turned[:cut + shift], turned], exif_transpose=True, truncated=True)
    assert np.array_equal(got[0].cpu().numpy(), want)


def test_route_resized_center_cropped_thumbnails(torch_cuda, ref):
    names = [ROUTE, ROUTE_PLAIN, ("s444_rst1", 777)]
    datas = [FILES[n][:c] for n, c in names]
    refs = [ref(FILES[n], c) for n, c in names]
    got = jpeggpu_amd.decode_resized(datas, 64, truncated=True).cpu().numpy()
    for g, a in zip(got, refs):
        assert np.array_equal(g, pillow_resample_ref.resize(a, 64, 64, "bilinear"))
    got = jpeggpu_amd.decode_center_cropped(datas, resize=40, crop=32, truncated=True).cpu().numpy()
    for g, a in zip(got, refs):
        assert np.array_equal(g, center_crop_ref.resize_center_crop(a, 40, 32, "bilinear"))
    views = jpeggpu_amd.decode_thumbnails(datas, (24, 24), truncated=True)
    for v, (n, c) in zip(views, names):
        d = FILES[n][:c]
        dec = T.decode(d)
        want, _ = thumbnail_ref.thumbnail(lambda s: T.rgb_of(dec, d, s), dec.width, dec.height, 24, 24)
        assert np.array_equal(v.cpu().numpy(), want), n


def test_route_cmyk(torch_cuda):
    data, model = color_ref.cases()["c21_adobe2"]  # 264 x 200 YCCK, luma and K at 2 x 1
    assert model == color_ref.YCCK
    b = T.scan_begin(data)
    cuts = [b + (len(data) - b) * k // 5 for k in (1, 3)] + [len(data) - 2]
    got = batch_rgb([data[:c] for c in cuts])
    for c, g in zip(cuts, got):
        assert np.array_equal(g, T.rgb(data[:c])), c


# ------------------------------------------------------------------------------------------------
# refusals, coefficient routes
# ------------------------------------------------------------------------------------------------

def test_refusals(torch_cuda):
    import os

    from tests.conftest import GOLDEN

    data, cut = FILES[ROUTE[0]], ROUTE[1]
    for call in (lambda: jpeggpu_amd.decode_to_rgb(data[:cut]), lambda: jpeggpu_amd.decode_batch_to_rgb([data, data[:cut]]),
                 lambda: jpeggpu_amd.decode_resized([data[:cut]], 32), lambda: jpeggpu_amd.read_coefficients([data[:cut]])):
        with pytest.raises(JpegGpuError) as e:  # without the flag: today's error
            call()
        assert e.value.status == Status.INVALID_JPEG
    prog = np.load(os.path.join(GOLDEN, "progressive_pins.npz"))["prog/p420_odd"].tobytes()
    for p in (prog, prog[:len(prog) // 2]):
        with pytest.raises(JpegGpuError) as e:
            jpeggpu_amd.decode_batch_to_rgb([p], truncated=True)
        assert e.value.status == Status.NOT_SUPPORTED
    with pytest.raises(JpegGpuError):  # a cut inside the headers stays an error under the flag
        jpeggpu_amd.decode_to_rgb(data[:T.scan_begin(data) - 3], truncated=True)


def test_coefficient_routes_give_the_zero_blocks(torch_cuda):
    """read_coefficients and transcode_jpeg on a truncated source see the data units the IDCT stage sees: the rule's
    coefficients, all zero behind the cut -- never what the entropy stage left there."""
    for name, cut in (ROUTE, ROUTE_PLAIN, ("s420_stuffed", 1421)):
        data = FILES[name]
        dec = T.decode(data[:cut])
        co = jpeggpu_amd.read_coefficients([data[:cut]], truncated=True)[0]
        for c in range(dec.ncomp):
            got = co.coefficients[c].cpu().numpy()
            want = dec.coef[c][:got.shape[0], :got.shape[1]]
            assert np.array_equal(got.reshape(want.shape), want), (name, c)
        out = jpeggpu_amd.transcode_jpeg([data[:cut]], optimize=True, truncated=True)[0]
        again = T.decode(out)
        assert again.ended == "eoi"
        for c in range(dec.ncomp):
            assert np.array_equal(again.coef[c], dec.coef[c]), (name, c)
