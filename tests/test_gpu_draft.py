"""libjpeg's scale mode on the GPU (jpeggpu_ext_set_scale_mode, decode_to_rgb(scale=), decode_resized(scales=)): planes,
RGB, crops, batches and the batched resize at 1/2, 1/4 and 1/8 against the numpy restatement (tests/draft_ref.py) and
Pillow's pinned outputs (tests/golden/draft_pins.npz), with guard bytes around every plane."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

from tests import cases, draft_ref, libjpeg_ref, scaled_ref
from tests import pillow_resample_ref as R
from tests.conftest import GOLDEN
from tests.test_gpu_scaled import GUARD, Guarded, _assert_planes, _tmp
from tools.crop_rate import random_resized_crop

pytestmark = pytest.mark.gpu

SCALES = draft_ref.SCALES


@pytest.fixture(scope="module")
def torch_cuda(gpu_lib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def files():
    return draft_ref.inputs()


@pytest.fixture(scope="module")
def decoded(files):
    from oracle import oracle

    return {name: oracle.decode(data) for name, data in files.items()}


@pytest.fixture(scope="module")
def pins():
    return np.load(os.path.join(GOLDEN, "draft_pins.npz"))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def decode_draft(torch, data, d, subseq_bytes=None, device_scan=False, crop=None, mode="libjpeg", method=None, shard=None):
    """Guarded planes of one lone decode: (planes, info, crop_info, scale_info)."""
    import jpeggpu_amd

    dec = jpeggpu_amd.Decoder(subseq_bytes)
    try:
        dec.set_scale(d)
        dec.set_scale_mode(mode)
        dec.set_device_scan(device_scan)
        if method is not None:
            dec.set_idct(method)
        if crop is not None:
            dec.set_crop(*crop)
        info = dec.parse_header(data)
        n = dec.get_buffer_size()
        tmp, base = _tmp(torch, n)
        g = Guarded(torch, info)
        dec.transfer(base, n, 0)
        dec.decode(g.ptrs, g.pitches, base, n, 0)
        torch.cuda.synchronize()
        if device_scan:
            assert dec.device_status(base, 0) == jpeggpu_amd.Status.SUCCESS
        return g.planes(), info, dec.crop_info(), dec.scale_info()
    finally:
        dec.cleanup()


def window_of(planes, ci, info):
    """The slices of the uncropped planes that a cropped decode's windows are."""
    return [p[ci.origin_y[c]:ci.origin_y[c] + info.sizes_y[c], ci.origin_x[c]:ci.origin_x[c] + info.sizes_x[c]] for c, p in enumerate(planes)]


@pytest.mark.parametrize("subseq_bytes,device_scan", [(32, False), (32, True), (256, False), (256, True)])
def test_planes_of_every_file_at_every_scale(torch_cuda, files, decoded, subseq_bytes, device_scan):
    n = 0
    for name, data in files.items():
        for d in SCALES:
            got, info, _, si = decode_draft(torch_cuda, data, d, subseq_bytes, device_scan)
            hs, vs = draft_ref.factors_of(decoded[name])
            assert list(si.block_size[:info.num_components]) == draft_ref.block_sizes(hs, vs, d)
            _assert_planes(got, draft_ref.draft_planes_of(decoded[name], d), (name, d, subseq_bytes, device_scan))
            n += 1
    assert n >= 3 * 100


def test_eight_by_eight_blocks_are_islow_whatever_the_method(torch_cuda, files, decoded):
    for name in ("ss_2x2", "sweep:y4x2_a", "q16_tables"):
        want = draft_ref.draft_planes_of(decoded[name], 2)
        for method in ("reference", "islow"):
            got, _, _, _ = decode_draft(torch_cuda, files[name], 2, method=method)
            _assert_planes(got, want, (name, method))


def test_scale_one_and_uniform_mode_are_unchanged(torch_cuda, files, decoded):
    for name in ("ss_2x2", "ss_2x1", "gray", "ni_420", "four_comp_opt"):
        dec = decoded[name]
        got, _, _, _ = decode_draft(torch_cuda, files[name], 1)
        _assert_planes(got, [p for p in dec.planes], (name, "scale 1"))
        got, _, _, _ = decode_draft(torch_cuda, files[name], 1, method="islow")
        _assert_planes(got, libjpeg_ref.islow_planes_of(dec), (name, "scale 1 islow"))
        for d in SCALES:
            got, _, _, _ = decode_draft(torch_cuda, files[name], d, mode="uniform")
            _assert_planes(got, scaled_ref.scaled_planes_of(dec, d), (name, d, "uniform"))


def test_rgb_equals_the_restatement_and_pillows_pins(torch_cuda, files, decoded, pins):
    import jpeggpu_amd

    n = pinned = replicated = 0
    for name, data in files.items():
        dec = decoded[name]
        if not draft_ref.has_rgb(dec):
            continue
        for d in SCALES:
            got = jpeggpu_amd.decode_to_rgb(data, scale=d, device_scan=bool(n & 1)).cpu().numpy()
            want = draft_ref.draft_rgb_of(dec, d)
            assert got.shape == want.shape and np.array_equal(got, want), (name, d, int((got != want).sum()) if got.shape == want.shape else got.shape)
            key = "%s/%d" % (name, d)
            if "rgb/" + key in pins.files:
                assert np.array_equal(got, pins["rgb/" + key]), key
                pinned += 1
            elif "rgb_sha256/" + key in pins.files:
                assert sha(got) == str(pins["rgb_sha256/" + key]), key
                pinned += 1
            else:
                assert not draft_ref.pillow_comparable(name, dec, d), key
            replicated += draft_ref.needs_replication(dec, d)
            n += 1
    assert pinned == sum(k.startswith(("rgb/", "rgb_sha256/")) for k in pins.files) >= 299
    assert replicated >= 20  # 1/8 with subsampling left: jpeggpu_ext_planes_to_rgbi_replicate


def test_replicating_rgb_stays_inside_its_rows(torch_cuda, files, decoded):
    """jpeggpu_ext_planes_to_rgbi_replicate into a padded, guarded buffer; and it is not the fancy call's output."""
    import jpeggpu_amd
    from jpeggpu_amd.api import Img, lib

    torch = torch_cuda
    differs = 0
    for name in ("ss_2x1", "ss_1x2", "ss_4x1", "sweep:y4x1_c2x1_a", "sweep:y1x1_c2x1_b"):
        dec = decoded[name]
        planes, info = jpeggpu_amd.decode_to_planes(files[name], scale=8, idct="islow", scale_mode="libjpeg")
        W, H = draft_ref.ceil_div(dec.width, 8), draft_ref.ceil_div(dec.height, 8)
        src = Img()
        for c in range(3):
            src.image[c], src.pitch[c] = planes[c].data_ptr(), planes[c].stride(0)
        pitch = 3 * W + 7
        out = torch.full((H + 2, pitch), GUARD, dtype=torch.uint8, device="cuda:0")
        assert lib().jpeggpu_ext_planes_to_rgbi_replicate(C.byref(info), C.byref(src), out[1:].data_ptr(), pitch, W, H, None) == 0
        torch.cuda.synchronize()
        a = out.cpu().numpy()
        assert (a[0] == GUARD).all() and (a[-1] == GUARD).all() and (a[1:-1, 3 * W:] == GUARD).all(), name
        got = a[1:-1, :3 * W].reshape(H, W, 3)
        assert np.array_equal(got, draft_ref.draft_rgb_of(dec, 8)), name
        differs += not np.array_equal(got, jpeggpu_amd.planes_to_rgb(planes, info).cpu().numpy())
    assert differs >= 3


def seeded_rects(rng, W, H, k):
    out = [(0, 0, W, H), (W - 1, H - 1, 1, 1), (0, 0, 1, 1)]
    for _ in range(k):
        w, h = int(rng.integers(1, W + 1)), int(rng.integers(1, H + 1))
        out.append((int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), w, h))
    return out


def test_crops_equal_the_slice_of_the_uncropped_result(torch_cuda, files, decoded):
    import jpeggpu_amd

    rng = np.random.default_rng(20261016)
    n = 0
    for k, (name, data) in enumerate(files.items()):
        if name == "photo":
            continue
        dec = decoded[name]
        for d in SCALES:
            W, H = draft_ref.ceil_div(dec.width, d), draft_ref.ceil_div(dec.height, d)
            full = draft_ref.draft_planes_of(dec, d)
            rgb = draft_ref.draft_rgb_of(dec, d) if draft_ref.has_rgb(dec) else None
            for rect in seeded_rects(rng, W, H, 2):
                got, info, ci, _ = decode_draft(torch_cuda, data, d, crop=rect, device_scan=bool((n + k) & 1), subseq_bytes=(None, 32, 256)[n % 3])
                _assert_planes(got, window_of(full, ci, info), (name, d, rect))
                if rgb is not None:
                    x, y, w, h = rect
                    out = jpeggpu_amd.decode_to_rgb(data, scale=d, crop=rect).cpu().numpy()
                    assert np.array_equal(out, rgb[y:y + h, x:x + w]), (name, d, rect)
                n += 1
    assert n > 1500


def test_photo_crops(torch_cuda, files, decoded):
    import jpeggpu_amd

    dec = decoded["photo"]
    rng = np.random.default_rng(5)
    for d in SCALES:
        W, H = draft_ref.ceil_div(dec.width, d), draft_ref.ceil_div(dec.height, d)
        rgb = draft_ref.draft_rgb_of(dec, d)
        for x, y, w, h in [random_resized_crop(rng, W, H) for _ in range(3)] + [(W - 57, H - 33, 57, 33)]:
            out = jpeggpu_amd.decode_to_rgb(files["photo"], scale=d, crop=(x, y, w, h)).cpu().numpy()
            assert np.array_equal(out, rgb[y:y + h, x:x + w]), (d, x, y, w, h)


def _batch(torch, items, hint):
    """items: [(bytes, d, mode, method, crop)] through ONE jpeggpu_ext_decode_batch call: [(planes, info, crop_info)]."""
    import jpeggpu_amd

    keep, entries, total = [], [], 0
    for k, (data, d, mode, method, crop) in enumerate(items):
        dec = jpeggpu_amd.Decoder()
        dec.set_batch_hint(hint)
        dec.set_scale(d)
        dec.set_scale_mode(mode)
        dec.set_idct(method)
        dec.set_device_scan(k % 3 == 1)
        if crop is not None:
            dec.set_crop(*crop)
        info = dec.parse_header(data)
        n = dec.get_buffer_size()
        tmp, base = _tmp(torch, n)
        g = Guarded(torch, info)
        dec.transfer(base, n, 0)
        total += dec.layout().num_scans
        keep.append((dec, tmp, g, base, info))
        entries.append((dec, g.ptrs, g.pitches, base, n))
    batch = jpeggpu_amd.Batch(total)
    scratch = torch.empty(batch.scratch_size, dtype=torch.uint8, device="cuda:0")
    batch.set_items(entries)
    batch.decode(scratch.data_ptr(), 0)
    torch.cuda.synchronize()
    out = []
    for dec, _t, g, base, info in keep:
        assert dec.device_status(base, 0) == jpeggpu_amd.Status.SUCCESS
        out.append((g.planes(), info, dec.crop_info()))
        dec.cleanup()
    batch.destroy()
    return out


def expected_planes(dec, d, mode, method):
    if d == 1:
        return libjpeg_ref.islow_planes_of(dec) if method == "islow" else [p for p in dec.planes]
    return draft_ref.draft_planes_of(dec, d) if mode == "libjpeg" else scaled_ref.scaled_planes_of(dec, d)


def test_one_batch_mixes_modes_scales_methods_and_crops(torch_cuda, files, decoded):
    import jpeggpu_amd

    names = ["multi_seq_dri", "ni_420_dri", "four_comp_opt", "gray", "ss_2x2", "cfg4_small", "dri_1", "odd_partial_mcu", "ss_4x1",
             "q16_tables", "dense_escapes", "ni_big_last", "ss_2x1", "sweep:y4x2_a", "sweep:y1x1_cb2x2_a", "sweep:y2x2_c1x2_b",
             "sweep:po_four_8du", "sweep:y2x4_rowdri"]
    items, what = [], []
    for k, name in enumerate(names + names[::-1]):
        d = (1, 2, 4, 8)[k % 4]
        mode = ("libjpeg", "uniform")[(k // 4) % 2] if k % 5 else "libjpeg"
        method = ("reference", "islow")[(k // 2) % 2]
        dec = decoded[name]
        W, H = draft_ref.ceil_div(dec.width, d), draft_ref.ceil_div(dec.height, d)
        crop = (W // 4, H // 5, max(1, W // 2), max(1, H // 3)) if k % 3 == 2 else None
        items.append((files[name], d, mode, method, crop))
        what.append((name, d, mode, method, crop))
    assert {(w[1], w[2]) for w in what} >= {(d, m) for d in (1, 2, 4, 8) for m in ("libjpeg", "uniform")}
    for hint in (0, 64):
        for (planes, info, ci), w in zip(_batch(torch_cuda, items, hint), what):
            name, d, mode, method, crop = w
            want = expected_planes(decoded[name], d, mode, method)
            _assert_planes(planes, window_of(want, ci, info) if crop else want, w + (hint,))
    assert jpeggpu_amd.fused_tail_timeouts() == 0


@pytest.mark.parametrize("d", [2, 8])
def test_full_batch_of_64_twelve_megapixel_images(torch_cuda, d):
    """BASELINE.json configs[2] (64 x 12 MP 4:2:0) in one call at 1/d in libjpeg's mode: plane hashes against the restatement."""
    import jpeggpu_amd
    from oracle import oracle
    from tools import jpegsynth

    datas = [jpegsynth.config(2, seed=100 + s) for s in range(4)]
    want = [[sha(p) for p in draft_ref.draft_planes_of(oracle.decode(x), d)] for x in datas]
    got = _batch(torch_cuda, [(datas[i % 4], d, "libjpeg", "reference", None) for i in range(64)], 64)
    bad = [i for i, (planes, _, _) in enumerate(got) if [sha(p) for p in planes] != want[i % 4]]
    assert not bad, bad
    assert [p.shape for p in got[0][0]] == [(3024 // d, 4032 // d)] * 3
    assert jpeggpu_amd.fused_tail_timeouts() == 0


def test_segment_shard_bands(torch_cuda, files, decoded):
    import jpeggpu_amd
    from oracle import oracle
    from tools import jpegsynth

    torch = torch_cuda
    inputs = {"dri_row": (files["dri_row"], decoded["dri_row"]), "sweep:y2x4_rowdri": (files["sweep:y2x4_rowdri"], decoded["sweep:y2x4_rowdri"])}
    two = jpegsynth.encode(333, 251, cases.S420, restart_interval=42, seed=78)
    inputs["two_rows"] = (two, oracle.decode(two))
    for name, (data, ref) in inputs.items():
        for d in SCALES:
            want = draft_ref.draft_planes_of(ref, d)
            for world in (2, 3):
                planes = [torch.full(p.shape, 0xAB, dtype=torch.uint8, device="cuda:0") for p in want]
                for rank in range(world):
                    dec = jpeggpu_amd.Decoder(32 if rank % 2 else 64)
                    dec.set_scale(d)
                    dec.set_scale_mode("libjpeg")
                    dec.set_segment_shard(rank, world)
                    info = dec.parse_header(data)
                    assert [(info.sizes_y[c], info.sizes_x[c]) for c in range(info.num_components)] == [p.shape for p in want]
                    n = dec.get_buffer_size()
                    tmp, base = _tmp(torch, n)
                    before = [p.clone() for p in planes]
                    dec.transfer(base, n, 0)
                    dec.decode([p.data_ptr() for p in planes], [p.stride(0) for p in planes], base, n, 0)
                    torch.cuda.synchronize()
                    for c in range(info.num_components):
                        a, cnt = dec.shard_rows(c)
                        assert torch.equal(planes[c][:a], before[c][:a]) and torch.equal(planes[c][a + cnt:], before[c][a + cnt:]), (name, d, world, rank, c)
                        assert np.array_equal(planes[c][a:a + cnt].cpu().numpy(), want[c][a:a + cnt]), (name, d, world, rank, c)
                    dec.cleanup()
                for c in range(len(want)):
                    assert np.array_equal(planes[c].cpu().numpy(), want[c]), (name, d, world, c)


@pytest.mark.parametrize("layout", ("NHWC", "NCHW"))
@pytest.mark.parametrize("filt", R.FILTERS)
def test_decode_resized_with_scales(torch_cuda, files, decoded, layout, filt):
    """Seeded RandomResizedCrop rectangles of the image at draft_scale's choice, against Pillow's resampling restated
    (tests/pillow_resample_ref.py) applied to the restatement's crops."""
    import jpeggpu_amd

    rng = np.random.default_rng(77)
    names = ["ss_2x2", "ss_2x1", "ss_1x2", "gray", "ss_4x1", "dri_7", "ni_420", "q100_noisy", "cfg2_small", "sweep:y4x2_a",
             "sweep:y1x1_cb2x2_a", "sweep:y2x2_c1x2_a", "ss_2x2", "gray", "ss_1x1", "photo"]
    datas, crops, scales, want = [], [], [], []
    for k, name in enumerate(names):
        dec = decoded[name]
        d = (1, 2, 4, 8)[k % 4]
        if d == 8 and draft_ref.needs_replication(dec, 8):
            d = 4
        W, H = draft_ref.ceil_div(dec.width, d), draft_ref.ceil_div(dec.height, d)
        rect = random_resized_crop(rng, W, H) if k % 5 else None
        rgb = draft_ref.draft_rgb_of(dec, d) if d > 1 else libjpeg_ref.libjpeg_rgb_of(dec)
        if rect is not None:
            x, y, w, h = rect
            rgb = rgb[y:y + h, x:x + w]
        datas.append(files[name]), crops.append(rect), scales.append(d), want.append(R.resize(rgb, 48, 40, filt))
    assert set(scales) == {1, 2, 4, 8}
    got = jpeggpu_amd.decode_resized(datas, (40, 48), crops=crops, scales=scales, filt=filt, layout=layout).cpu().numpy()
    assert got.shape == ((16, 40, 48, 3) if layout == "NHWC" else (16, 3, 40, 48))
    for i in range(16):
        g = got[i] if layout == "NHWC" else got[i].transpose(1, 2, 0)
        assert np.array_equal(g, want[i]), (names[i], scales[i], crops[i], int((g != want[i]).sum()))


def test_decode_resized_pillow_pins(torch_cuda, files, decoded, pins):
    import jpeggpu_amd

    n = 0
    for key in pins.files:
        if not key.startswith("resize/"):
            continue
        _, name, d, box, size, filt = key.split("/")
        x0, y0, x1, y1 = (int(v) for v in box.split(","))
        w, h = (int(v) for v in size.split("x"))
        d = int(d)
        if draft_ref.needs_replication(decoded[name], d):  # libjpeg replicates there: refused below
            continue
        got = jpeggpu_amd.decode_resized([files[name]], (h, w), crops=[(x0, y0, x1 - x0, y1 - y0)], scales=[d], filt=filt).cpu().numpy()[0]
        assert np.array_equal(got, pins[key]), (key, int((got != pins[key]).sum()))
        n += 1
    assert n >= 80


def test_decode_resized_refuses_what_needs_replication(torch_cuda, files):
    import jpeggpu_amd

    for name in ("ss_2x1", "ss_1x2", "ss_4x1"):
        with pytest.raises(ValueError, match="replicates"):
            jpeggpu_amd.decode_resized([files["ss_2x2"], files[name]], 16, scales=[8, 8])
        jpeggpu_amd.decode_resized([files["ss_2x2"], files[name]], 16, scales=[8, 4])
    with pytest.raises(ValueError):
        jpeggpu_amd.decode_resized([files["ss_2x2"]], 16, scales=[3])
    with pytest.raises(ValueError):
        jpeggpu_amd.decode_resized([files["ss_2x2"]], 16, scales=[2, 2])


def test_draft_scale_recipe(torch_cuda, files, decoded):
    """The INTEGRATION.md recipe: the scale Pillow's draft() would pick for the output size, then the crop at that scale."""
    import jpeggpu_amd

    dec = decoded["photo"]
    d = jpeggpu_amd.draft_scale(dec.width, dec.height, (224, 224))
    assert d == 8
    W, H = draft_ref.ceil_div(dec.width, d), draft_ref.ceil_div(dec.height, d)
    rect = (W // 5, H // 6, W // 2, H // 2)
    got = jpeggpu_amd.decode_resized([files["photo"]], 224, crops=[rect], scales=[d], filt="bicubic").cpu().numpy()[0]
    x, y, w, h = rect
    assert np.array_equal(got, R.resize(draft_ref.draft_rgb_of(dec, d)[y:y + h, x:x + w], 224, 224, "bicubic"))


def test_corrupt_entropy_data_is_memory_safe(torch_cuda, files):
    """Random damage inside the entropy-coded segment, decoded in libjpeg's mode alone and as a batch item, whole and
    cropped: every decode completes, stays inside d_tmp and the planes' guards, and the device decodes correctly
    afterwards. (It damages bytes and checks memory; nothing here provokes a fault.)"""
    import jpeggpu_amd
    from oracle import oracle

    torch = torch_cuda
    rng = np.random.default_rng(8642)
    for name in ("multi_seq_dri", "multi_seq_nodri", "four_comp_opt", "ni_420_dri", "ss_2x2"):
        good = files[name]
        lo, hi = oracle.scan_info(good, 0, 128).scan_begin, oracle.scan_info(good, 0, 128).scan_end
        for trial in range(4):
            bad = bytearray(good)
            for pos in rng.integers(lo + 4, hi - 4, size=int(rng.integers(1, 40))):
                if bad[pos] != 0xFF and bad[pos - 1] != 0xFF:
                    bad[pos] = int(rng.integers(0, 255))
            for batched in (False, True):
                dec = jpeggpu_amd.Decoder(int(rng.choice([32, 64, 128])))
                dec.set_scale((2, 4, 8, 2)[trial])
                dec.set_scale_mode("libjpeg")
                dec.set_device_scan(bool(trial & 1))
                if trial >= 2:
                    dec.set_crop(3, 2, 20, 15)
                if batched:
                    dec.set_batch_hint(64)
                try:
                    info = dec.parse_header(bytes(bad))
                except jpeggpu_amd.JpegGpuError:
                    dec.cleanup()
                    continue
                n = dec.get_buffer_size()
                guard = 4096
                tmp = torch.full((n + 256 + 2 * guard,), GUARD, dtype=torch.uint8, device="cuda:0")
                base = (tmp.data_ptr() + guard + 255) // 256 * 256
                g = Guarded(torch, info)
                dec.transfer(base, n, 0)
                if batched:
                    batch = jpeggpu_amd.Batch(dec.layout().num_scans)
                    scratch = torch.empty(batch.scratch_size, dtype=torch.uint8, device="cuda:0")
                    batch.set_items([(dec, g.ptrs, g.pitches, base, n)])
                    batch.decode(scratch.data_ptr(), 0)
                else:
                    dec.decode(g.ptrs, g.pitches, base, n, 0)
                torch.cuda.synchronize()
                off = base - tmp.data_ptr()
                assert (tmp[:off] == GUARD).all() and (tmp[off + n:] == GUARD).all(), (name, trial, batched, "tmp overrun")
                g.planes()  # raises if a guard byte was written
                if batched:
                    batch.destroy()
                dec.cleanup()
        got, _, _, _ = decode_draft(torch, good, 2)
        _assert_planes(got, draft_ref.draft_planes_of(oracle.decode(good), 2), (name, "after damage"))
    assert jpeggpu_amd.fused_tail_timeouts() == 0
