"""Encoding on the device (jpeggpu_ext_encode_batch, encode_jpeg): every case of tests/encode_cases.py equals Pillow's pinned
file byte for byte; strides, mixed batches, slots that are too small, the round trip through the decoder, streams. Every
output slot lies between guard bytes (0xA5, 64 on each side), which are checked."""
import numpy as np
import pytest

import jpeggpu_amd
from tests import encode_cases as K
from tests import encode_ref as E

pytestmark = pytest.mark.gpu

GUARD, G = 0xA5, 64
CASES = K.cases()
DEV = "cuda:0"


@pytest.fixture(scope="module")
def torch(gpu_lib):
    import torch

    assert torch.cuda.is_available()
    return torch


def _params(c):
    return dict(quality=c["quality"], subsampling=c["subsampling"], restart_interval=c["restart_interval"])


def _bound(c):
    return jpeggpu_amd.encode_bound(c["w"], c["h"], 1 if c["grey"] else 3, c["quality"], c["subsampling"], c["restart_interval"])


def encode_guarded(torch, images, capacities, layout="HWC", **params):
    """One jpeggpu_ext_encode_batch call into guarded slots of the given capacities. Returns (files, sizes, status): files[i]
    the bytes of slot i up to its reported size, or None where the slot was too small. Asserts that nothing outside
    [slot start, slot start + size) was written -- for a slot that was too small, nothing at all."""
    offsets, total = [], G
    for cap in capacities:
        offsets.append(total)
        total += cap + G
    buf = torch.full((total,), GUARD, dtype=torch.uint8, device=DEV)
    outs = [buf[o:o + cap] for o, cap in zip(offsets, capacities)]
    sizes, status = jpeggpu_amd.encode_into(images, outs, layout=layout, **params)
    sizes, status = sizes.cpu().tolist(), status.cpu().tolist()
    host = buf.cpu().numpy()
    untouched = np.ones(total, bool)
    files = []
    for o, cap, size, st in zip(offsets, capacities, sizes, status):
        assert st == (1 if size > cap else 0)
        if st == 0:
            untouched[o:o + size] = False
            files.append(host[o:o + size].tobytes())
        else:
            files.append(None)
    assert (host[untouched] == GUARD).all(), "bytes outside the files were written"
    return files, sizes, status


def _first_difference(a, b):
    n = next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))
    return "lengths %d / %d, first difference at byte %d" % (len(a), len(b), n)


@pytest.fixture(scope="module")
def device_images(torch):
    return [torch.from_numpy(K.image(c)).to(DEV) for c in CASES]


def test_every_case_equals_its_pin(torch, device_images):
    """One call per case; the slot is the bound for even cases and exactly the pinned length for odd ones."""
    pins = K.pins()[0]
    wrong = []
    for i, (c, x) in enumerate(zip(CASES, device_images)):
        cap = _bound(c) if i % 2 == 0 else pins[c["name"]]["length"]
        files, sizes, status = encode_guarded(torch, [x], [cap], **_params(c))
        if status != [0] or sizes != [pins[c["name"]]["length"]] or not K.equals_pin(c["name"], files[0]):
            detail = _first_difference(files[0], pins[c["name"]]["data"]) if files[0] is not None and pins[c["name"]]["data"] else "size %s status %s" % (sizes, status)
            wrong.append("%s: %s" % (c["name"], detail))
    assert not wrong, "%d of %d cases differ from Pillow:\n%s" % (len(wrong), len(CASES), "\n".join(wrong[:20]))


def test_strides(torch):
    """The same pixels as an HWC tensor, a CHW tensor, a row-padded view and a crop of a larger tensor."""
    rng = np.random.default_rng(21)
    big = torch.from_numpy(rng.integers(0, 256, (60, 70, 3), dtype=np.uint8)).to(DEV)
    crop = big[10:47, 5:58]  # 37 x 53, not contiguous
    assert not crop.is_contiguous()
    hwc = crop.contiguous()
    chw = hwc.permute(2, 0, 1).contiguous()
    padded = torch.zeros((37, 64, 3), dtype=torch.uint8, device=DEV)
    padded[:, :53] = hwc
    want = E.encode(hwc.cpu().numpy(), 90, "4:2:0", 3)
    for name, x, layout in (("hwc", hwc, "HWC"), ("chw", chw, "CHW"), ("row-padded", padded[:, :53], "HWC"), ("crop", crop, "HWC"),
                            ("chw view of hwc", hwc.permute(2, 0, 1), "CHW")):
        files, _, _ = encode_guarded(torch, [x], [len(want)], layout=layout, quality=90, subsampling="4:2:0", restart_interval=3)
        assert files[0] == want, "%s: %s" % (name, _first_difference(files[0], want))
    grey = hwc[:, :, 1]  # a grey image with a pixel stride of 3
    want = E.encode(grey.cpu().numpy(), 75, "4:4:4", 0)
    for x, layout in ((grey, "HWC"), (grey.unsqueeze(0), "CHW"), (grey.unsqueeze(2), "HWC")):
        files, _, _ = encode_guarded(torch, [x], [len(want) + 5], layout=layout, quality=75, subsampling="4:4:4", restart_interval=0)
        assert files[0] == want


def _mixed(torch, device_images):
    names = ["1x1_noise_rgb_q1_444_r0", "37x53_noise_rgb_q95_422_r3", "rst_wrap_37x53", "tile_plus_one_block", "chunk_plus_few_bytes", "dc11_black_white_blocks",
             "ac10_checkerboard_rgb", "zrl_sparse_rgb", "real_640x427", "40x8_noise_rgb_q75_420_bottom", "real_640x427_grey_r3", "qsweep_q50"]
    by_name = {c["name"]: i for i, c in enumerate(CASES)}
    picked = [by_name[n] for n in names]
    cs = [CASES[i] for i in picked]
    params = dict(quality=[c["quality"] for c in cs], subsampling=[c["subsampling"] for c in cs], restart_interval=[c["restart_interval"] for c in cs])
    return cs, [device_images[i] for i in picked], params


def test_mixed_batch(torch, device_images):
    """Items that differ in size, channels, quality, subsampling and interval in one call: each equals its own file."""
    cs, images, params = _mixed(torch, device_images)
    pins = K.pins()[0]
    files, sizes, status = encode_guarded(torch, images, [_bound(c) for c in cs], **params)
    assert status == [0] * len(cs)
    assert sizes == [pins[c["name"]]["length"] for c in cs]
    for c, f in zip(cs, files):
        assert K.equals_pin(c["name"], f), c["name"]


def test_overflow(torch, device_images):
    """One slot a byte too small and one of capacity 0: both report their true size and stay untouched (encode_guarded checks
    every byte outside the files); the others are what they were. encode_jpeg gets all files after its retry."""
    cs, images, params = _mixed(torch, device_images)
    pins = K.pins()[0]
    lengths = [pins[c["name"]]["length"] for c in cs]
    caps = [_bound(c) for c in cs]
    caps[2], caps[8] = lengths[2] - 1, 0
    files, sizes, status = encode_guarded(torch, images, caps, **params)
    assert sizes == lengths
    assert status == [1 if i in (2, 8) else 0 for i in range(len(cs))]
    for i, (c, f) in enumerate(zip(cs, files)):
        assert (f is None) if i in (2, 8) else K.equals_pin(c["name"], f), c["name"]
    # the default capacity (raw samples + header) is too small for some of these: noise at quality 100 grows
    assert any(n > c["w"] * c["h"] * (1 if c["grey"] else 3) + 700 for c, n in zip(cs, lengths)), "the retry is exercised"
    got = jpeggpu_amd.encode_jpeg(images, **params)
    for c, f in zip(cs, got):
        assert K.equals_pin(c["name"], f), c["name"]
    buf, offsets, sizes = jpeggpu_amd.encode_jpeg_to_device(images, capacities=[16] * len(cs), **params)  # every item retried
    assert sizes == lengths
    host = buf.cpu().numpy()
    for c, o, n in zip(cs, offsets, sizes):
        assert K.equals_pin(c["name"], host[o:o + n].tobytes()), c["name"]


def test_batch_tensor_and_layouts(torch):
    rng = np.random.default_rng(22)
    batch = torch.from_numpy(rng.integers(0, 256, (3, 24, 40, 3), dtype=np.uint8)).to(DEV)
    want = [E.encode(batch[i].cpu().numpy(), 75, "4:2:0", 0) for i in range(3)]
    assert jpeggpu_amd.encode_jpeg(batch) == want
    assert jpeggpu_amd.encode_jpeg(batch.permute(0, 3, 1, 2), layout="CHW") == want
    assert jpeggpu_amd.encode_jpeg([]) == []
    with pytest.raises(ValueError):
        jpeggpu_amd.encode_jpeg(batch, subsampling="4:1:1")
    with pytest.raises(ValueError):
        jpeggpu_amd.encode_jpeg([batch[0].float()])
    with pytest.raises(jpeggpu_amd.JpegGpuError):
        jpeggpu_amd.encode_jpeg(batch, quality=0)


def test_round_trip_through_the_decoder(torch, device_images):
    from tests.libjpeg_ref import libjpeg_rgb

    for name in ("37x53_noise_rgb_q95_422_r3", "real_640x427"):
        i = next(i for i, c in enumerate(CASES) if c["name"] == name)
        data = jpeggpu_amd.encode_jpeg([device_images[i]], **_params(CASES[i]))[0]
        assert K.equals_pin(name, data)
        rgb = jpeggpu_amd.decode_to_rgb(data, device=DEV)
        assert np.array_equal(rgb.cpu().numpy(), libjpeg_rgb(data))


def test_stream_semantics(torch, device_images):
    """The call only enqueues: two calls follow each other on one non-default stream, each with its own scratch, and nothing is
    read before the stream is synchronised once."""
    a = next(i for i, c in enumerate(CASES) if c["name"] == "real_640x427")
    b = next(i for i, c in enumerate(CASES) if c["name"] == "scan_lanes_plus_420_r11")
    pins = K.pins()[0]
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    results = []
    with torch.cuda.stream(stream):
        for i in (a, b, a):
            slot = torch.full((pins[CASES[i]["name"]]["length"] + 2 * G,), GUARD, dtype=torch.uint8, device=DEV)
            results.append((i, slot, jpeggpu_amd.encode_into([device_images[i]], [slot[G:-G]], **_params(CASES[i]))))
    stream.synchronize()
    for i, slot, (sizes, status) in results:
        host = slot.cpu().numpy()
        assert status.cpu().tolist() == [0] and sizes.cpu().tolist() == [len(host) - 2 * G]
        assert K.equals_pin(CASES[i]["name"], host[G:-G].tobytes())
        assert (host[:G] == GUARD).all() and (host[-G:] == GUARD).all()
    torch.cuda.current_stream(DEV).wait_stream(stream)
