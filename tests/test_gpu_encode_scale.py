"""The encoder on the device where its first suite (tests/test_gpu_encode.py) does not reach: a seeded sweep of geometries and
parameters and the block kernel's arithmetic edges, one call each; a call of more than 600 items whose tile scan composes
runs of several tiles with item boundaries inside; a call with more chunks than the grid of the byte kernels, so that their
loops go round again; more calls in flight than the staging ring has buffers; the strides torch's views really have; the
round trip through the decoder. The expected file is Pillow's, pinned by length and SHA-256
(tests/golden/encode_sweep_pins.npz); tests/test_encode_ref.py asserts on the host that the calls have the structure they are
here for. Every slot lies between guard bytes and every byte outside the files is checked (encode_guarded). Where a file
differs, tests/encode_diff.py says in which stage."""
import functools

import numpy as np
import pytest

import jpeggpu_amd
from tests import encode_cases as K
from tests import encode_ref as E
from tests.encode_diff import where_files_differ
from tests.test_gpu_encode import DEV, GUARD, G, encode_guarded

pytestmark = pytest.mark.gpu

SWEEP, EDGES = K.sweep(), K.edge_cases()


@pytest.fixture(scope="module")
def torch(gpu_lib):
    import torch

    assert torch.cuda.is_available()
    return torch


BY_NAME = {c["name"]: c for c in K.new_cases()}


@functools.lru_cache(maxsize=None)
def _pixels(name):
    """The case's pixels on the host, made once per name (the big calls repeat their images)."""
    return K.image(BY_NAME[name])


@pytest.fixture(scope="module")
def on_device(torch):
    """case -> its pixels on the device; every image of the lists is made and sent once, here."""
    cache = {c["name"]: torch.from_numpy(_pixels(c["name"])).to(DEV) for c in K.new_cases()}
    return lambda c: cache[c["name"]]


def _args(c):
    return c["w"], c["h"], 1 if c["grey"] else 3, c["quality"], c["subsampling"], c["restart_interval"]


def _params(cs):
    return dict(quality=[c["quality"] for c in cs], subsampling=[c["subsampling"] for c in cs], restart_interval=[c["restart_interval"] for c in cs])


def _report(c, got):
    """Why `got` is not the pinned file of case c; the expected bytes are the restatement's, which the host tests hold to the pin."""
    want = E.encode(_pixels(c["name"]), c["quality"], c["subsampling"], c["restart_interval"])
    return "%s: %s" % (c["name"], where_files_differ(got, want))


def _check_files(cs, files, sizes, status, refused=()):
    """Every item of a call against its pin: exact sizes and status, no file for a refused slot, the pinned bytes elsewhere."""
    lengths = [K.pin_of(c["name"])["length"] for c in cs]
    assert sizes == lengths, [(i, cs[i]["name"], sizes[i], lengths[i]) for i in range(len(cs)) if sizes[i] != lengths[i]][:10]
    assert status == [1 if i in refused else 0 for i in range(len(cs))]
    wrong = [i for i, (c, f) in enumerate(zip(cs, files)) if f is not None and not K.equals_pin(c["name"], f)]
    assert all(files[i] is None for i in refused)
    assert not wrong, "%d of %d items differ from Pillow:\n%s" % (len(wrong), len(cs), "\n".join("item %d, %s" % (i, _report(cs[i], files[i])) for i in wrong[:8]))


def _one_call_each(torch, on_device, cases):
    wrong = []
    for i, c in enumerate(cases):
        length = K.pin_of(c["name"])["length"]
        cap = length if i % 2 else jpeggpu_amd.encode_bound(*_args(c))
        files, sizes, status = encode_guarded(torch, [on_device(c)], [cap], quality=c["quality"], subsampling=c["subsampling"], restart_interval=c["restart_interval"])
        if status != [0] or sizes != [length] or not K.equals_pin(c["name"], files[0]):
            wrong.append((c, files[0], sizes, status))
    assert not wrong, "%d of %d cases differ from Pillow:\n%s" % (
        len(wrong), len(cases), "\n".join("%s (size %s, status %s)" % (_report(c, f), sz, st) for c, f, sz, st in wrong[:8]))


def test_every_sweep_case_equals_its_pin(torch, on_device):
    """One call per case; the slot is the bound for even cases and exactly the pinned length for odd ones."""
    _one_call_each(torch, on_device, SWEEP)


def test_every_edge_case_equals_its_pin(torch, on_device):
    """Every basis function at full swing in either sign, and every colour of the lattice: the largest coefficients, the
    roundings of the forward DCT's descales and of the colour conversion."""
    _one_call_each(torch, on_device, EDGES)


@pytest.mark.parametrize("reverse", [False, True], ids=["in order", "reversed"])
def test_many_items_in_one_call(torch, on_device, reverse):
    """The whole sweep and the medium images between: more than 600 items and 4 * kScanThreads tiles, parameters per item. Odd
    items get a slot of exactly their file's length."""
    cs = K.many_call(reverse)
    caps = [K.pin_of(c["name"])["length"] if i % 2 else jpeggpu_amd.encode_bound(*_args(c)) for i, c in enumerate(cs)]
    files, sizes, status = encode_guarded(torch, [on_device(c) for c in cs], caps, **_params(cs))
    _check_files(cs, files, sizes, status)


def test_more_chunks_than_the_byte_kernels_grid(torch, on_device):
    """61 items of 256 x 256 with more than CHUNK_GRID chunks: the byte kernels' workgroups go round their loops again. Two slots
    a byte too small, one in front of chunk CHUNK_GRID and one behind it, and one of capacity 0 are refused and stay untouched."""
    call = K.grid_call()
    cs = call["items"]
    assert K.starts(cs, "chunks")[-1] > K.CHUNK_GRID
    caps = [jpeggpu_amd.encode_bound(*_args(c)) for c in cs]
    for i in call["short"]:
        caps[i] = K.pin_of(cs[i]["name"])["length"] - 1
    caps[call["zero"]] = 0
    files, sizes, status = encode_guarded(torch, [on_device(c) for c in cs], caps, **_params(cs))
    _check_files(cs, files, sizes, status, refused=set(call["short"]) | {call["zero"]})


def _ring_cases():
    """Nine different sweep cases, the largest first: the staging buffer a call reuses held the descriptors of a larger call, so
    a call that met another's descriptors (a ring that did not wait) would give wrong files and still stay inside its scratch."""
    cs = [SWEEP[i] for i in range(0, 9 * 61, 61)]
    return sorted(cs, key=lambda c: (K.counts(c)["chunks"], K.counts(c)["blocks"], K.counts(c)["segments"]), reverse=True)


def _enqueue(torch, on_device, c, results):
    length = K.pin_of(c["name"])["length"]
    slot = torch.full((length + 2 * G,), GUARD, dtype=torch.uint8, device=DEV)
    sizes, status = jpeggpu_amd.encode_into([on_device(c)], [slot[G:-G]], quality=c["quality"], subsampling=c["subsampling"], restart_interval=c["restart_interval"])
    results.append((c, slot, sizes, status))


def _check_enqueued(results):
    for c, slot, sizes, status in results:
        host = slot.cpu().numpy()
        assert status.cpu().tolist() == [0] and sizes.cpu().tolist() == [len(host) - 2 * G], c["name"]
        assert K.equals_pin(c["name"], host[G:-G].tobytes()), _report(c, host[G:-G].tobytes())
        assert (host[:G] == GUARD).all() and (host[-G:] == GUARD).all(), c["name"]


@pytest.mark.parametrize("two_streams", [False, True], ids=["one stream", "two streams in turn"])
def test_more_calls_in_flight_than_the_staging_ring_holds(torch, on_device, two_streams):
    """Nine calls without a synchronisation between them: the ring has four page-locked buffers, so the fifth call and those
    behind it reuse one, after its copy. Each stream first gets some tens of milliseconds of other work, so that the calls are enqueued
    while the copies of the first ones still wait: the calls' files tell whether a buffer was refilled too early."""
    cs = _ring_cases()
    assert len({c["name"] for c in cs}) == 9
    for c in cs:
        on_device(c)
    ballast = torch.zeros(1 << 26, dtype=torch.float32, device=DEV)  # 256 MB: a pass over it takes a good tenth of a millisecond
    torch.cuda.synchronize(DEV)
    streams = [torch.cuda.Stream(device=DEV) for _ in range(2 if two_streams else 1)]
    results = []
    for s in streams:
        s.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(s):
            for _ in range(200):
                ballast.add_(1.0)
    for k, c in enumerate(cs):
        with torch.cuda.stream(streams[k % len(streams)]):
            _enqueue(torch, on_device, c, results)
    for s in streams:
        s.synchronize()
    _check_enqueued(results)
    for s in streams:
        torch.cuda.current_stream(DEV).wait_stream(s)


def test_views_torch_really_makes(torch):
    """Row pitch 0, channel stride 0, a pixel stride of 4, a row pitch smaller than the pixel stride, a channel slice of an NCHW
    batch and an odd data pointer; the expected file is the restatement's of the same view on the host."""
    rng = np.random.default_rng(23)
    h, w = 37, 53
    row = torch.from_numpy(rng.integers(0, 256, (1, w), dtype=np.uint8)).to(DEV)
    grey = torch.from_numpy(rng.integers(0, 256, (h, w), dtype=np.uint8)).to(DEV)
    rgba = torch.from_numpy(rng.integers(0, 256, (h, w, 4), dtype=np.uint8)).to(DEV)
    wide = torch.from_numpy(rng.integers(0, 256, (w, h, 3), dtype=np.uint8)).to(DEV)
    nchw = torch.from_numpy(rng.integers(0, 256, (3, 4, h, w), dtype=np.uint8)).to(DEV)
    flat = torch.from_numpy(rng.integers(0, 256, (h * w * 3 + 1,), dtype=np.uint8)).to(DEV)
    views = [("row expanded", row.expand(h, w), "HWC", (0, 1)), ("grey expanded to three channels", grey.unsqueeze(2).expand(h, w, 3), "HWC", (w, 1, 0)),
             ("rgba[..., :3]", rgba[..., :3], "HWC", (4 * w, 4, 1)), ("transpose(0, 1)", wide.transpose(0, 1), "HWC", (3, 3 * h, 1)),
             ("channels 1..3 of item 2 of NCHW", nchw[2, 1:4], "CHW", (h * w, w, 1)), ("odd data pointer", flat[1:].view(h, w, 3), "HWC", (3 * w, 3, 1))]
    assert flat[1:].data_ptr() % 2 == 1
    for name, x, layout, strides in views:
        assert tuple(x.stride()) == strides, name
        host = x.cpu().numpy()
        want = E.encode(host if layout == "HWC" else np.ascontiguousarray(host.transpose(1, 2, 0)), 85, "4:2:0", 3)
        files, _, _ = encode_guarded(torch, [x], [len(want)], layout=layout, quality=85, subsampling="4:2:0", restart_interval=3)
        assert files[0] == want, "%s: %s" % (name, where_files_differ(files[0], want))


def _round_trip_cases():
    """The first sweep case of every (grey or subsampling, interval) pair, and of every (subsampling, grey) pair: about 40."""
    picked = {}
    for c in SWEEP:
        picked.setdefault(("grey" if c["grey"] else c["subsampling"], c["restart_interval"]), c)
        picked.setdefault((c["subsampling"], c["grey"]), c)
    return sorted({c["name"]: c for c in picked.values()}.values(), key=lambda c: c["name"]) + [c for c in EDGES if c["content"] == "basis" and c["quality"] == 100 and c["restart_interval"] == 0]


def test_round_trip_through_the_decoder(torch, on_device):
    from tests.libjpeg_ref import libjpeg_rgb

    cs = _round_trip_cases()
    assert 30 <= len(cs) <= 50
    assert {(c["subsampling"], c["grey"]) for c in cs} == {(s, g) for s in K.SUBSAMPLINGS for g in (False, True)}
    assert {c["restart_interval"] for c in cs} == set(K.SWEEP_INTERVALS)
    files = jpeggpu_amd.encode_jpeg([on_device(c) for c in cs], **_params(cs))
    for c, data in zip(cs, files):
        assert K.equals_pin(c["name"], data), _report(c, data)
        rgb = jpeggpu_amd.decode_to_rgb(data, device=DEV)
        assert np.array_equal(rgb.cpu().numpy(), libjpeg_rgb(data)), c["name"]

