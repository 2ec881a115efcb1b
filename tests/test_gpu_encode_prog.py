"""Progressive encoding on the device (progressive=True; jg_encode_prog.hip): every case of tests/encode_cases.py and the edge
images of tests/encode_prog_ref.py against Pillow's pinned progressive=True files, calls that mix baseline, optimised and
progressive items, slots that are too small, calls in flight, and the way back through the decoder. Every output slot lies
between guard bytes."""
import numpy as np
import pytest

import jpeggpu_amd
from tests import encode_cases as K
from tests import encode_diff as D
from tests import encode_opt_ref as O
from tests import encode_prog_ref as R

pytestmark = pytest.mark.gpu

GUARD, G = 0xA5, 64
CASES = K.cases()
EDGES = R.edge_cases()
DEV = "cuda:0"


@pytest.fixture(scope="module")
def torch(gpu_lib):
    import torch

    assert torch.cuda.is_available()
    return torch


def _params(c):
    return dict(quality=c["quality"], subsampling=c["subsampling"], restart_interval=c["restart_interval"])


def _batch_params(cs, **flags):
    return dict(quality=[c["quality"] for c in cs], subsampling=[c["subsampling"] for c in cs], restart_interval=[c["restart_interval"] for c in cs], **flags)


@pytest.fixture(scope="module")
def images(torch):
    """Every case's and every edge image's pixels on the device, by name, and the host arrays."""
    host = {c["name"]: K.image(c) for c in CASES}
    host.update({c["name"]: img for c, img in EDGES})
    host.update({c["name"]: img for c, img in O.edge_cases()})
    return {name: torch.from_numpy(a).to(DEV) for name, a in host.items()}, host


def _why(c, host, got):
    want = R.pins()[0][c["name"]]["data"] or R.encode(host[c["name"]], c["quality"], c["subsampling"], c["restart_interval"])
    return "%s: %s" % (c["name"], D.where_files_differ(got, want))


def encode_guarded(torch, xs, capacities, **params):
    """One jpeggpu_ext_encode_batch call into guarded slots. Returns (files, sizes, status): files[i] the slot's bytes up to its
    reported size, None where status is not 0. Asserts that nothing outside the files was written."""
    offsets, total = [], G
    for cap in capacities:
        offsets.append(total)
        total += cap + G
    buf = torch.full((total,), GUARD, dtype=torch.uint8, device=DEV)
    sizes, status = jpeggpu_amd.encode_into(xs, [buf[o:o + cap] for o, cap in zip(offsets, capacities)], **params)
    sizes, status = sizes.cpu().tolist(), status.cpu().tolist()
    host = buf.cpu().numpy()
    untouched = np.ones(total, bool)
    files = []
    for o, cap, size, st in zip(offsets, capacities, sizes, status):
        assert st == (1 if size > cap else 0)
        if st == 0:
            untouched[o:o + size] = False
        files.append(host[o:o + size].tobytes() if st == 0 else None)
    assert (host[untouched] == GUARD).all(), "bytes outside the files were written"
    return files, sizes, status


def test_every_case_equals_its_progressive_pin(torch, images):
    """All cases in ONE encode_jpeg call. Every progressive file without restart markers is shorter than the baseline one.
    With a restart interval it need not be: every one of the ten scans carries its own markers, and 19 of Pillow's own
    103 pinned files with an interval are longer than their baseline pins (37x53_noise_grey_q1_420_r1: 1042 against 686
    bytes), so for those the comparison with the pin above is the whole statement."""
    dev, host = images
    got = jpeggpu_amd.encode_jpeg([dev[c["name"]] for c in CASES], **_batch_params(CASES, progressive=True))
    wrong = [c for c, f in zip(CASES, got) if not R.equals_pin(c["name"], f)]
    assert not wrong, "%d of %d cases differ from Pillow's progressive=True:\n%s" % (
        len(wrong), len(CASES), "\n".join(_why(c, host, got[CASES.index(c)]) for c in wrong[:8]))
    plain = K.pins()[0]
    longer = [c for c, f in zip(CASES, got) if len(f) >= plain[c["name"]]["length"]]
    assert not [c["name"] for c in longer if c["restart_interval"] == 0]
    assert sum(c["restart_interval"] == 0 for c in CASES) == 144 and len(longer) == 19


@pytest.mark.parametrize("index", range(len(EDGES)), ids=[c["name"] for c, _ in EDGES])
def test_edge_image(torch, images, index):
    """Each edge image alone, into a slot of exactly the pinned length."""
    dev, host = images
    c = EDGES[index][0]
    pin = R.pins()[0][c["name"]]
    files, sizes, status = encode_guarded(torch, [dev[c["name"]]], [pin["length"]], progressive=True, **_params(c))
    assert status == [0] and sizes == [pin["length"]]
    assert R.equals_pin(c["name"], files[0]), _why(c, host, files[0])


def _mixed():
    """Sixteen items, baseline / optimised / progressive in turn: the geometry cases (every size of encode_cases.SIZES, RGB and
    grey), a two-tile edge image and a two-tile case."""
    cs = [c for c in CASES if c["name"].startswith("geometry_")]
    assert len(cs) == 2 * len(K.SIZES) == 14
    cs += [O.edge_cases()[2][0], next(c for c in CASES if c["name"] == "tile_plus_one_block")]
    return cs, [i % 3 for i in range(len(cs))]


def _edge_as_progressive(name):
    """The optimised encoder's two-tile edge image has the pixels of this module's."""
    return "prog_two_tiles_136x136_grey_r3" if name == "opt_two_tiles_136x136_grey_r3" else name


@pytest.mark.parametrize("reverse", [False, True], ids=["in order", "reversed"])
def test_mixed_call(torch, images, reverse):
    dev, host = images
    cs, kinds = _mixed()
    if reverse:
        cs, kinds = cs[::-1], kinds[::-1]
    assert (host["opt_two_tiles_136x136_grey_r3"] == host["prog_two_tiles_136x136_grey_r3"]).all()
    caps = [jpeggpu_amd.encode_bound(c["w"], c["h"], 1 if c["grey"] else 3, c["quality"], c["subsampling"], c["restart_interval"], optimize=k == 1, progressive=k == 2)
            for c, k in zip(cs, kinds)]
    files, sizes, status = encode_guarded(torch, [dev[c["name"]] for c in cs], caps,
                                          **_batch_params(cs, optimize=[k == 1 for k in kinds], progressive=[k == 2 for k in kinds]))
    assert status == [0] * len(cs)
    for c, k, data in zip(cs, kinds, files):
        if k == 2:
            assert R.equals_pin(_edge_as_progressive(c["name"]), data), "progressive " + c["name"]
        elif k == 1:
            assert O.equals_pin(c["name"], data), "optimised " + c["name"]
        else:
            pin = K.pins()[0].get(c["name"])
            assert (K.equals_pin(c["name"], data) if pin else data == O.encode(host[c["name"]], optimize=False, **_params(c))), "standard " + c["name"]


def test_capacity(torch, images):
    """A slot one byte short of the progressive file: status 1, the size it needs, not a byte written (encode_guarded checks
    the fill); its neighbours are written. encode_jpeg_to_device with slots of one byte retries every item."""
    dev, host = images
    cs = [c for c in CASES if c["name"] in ("37x53_noise_rgb_q95_422_r3", "rst_wrap_37x53", "zrl_sparse_rgb")]
    assert len(cs) == 3
    lengths = [R.pins()[0][c["name"]]["length"] for c in cs]
    caps = [lengths[0], lengths[1] - 1, lengths[2]]
    files, sizes, status = encode_guarded(torch, [dev[c["name"]] for c in cs], caps, **_batch_params(cs, progressive=True))
    assert status == [0, 1, 0] and sizes == lengths
    assert files[1] is None and R.equals_pin(cs[0]["name"], files[0]) and R.equals_pin(cs[2]["name"], files[2])
    buf, offsets, sizes = jpeggpu_amd.encode_jpeg_to_device([dev[c["name"]] for c in cs], capacities=1, **_batch_params(cs, progressive=True))
    assert sizes == lengths
    data = buf.cpu().numpy()
    for c, o, n in zip(cs, offsets, sizes):
        assert R.equals_pin(c["name"], data[o:o + n].tobytes()), c["name"]


def test_calls_in_flight(torch, images):
    """Nine progressive calls queued on one stream, each with its own scratch -- more than the ring of four staging buffers --
    and nothing read before one synchronise."""
    dev, host = images
    names = ["real_640x427", "prog_two_tiles_136x136_grey_r3", "37x53_noise_rgb_q95_422_r3", "real_640x427_grey_r3", "prog_33x17_rgb_420_r1",
             "zrl_sparse_rgb", "prog_flat_16x16_rgb", "real_640x427", "prog_binary_256_grey_q100"]
    by_name = {c["name"]: c for c in CASES + [c for c, _ in EDGES]}
    pins = R.pins()[0]
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    results = []
    with torch.cuda.stream(stream):
        for name in names:
            slot = torch.full((pins[name]["length"] + 2 * G,), GUARD, dtype=torch.uint8, device=DEV)
            results.append((name, slot, jpeggpu_amd.encode_into([dev[name]], [slot[G:-G]], progressive=True, **_params(by_name[name]))))
    stream.synchronize()
    for name, slot, (sizes, status) in results:
        data = slot.cpu().numpy()
        assert status.cpu().tolist() == [0] and sizes.cpu().tolist() == [len(data) - 2 * G], name
        assert R.equals_pin(name, data[G:-G].tobytes()), name
        assert (data[:G] == GUARD).all() and (data[-G:] == GUARD).all()
    torch.cuda.current_stream(DEV).wait_stream(stream)


@pytest.mark.parametrize("name", ["real_640x427", "prog_37x53_rgb_420"])
def test_round_trip(torch, images, name):
    """The decoder reads the same pixels from the progressive file as from the optimised one: the coefficients are the same."""
    dev, _ = images
    c = {c["name"]: c for c in CASES + [c for c, _ in EDGES]}[name]
    prog = jpeggpu_amd.encode_jpeg([dev[name]], progressive=True, **_params(c))[0]
    opt = jpeggpu_amd.encode_jpeg([dev[name]], optimize=True, **_params(c))[0]
    assert prog != opt and prog[:2] == b"\xff\xd8" and b"\xff\xc2" in prog[:700]
    a, b = jpeggpu_amd.decode_to_rgb(prog), jpeggpu_amd.decode_to_rgb(opt)
    assert a.shape == b.shape == (c["h"], c["w"], 3) and torch.equal(a, b)


def test_arguments(torch, images):
    dev, _ = images
    x = dev["8x8_noise_rgb_q75_420_bottom"]
    with pytest.raises(ValueError):
        jpeggpu_amd.encode_jpeg([x, x], progressive=[True])
    with pytest.raises(jpeggpu_amd.JpegGpuError):
        jpeggpu_amd.encode_jpeg([x], progressive=2)
    both = jpeggpu_amd.encode_jpeg([x, x, x], progressive=[False, True, True], optimize=[False, False, True])
    assert both[0] == jpeggpu_amd.encode_jpeg([x])[0] and both[1] == both[2] == jpeggpu_amd.encode_jpeg([x], progressive=True)[0]
