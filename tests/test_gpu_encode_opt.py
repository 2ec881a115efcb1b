"""Encoding with optimised Huffman tables on the device (optimize=True; count_symbols and build_tables of jg_encode.hip):
jpeg_gen_optimal_table through jpeggpu_ext_encode_tables_from_counts against the restatement, every case of
tests/encode_cases.py and the edge images of tests/encode_opt_ref.py against Pillow's pinned optimize=True files, calls that
mix both kinds of item, slots that are too small, calls in flight. Every output slot lies between guard bytes."""
import numpy as np
import pytest

import jpeggpu_amd
from tests import encode_cases as K
from tests import encode_diff as D
from tests import encode_opt_ref as R
from tests import encode_ref as E

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


def _batch_params(cs, optimize):
    return dict(quality=[c["quality"] for c in cs], subsampling=[c["subsampling"] for c in cs], restart_interval=[c["restart_interval"] for c in cs],
                optimize=optimize)


def _bound(c, optimize=True):
    return jpeggpu_amd.encode_bound(c["w"], c["h"], 1 if c["grey"] else 3, c["quality"], c["subsampling"], c["restart_interval"], optimize=optimize)


@pytest.fixture(scope="module")
def images(torch):
    """Every case's and every edge image's pixels on the device, by name, and the host arrays."""
    host = {c["name"]: K.image(c) for c in CASES}
    host.update({c["name"]: img for c, img in EDGES})
    return {name: torch.from_numpy(a).to(DEV) for name, a in host.items()}, host


def _why(c, host, got):
    """On a mismatch: whether the coefficients differ (encode_blocks) or what lies behind them (the new kernels, the header)."""
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


# ------------------------------------------------------------------------------------------------
# jpeg_gen_optimal_table alone
# ------------------------------------------------------------------------------------------------

def _crafted():
    one = np.zeros(256, np.int64)
    one[0x21] = 5
    two = np.zeros(256, np.int64)
    two[[3, 9]] = 5
    ties = np.zeros(256, np.int64)
    ties[[10, 20, 30, 40]] = [1, 1, 2, 2]
    last = np.zeros(256, np.int64)
    last[255] = 1
    return [("one symbol", one), ("two equal", two), ("256 equal", np.full(256, 7, np.int64)), ("fibonacci 20", R.fib_counts(20)),
            ("fibonacci 32", R.fib_counts(32)), ("fibonacci 33", R.fib_counts(33)), ("merged sums tie", ties), ("all zero", np.zeros(256, np.int64)),
            ("symbol 255 alone", last), ("the largest counts", np.full(256, (10 ** 9 - 1) // 256, np.int64)),
            ("a count of 2^28", np.where(np.arange(256) == 7, 1 << 28, 1)), ("a sum of 10^9", np.full(256, 10 ** 9 // 256 + 1, np.int64))]


def _seeded(n=200):
    rng = np.random.default_rng(31337)
    out = []
    for i in range(n):
        k = int(rng.integers(1, 257)) if i % 10 else (1, 2, 256, 255, 17, 33, 64, 65, 128, 129)[i // 10 % 10]
        c = np.zeros(256, np.int64)
        idx = rng.choice(256, k, replace=False)
        kind = i % 3
        if kind == 0:  # geometric: deep codes, length limiting
            c[idx] = np.maximum(1, (rng.integers(1, 1 << 20) * 0.5 ** (np.arange(k) * rng.uniform(0.3, 1.2))).astype(np.int64))
        elif kind == 1:  # flat: every choice of the two least is a tie
            c[idx] = int(rng.integers(1, 1000))
        else:  # sparse small counts: ties between symbols and merged sums
            c[idx] = rng.integers(1, 4, k)
        out.append(("seeded %d (%s, %d symbols)" % (i, ("geometric", "flat", "sparse")[kind], k), c))
    return out


def test_tables_from_counts(torch):
    """One call on the crafted counts and 200 seeded tables: bits and values are libjpeg's, a code longer than 32 bits reports
    status 2, an empty table and counts beyond libjpeg's range status 3, and their neighbours in the call are right."""
    tables = _crafted() + _seeded()
    counts = torch.from_numpy(np.stack([c for _, c in tables]).astype(np.int32)).to(DEV)
    out, status = jpeggpu_amd.encode_tables_from_counts(counts)
    out, status = out.cpu().numpy(), status.cpu().tolist()
    assert out.shape == (len(tables), 272)
    seen, limited, wrong = set(), 0, []
    for (name, c), row, st in zip(tables, out, status):
        bits, values, want = R.gen_optimal_table(c)
        seen.add(want)
        if want == R.OK:
            limited += R.depth_before_limiting(c) > 16
            ok = st == 0 and row[:16].tolist() == bits and row[16:16 + len(values)].tolist() == values and not row[16 + len(values):].any()
        else:
            ok = st == want and not row.any()
        if not ok:
            wrong.append("%s: status %d, expected %d" % (name, st, want))
    assert not wrong, "\n".join(wrong[:20])
    assert seen == {R.OK, R.OVERFLOW, R.EMPTY} and limited >= 5
    by_name = dict(zip((n for n, _ in tables), status))
    assert by_name["fibonacci 33"] == 2 and by_name["fibonacci 32"] == 0 and by_name["all zero"] == 3
    assert by_name["a count of 2^28"] == 3 and by_name["a sum of 10^9"] == 3 and by_name["the largest counts"] == 0
    with pytest.raises(ValueError):
        jpeggpu_amd.encode_tables_from_counts(counts.long())
    with pytest.raises(ValueError):
        jpeggpu_amd.encode_tables_from_counts(counts[:, :255])


# ------------------------------------------------------------------------------------------------
# files
# ------------------------------------------------------------------------------------------------

def test_every_case_equals_its_optimised_pin(torch, images):
    """All cases in ONE encode_jpeg call."""
    dev, host = images
    got = jpeggpu_amd.encode_jpeg([dev[c["name"]] for c in CASES], **_batch_params(CASES, True))
    wrong = [c for c, f in zip(CASES, got) if not R.equals_pin(c["name"], f)]
    assert not wrong, "%d of %d cases differ from Pillow's optimize=True:\n%s" % (
        len(wrong), len(CASES), "\n".join(_why(c, host, got[CASES.index(c)]) for c in wrong[:8]))
    plain = K.pins()[0]
    assert all(len(f) < plain[c["name"]]["length"] for c, f in zip(CASES, got))


@pytest.mark.parametrize("index", range(len(EDGES)), ids=[c["name"] for c, _ in EDGES])
def test_edge_image(torch, images, index):
    """Single-symbol tables, the pseudo-symbol beside one code, counts summed over two tiles with a restart across the tile
    edge, a DC reset in every MCU, length limiting of an 18-bit code: each alone, into a slot of exactly the pinned length."""
    dev, host = images
    c = EDGES[index][0]
    pin = R.pins()[0][c["name"]]
    files, sizes, status = encode_guarded(torch, [dev[c["name"]]], [pin["length"]], optimize=True, **_params(c))
    assert status == [0] and sizes == [pin["length"]]
    assert R.equals_pin(c["name"], files[0]), _why(c, host, files[0])
    if c["name"] == "opt_two_tiles_136x136_grey_r3":
        assert K.counts(c)["tiles"] == 2 and K.TILE_BLOCKS % c["restart_interval"], "a restart segment lies across the tile edge"


def _mixed():
    """Sixteen items, every other one with the flag: the geometry cases (every size of encode_cases.SIZES, RGB and grey), the
    two-tile edge image with the flag and a two-tile case without."""
    cs = [c for c in CASES if c["name"].startswith("geometry_")]
    assert len(cs) == 2 * len(K.SIZES) == 14
    cs += [EDGES[2][0], next(c for c in CASES if c["name"] == "tile_plus_one_block")]
    return cs, [i % 2 == 0 for i in range(len(cs))]


@pytest.mark.parametrize("reverse", [False, True], ids=["in order", "reversed"])
def test_mixed_call(torch, images, reverse):
    dev, host = images
    cs, flags = _mixed()
    if reverse:
        cs, flags = cs[::-1], flags[::-1]
    files, sizes, status = encode_guarded(torch, [dev[c["name"]] for c in cs], [_bound(c, f) for c, f in zip(cs, flags)], **_batch_params(cs, flags))
    assert status == [0] * len(cs)
    for c, f, data in zip(cs, flags, files):
        if f:
            assert R.equals_pin(c["name"], data), "optimised " + _why(c, host, data)
        else:
            assert K.equals_pin(c["name"], data), "standard %s: %s" % (c["name"], D.where_files_differ(data, E.encode(host[c["name"]], **_params(c))))


def test_capacity(torch, images):
    """A slot one byte short of the optimised file: status 1, the size it needs, not a byte written (encode_guarded checks the
    fill); its neighbours are written. encode_jpeg_to_device with slots of one byte retries every item."""
    dev, host = images
    cs = [c for c in CASES if c["name"] in ("37x53_noise_rgb_q95_422_r3", "rst_wrap_37x53", "zrl_sparse_rgb")]
    assert len(cs) == 3
    lengths = [R.pins()[0][c["name"]]["length"] for c in cs]
    caps = [lengths[0], lengths[1] - 1, lengths[2]]
    files, sizes, status = encode_guarded(torch, [dev[c["name"]] for c in cs], caps, **_batch_params(cs, True))
    assert status == [0, 1, 0] and sizes == lengths
    assert files[1] is None and R.equals_pin(cs[0]["name"], files[0]) and R.equals_pin(cs[2]["name"], files[2])
    buf, offsets, sizes = jpeggpu_amd.encode_jpeg_to_device([dev[c["name"]] for c in cs], capacities=1, **_batch_params(cs, True))
    assert sizes == lengths
    data = buf.cpu().numpy()
    for c, o, n in zip(cs, offsets, sizes):
        assert R.equals_pin(c["name"], data[o:o + n].tobytes()), c["name"]


def test_calls_in_flight(torch, images):
    """Nine optimised calls queued on one stream, each with its own scratch -- more than the ring of four staging buffers --
    and nothing read before one synchronise."""
    dev, host = images
    names = ["real_640x427", "opt_two_tiles_136x136_grey_r3", "37x53_noise_rgb_q95_422_r3", "real_640x427_grey_r3", "opt_33x17_rgb_420_r1",
             "zrl_sparse_rgb", "opt_flat_16x16_rgb", "real_640x427", "opt_fibonacci_664_grey"]
    by_name = {c["name"]: c for c in CASES + [c for c, _ in EDGES]}
    pins = R.pins()[0]
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    results = []
    with torch.cuda.stream(stream):
        for name in names:
            slot = torch.full((pins[name]["length"] + 2 * G,), GUARD, dtype=torch.uint8, device=DEV)
            results.append((name, slot, jpeggpu_amd.encode_into([dev[name]], [slot[G:-G]], optimize=True, **_params(by_name[name]))))
    stream.synchronize()
    for name, slot, (sizes, status) in results:
        data = slot.cpu().numpy()
        assert status.cpu().tolist() == [0] and sizes.cpu().tolist() == [len(data) - 2 * G], name
        assert R.equals_pin(name, data[G:-G].tobytes()), name
        assert (data[:G] == GUARD).all() and (data[-G:] == GUARD).all()
    torch.cuda.current_stream(DEV).wait_stream(stream)


def test_arguments(torch, images):
    dev, _ = images
    x = dev["8x8_noise_rgb_q75_420_bottom"]
    with pytest.raises(ValueError):
        jpeggpu_amd.encode_jpeg([x, x], optimize=[True])
    with pytest.raises(jpeggpu_amd.JpegGpuError):
        jpeggpu_amd.encode_jpeg([x], optimize=2)
    assert jpeggpu_amd.encode_jpeg([x, x], optimize=[False, True]) == [jpeggpu_amd.encode_jpeg([x])[0], jpeggpu_amd.encode_jpeg([x], optimize=True)[0]]
