"""The encoder's seeded case list: geometry, content and parameters of every pinned file. No image is stored: image(case)
regenerates it. tools/make_encode_pins.py runs Pillow on the list (tests/golden/encode_pins.npz); tests/test_encode_ref.py
checks the restatement against the pins and that the list covers what it must; tests/test_gpu_encode.py runs the device.

The sizes are the smallest at which each stage can go wrong: single blocks and partial MCUs, dummy blocks at either edge and
in the corner, one block more than a tile of the block kernels, a few bytes more than a chunk of the byte kernels, more
tiles and chunks than the scans have lanes, and one ordinary 640 x 427 image.

Beside that list stand the inputs of tests/test_gpu_encode_scale.py, pinned in tests/golden/encode_sweep_pins.npz by length and
SHA-256 (tools/make_encode_pins.py --sweep): a seeded sweep of small geometries and parameters (sweep), images at the
arithmetic edges of the block kernel (edge_cases), a few images of several tiles (medium) and the two big calls built from
them: many_call, whose tile scan composes runs with item boundaries inside, and grid_call, whose chunks outnumber the grid of
the byte kernels. counts() restates an item's tiles and chunks, so that the host tests can assert that structure."""
import hashlib
import itertools
import json
import os

import numpy as np

# what jg_encode.hpp calls kTileBlocks, kChunkBytes, kScanThreads
TILE_BLOCKS = 256
CHUNK_BYTES = 8192
SCAN_THREADS = 128
# the literal in launch_encode: the byte kernels are launched with min(chunks, CHUNK_GRID) workgroups and stride over the rest
CHUNK_GRID = 4096
MAX_BLOCK_BITS = 1660  # kMaxBlockBits

SIZES = [(1, 1), (8, 8), (3, 19), (37, 53), (40, 8), (33, 17), (16, 16)]  # (h, w)
QUALITIES = [1, 30, 75, 95, 100]
SUBSAMPLINGS = ["4:4:4", "4:2:2", "4:2:0"]
INTERVALS = [0, 1, 3, 11]


def _case(name, h, w, grey, content, quality, subsampling, restart_interval, seed=0):
    return dict(name=name, h=h, w=w, grey=grey, content=content, quality=quality, subsampling=subsampling, restart_interval=restart_interval, seed=seed)


def cases():
    out = []
    combos = list(itertools.product(SIZES, ("noise", "gradient"), (False, True)))
    for idx, ((h, w), content, grey) in enumerate(combos):
        for t in range(4):  # every size, content and colour with four of the parameter triples, rotating through all values
            q, s, r = QUALITIES[(idx + t) % 5], SUBSAMPLINGS[(idx // 2 + t) % 3], INTERVALS[(idx // 4 + 3 * t) % 4]
            out.append(_case("%dx%d_%s_%s_q%d_%s_r%d" % (h, w, content, "grey" if grey else "rgb", q, s.replace(":", ""), r), h, w, grey, content, q, s, r, seed=idx))
    # the 4:2:0 bottom rule on even heights that are no multiple of 16, at every quality
    for q in QUALITIES:
        out.append(_case("8x8_noise_rgb_q%d_420_bottom" % q, 8, 8, False, "noise", q, "4:2:0", 0, seed=100 + q))
    out.append(_case("40x8_noise_rgb_q75_420_bottom", 40, 8, False, "noise", 75, "4:2:0", 1, seed=106))
    # symbols at the ends of the tables
    out.append(_case("dc11_black_white_blocks", 16, 64, True, "black_white_blocks", 100, "4:4:4", 0))
    out.append(_case("dc11_black_white_blocks_rgb", 16, 48, False, "black_white_blocks", 100, "4:2:2", 3))
    out.append(_case("ac10_checkerboard", 16, 24, True, "checkerboard", 100, "4:4:4", 0))
    out.append(_case("ac10_checkerboard_rgb", 24, 24, False, "checkerboard", 100, "4:4:4", 1))
    out.append(_case("zrl_sparse", 32, 40, True, "sparse", 75, "4:4:4", 0, seed=7))
    out.append(_case("zrl_sparse_rgb", 24, 40, False, "sparse", 90, "4:2:0", 3, seed=8))
    # a restart counter that wraps several times, with segments that end in a stuffed padding byte
    out.append(_case("rst_wrap_37x53", 37, 53, False, "noise", 95, "4:2:0", 1, seed=11))
    out.append(_case("rst_wrap_grey_24x200", 24, 200, True, "noise", 100, "4:4:4", 1, seed=12))
    # one block more than a tile of the block kernels
    out.append(_case("tile_plus_one_block", 8, 8 * (TILE_BLOCKS + 1), True, "noise", 75, "4:4:4", 0, seed=13))
    out.append(_case("tile_plus_one_block_r11", 8, 8 * (TILE_BLOCKS + 1), True, "gradient", 30, "4:4:4", 11, seed=14))
    # a few bytes more than a chunk of the byte kernels (CHUNK_BYTES of unstuffed stream; the test asserts the length)
    out.append(_case("chunk_plus_few_bytes", 8, 650, True, "noise", 100, "4:4:4", 0, seed=15))
    # more tiles than the tile scan has lanes and more chunks than the chunk scan has: lanes own runs of two and more
    out.append(_case("scan_lanes_plus", 840, 840, False, "noise", 97, "4:4:4", 0, seed=16))
    out.append(_case("scan_lanes_plus_420_r11", 600, 1000, False, "noise", 100, "4:2:0", 11, seed=17))
    # for the header: every quality on one geometry, and every geometry at quality 75
    for q in range(1, 101):
        out.append(_case("qsweep_q%d" % q, 8, 8, False, "gradient", q, "4:2:0", 0, seed=20))
    for idx, ((h, w), grey) in enumerate(itertools.product(SIZES, (False, True))):
        out.append(_case("geometry_%dx%d_%s_q75" % (h, w, "grey" if grey else "rgb"), h, w, grey, "noise", 75, SUBSAMPLINGS[idx % 3], INTERVALS[idx % 4], seed=30 + idx))
    # an ordinary image
    out.append(_case("real_640x427", 427, 640, False, "photo", 75, "4:2:0", 0, seed=18))
    out.append(_case("real_640x427_grey_r3", 427, 640, True, "photo", 90, "4:2:0", 3, seed=19))
    return out


SWEEP_COUNT = 600
SWEEP_SEED = 20240
SWEEP_INTERVALS = [0, 1, 2, 3, 5, 7, 8, 64, 65535]
SWEEP_CONTENTS = ["noise", "two_level", "near_flat"]


def sweep():
    """SWEEP_COUNT seeded cases: h and w in 1..49, grey or RGB, the three subsamplings, quality 1..100, an interval of
    SWEEP_INTERVALS, one of SWEEP_CONTENTS. tests/test_encode_ref.py asserts what the draw covers."""
    rng = np.random.default_rng(SWEEP_SEED)
    out = []
    for i in range(SWEEP_COUNT):
        h, w = (int(v) for v in rng.integers(1, 50, 2))
        grey = bool(rng.integers(0, 2))
        s = SUBSAMPLINGS[int(rng.integers(0, 3))]
        q = int(rng.integers(1, 101))
        r = SWEEP_INTERVALS[int(rng.integers(0, len(SWEEP_INTERVALS)))]
        content = SWEEP_CONTENTS[int(rng.integers(0, 3))]
        out.append(_case("sweep_%03d_%dx%d_%s_%s_q%d_%s_r%d" % (i, h, w, content, "grey" if grey else "rgb", q, s.replace(":", ""), r), h, w, grey, content, q, s, r, seed=5000 + i))
    return out


LATTICE_LEVELS = [0, 1, 16, 32, 48, 64, 80, 96, 112, 127, 128, 129, 144, 160, 176, 192, 208, 224, 240, 254, 255]
LATTICE_SIDE = 776  # 97 x 97 blocks, the first 21^3 of them one colour each


def basis_image(h=64, w=128):
    """One 8 x 8 block per basis function cos((2x+1)u pi/16) cos((2y+1)v pi/16) and sign: 255 where the function is positive
    and 0 elsewhere in blocks 0..63 (u = n // 8, v = n % 8), the inverse in blocks 64..127; 16 blocks a row. Every
    coefficient meets its largest value of either sign. The RGB image's channels are this, this rolled by one block, and
    its inverse."""
    assert (h, w) == (64, 128)
    k = np.arange(8)
    img = np.zeros((h, w), np.uint8)
    for n in range(128):
        u, v = divmod(n % 64, 8)
        f = np.cos((2 * k[None, :] + 1) * u * np.pi / 16) * np.cos((2 * k[:, None] + 1) * v * np.pi / 16)  # never 0: (2x+1)u is no odd multiple of 8
        by, bx = divmod(n, 16)
        img[8 * by:8 * by + 8, 8 * bx:8 * bx + 8] = np.where((f > 0) == (n < 64), 255, 0)
    return np.stack([img, np.roll(img, 8, axis=1), 255 - img], -1)


def lattice_image(h=LATTICE_SIDE, w=LATTICE_SIDE):
    """One flat 8 x 8 block per colour: block n (row by row) has R, G, B = LATTICE_LEVELS[n // 441 % 21], [n // 21 % 21],
    [n % 21]; the blocks behind the 9261st begin again."""
    assert h % 8 == 0 and w % 8 == 0 and (h // 8) * (w // 8) >= len(LATTICE_LEVELS) ** 3
    levels = np.asarray(LATTICE_LEVELS, np.uint8)
    n = np.arange((h // 8) * (w // 8)).reshape(h // 8, w // 8)
    blocks = np.stack([levels[n // 441 % 21], levels[n // 21 % 21], levels[n % 21]], -1)
    return np.repeat(np.repeat(blocks, 8, 0), 8, 1)


def edge_cases():
    """The block kernel's arithmetic edges: the basis-pattern image, grey and RGB, and the colour lattice."""
    out = []
    for q in (100, 99, 50, 1):
        for r in (0, 1):
            out.append(_case("basis_grey_q%d_r%d" % (q, r), 64, 128, True, "basis", q, "4:4:4", r))
            for s in SUBSAMPLINGS:
                out.append(_case("basis_rgb_q%d_%s_r%d" % (q, s.replace(":", ""), r), 64, 128, False, "basis", q, s, r))
    for s in SUBSAMPLINGS:
        out.append(_case("lattice_q100_%s" % s.replace(":", ""), LATTICE_SIDE, LATTICE_SIDE, False, "lattice", 100, s, 0))
    return out


def medium():
    """Images of 2..12 tiles, for between the one-tile items of many_call."""
    spec = [(104, 200, False, "noise", 90, "4:2:0", 5), (200, 160, True, "photo", 75, "4:4:4", 0), (240, 250, False, "photo", 85, "4:4:4", 7),
            (131, 257, False, "noise", 100, "4:2:2", 1), (255, 101, False, "two_level", 50, "4:2:0", 64), (180, 180, False, "gradient", 30, "4:4:4", 0),
            (150, 220, False, "near_flat", 95, "4:2:0", 3), (256, 256, False, "noise", 60, "4:2:2", 8)]
    return [_case("medium_%d_%dx%d_%s_%s_q%d_%s_r%d" % (i, h, w, c, "grey" if g else "rgb", q, s.replace(":", ""), r), h, w, g, c, q, s, r, seed=7000 + i)
            for i, (h, w, g, c, q, s, r) in enumerate(spec)]


def grid_images():
    """The distinct 256 x 256 items of grid_call: noise at quality 100 with an interval of 1 and of 0 (streams of many chunks,
    stuffed bytes, markers), the same under 4:2:0, a smooth image and a grey one."""
    spec = [("noise_r1", False, "noise", 100, "4:4:4", 1), ("noise_r0", False, "noise", 100, "4:4:4", 0), ("noise_420_r1", False, "noise", 100, "4:2:0", 1),
            ("smooth", False, "photo", 75, "4:2:0", 0), ("grey", True, "noise", 90, "4:4:4", 3)]
    return [_case("grid_256_%s" % name, 256, 256, g, c, q, s, r, seed=8000 + i) for i, (name, g, c, q, s, r) in enumerate(spec)]


def counts(case):
    """What jg_encode_plan.cpp plans for an item: blocks, restart segments, tiles of the block kernels, the worst-case bound of
    its unstuffed stream and the chunks of the byte kernels that cover it."""
    hs, vs = (1, 1) if case["grey"] else {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}[case["subsampling"]]
    mcus_x, mcus_y = -(-case["w"] // (8 * hs)), -(-case["h"] // (8 * vs))
    mcus = mcus_x * mcus_y
    blocks = mcus * (1 if case["grey"] else hs * vs + 2)
    ri = case["restart_interval"]
    segments = -(-mcus // ri) if ri else 1
    stream_bound = -(-blocks * MAX_BLOCK_BITS // 8) + segments
    return dict(mcus_x=mcus_x, mcus=mcus, blocks=blocks, segments=segments, tiles=-(-blocks // TILE_BLOCKS), stream_bound=stream_bound,
                chunks=-(-stream_bound // CHUNK_BYTES))


def starts(items, what):
    """The first tile (what="tiles") or chunk ("chunks") of every item of a call, and the call's total behind them."""
    out, at = [], 0
    for c in items:
        out.append(at)
        at += counts(c)[what]
    return out + [at]


def many_call(reverse=False):
    """The whole sweep, every item one tile, with the medium() items at seeded places: the tile scan's lanes own runs of
    several tiles, item boundaries fall inside the runs, and run boundaries inside the larger items."""
    items = sweep()
    rng = np.random.default_rng(SWEEP_SEED + 1)
    for c, at in zip(medium(), sorted(int(v) for v in rng.integers(0, len(items), len(medium())))):
        items.insert(at, c)
    return items[::-1] if reverse else items


def grid_call():
    """About 60 items of 256 x 256 with more than CHUNK_GRID chunks: dict(items, short, zero) -- the call's cases in order, the
    indices of the two items whose slot is a byte too small (one in front of chunk CHUNK_GRID, one whose chunks all lie
    behind it) and of the item whose slot has capacity 0. The last items lie wholly behind the grid: one with restart markers
    and stuffed bytes, the one with the short slot, a smooth one and a grey one."""
    noise_r1, noise_r0, noise_420, smooth, grey = grid_images()
    front = [noise_r1, noise_r0, noise_420, smooth, grey] + [noise_r0, noise_r1] * 25  # 260 + 50 * 78 chunks: the last one straddles the grid's end
    tail = [noise_r1, noise_r0, smooth, grey, noise_420, noise_r1]
    return dict(items=front + tail, short=(9, len(front) + 1), zero=len(front) + 5)


def image(case):
    """The case's pixels: H x W x 3 or H x W uint8."""
    h, w = case["h"], case["w"]
    rng = np.random.default_rng(1000 + case["seed"])
    yy, xx = np.mgrid[0:h, 0:w]
    kind = case["content"]
    if kind == "noise":
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    elif kind == "gradient":
        a = np.stack([(xx * 5 + yy) % 256, (yy * 7 + 3 * xx) % 256, ((xx + yy) * 3) % 256], -1).astype(np.uint8)
    elif kind == "black_white_blocks":  # neighbouring blocks at the two ends of the range: DC differences of category 11
        a = np.repeat((((xx // 8) + (yy // 8)) % 2 * 255)[..., None], 3, -1).astype(np.uint8)
    elif kind == "checkerboard":  # the highest frequency at full swing: an AC coefficient of category 10
        a = np.repeat((((xx + yy) % 2) * 255)[..., None], 3, -1).astype(np.uint8)
    elif kind == "sparse":  # flat blocks with single high-frequency dots: long zero runs in front of late coefficients
        a = np.full((h, w, 3), 128, np.uint8)
        dots = rng.random((h, w)) < 0.02
        a[dots] = rng.integers(0, 256, (int(dots.sum()), 3), dtype=np.uint8)
    elif kind == "photo":  # smooth shapes, an edge or two and some noise, in integers only: a photograph's statistics, roughly
        tri = lambda t, period: np.abs(t % period - period // 2)  # noqa: E731
        base = 40 + tri(3 * xx + yy, 397) // 2 + tri(2 * yy - xx, 151) + 40 * ((xx // 97 + yy // 61) % 2)
        noise = rng.integers(-6, 7, (h, w, 3))
        a = np.clip(np.stack([base, (4 * base) // 5 + 20, 255 - base], -1) + noise, 0, 255).astype(np.uint8)
    elif kind == "two_level":  # two seeded levels, chosen per sample
        lo, hi = rng.integers(0, 256, 2)
        a = np.where(rng.random((h, w, 3)) < 0.5, lo, hi).astype(np.uint8)
    elif kind == "near_flat":  # a seeded colour and a little noise: coefficients around the quantiser's rounding
        a = np.clip(rng.integers(0, 256, 3) + rng.integers(-2, 3, (h, w, 3)), 0, 255).astype(np.uint8)
    elif kind == "basis":
        a = basis_image(h, w)
    elif kind == "lattice":
        a = lattice_image(h, w)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(a[..., 0]) if case["grey"] else a


_pins = None


def pins():
    """{case name: dict(length, sha256, data or None)} and the recorded versions, from tests/golden/encode_pins.npz."""
    global _pins
    if _pins is None:
        z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encode_pins.npz"))
        meta = json.loads(z["meta"].tobytes().decode())
        table = {}
        for e in meta["cases"]:
            table[e["name"]] = dict(length=e["length"], sha256=e["sha256"], data=z["file_" + e["name"]].tobytes() if e["whole"] else None)
        _pins = (table, {k: v for k, v in meta.items() if k != "cases"})
    return _pins


def new_cases():
    """Every case pinned in tests/golden/encode_sweep_pins.npz."""
    return sweep() + edge_cases() + medium() + grid_images()


_sweep_pins = None


def sweep_pins():
    """pins() of tests/golden/encode_sweep_pins.npz, which holds no whole files: every `data` is None."""
    global _sweep_pins
    if _sweep_pins is None:
        z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encode_sweep_pins.npz"))
        meta = json.loads(z["meta"].tobytes().decode())
        table = {e["name"]: dict(length=e["length"], sha256=e["sha256"], data=None) for e in meta["cases"]}
        _sweep_pins = (table, {k: v for k, v in meta.items() if k != "cases"})
    return _sweep_pins


def pin_of(name):
    """The pin of a case of either list."""
    return pins()[0][name] if name in pins()[0] else sweep_pins()[0][name]


def equals_pin(name, data):
    """Whether `data` is the pinned file: its bytes where the pin holds them, its length and SHA-256 otherwise."""
    pin = pin_of(name)
    if pin["data"] is not None:
        return data == pin["data"]
    return len(data) == pin["length"] and hashlib.sha256(data).hexdigest() == pin["sha256"]
