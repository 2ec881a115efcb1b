"""The encoder's seeded case list: geometry, content and parameters of every pinned file. No image is stored: image(case)
regenerates it. tools/make_encode_pins.py runs Pillow on the list (tests/golden/encode_pins.npz); tests/test_encode_ref.py
checks the restatement against the pins and that the list covers what it must; tests/test_gpu_encode.py runs the device.

The sizes are the smallest at which each stage can go wrong: single blocks and partial MCUs, dummy blocks at either edge and
in the corner, one block more than a tile of the block kernels, a few bytes more than a chunk of the byte kernels, more
tiles and chunks than the scans have lanes, and one ordinary 640 x 427 image."""
import hashlib
import itertools
import json
import os

import numpy as np

# what jg_encode.hpp calls kTileBlocks, kChunkBytes, kScanThreads
TILE_BLOCKS = 256
CHUNK_BYTES = 8192
SCAN_THREADS = 128

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


def equals_pin(name, data):
    """Whether `data` is the pinned file: its bytes where the pin holds them, its length and SHA-256 otherwise."""
    pin = pins()[0][name]
    if pin["data"] is not None:
        return data == pin["data"]
    return len(data) == pin["length"] and hashlib.sha256(data).hexdigest() == pin["sha256"]
