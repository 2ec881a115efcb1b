"""The host side of progressive encoding (jg_encode_plan.cpp): the item's layout, argument checks, the header call, the bound
against Pillow's pinned files and the restatement's worst inputs, and that nothing changed for items without the flag. No
device is needed."""
import ctypes as C

import numpy as np
import pytest

import jpeggpu_amd
from jpeggpu_amd import api as A
from tests import encode_cases as K
from tests import encode_prog_ref as R

BY_NAME = {c["name"]: c for c in K.cases()}

# jpeggpu_ext_encode_bound and jpeggpu_ext_encode_scratch_size of single items, optimize 0 and 1, recorded from the commit
# before `progressive` existed, and the scratch size of the call of all six (every other one optimised)
BEFORE = {"37x53_noise_rgb_q95_422_r3|0": [33857, 44288], "37x53_noise_rgb_q95_422_r3|1": [33957, 49408], "real_640x427|0": [2689827, 2386176],
          "real_640x427|1": [2697927, 2391296], "real_640x427_grey_r3|0": [1798894, 1591808], "real_640x427_grey_r3|1": [1804294, 1597184],
          "tile_plus_one_block_r11|0": [107086, 104704], "tile_plus_one_block_r11|1": [107408, 110080], "scan_lanes_plus|0": [13726753, 12118272],
          "scan_lanes_plus|1": [13768097, 12151040], "8x8_noise_rgb_q75_420_bottom|0": [3117, 16384], "8x8_noise_rgb_q75_420_bottom|1": [3125, 21504]}
BEFORE_CALL = 16256256


@pytest.fixture(scope="module")
def lib():
    from jpeggpu_amd import build as jbuild

    jbuild.build()
    return jpeggpu_amd.lib()


def _args(c):
    return (c["w"], c["h"], 1 if c["grey"] else 3, c["quality"], c["subsampling"], c["restart_interval"])


def test_item_layout(lib):
    """`progressive` lies in what was padding: the size and every other offset are what they were."""
    offsets = {name: getattr(A.EncodeItem, name).offset for name, _ in A.EncodeItem._fields_}
    assert C.sizeof(A.EncodeItem) == 80
    assert offsets == dict(data=0, width=8, height=12, channels=16, progressive=20, row_pitch=24, pixel_stride=32, channel_stride=40, quality=48,
                           subsampling=52, restart_interval=56, optimize=60, out=64, capacity=72)


def test_progressive_2_is_refused(lib):
    it = A.encode_item(16, 16, 3, progressive=2)
    size = C.c_size_t(0)
    assert lib.jpeggpu_ext_encode_header(C.byref(it), None, C.byref(size)) == A.Status.INVALID_ARGUMENT
    assert lib.jpeggpu_ext_encode_bound(C.byref(it)) == 0
    assert lib.jpeggpu_ext_encode_scratch_size((A.EncodeItem * 1)(it), 1) == 0
    with pytest.raises(jpeggpu_amd.JpegGpuError):
        jpeggpu_amd.encode_bound(16, 16, 3, progressive=2)


@pytest.mark.parametrize("channels,interval,dhts,scans", [(3, 0, 10, 10), (3, 7, 10, 10), (1, 0, 5, 6), (1, 2, 5, 6)])
def test_header_is_not_supported_with_a_size(lib, channels, interval, dhts, scans):
    """NOT_SUPPORTED, and *size bounds all marker segments of the file: SOI .. SOF2, every DHT at 277 bytes, DRI, every SOS."""
    it = A.encode_item(37, 53, channels, 75, "4:2:0", interval, progressive=True)
    size = C.c_size_t(0)
    assert lib.jpeggpu_ext_encode_header(C.byref(it), None, C.byref(size)) == A.Status.NOT_SUPPORTED
    prefix = 2 + 18 + 69 * (1 if channels == 1 else 2) + 10 + 3 * channels
    sos = 2 * 14 + 8 * 10 if channels == 3 else 6 * 10
    assert size.value == prefix + dhts * 277 + sos + (6 if interval else 0)
    with pytest.raises(jpeggpu_amd.JpegGpuError):
        jpeggpu_amd.encode_header(37, 53, channels, progressive=True)
    # the real marker segments of a file of this geometry fit
    img = np.random.default_rng(3).integers(0, 256, (53, 37) if channels == 1 else (53, 37, 3), dtype=np.uint8)
    data = R.encode(img, 75, "4:2:0", interval)
    markers, at = 2, 2
    while data[at:at + 2] != b"\xff\xd9":
        if data[at] == 0xFF and data[at + 1] not in (0x00, 0xFF) and not 0xD0 <= data[at + 1] <= 0xD7:
            n = 2 + int.from_bytes(data[at + 2:at + 4], "big")
            markers += n
            at += n
        else:
            at += 1
    assert markers <= size.value


def test_bound_covers_every_pin_and_the_worst_inputs(lib):
    pins = R.pins()[0]
    for c in K.cases() + [c for c, _ in R.edge_cases()]:
        assert jpeggpu_amd.encode_bound(*_args(c), progressive=True) >= pins[c["name"]]["length"], c["name"]
    binary = R.edge_cases()[7]
    assert binary[0]["name"] == "prog_binary_256_grey_q100"
    assert jpeggpu_amd.encode_bound(*_args(binary[0]), progressive=True) >= len(R.encode(binary[1], 100, "4:4:4", 0)) == 75909
    rgb = np.random.default_rng(2).integers(0, 2, (96, 96, 3), dtype=np.uint8) * 255
    for interval in (0, 1):
        assert jpeggpu_amd.encode_bound(96, 96, 3, 100, "4:4:4", interval, progressive=True) >= len(R.encode(rgb, 100, "4:4:4", interval))


def test_items_without_the_flag_are_what_they_were(lib):
    cs = []
    for key, (bound, scratch) in BEFORE.items():
        name, opt = key.split("|")
        c = BY_NAME[name]
        it = A.encode_item(*_args(c), optimize=int(opt))
        assert lib.jpeggpu_ext_encode_bound(C.byref(it)) == bound, key
        assert lib.jpeggpu_ext_encode_scratch_size((A.EncodeItem * 1)(it), 1) == scratch, key
        if c not in cs:
            cs.append(c)
    items = (A.EncodeItem * len(cs))(*[A.encode_item(*_args(c), optimize=i % 2) for i, c in enumerate(cs)])
    assert lib.jpeggpu_ext_encode_scratch_size(items, len(cs)) == BEFORE_CALL
    # `optimize` is ignored for a progressive item
    a, b = (A.encode_item(*_args(cs[0]), optimize=o, progressive=True) for o in (0, 1))
    assert lib.jpeggpu_ext_encode_bound(C.byref(a)) == lib.jpeggpu_ext_encode_bound(C.byref(b)) > BEFORE["37x53_noise_rgb_q95_422_r3|1"][0]
    assert lib.jpeggpu_ext_encode_scratch_size((A.EncodeItem * 1)(a), 1) == lib.jpeggpu_ext_encode_scratch_size((A.EncodeItem * 1)(b), 1)
