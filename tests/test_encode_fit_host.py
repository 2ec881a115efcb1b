"""The host half of encoding to a byte budget: struct jpeggpu_ext_encode_fit_item and the checks of
jpeggpu_ext_encode_fit_batch, the scratch size, the launch formula, and the quality-table header that host and device share
(jpeggpu_amd/csrc/jg_quant.h), compiled with the host compiler alone. No GPU needed."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import jpeggpu_amd
from jpeggpu_amd import Status
from jpeggpu_amd import build as jbuild
from jpeggpu_amd.api import EncodeFitItem, EncodeItem, EncodeStatus, encode_item
from tests import encode_cases as K
from tests import encode_fit_ref as F
from tests import encode_ref as E

CASES = F.cases()


@pytest.fixture(scope="module")
def L():
    jbuild.build()
    return jpeggpu_amd.lib()


def _fit_item(c, max_bytes=1000, lo=None, hi=None, pointers=True):
    f = EncodeFitItem()
    f.item = encode_item(c["w"], c["h"], 1 if c["grey"] else 3, 75, c["subsampling"], c["restart_interval"], c["optimize"])
    if pointers:  # never followed: every call below is refused before anything is enqueued
        f.item.data, f.item.out, f.item.capacity = 256, 512, 64
        f.item.row_pitch, f.item.pixel_stride, f.item.channel_stride = 3 * c["w"], 3, 1
    f.max_bytes, f.quality_min, f.quality_max = max_bytes, c["lo"] if lo is None else lo, c["hi"] if hi is None else hi
    return f


def _call(L, items, scratch=256, size=1 << 40, sizes=256, status=256, quality=256):
    arr = (EncodeFitItem * len(items))(*items)
    return L.jpeggpu_ext_encode_fit_batch(arr, len(items), scratch, size, sizes, status, quality, None)


def test_struct_and_enum():
    assert C.sizeof(EncodeFitItem) == 96 and EncodeFitItem.item.offset == 0 and EncodeFitItem.max_bytes.offset == 80
    assert EncodeFitItem.quality_min.offset == 88 and EncodeFitItem.quality_max.offset == 92
    assert C.sizeof(EncodeItem) == 80, "the existing struct is what it was"
    assert [int(v) for v in EncodeStatus] == [0, 1, 2, 3, 4, 5] and EncodeStatus.OVER_BUDGET == F.OVER_BUDGET == 5
    for name in ("encode_fit_into", "encode_jpeg_fit", "encode_fit_launches", "EncodeStatus"):
        assert hasattr(jpeggpu_amd, name)


def test_argument_checks(L):
    c = CASES[10]
    good = _fit_item(c)
    assert L.jpeggpu_ext_encode_fit_scratch_size((EncodeFitItem * 1)(good), 1) > 0
    for lo, hi in ((0, 50), (1, 101), (51, 50), (-3, -1), (101, 101), (100, 1)):
        bad = _fit_item(c, lo=lo, hi=hi)
        assert _call(L, [good, bad]) == Status.INVALID_ARGUMENT, (lo, hi)
        assert L.jpeggpu_ext_encode_fit_scratch_size((EncodeFitItem * 2)(good, bad), 2) == 0
        assert L.jpeggpu_ext_encode_fit_launches((EncodeFitItem * 2)(good, bad), 2) == 0
    assert _call(L, [good], quality=None) == Status.INVALID_ARGUMENT
    assert _call(L, [good], sizes=None) == Status.INVALID_ARGUMENT
    assert _call(L, [good], status=None) == Status.INVALID_ARGUMENT
    assert _call(L, [good], scratch=None) == Status.INVALID_ARGUMENT
    assert _call(L, [good], size=1024) == Status.INVALID_ARGUMENT, "scratch_size too small"
    assert L.jpeggpu_ext_encode_fit_batch(None, 1, 256, 1 << 40, 256, 256, 256, None) == Status.INVALID_ARGUMENT
    assert L.jpeggpu_ext_encode_fit_batch((EncodeFitItem * 1)(good), 0, 256, 1 << 40, 256, 256, 256, None) == Status.INVALID_ARGUMENT
    # what jpeggpu_ext_encode_batch refuses in an item
    for field, value in (("width", 0), ("height", 65536), ("channels", 2), ("subsampling", 3), ("restart_interval", -1), ("optimize", 2), ("data", None)):
        bad = _fit_item(c)
        setattr(bad.item, field, value)
        assert _call(L, [good, bad]) == Status.INVALID_ARGUMENT, field
    bad = _fit_item(c)
    bad.item.out = None  # a NULL slot with a capacity
    assert _call(L, [bad]) == Status.INVALID_ARGUMENT
    # item.quality is ignored, whatever it holds
    odd = _fit_item(c)
    odd.item.quality = 0
    assert L.jpeggpu_ext_encode_fit_scratch_size((EncodeFitItem * 1)(odd), 1) == L.jpeggpu_ext_encode_fit_scratch_size((EncodeFitItem * 1)(good), 1)


def test_progressive_is_refused(L):
    c = CASES[10]
    good, prog = _fit_item(c), _fit_item(c)
    prog.item.progressive = 1
    assert _call(L, [good, prog]) == Status.NOT_SUPPORTED
    assert L.jpeggpu_ext_encode_fit_scratch_size((EncodeFitItem * 2)(good, prog), 2) == 0
    prog.item.progressive = 2
    assert _call(L, [prog]) == Status.INVALID_ARGUMENT


def test_scratch_size_is_the_plain_size_and_the_transform_and_the_state(L):
    """At least the plain call's size for the same items; beyond it 2 bytes per padded sample and 64 bytes of state per item,
    each part on the plan's 256-byte grid."""
    for items in [[c] for c in CASES[::4]] + [CASES[:12], CASES[12:]]:
        n = len(items)
        fit = (EncodeFitItem * n)(*[_fit_item(c, pointers=False) for c in items])
        plain = (EncodeItem * n)(*[f.item for f in fit])
        for p, c in zip(plain, items):
            p.quality = c["hi"]
        a, b = L.jpeggpu_ext_encode_scratch_size(plain, n), L.jpeggpu_ext_encode_fit_scratch_size(fit, n)
        up = lambda v: -(-v // 256) * 256  # noqa: E731
        blocks = [K.counts(c)["blocks"] for c in items]
        assert 0 < a <= b and b == a + up(64 * n) + sum(up(128 * k) for k in blocks), items[0]["name"]


def test_launch_formula(L):
    """10 + 8 P launches, 12 + 10 P with an `optimize` item, P from the widest range of the call -- whatever n and the sizes."""
    c_std = next(c for c in CASES if not c["optimize"])
    c_opt = next(c for c in CASES if c["optimize"])
    for lo, hi in [(1, 100), (50, 50), (40, 41), (1, 3), (1, 4), (1, 5), (1, 6), (10, 90), (1, 95), (1, 66), (1, 67)]:
        for c in (c_std, c_opt):
            one = (EncodeFitItem * 1)(_fit_item(c, lo=lo, hi=hi))
            assert L.jpeggpu_ext_encode_fit_launches(one, 1) == F.launches(lo, hi, c["optimize"]), (lo, hi)
            assert jpeggpu_amd.encode_fit_launches(c["w"], c["h"], 1 if c["grey"] else 3, 1000, hi, lo, c["subsampling"], c["restart_interval"],
                                                   c["optimize"]) == F.launches(lo, hi, c["optimize"])
    assert F.launches(1, 100, False) == 10 + 8 * 9 and F.launches(1, 100, True) == 12 + 10 * 9 and F.launches(50, 50, False) == 18
    # many items of many sizes: the widest range and one optimised item decide
    big = dict(c_std, w=4000, h=3000)
    items = [_fit_item(c, lo=50, hi=50) for c in CASES if not c["optimize"]] + [_fit_item(big, lo=20, hi=30)]
    assert L.jpeggpu_ext_encode_fit_launches((EncodeFitItem * len(items))(*items), len(items)) == F.launches(20, 30, False)
    items.append(_fit_item(c_opt, lo=60, hi=61))
    assert L.jpeggpu_ext_encode_fit_launches((EncodeFitItem * len(items))(*items), len(items)) == F.launches(20, 30, True)


QUANT_MAIN = r"""
#include "jg_quant.h"
#include <cstdio>
int main()
{
    for (int q = 1; q <= 100; ++q)
        for (int t = 0; t < 2; ++t) {
            for (int i = 0; i < 64; ++i) std::printf("%d ", jg::enc::quantizer(t, q, i));
            std::printf("\n");
        }
    return 0;
}
"""


def test_shared_quality_tables_equal_the_restatement(tmp_path):
    """jg_quant.h through the host compiler, without a HIP header in sight: every quality 1..100, both tables, equal
    encode_ref.quant_table."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    src, exe = tmp_path / "quant_main.cpp", tmp_path / "quant_main"
    src.write_text(QUANT_MAIN)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + jbuild.CSRC, str(src), "-o", str(exe)])
    rows = np.loadtxt(subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE).stdout.decode().splitlines(), dtype=np.int64)
    assert rows.shape == (200, 64)
    for q in range(1, 101):
        assert np.array_equal(rows[2 * (q - 1)], E.quant_table(E.BASE_LUMA, q)), q
        assert np.array_equal(rows[2 * (q - 1) + 1], E.quant_table(E.BASE_CHROMA, q)), q
    assert rows.min() == 1 and rows.max() == 255, "both ends of the clamp are met"
    assert os.path.exists(os.path.join(jbuild.CSRC, "jg_quant.h"))
