"""The batched resize as a model's input on the host (jpeggpu_ext_resize_to_tensor): the exported symbol, every refusal --
each returned before anything is staged or enqueued, so with made-up device addresses and without a device -- and the
ctypes mirror of struct jpeggpu_ext_tensor_spec against the header as a C compiler lays it out. No GPU needed."""
import ctypes as C
import math
import os
import subprocess

import pytest

import jpeggpu_amd
from jpeggpu_amd import Status
from jpeggpu_amd import build as jbuild
from jpeggpu_amd.api import TENSOR_TYPE_NAMES, TensorSpec
from tests.test_resize_host import BICUBIC, BILINEAR, FAKE, arr, item

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U8, F32, F16, BF16 = 0, 1, 2, 3
YCBCR, GRAY = 2, 1
IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
INV, NS = Status.INVALID_ARGUMENT, Status.NOT_SUPPORTED


@pytest.fixture(scope="module")
def L():
    jbuild.build()
    return jpeggpu_amd.lib()


def spec(type_=F32, mean=IMAGENET[0], std=IMAGENET[1], flips=None):
    s = TensorSpec()
    s.type = type_
    s.mean[:] = mean
    s.std[:] = std
    if flips is not None:
        s.flips = C.cast((C.c_ubyte * len(flips))(*flips), C.POINTER(C.c_ubyte))
    return s


def ints(v):
    return (C.c_int * len(v))(*v)


def call(L, items, sp, n=None, w=32, h=24, filt=BILINEAR, layout=0, dst=FAKE, scratch=FAKE, size=None, colors=None, orients=None):
    """jpeggpu_ext_resize_to_tensor with fake device addresses; the scratch size is the uint8 call's unless given."""
    n = len(items) if n is None else n
    if size is None:
        size = L.jpeggpu_ext_resize_scratch_size(items, n, w, h, filt) if items is not None else 0
    return L.jpeggpu_ext_resize_to_tensor(items, colors, orients, n, w, h, filt, layout, C.byref(sp) if sp is not None else None, dst, scratch,
                                          size, None)


def good():
    return arr(item(), item(((1, 1),)), item(crop=(3, 5, 20, 17)))


def test_the_library_exports_the_call(L):
    assert hasattr(L, "jpeggpu_ext_resize_to_tensor")
    assert TENSOR_TYPE_NAMES == {"uint8": U8, "float32": F32, "float16": F16, "bfloat16": BF16}


def test_spec_refusals(L):
    """A NULL spec, an unknown type, a zero in std, NaN or an infinity in mean or std: INVALID_ARGUMENT, whatever else the
    call holds -- and nothing is dereferenced on the way (the addresses are made up)."""
    g = good()
    assert call(L, g, None) == INV
    for t in (-1, 4, 99):
        assert call(L, g, spec(t)) == INV
    for t in (F32, F16, BF16):
        for c in range(3):
            std = list(IMAGENET[1])
            std[c] = 0.0
            assert call(L, g, spec(t, std=std)) == INV
            std[c] = -0.0
            assert call(L, g, spec(t, std=std)) == INV
            for bad in (math.nan, math.inf, -math.inf):
                v = list(IMAGENET[1])
                v[c] = bad
                assert call(L, g, spec(t, std=v)) == INV
                v = list(IMAGENET[0])
                v[c] = bad
                assert call(L, g, spec(t, mean=v)) == INV
    # a float destination that does not lie on an element
    assert call(L, g, spec(F32), dst=FAKE + 2) == INV
    assert call(L, g, spec(F16), dst=FAKE + 1) == INV
    assert call(L, g, spec(BF16), dst=FAKE + 3) == INV


def test_the_uint8_calls_refusals_are_kept(L):
    """n <= 0, sizes, the filter, the layout, NULL dst and scratch, a short scratch and the items' own checks behave as in
    jpeggpu_ext_resize_to_rgb, for every type."""
    g = good()
    need = L.jpeggpu_ext_resize_scratch_size(g, 3, 32, 24, BILINEAR)
    assert need > 0
    for t in (U8, F32, F16, BF16):
        sp = spec(t)
        assert call(L, None, sp, n=1) == INV
        assert call(L, g, sp, n=0) == INV
        assert call(L, g, sp, n=-3) == INV
        assert call(L, g, sp, w=0) == INV
        assert call(L, g, sp, h=-1) == INV
        assert call(L, g, sp, filt=2, size=1 << 30) == NS
        assert call(L, g, sp, layout=2) == INV
        assert call(L, g, sp, dst=None) == INV
        assert call(L, g, sp, scratch=None) == INV
        assert call(L, g, sp, size=need - 1) == INV
        assert call(L, g, sp, filt=BICUBIC, size=need) == INV  # the bicubic tables are larger: this scratch is short for them
    sp = spec(F32)
    for bad, want in ((item(((2, 1), (1, 1))), NS), (item(((1, 1),) * 4), NS), (item(((3, 1), (2, 1), (1, 1))), NS),
                      (item(crop=(0, 0, 0, 10)), INV), (item(crop=(-1, 0, 10, 10)), INV)):
        assert call(L, arr(item(), bad), sp, size=1 << 30) == want
    # with colours and orientations: a model that does not fit, an orientation outside 1..8
    two = arr(item(), item(((1, 1),)))
    assert call(L, two, sp, size=1 << 30, colors=ints([YCBCR, YCBCR])) == NS
    assert call(L, two, sp, size=1 << 30, colors=ints([YCBCR, GRAY]), orients=ints([1, 9])) == INV
    assert call(L, two, sp, size=1 << 30, orients=ints([0, 1])) == INV
    # the uint8 type takes any mean and std: they are ignored, so the call gets as far as the scratch check
    junk = spec(U8, mean=(math.nan,) * 3, std=(0.0,) * 3)
    assert call(L, g, junk, size=need - 1) == INV
    assert call(L, g, junk, dst=None) == INV


def test_the_scratch_is_the_uint8_calls(L):
    """There is no size call of its own: one byte less than jpeggpu_ext_resize_scratch_size_oriented of the same items,
    colours and orientations is refused (a scratch of the full size would be used: not called without a device)."""
    two = arr(item(size=(64, 48)), item(((1, 1),), size=(40, 72)))
    cs, os_ = ints([YCBCR, GRAY]), ints([6, 3])
    need = L.jpeggpu_ext_resize_scratch_size_oriented(two, cs, os_, 2, 32, 24, BILINEAR)
    assert need > L.jpeggpu_ext_resize_scratch_size(two, 2, 32, 24, BILINEAR) > 0  # the transposed item's list and rows
    assert call(L, two, spec(F16, flips=[1, 0]), size=need - 1, colors=cs, orients=os_) == INV


_PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include <jpeggpu/jpeggpu_ext.h>
#define F(f) (int)offsetof(struct jpeggpu_ext_tensor_spec, f)
int main(void) {
    printf("%d %d %d %d %d %d %d %d %d\n", (int)sizeof(struct jpeggpu_ext_tensor_spec), F(type), F(mean), F(std), F(flips),
           (int)JPEGGPU_EXT_TENSOR_U8, (int)JPEGGPU_EXT_TENSOR_F32, (int)JPEGGPU_EXT_TENSOR_F16, (int)JPEGGPU_EXT_TENSOR_BF16);
    return 0;
}
"""


def test_ctypes_mirror_is_the_header(tmp_path):
    """struct jpeggpu_ext_tensor_spec as a C compiler lays it out (the header is C: -std=c11 -Wall -Wextra -Werror)."""
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(_PROBE)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, check=True, timeout=60).stdout.split()]
    want = [C.sizeof(TensorSpec)] + [getattr(TensorSpec, f).offset for f, _ in TensorSpec._fields_] + [U8, F32, F16, BF16]
    assert got == want
    assert [f for f, _ in TensorSpec._fields_] == ["type", "mean", "std", "flips"]


def test_python_argument_checks():
    """resize_to_tensor refuses what it can without a device: a dtype that is not offered."""
    import torch

    assert set(jpeggpu_amd.TENSOR_TYPES) == {torch.uint8, torch.float32, torch.float16, torch.bfloat16}
    assert jpeggpu_amd.TENSOR_TYPES[torch.bfloat16] == BF16
    with pytest.raises(ValueError, match="dtype"):
        jpeggpu_amd.resize_to_tensor([[torch.zeros(1, dtype=torch.uint8)]], [None], 8, dtype=torch.float64)
    with pytest.raises(ValueError, match="layout"):
        jpeggpu_amd.resize_to_tensor([[torch.zeros(1, dtype=torch.uint8)]], [None], 8, layout="CHW")


def test_the_reference_tells_the_forms_apart():
    """All 3 x 256 values of the contract's form against the reciprocal and the folded forms, in float32 on the CPU: the
    expected value of tests/test_gpu_tensor.py would not pass a kernel that computed either."""
    import torch

    u = torch.arange(256, dtype=torch.float32).view(256, 1)
    m, s = (torch.tensor(v, dtype=torch.float32) for v in IMAGENET)
    want = u.div(255).sub(m).div(s)
    recip = (u * (torch.tensor(1.0) / 255) - m) * (1.0 / s)
    folded = torch.addcmul(-m / s, u, 1.0 / (255 * s))
    assert int((want.view(torch.int32) != recip.view(torch.int32)).sum()) > 100
    assert int((want.view(torch.int32) != folded.view(torch.int32)).sum()) > 100
