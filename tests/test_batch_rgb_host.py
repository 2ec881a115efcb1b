"""Batched conversion to RGB on the host (jpeggpu_ext_batch_rgb_scratch_size, jpeggpu_ext_batch_to_rgb): the scratch size,
every refusal -- each returned before anything is enqueued, so with made-up device addresses and without a device -- and
the ctypes mirror of struct jpeggpu_ext_rgb_item against the header as a C compiler lays it out. No GPU needed."""
import ctypes as C
import os
import subprocess

import pytest

import jpeggpu_amd
from jpeggpu_amd import Status
from jpeggpu_amd import build as jbuild
from jpeggpu_amd.api import CropInfo, Img, ImgInfo, RgbItem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HWC, CHW = 0, 1
GRAY, YCBCR, CMYK = 1, 2, 4
FAKE = 1 << 40  # a device address that is never dereferenced: every call below is refused before anything is enqueued
S420 = ((2, 2), (1, 1), (1, 1))


@pytest.fixture(scope="module")
def L():
    jbuild.build()
    return jpeggpu_amd.lib()


def test_scratch_size(L):
    size = L.jpeggpu_ext_batch_rgb_scratch_size
    assert size(0) == 0 and size(-1) == 0 and size(-65536) == 0
    assert size(65536) == 0
    sizes = [size(n) for n in range(1, 41)]
    assert all(s > 0 for s in sizes)
    assert all(b >= a for a, b in zip(sizes, sizes[1:]))
    assert size(65535) >= sizes[-1]


def item(sampling=S420, size=(64, 48), crop=None, color=None, o=1, layout=HWC, pitch=None, plane=None, dst=FAKE + (1 << 30)):
    """(RgbItem, objects to keep) of a made-up decoded image of `size` pixels with fake plane and dst addresses; the
    pitch and the plane stride are the smallest the layout allows unless given."""
    info, src = ImgInfo(), Img()
    n = len(sampling)
    info.num_components = n
    hmax, vmax = max(s[0] for s in sampling), max(s[1] for s in sampling)
    for c, (h, v) in enumerate(sampling):
        info.subsampling.x[c], info.subsampling.y[c] = h, v
        info.sizes_x[c] = -(-size[0] * h // hmax)
        info.sizes_y[c] = -(-size[1] * v // vmax)
        src.image[c], src.pitch[c] = FAKE + c * (1 << 20), info.sizes_x[c]
    it = RgbItem()
    it.info, it.src = C.pointer(info), C.pointer(src)
    ci = None
    w, h = size
    if crop is not None:
        ci = CropInfo()
        ci.x, ci.y, ci.width, ci.height = crop
        for c in range(n):
            ci.full_x[c], ci.full_y[c] = info.sizes_x[c], info.sizes_y[c]
        it.crop = C.pointer(ci)
        w, h = crop[2:]
    ow, oh = (h, w) if o >= 5 else (w, h)
    it.color = (GRAY if n == 1 else YCBCR) if color is None else color
    it.orientation, it.replicate = o, 0
    it.dst = dst
    it.dst_pitch = ((3 * ow) if layout == HWC else ow) if pitch is None else pitch
    it.plane_stride = it.dst_pitch * oh if plane is None else plane
    return it, (info, src, ci)


def arr(*its):
    a = (RgbItem * len(its))()
    for i, (it, _) in enumerate(its):
        a[i] = it
    return a


def call(L, items, n=None, layout=HWC, scratch=FAKE, size=None):
    n = len(items) if n is None else n
    if size is None:
        size = L.jpeggpu_ext_batch_rgb_scratch_size(n)
    return L.jpeggpu_ext_batch_to_rgb(items, n, layout, scratch, size, None)


def test_refusals(L):
    INV, NS = Status.INVALID_ARGUMENT, Status.NOT_SUPPORTED
    assert call(L, None, n=1) == INV  # NULL items
    assert call(L, arr(item()), n=0) == INV
    assert call(L, arr(item()), n=65536, size=1 << 30) == INV
    assert call(L, arr(item(), item(dst=None), item())) == INV  # NULL dst of the second item
    for o in (0, 9):
        assert call(L, arr(item(), item(o=o))) == INV
    # HWC: 3 x the displayed width less one; for 6 the displayed width is the stored height (48, not 64)
    assert call(L, arr(item(o=1, pitch=3 * 64 - 1))) == INV
    assert call(L, arr(item(o=6, pitch=3 * 48 - 1))) == INV
    assert call(L, arr(item(o=6, pitch=3 * 20 - 1, crop=(2, 2, 30, 20)))) == INV  # of a crop: its stored height
    # CHW: a pitch below the displayed width, a plane stride one byte short
    assert call(L, arr(item(layout=CHW, pitch=63)), layout=CHW) == INV
    assert call(L, arr(item(layout=CHW, plane=64 * 48 - 1)), layout=CHW) == INV
    assert call(L, arr(item(layout=CHW, o=5, pitch=50, plane=50 * 64 - 1)), layout=CHW) == INV
    assert call(L, arr(item()), layout=2) == INV  # an unknown layout
    assert call(L, arr(item()), layout=-1) == INV
    good = arr(item(), item(((1, 1),)), item(crop=(3, 5, 20, 17), o=7))
    need = L.jpeggpu_ext_batch_rgb_scratch_size(3)
    assert call(L, good, size=need - 1) == INV  # a scratch one byte short
    assert call(L, good, scratch=None) == INV
    # a colour that does not fit the component count
    assert call(L, arr(item(), item(color=CMYK))) == NS
    assert call(L, arr(item(((1, 1),), color=YCBCR))) == NS
    assert call(L, arr(item(color=0))) == NS
    assert call(L, arr(item(((3, 1), (2, 1), (1, 1))))) == NS  # non-integral ratios, as the per-image calls
    # a crop whose window does not hold its halo
    it, keep = item(crop=(3, 5, 20, 17))
    keep[2].origin_x[0] = 8
    assert call(L, arr((it, keep))) == INV
    for bad in (item(crop=(0, 0, 0, 10)), item(crop=(-1, 0, 10, 10))):
        assert call(L, arr(item(), bad)) == INV
    it, keep = item()
    it.src.contents.image[1] = None
    assert call(L, arr((it, keep))) == INV
    it, keep = item()
    it.info = None
    assert call(L, arr((it, keep))) == INV


def test_a_window_outside_its_plane_is_refused_before_the_ratios(L):
    """The order of jpeggpu_ext_crop_to_rgbi_*: fancy_source with window_first."""
    it, keep = item(((3, 1), (2, 1), (1, 1)), crop=(3, 5, 20, 17))
    assert call(L, arr((it, keep))) == Status.NOT_SUPPORTED
    keep[2].origin_x[0] = 1000
    assert call(L, arr((it, keep))) == Status.INVALID_ARGUMENT


_PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include <jpeggpu/jpeggpu_ext.h>
#define F(f) (int)offsetof(struct jpeggpu_ext_rgb_item, f)
int main(void) {
    printf("%d %d %d %d %d %d %d %d %d %d %d %d\n", (int)sizeof(struct jpeggpu_ext_rgb_item), F(info), F(crop), F(src), F(color), F(orientation),
           F(replicate), F(dst), F(dst_pitch), F(plane_stride), (int)JPEGGPU_EXT_HWC, (int)JPEGGPU_EXT_CHW);
    return 0;
}
"""


def test_ctypes_mirror_is_the_header(tmp_path):
    """struct jpeggpu_ext_rgb_item as a C compiler lays it out (the header is C: -std=c11 -Wall -Wextra -Werror)."""
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(_PROBE)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, check=True, timeout=60).stdout.split()]
    want = [C.sizeof(RgbItem)] + [getattr(RgbItem, f).offset for f, _ in RgbItem._fields_] + [jpeggpu_amd.IMAGE_LAYOUTS["HWC"], jpeggpu_amd.IMAGE_LAYOUTS["CHW"]]
    assert got == want
    assert [f for f, _ in RgbItem._fields_] == ["info", "crop", "src", "color", "orientation", "replicate", "dst", "dst_pitch", "plane_stride"]
