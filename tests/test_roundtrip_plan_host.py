"""The round trip's host plan under AddressSanitizer + UBSan: jg_roundtrip_plan.cpp as it is (with jg_output_plan.cpp, whose
batched conversion is its second stage) in a stand-alone program (tests/emu/roundtrip_plan_check_main.cpp) that plans calls
without a device -- every refusal, tile starts around the tile size, the scratch layout and its size as the list grows, the
staged bytes filled into an exact-size heap buffer -- and prints item geometries and quantisation tables, which are compared
with tests/encode_ref.py here. Nothing is loaded into Python under a sanitizer. No GPU needed."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import encode_ref as E
from tests import roundtrip_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("roundtrip_plan") / "roundtrip_plan_check_main")
    csrc = os.path.join(ROOT, "jpeggpu_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "emu", "roundtrip_plan_check_main.cpp"), os.path.join(csrc, "jg_roundtrip_plan.cpp"),
            os.path.join(csrc, "jg_output_plan.cpp")]
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fwrapv", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-I" + csrc] + srcs + ["-o", path])
    return path


@pytest.mark.timeout(300)
def test_plans_under_asan_ubsan(exe):
    r = subprocess.run([exe], env=ENV, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=240)
    sys.stdout.write(r.stdout.decode())
    assert r.returncode == 0, (r.returncode, r.stderr.decode()[-4000:])
    m = re.search(rb"roundtrip plan check: (\d+) checks passed", r.stdout)
    assert m and int(m.group(1)) >= 1374, r.stdout  # the floor: a check that is no longer made must not go unnoticed


def test_ctypes_mirror_has_the_layout_the_library_asserts():
    """jg_roundtrip_plan.cpp holds the static_assert on struct jpeggpu_ext_roundtrip_item with these numbers."""
    from jpeggpu_amd.api import RoundtripItem as T

    assert ctypes.sizeof(T) == 80
    assert (T.row_pitch.offset, T.quality.offset, T.dst.offset, T.dst_pitch.offset, T.plane_stride.offset) == (24, 48, 56, 64, 72)


@pytest.mark.timeout(300)
def test_geometry_and_tables_are_the_encoders(exe):
    """Every size of the pins, grey and RGB, every subsampling, every quality of the pins and the edges between them."""
    asked = [(w, h, ch, ss, q) for w, h in R.SIZES for ch in (1, 3) for ss in range(3) for q in R.QUALITIES + [2, 49, 51, 99]]
    r = subprocess.run([exe] + [str(v) for a in asked for v in a], env=ENV, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=240)
    assert r.returncode == 0, (r.returncode, r.stderr.decode()[-4000:])
    lines = r.stdout.decode().splitlines()
    assert len(lines) == len(asked)
    for (w, h, ch, ss, q), line in zip(asked, lines):
        geo, luma, chroma = ([int(v) for v in part.split()] for part in line.split("|"))
        hs, vs, mx, my, _ = E.geometry(w, h, ch, *E.SUBSAMPLINGS[ss])
        gw, gh = -(-w // 8), -(-h // 8)
        assert geo == [hs, vs, mx, my, gw, gh, gw * gh + (2 * mx * my if ch == 3 else 0)], (w, h, ch, ss)
        assert np.array_equal(luma, E.quant_table(E.BASE_LUMA, q)) and np.array_equal(chroma, E.quant_table(E.BASE_CHROMA, q)), q
