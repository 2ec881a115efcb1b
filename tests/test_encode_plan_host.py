"""The encoder's host plan under AddressSanitizer + UBSan: jg_encode_plan.cpp as it is, in a stand-alone program
(tests/emu/encode_plan_check_main.cpp) that plans the smallest shapes at which the arithmetic can go wrong -- sizes around
the block and MCU edges and the extremes, every option, calls mixing the kinds, budget calls, synthetic transcode specs in
the encoder's layouts and with frames of their own, and the calls that must be refused --, fills each blob into an
exact-size heap buffer and checks offsets, regions, running sums and determinism. The digests it prints of every blob, Plan
and header are compared with tests/golden/encode_plan_digests.txt, made by the same sweep driven through the code of the
commit before the plan was split out of jg_encode.cpp; and the shipped library's host exports are compared with
tests/golden/encode_plan_pins.npz, made from that commit's library (tools/make_encode_plan_pins.py).
Nothing is loaded into Python but the shipped library. No GPU needed."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import jpeggpu_amd
from jpeggpu_amd import build as jbuild
from tools import make_encode_plan_pins as pins

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """The check program built and run once: its returncode, stdout and stderr."""
    path = str(tmp_path_factory.mktemp("encode_plan") / "encode_plan_check_main")
    csrc = os.path.join(ROOT, "jpeggpu_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "emu", "encode_plan_check_main.cpp"), os.path.join(csrc, "jg_encode_plan.cpp")]
    # no ROCm include path: the plan and its records are free of HIP
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fwrapv", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-I" + csrc] + srcs + ["-o", path])
    r = subprocess.run([path], env=ENV, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=240)
    sys.stdout.write(r.stdout.decode()[-600:])
    return r


@pytest.mark.timeout(300)
def test_plans_under_asan_ubsan(run):
    assert run.returncode == 0, (run.returncode, run.stderr.decode()[-4000:])
    m = re.search(rb"encode plan check: (\d+) pixel items, (\d+) calls, (\d+) budget calls, (\d+) encoder-layout specs, (\d+) frame specs, (\d+) refused", run.stdout)
    assert m, run.stdout[-600:]
    pixel, calls, budget, layout, frame, refused = (int(x) for x in m.groups())
    # the floors: what the sweep gives; a case that is no longer enumerated must not go unnoticed
    assert pixel >= 19008 and calls >= 48 and budget >= 18 and layout >= 480 and frame >= 17296 and refused >= 54


@pytest.mark.timeout(300)
def test_blobs_plans_and_headers_are_the_pinned_ones(run):
    assert run.returncode == 0, (run.returncode, run.stderr.decode()[-4000:])
    got = dict(line.split()[1:] for line in run.stdout.decode().splitlines() if line.startswith("digest "))
    with open(os.path.join(ROOT, "tests", "golden", "encode_plan_digests.txt")) as f:
        want = dict(line.split()[1:] for line in f if line.startswith("digest "))
    assert len(want) >= 37 and sorted(got) == sorted(want)
    assert [k for k in want if got[k] != want[k]] == []


@pytest.mark.timeout(300)
def test_host_exports_are_the_pinned_ones():
    jbuild.build()
    want = np.load(os.path.join(ROOT, "tests", "golden", "encode_plan_pins.npz"))
    got = pins.collect(jpeggpu_amd.lib())
    assert sorted(got) == sorted(want.files)
    assert len(want["pixel"]) >= 6912 and len(want["pixel_calls"]) >= 48 and len(want["transcode"]) >= 972 and len(want["coefficients"]) >= 156
    for name in got:
        assert got[name].shape == want[name].shape, name
        rows = np.flatnonzero((got[name] != want[name]).any(axis=1))
        assert rows.size == 0, (name, rows[:8], got[name][rows[:1]], want[name][rows[:1]])
