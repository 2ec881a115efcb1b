"""Mutation fuzzing of the parser's Exif reader under AddressSanitizer + UBSan: jg_reader.cpp as it is, in a stand-alone
program (tests/emu/exif_fuzz_main.cpp) that parses seeded mutations of files carrying every Exif segment of
tests/exif_ref.segments() -- length fields, offsets, counts and the byte order damaged, files truncated. Nothing is loaded
into Python. No GPU needed."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from tests import exif_ref
from tests.conftest import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(600)
def test_mutated_exif_segments_under_asan_ubsan():
    from tools import jpegsynth

    base = jpegsynth.encode(24, 16, ((2, 2), (1, 1), (1, 1)), seed=77)
    prog = np.load(os.path.join(GOLDEN, "progressive_pins.npz"))["prog/p420_odd"].tobytes()
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "exif_fuzz_main")
        srcs = [os.path.join(ROOT, "tests", "emu", "exif_fuzz_main.cpp"), os.path.join(ROOT, "jpeggpu_amd", "csrc", "jg_reader.cpp")]
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fwrapv", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "jpeggpu_amd", "csrc")] + srcs + ["-o", exe])
        files = []
        for k, (name, (data, _)) in enumerate(sorted(exif_ref.cases(base).items()) + sorted(exif_ref.cases(prog).items())):
            p = os.path.join(d, "%03d.jpg" % k)
            with open(p, "wb") as f:
                f.write(data)
            files.append(p)
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
        r = subprocess.run([exe, "4000", "20261018"] + files, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=540)
        sys.stdout.write(r.stdout.decode())
        assert r.returncode == 0, (r.returncode, r.stderr.decode()[-4000:])
        assert b"parsed" in r.stdout
