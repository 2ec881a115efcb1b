"""The plan under AddressSanitizer + UBSan: jg_reader.cpp and jg_plan.cpp as they are, in a stand-alone program
(tests/emu/plan_check_main.cpp) that plans every file below under every setting, fills the table blob into an exact-size
heap buffer, builds the jobs against a fake base and checks region bounds, pointer bounds and determinism. Nothing is
loaded into Python. No GPU needed."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from tests import cases
from tests.conftest import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(600)
def test_plans_under_asan_ubsan():
    files = sorted(cases.matrix().items())
    files += [("big_last_0", cases.big_last_scan_case(0)), ("big_last_4", cases.big_last_scan_case(4))]
    prog = np.load(os.path.join(GOLDEN, "progressive_pins.npz"))["prog/p420_odd"].tobytes()
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "plan_check_main")
        csrc = os.path.join(ROOT, "jpeggpu_amd", "csrc")
        srcs = [os.path.join(ROOT, "tests", "emu", "plan_check_main.cpp"), os.path.join(csrc, "jg_reader.cpp"), os.path.join(csrc, "jg_plan.cpp")]
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fwrapv", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I" + os.path.join(ROOT, "include"), "-I" + csrc] + srcs + ["-o", exe])
        paths = []
        for name, data in files + [("prog_p420_odd", prog)]:
            paths.append(os.path.join(d, name + ".jpg"))
            with open(paths[-1], "wb") as f:
                f.write(data)
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
        r = subprocess.run([exe] + paths[:-1] + ["--progressive", paths[-1]], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=540)
        sys.stdout.write(r.stdout.decode())
        assert r.returncode == 0, (r.returncode, r.stderr.decode()[-4000:])
        m = re.search(rb"plan check: (\d+) files, (\d+) pairs checked, (\d+) skipped, (\d+) plans with mh > 1, (\d+) with mh_blocks, "
                      rb"(\d+) device-walked, (\d+) progressive", r.stdout)
        assert m, r.stdout
        n_files, checked, skipped, mh, mh_blocks, device_walked, progressive = (int(x) for x in m.groups())
        assert n_files == len(paths) and checked + skipped == 64 * n_files
        # the floors: a setting the parse refuses for a file is skipped, which must not hide a failure
        # (at least 8 per file, and one plan of each kind; raised to what the files above give)
        assert checked >= 1744 >= 8 * n_files
        assert mh >= 492 and mh_blocks >= 12 and device_walked >= 732 and progressive >= 40
