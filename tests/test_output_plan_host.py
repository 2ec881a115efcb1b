"""The output stage's host plan under AddressSanitizer + UBSan: jg_output_plan.cpp as it is, in a stand-alone program
(tests/emu/output_plan_check_main.cpp) that plans the smallest shapes at which the arithmetic can go wrong -- sizes, crop
rectangles, views, orientations, colour models, batch sizes, thumbnail requests --, fills each plan's staged part into an
exact-size heap buffer and checks table rows, scratch layout, tile counts and determinism; and the same program's tables
and thumbnail plans against those of the shipped library, so that the sanitized build is seen to compute what ships.
Nothing is loaded into Python but the shipped library. No GPU needed."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import jpeggpu_amd
from jpeggpu_amd import build as jbuild
from jpeggpu_amd.api import FILTERS
from tests import thumbnail_cases as TC
from tests.test_resize_host import table_pairs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("output_plan") / "output_plan_check_main")
    csrc = os.path.join(ROOT, "jpeggpu_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "emu", "output_plan_check_main.cpp"), os.path.join(csrc, "jg_output_plan.cpp")]
    # -ffp-contract=off: what `#pragma clang fp contract(off)` is for the shipped build (g++ does not know the pragma)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fwrapv", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-I" + csrc] + srcs + ["-o", path])
    return path


@pytest.mark.timeout(300)
def test_plans_under_asan_ubsan(exe):
    r = subprocess.run([exe], env=ENV, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=240)
    sys.stdout.write(r.stdout.decode())
    assert r.returncode == 0, (r.returncode, r.stderr.decode()[-4000:])
    m = re.search(rb"output plan check: (\d+) cases enumerated; (\d+) tables \((\d+) refused\), (\d+) resize plans \((\d+) refused\), "
                  rb"(\d+) rgb batch plans \((\d+) refused\), (\d+) thumbnail sizes \((\d+) refused\), (\d+) thumbnail plans \((\d+) refused\), "
                  rb"(\d+) bad arguments \((\d+) refused\)", r.stdout)
    assert m, r.stdout
    n, tables, tables_no, resize, resize_no, rgb, rgb_no, sizes, sizes_no, thumbs, thumbs_no, bad, bad_no = (int(x) for x in m.groups())
    assert tables + resize + rgb + sizes + thumbs + bad == n  # every enumerated case ended with the status it carries
    # the floors: what the sweep gives; a case that is no longer enumerated must not go unnoticed
    assert tables >= 498 and tables_no == 0
    assert resize >= 1711 and 15 <= resize_no <= resize - 1696
    assert rgb >= 173 and 11 <= rgb_no <= rgb - 162
    assert sizes >= 1730 and 45 <= sizes_no <= sizes - 1685
    assert thumbs >= 463 and 8 <= thumbs_no <= thumbs - 455
    assert bad >= 84 and bad_no >= 82


@pytest.mark.timeout(300)
def test_sanitized_build_computes_what_ships(exe, tmp_path):
    """The weight tables of tests/test_resize_host.py's size pairs and the plans of tests/thumbnail_cases.py's cases, exactly."""
    jbuild.build()
    pairs = [(i, o, f) for f in sorted(FILTERS, key=FILTERS.get) for i, o in table_pairs()]
    thumbs = []
    for case, source, req, gap in TC.CASES:
        how = TC.SOURCES[source]
        w, h = how[2:4] if how[0] == "pillow" else how[1:3]
        thumbs += [(case, w, h, req, f, gap) for f in TC.FILTERS]
    cases, result = str(tmp_path / "cases.txt"), str(tmp_path / "result.bin")
    with open(cases, "w") as f:
        for i, o, filt in pairs:
            f.write("W %d %d %d\n" % (i, o, FILTERS[filt]))
        for _, w, h, req, filt, gap in thumbs:
            f.write("T %d %d %d %d %d %s\n" % (w, h, req[0], req[1], FILTERS[filt], float(gap or 0.0).hex()))
    r = subprocess.run([exe, cases, result], env=ENV, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=240)
    assert r.returncode == 0, (r.returncode, r.stderr.decode()[-4000:])
    got = np.fromfile(result, np.int32)
    at = 0
    for i, o, filt in pairs:
        first, count, w = jpeggpu_amd.resize_weights(i, o, filt)
        want = np.concatenate([np.array([0, w.shape[1]], np.int32), first, count, w.ravel()])
        assert np.array_equal(got[at:at + want.size], want), (i, o, filt)
        at += want.size
    for case, w, h, req, filt, gap in thumbs:
        plan = jpeggpu_amd.thumbnail_plan(w, h, req, filt, gap)
        want = np.concatenate([np.zeros(1, np.int32), np.frombuffer(bytes(plan), np.int32)])
        assert np.array_equal(got[at:at + want.size], want), (case, filt)
        at += want.size
    assert at == got.size and len(pairs) > 700 and len(thumbs) == 2 * len(TC.CASES)
