"""The batched sequence kernel's schedule with RUNS of subsequences per lane (jpeggpu_amd/csrc/jg_sync_runs.h), on the
host: the product's lane functions called one lane at a time over whole scans (tests/syncruns compiles them with g++),
for runs of 1, 2 and 4 at 128- and 256-byte subsequences. CPU only.

What is asserted per scan: (a) after the tail's rule -- a flow from every marked entry and every sequence boundary until
the stored state is met -- every stored (p, n, cz, dc01, dc23) is the sequential decoder's; (b) the table and marks of
R = 1 are those of today's one-subsequence-per-lane schedule; (c) the schedule takes one flow decode per subsequence and
one speculative decode per run and per overlap lane, (R + 1) / R per subsequence; (d) marks sit at run starts only.
(e) is a report: the share of wrong states and of marks on the flagship image and the photo (pytest -s shows it).

Measured (shares of all subsequences, 256-byte subsequences; 128-byte in brackets):
    cfg 2 seed 0   R = 1: wrong 0.53 % marks 7.6 %   R = 2: 0.30 % / 3.8 %   R = 4: 0.20 % / 2.0 %
                   (R = 1: 7.8 % / 29.3 %            R = 2: 4.9 % / 14.7 %   R = 4: 2.7 % / 7.3 %)
    IMG_6510.JPG   R = 1: wrong 5.8 % marks 22.5 %   R = 2: 3.6 % / 11.2 %   R = 4: 1.9 % / 5.5 %
                   (R = 1: 22.9 % / 44.8 %           R = 2: 17.2 % / 22.4 %  R = 4: 10.3 % / 11.1 %)"""
import os
import subprocess

import pytest

from tests import cases
from tests.syncprobe import crafted
from tests.syncruns import inputs, syncruns
from tools import jpegsynth

RUNS = (1, 2, 4)
SIZES = (128, 256)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def big():
    return {"cfg2_seed0": jpegsynth.config(2, seed=0), "IMG_6510": open(os.path.join(GOLDEN, "IMG_6510.JPG"), "rb").read()}


def _scans(data, subseq_bytes):
    n = 0
    while syncruns.num_subseq(data, subseq_bytes, n) >= 0:
        n += 1
    return n


def _check(name, data, subseq_bytes, r):
    for scan in range(_scans(data, subseq_bytes)):
        x = syncruns.run(data, subseq_bytes, r, scan)
        what = (name, subseq_bytes, r, scan)
        S = x.subsequences
        assert x.never_stored == 0, what
        assert x.wrong_after_tail == 0, what                      # (a)
        if r == 1:
            assert x.differ_from_today == 0, what                 # (b)
        # (c) every subsequence is decoded by exactly one flow; a speculative decode per run, and one per overlap lane
        # that has a subsequence in front of its group (every group but the scan's first)
        per_group = inputs.SEQ * r
        runs = sum((min(per_group, S - g0) + r - 1) // r for g0 in range(0, S, per_group))
        assert x.groups == (S + per_group - 1) // per_group, what
        assert x.flow_decodes == S and x.spec_decodes == runs + x.groups - 1, what
        assert x.spec_decodes + x.flow_decodes <= S * (r + 1) // r + r + x.groups, what
        assert x.marks_inside_runs == 0, what                     # (d)
    return x


@pytest.mark.parametrize("subseq_bytes", SIZES)
@pytest.mark.parametrize("r", RUNS)
def test_crafted_cases(r, subseq_bytes):
    """Segments of 1, 2, 3 and R + 1 subsequences, no restart markers, fewer than R subsequences, exactly 255 R and
    255 R + 1, interleaved / three scans / four components, the long-magnitude file."""
    files = inputs.files(r, subseq_bytes)
    files["long_magnitudes"] = crafted.long_magnitude_case()
    opens = [0] * 4
    for name, data in files.items():
        x = _check(name, data, subseq_bytes, r)
        if name.startswith("segments_of_"):
            k = int(name.rsplit("_", 1)[1])
            assert x.segments_of[k] * 5 >= x.segments * 4, (name, x.segments_of)
            opens = [a + b for a, b in zip(opens, x.opens_at)]
    assert all(opens[k] > 0 for k in range(r)), opens  # a segment opens at every position of a run
    assert syncruns.run(files["255r"], subseq_bytes, r).subsequences == inputs.SEQ * r
    assert syncruns.run(files["255r_plus_1"], subseq_bytes, r).subsequences == inputs.SEQ * r + 1
    assert syncruns.run(files["fewer_than_r"], subseq_bytes, r).subsequences == max(r - 1, 1)


@pytest.mark.parametrize("subseq_bytes", SIZES)
@pytest.mark.parametrize("r", RUNS)
def test_streams_that_synchronise_slowly(r, subseq_bytes):
    """tests/cases.slow_sync: nearly every speculated state is wrong, so nearly every run start is marked."""
    marked = 0
    for name, v in cases.slow_sync().items():
        marked += _check(name, v.data, subseq_bytes, r).marks
    assert marked > 0


@pytest.mark.parametrize("subseq_bytes", SIZES)
def test_flagship_image_and_photo(big, subseq_bytes):
    for name, data in big.items():
        marks = {}
        for r in RUNS:
            x = _check(name, data, subseq_bytes, r)
            marks[r] = x.marks
            print("%s %d-byte subsequences R=%d: %d subsequences, wrong states %.2f %%, marks %.2f %%, decodes per subsequence %.3f, tail decodes %d"
                  % (name, subseq_bytes, r, x.subsequences, 100.0 * x.wrong_states / x.subsequences, 100.0 * x.marks / x.subsequences,
                     (x.spec_decodes + x.flow_decodes) / x.subsequences, x.tail_decodes))
        # marks only at run starts, and there at the rate of R = 1: no more than its marks / R, give or take the rate's noise
        assert marks[2] <= marks[1] * 0.6 and marks[4] <= marks[1] * 0.35, (name, marks)


def test_refuses_other_run_lengths(big):
    import numpy as np

    out = np.zeros(24, np.int64)
    data = crafted.long_magnitude_case()
    for r in (0, 3, 8):
        assert syncruns.lib().probe_sync_runs(data, len(data), 128, 0, r, out.ctypes.data) == -1


def test_probe_under_address_and_ub_sanitizers(tmp_path, big):
    """The probe and a small main as a stand-alone host program built with -fsanitize=address,undefined, once over the
    inputs above (the flagship image and the photo included)."""
    exe = str(tmp_path / "syncruns_asan")
    main = os.path.join(os.path.dirname(syncruns.SOURCES[0]), "syncruns_main.cpp")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + syncruns.FLAGS
                          + syncruns.SOURCES + [main, "-o", exe])
    files = dict(big)
    files["long_magnitudes"] = crafted.long_magnitude_case()
    files["slow_dri48"] = cases.slow_sync()["s420_763_dri48"].data
    for r in (2, 4):
        for b in SIZES:
            for name, data in inputs.files(r, b).items():
                files["%s_r%d_%d" % (name, r, b)] = data
    paths = []
    for name, data in files.items():
        paths.append(str(tmp_path / (name + ".jpg")))
        with open(paths[-1], "wb") as f:
            f.write(data)
    r = subprocess.run([exe] + paths, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "FAILED" not in r.stdout, r.stdout[-4000:]
