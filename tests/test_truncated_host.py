"""The host side of truncated decoding (jpeggpu_ext_set_truncated): what jpeggpu_decoder_parse_header answers with the flag off
and on, what jpeggpu_ext_get_truncated reports, what is refused -- and jg_reader.cpp / jg_plan.cpp on every cut of every
small file under AddressSanitizer + UBSan in a stand-alone program (tests/emu/trunc_plan_check_main.cpp; nothing loaded into
Python runs under a sanitizer). No GPU needed: the files are the pinned ones (tests/golden/truncated_pins.npz)."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import jpeggpu_amd
from jpeggpu_amd import JpegGpuError, Status
from tests import truncated_ref as T
from tests.conftest import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = T.pinned_files()
NAMES = sorted(FILES)


def parse(data, truncated, **settings):
    """(status, TruncatedInfo or None, ExtLayout or None) of one parse_header."""
    dec = jpeggpu_amd.Decoder()
    try:
        if truncated:
            dec.set_truncated(True)
        for k, v in settings.items():
            getattr(dec, "set_" + k)(*v)
        try:
            dec.parse_header(data)
        except JpegGpuError as e:
            return e.status, None, None
        return Status.SUCCESS, dec.truncated(), dec.layout()
    finally:
        dec.cleanup()


@pytest.mark.parametrize("name", NAMES)
def test_flag_off_cut_files_are_refused_as_ever(name):
    """Every cut behind the SOS header: INVALID_JPEG, the parent's answer (tests/test_host_api.py pins it for half a file)."""
    data = FILES[name]
    for cut in list(T.cuts(data))[:-1]:
        assert parse(data[:cut], False)[0] == Status.INVALID_JPEG, cut
    st, info, _ = parse(data, False)
    assert st == Status.SUCCESS and info.truncated == 0 and info.scan == -1


@pytest.mark.parametrize("name", NAMES)
def test_flag_on_every_cut_behind_the_header_parses(name):
    data = FILES[name]
    b = T.scan_begin(data)
    for cut in T.cuts(data):
        st, info, lay = parse(data[:cut], True)
        assert st == Status.SUCCESS, cut
        if cut == len(data):
            assert (info.truncated, info.scan, info.scan_bytes, info.first_missing_interval) == (0, -1, 0, -1)
        else:
            assert (info.truncated, info.scan, info.scan_bytes) == (1, 0, cut - b), cut
    # in front of the end of the SOS header: today's errors, the same with and without the flag
    for cut in list(range(b - 12, b)) + [2, 3, 20, b // 2]:
        off, on = parse(data[:cut], False)[0], parse(data[:cut], True)[0]
        assert off == on and off != Status.SUCCESS, cut


def test_whole_file_parses_the_same_under_the_flag():
    for name in NAMES:
        _, _, a = parse(FILES[name], False)
        _, _, b = parse(FILES[name], True)
        assert bytes(a) == bytes(b), name


def test_truncated_info_in_data_in_a_marker_and_at_the_eoi():
    data = FILES["s420_rst5"]
    b, sp = T.scan_begin(data), T.special_cuts(data)
    marks = [m.start() for m in re.finditer(b"\xff[\xd0-\xd7]", data[b:])]
    assert len(marks) >= 2  # 12 MCUs in intervals of 5
    # in the data of interval 1: interval 2 is the first without any
    mid = b + (marks[0] + 2 + marks[1]) // 2
    _, info, _ = parse(data[:mid], True)
    assert (info.truncated, info.scan, info.scan_bytes, info.first_missing_interval) == (1, 0, mid - b, 2)
    # at the end of interval 0's data, inside its restart marker and right behind it: interval 1 has none
    for key in ("interval_end", "in_rst", "behind_rst"):
        _, info, _ = parse(data[:sp[key]], True)
        assert (info.truncated, info.first_missing_interval, info.scan_bytes) == (1, 1, sp[key] - b), key
    # one byte of interval 1: it is there
    _, info, _ = parse(data[:sp["behind_rst"] + 1], True)
    assert info.first_missing_interval == 2
    # in the last interval, and at the EOI (none of it, half of it): nothing is missing but the marker
    for cut in (len(data) - 6, sp["no_eoi"], sp["eoi_ff"]):
        _, info, _ = parse(data[:cut], True)
        assert (info.truncated, info.scan, info.first_missing_interval) == (1, 0, -1), cut
    # a file without restart markers has no intervals to miss
    plain = FILES["s420_plain"]
    _, info, _ = parse(plain[:len(plain) // 2 + 200], True)
    assert (info.truncated, info.first_missing_interval) == (1, -1)


def test_restart_counts_fewer_accepted_more_refused():
    data = FILES["gray_rst1"]
    b = T.scan_begin(data)
    marks = [b + m.start() for m in re.finditer(b"\xff[\xd0-\xd7]", data[b:])]
    assert parse(data[:marks[3]], True)[0] == Status.SUCCESS  # four intervals of 24
    # one restart marker more than the geometry has intervals, then the end of the file: refused as ever
    extra = data[:-2] + b"\xff" + bytes([0xD0 + len(marks) % 8]) + b"\x12"
    assert parse(extra, True)[0] == Status.INVALID_JPEG and parse(extra, False)[0] == Status.INVALID_JPEG


def test_progressive_is_not_supported_under_the_flag():
    prog = np.load(os.path.join(GOLDEN, "progressive_pins.npz"))["prog/p420_odd"].tobytes()
    assert parse(prog, False, progressive=(True,))[0] == Status.SUCCESS
    assert parse(prog, True, progressive=(True,))[0] == Status.NOT_SUPPORTED
    assert parse(prog[:len(prog) // 2], True, progressive=(True,))[0] == Status.NOT_SUPPORTED
    assert parse(prog, True)[0] == Status.NOT_SUPPORTED


def test_segment_shard_is_not_supported_and_device_scan_keeps_the_host_walk():
    data = FILES["s420_rstrow"]
    assert parse(data[:len(data) - 40], True, segment_shard=(0, 2))[0] == Status.NOT_SUPPORTED
    st, info, lay = parse(data[:len(data) - 40], True, device_scan=(True,))
    _, _, host = parse(data[:len(data) - 40], True)
    assert st == Status.SUCCESS and info.truncated == 1 and bytes(lay) == bytes(host)


def test_python_wrappers_take_the_keyword():
    import inspect

    for fn in ("decode_to_planes", "decode_to_rgb", "decode_to_gray", "decode_batch_to_rgb", "decode_batch_to_gray", "decode_resized",
               "decode_center_cropped", "decode_thumbnails", "thumbnail_jpeg", "read_coefficients", "transcode_jpeg"):
        p = inspect.signature(getattr(jpeggpu_amd, fn)).parameters
        assert "truncated" in p and p["truncated"].default is False, fn
    assert inspect.signature(jpeggpu_amd.BatchDecode.__init__).parameters["truncated"].default is False


@pytest.mark.timeout(600)
def test_walk_and_plan_of_every_cut_under_asan_ubsan():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "trunc_plan_check_main")
        csrc = os.path.join(ROOT, "jpeggpu_amd", "csrc")
        srcs = [os.path.join(ROOT, "tests", "emu", "trunc_plan_check_main.cpp"), os.path.join(csrc, "jg_reader.cpp"), os.path.join(csrc, "jg_plan.cpp")]
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fwrapv", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I" + os.path.join(ROOT, "include"), "-I" + csrc] + srcs + ["-o", exe])
        paths = []
        for name in NAMES:
            paths.append(os.path.join(d, name + ".jpg"))
            with open(paths[-1], "wb") as f:
                f.write(FILES[name])
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
        r = subprocess.run([exe] + paths, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=540)
        sys.stdout.write(r.stdout.decode())
        assert r.returncode == 0, (r.returncode, r.stderr.decode()[-4000:])
        m = re.search(rb"truncated plan check: (\d+) files, (\d+) plans, (\d+) cut scans, (\d+) with an all-zero segment, (\d+) without data", r.stdout)
        assert m, r.stdout
        n_files, plans, cut_scans, zero_segments, no_data = (int(x) for x in m.groups())
        cuts = sum(len(T.cuts(FILES[name])) for name in NAMES)
        assert n_files == len(NAMES) and plans == 4 * cuts and cut_scans == 4 * (cuts - len(NAMES))
        assert zero_segments >= 4 * 1000 and no_data >= 4 * len(NAMES)
