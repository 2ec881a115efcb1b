"""The CPU restatement of truncated decoding (tests/truncated_ref.py) against Pillow with ImageFile.LOAD_TRUNCATED_IMAGES, at
EVERY cut offset from the end of the SOS header to the end of the file, for grey, 4:4:4, 4:2:2 and 4:2:0 files written plain,
with optimised tables and with restart intervals of one MCU, one MCU row and five blocks, and for a file whose scan holds
stuffed FF 00 pairs. No GPU needed; the flag is set inside truncated_ref.pillow_rgb and restored there.

One thing is not the rule's: the MCU that is finished from zero bits can hold blocks no encoder writes (63 coefficients of
-(2^s - 1)), on which libjpeg-turbo's SIMD IDCT, which Pillow runs, saturates where jidctint.c -- the library's ISLOW transform
and tests/libjpeg_ref.py -- wraps (tests/test_idct_cases_host.py, pillow_comparable_units). truncated_ref.simd_comparable says
from the coefficients alone where that is so; there the comparison leaves out the pixels that MCU reaches, every other pixel
must still be equal, and the same cuts are compared whole in a child process with JSIMD_FORCENONE=1, which makes libjpeg-turbo
run jidctint.c."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import truncated_ref as T

pytest.importorskip("PIL")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["%s_%s" % (lay[0], var[0]) for lay in T.LAYOUTS for var in T.VARIANTS] + ["s420_stuffed"]


@pytest.fixture(scope="module")
def files():
    return T.files()


@pytest.fixture(scope="module")
def incomparable():
    """(name, cut) of the cuts whose MCU Pillow's SIMD IDCT computes differently, collected by the sweep below."""
    return []


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_pillow_at_every_cut(files, incomparable, name):
    data = files[name]
    assert 48 <= T.decode(data).width <= 64 and 32 <= T.decode(data).height <= 48
    masked = 0
    for cut in T.cuts(data):
        d = data[:cut]
        dec = T.decode(d)
        ours, theirs = T.rgb_of(dec, d), T.pillow_rgb(d)
        assert ours.shape == theirs.shape
        if not T.pillow_comparable(dec):
            x0, y0, x1, y1 = T.cut_mcu_rect(dec)
            theirs = theirs.copy()
            theirs[y0:y1, x0:x1] = ours[y0:y1, x0:x1]
            incomparable.append((name, cut))
            masked += 1
        assert np.array_equal(ours, theirs), (name, cut, dec.cut_mcu)
    assert masked * 2 <= len(T.cuts(data)), (name, masked)  # (as tests/test_idct_cases_host.py asks of its files: most compare whole)


def test_incomparable_cuts_equal_pillow_without_simd(files, incomparable):
    """The cuts left out above, whole, against Pillow on jidctint.c (a fresh process: libjpeg-turbo reads the variable once)."""
    if not incomparable:
        pytest.skip("the sweep did not run, or found no such cut")
    script = ("import sys, numpy as np\nsys.path.insert(0, %r)\nfrom tests import truncated_ref as T\nfs = T.files()\n"
              "for a in sys.argv[1:]:\n    name, cut = a.rsplit(':', 1)\n    d = fs[name][:int(cut)]\n"
              "    assert np.array_equal(T.rgb(d), T.pillow_rgb(d)), a\nprint('ok', len(sys.argv) - 1)\n" % ROOT)
    r = subprocess.run([sys.executable, "-c", script] + ["%s:%d" % nc for nc in incomparable], env=dict(os.environ, JSIMD_FORCENONE="1"),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0 and r.stdout.split()[:1] == [b"ok"], r.stderr.decode()[-2000:]


def test_stuffed_file_holds_stuffed_pairs(files):
    data = files["s420_stuffed"]
    assert data.count(b"\xff\x00", T.scan_begin(data)) >= 2


@pytest.mark.parametrize("name", ["s420_stuffed", "s420_rst5", "gray_rst1", "s444_rstrow", "s422_plain"])
def test_special_ends(files, name):
    """The ends the rule leaves open, pinned: a trailing FF is not data, whether it is half of FF 00, of a restart marker or of
    the EOI; data that ends with an interval -- in front of, inside or right behind the restart marker -- makes the NEXT
    interval's first MCU the one decoded from zero bits; a file without its EOI is the whole file."""
    data = files[name]
    sp = T.special_cuts(data)
    whole = T.pillow_rgb(data)
    assert np.array_equal(T.rgb(data), whole)
    for key in ("no_eoi", "eoi_ff"):
        d = data[:sp[key]]
        assert T.decode(d).cut_mcu is None and T.decode(d).ended == "eof"
        assert np.array_equal(T.rgb(d), whole) and np.array_equal(T.pillow_rgb(d), whole)
    if "in_ff00" in sp:
        a, b = data[:sp["in_ff00"]], data[:sp["in_ff00"] - 1]  # with and without the pair's FF
        assert np.array_equal(T.pillow_rgb(a), T.pillow_rgb(b)) and np.array_equal(T.rgb(a), T.rgb(b))
        assert np.array_equal(T.rgb(a), T.pillow_rgb(a))
        c = data[:sp["behind_ff00"]]
        assert np.array_equal(T.rgb(c), T.pillow_rgb(c))
    if "interval_end" in sp:
        dec = T.decode(data)
        outs = []
        for key in ("interval_end", "in_rst", "behind_rst"):
            d = data[:sp[key]]
            cut = T.decode(d)
            assert cut.cut_mcu == (0, dec.restart_interval), (key, cut.cut_mcu)  # interval 1's first MCU
            assert T.pillow_comparable(cut)
            outs.append(T.rgb(d))
            assert np.array_equal(outs[-1], T.pillow_rgb(d)), key
        assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])


def test_header_cuts_are_refused(files):
    data = files["s420_plain"]
    for cut in (T.scan_begin(data) - 1, T.scan_begin(data) - 7, 40, 3):
        with pytest.raises((T.Truncated, IndexError)):
            T.decode(data[:cut])


def test_rows_above_the_cut_are_the_whole_files(files):
    """What the issue measured on 304 x 200 files, on the small ones: whole iMCU rows less the upsampler's one row of context."""
    data = files["s420_plain"]
    whole = T.rgb(data)
    for cut in list(T.cuts(data))[::25]:
        dec = T.decode(data[:cut])
        if dec.cut_mcu is None:
            continue
        rows = (dec.cut_mcu[1] // 4) * 16 - 1  # 64 pixels wide: four MCUs per row
        if rows > 0:
            assert np.array_equal(T.rgb_of(dec, data[:cut])[:rows], whole[:rows]), cut


def test_pins_are_current(files):
    """tests/golden/truncated_pins.npz holds these files and Pillow's digests at the pinned cuts (tools/make_truncated_pins.py)."""
    import PIL

    pins = T.pinned()
    if bytes(np.load(T.PINS)["pillow_version"]).decode() != PIL.__version__:
        pytest.skip("the pins were made with another Pillow, whose encoder may write other files")
    assert sorted(pins) == sorted(files)
    for name, (data, cuts, shas) in pins.items():
        assert data == files[name] and cuts == T.pin_cuts(data) and len(cuts) >= 10
        for cut, sha in zip(cuts, shas):
            assert T.sha(T.pillow_rgb(data[:cut])) == sha, (name, cut)


def test_restatement_equals_the_pins():
    """Without Pillow: the restatement gives the pinned digests."""
    for name, (data, cuts, shas) in T.pinned().items():
        for cut, sha in zip(cuts, shas):
            assert T.sha(T.rgb(data[:cut])) == sha, (name, cut)
