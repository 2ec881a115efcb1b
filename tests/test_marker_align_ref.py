"""tests/marker_align_cases.py on the CPU: every variant lies where it claims to lie, no cell of the grid is left out,
every variant decodes to its base file's planes (oracle, Pillow), and the host walk (jg_reader.cpp, walk_scan and
scan_window_*) gives the base file's destuffed bytes, segment index and coefficients for every variant under every
JPEGGPU_HOST_SIMD pin. No GPU needed.

The refusal cases on the oracle: it refuses the file cut behind an FF and the empty segments, and ACCEPTS FF FF 00 inside
the scan (it takes any run of FF in front of a 00 as fill bytes in front of nothing and goes on), as it accepts the three
bytes behind EOI; the library's two walks refuse the former (tests/test_gpu_marker_align.py)."""
import io

import numpy as np
import pytest

import jpeggpu_amd
from jpeggpu_amd import JpegGpuError, Status
from jpeggpu_amd import build as jbuild
from oracle import oracle
from tests import marker_align_cases as M
from tests.emu import emu

SIMD = ["auto", "avx2", "sse2", "scalar"]


@pytest.fixture(scope="module")
def E():
    return M.everything()


@pytest.fixture(scope="module")
def decoded(E):
    return {name: oracle.decode(data) for name, data in E["bases"].items()}


@pytest.fixture(scope="module")
def L():
    jbuild.build()
    return jpeggpu_amd.lib()


def test_base_files_are_what_the_cells_need(E):
    a, b, c = (M.parse(E["bases"][k]) for k in "ABC")
    assert len(a.rst) == 63 and len(a.stuffed) == 242 and a.end[1] - a.begin > 17 * M.WIN
    # B: more segments than two passes of front_plan's 1024 lanes, more than two windows (beyond window 8, for the far cells), and
    # lanes that hold several markers
    assert len(b.rst) + 1 > 2048 and b.end[1] - b.begin > 9 * M.WIN and not b.stuffed
    gaps = np.diff([j for _, j in b.rst])
    assert (gaps <= 5).mean() > 0.9
    assert not c.rst and len(c.stuffed) > 200


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_every_variant_lies_where_it_claims(E, name):
    for c in M.variants(name):
        assert c.kind in M.kind_at(c.data, c.pos), (c, M.kind_at(c.data, c.pos))
        if c.grid is None:  # a long fill: its length is the claim
            q, j = next((q, j) for q, j in M.fill_runs(c.data) if q == c.pos)
            assert j - q == c.fill and c.data[q:j + 1] == b"\xff" * (c.fill + 1)
            continue
        off = M.grid_offset(c.data, c.pos)
        assert (off - c.want) % c.grid == 0 and off >= 1, (c, off)
        if c.kind == "lead":
            assert off == c.want and 1 <= off <= 16
        if c.cell.endswith("/near"):
            assert off // M.WIN < 4, (c, off)
        if c.cell.endswith("/far"):
            assert off // M.WIN > 8, (c, off)
        # the fill that moved it lies in front of a marker two markers ahead, and nowhere else
        runs = [(k, j - q) for k, (q, j) in enumerate(M.fill_runs(c.data)) if j > q]
        assert dict(runs) == {k: n for k, n in c.fills.items() if n}, (c, runs)
        if c.fill:
            at = min(c.fills)
            p = M.parse(c.data)
            assert c.fills[at] == c.fill and ([q for q, _ in p.rst] + [p.end[0]])[at + 2] <= c.pos, c


def test_no_cell_is_left_out(E):
    """A condition, not a measurement: every cell of {pattern} x {16, 1024, 4096} x {position} has its variant for files A and
    B, except the cells named in IMPOSSIBLE, and those are exactly the ones placements() could not make."""
    for name in ("A", "B"):
        made = [c.cell for c in E["cases"][name]]
        assert len(set(made)) == len(made)
        assert sorted(E["skipped"][name]) == sorted(M.IMPOSSIBLE[name]), name
        assert sorted(made + E["skipped"][name]) == sorted(M.cells()), name
        assert [c.fill for c in E["long"][name]] == list(M.LONG_FILLS)
    # between them the two files leave out only the stuffed pair behind a restart marker
    assert {c.split("/")[0] for c in set(M.IMPOSSIBLE["A"]) & set(M.IMPOSSIBLE["B"])} == {"stuffed_rst"}
    # the scan's first byte at every offset 1..16 of its lane
    for name in "ABC":
        assert sorted(c.want for c in E["cases"][name] if c.kind == "lead") == list(range(1, 17)), name
    # file C: header pads only; what its stuffed pairs reach on the coarse grids is recorded, not searched for
    hit = set()
    for c in E["cases"]["C"]:
        hit |= M.cells_hit(c.data)
    assert sorted(hit) == sorted(M.C_CELLS)


def test_window_crossing_fills_are_known(E):
    """extra_device_chunks: zero unless a fill byte lies on a window's first byte."""
    for name in "ABC":
        for c in M.variants(name):
            xb = M.xfer_begin(c.data)
            want = sum(1 for q, j in M.fill_runs(c.data) for at in range(q, j) if (at - xb) % M.WIN == 0)
            assert M.extra_device_chunks(c.data) == want, c
    by = {c.cell: M.extra_device_chunks(c.data) for c in M.variants("A")}
    assert by["fill_rst/4096/b0"] >= 1 and by["fill_rst/4096/b1"] == by["fill_rst/4096/b2"] == by["fill_rst/4096/b3"]
    for n in M.LONG_FILLS:  # a run of n bytes covers n // 4096 window starts, or one more
        assert n // M.WIN <= by["long_fill/%d" % n] <= n // M.WIN + 1 and by["long_fill/4096"] == 1, (n, by)


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_every_variant_decodes_to_the_base_file(E, decoded, name):
    ref = decoded[name]
    try:
        from PIL import Image
    except ImportError:
        Image = None
    rgb = None if Image is None else np.asarray(Image.open(io.BytesIO(E["bases"][name])).convert("RGB"))
    for c in M.variants(name):
        d = oracle.decode(c.data)
        assert d.ncomp == ref.ncomp
        for k in range(ref.ncomp):
            assert np.array_equal(d.planes[k], ref.planes[k]), (c, k)
        if Image is not None:
            assert np.array_equal(np.asarray(Image.open(io.BytesIO(c.data)).convert("RGB")), rgb), c


def test_refusal_cases_on_the_oracle(E, decoded):
    want = {"ffff00": "accepted", "ffff00_behind_eoi": "accepted", "cut_behind_ff": "refused", "empty_segment": "refused"}
    for r in E["refusals"]:
        assert (M.grid_offset(r.data, r.pos) - r.want) % r.grid == 0, r
        if r.name.startswith("ffff00/"):
            assert r.data[r.pos:r.pos + 3] == b"\xff\xff\x00" and "ffff00" in M.kind_at(r.data, r.pos), r
        if r.name.startswith("empty_segment"):
            assert r.data[r.pos] == r.data[r.pos + 2] == 0xFF and all(0xD0 <= r.data[r.pos + k] <= 0xD7 for k in (1, 3)), r
        if r.name == "cut_behind_ff":
            assert r.pos == len(r.data) - 1 and r.data[-1] == 0xFF
        try:
            d = oracle.decode(r.data)
            got = "accepted"
        except oracle.OracleError:
            got = "refused"
        assert got == want[r.name.split("/")[0]], r
        if r.accepted:
            assert all(np.array_equal(a, b) for a, b in zip(d.planes, decoded["A"].planes)), r


@pytest.mark.parametrize("simd", SIMD)
def test_refusal_cases_on_the_host_walk(E, L, simd, monkeypatch):
    if simd != "auto":
        monkeypatch.setenv("JPEGGPU_HOST_SIMD", simd)
    for r in E["refusals"]:
        dec = jpeggpu_amd.Decoder(64)
        try:
            dec.parse_header(r.data)
            got = Status.SUCCESS
        except JpegGpuError as e:
            got = e.status
        finally:
            dec.cleanup()
        assert got == (Status.SUCCESS if r.accepted else Status.INVALID_JPEG), (r, got)


@pytest.mark.parametrize("simd", SIMD)
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_host_walk_on_every_variant(E, name, simd, monkeypatch):
    """As tests/test_emulation.py::test_marker_walk_at_every_alignment, whose COM shifts move the bytes modulo 16 only:
    here the patterns lie on the wave and window edges too, and the long fills end a 64-byte block scan in its middle and
    leave whole windows without a data byte."""
    if simd != "auto":
        monkeypatch.setenv("JPEGGPU_HOST_SIMD", simd)
    tw = oracle.scan_stages(E["bases"][name], 0, 64)
    for c in M.variants(name) + ([cc for cc, _ in E["crops"]] if name == "A" else []):
        rc, r = emu.decode_scan(c.data, 0, 64, 256)
        assert rc == 0, c
        assert np.array_equal(r.destuffed, tw.destuffed), (c, "destuffed bytes")
        assert np.array_equal(r.seg_index, tw.seg_index), (c, "segment index")
        assert np.array_equal(r.coef, tw.stream_coef), (c, "coefficients")


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_chunk_bound_of_the_device_scan_holds(E, L, name):
    """The device's chunk list is sized from the header (windows + segments + 1): the host walk's count plus the chunks the
    device adds for window-crossing fills stays inside it."""
    for c in M.variants(name):
        counts = []
        for dev in (False, True):
            dec = jpeggpu_amd.Decoder(32)
            try:
                dec.set_device_scan(dev)
                dec.parse_header(c.data)
                sc = dec.layout().scans[0]
                assert bool(sc.device_scan) == dev
                counts.append(sc.num_chunks)
            finally:
                dec.cleanup()
        assert counts[0] + M.extra_device_chunks(c.data) <= counts[1], (c, counts)
