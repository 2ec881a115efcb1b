"""Progressive JPEGs without a GPU: what the parser accepts and refuses through the C ABI, and the host twin of the scan
kernels (tests/emu/prog_twin.cpp: the product's parser and jg_prog_core.h, driven level by level) against the Python
restatement written from T.81 Annex G (tests/progressive_ref.py)."""
import numpy as np
import pytest

import jpeggpu_amd
from jpeggpu_amd import ColorSpace, Status
from jpeggpu_amd import build as jbuild
from tests import progressive_cases as pc
from tests import progressive_ref as pr
from tests.emu import prog_twin


@pytest.fixture(scope="module")
def L():
    jbuild.build()
    return jpeggpu_amd.lib()


def parse_status(data, progressive=True, shard=None):
    dec = jpeggpu_amd.Decoder()
    try:
        dec.set_progressive(progressive)
        if shard:
            dec.set_segment_shard(*shard)
        try:
            dec.parse_header(data)
        except jpeggpu_amd.JpegGpuError as e:
            return e.status
        return Status.SUCCESS
    finally:
        dec.cleanup()


def test_default_decoder_still_refuses_sof2(L):
    for name, (prog, twin, _) in pc.pins().items():
        assert parse_status(prog, progressive=False) == Status.NOT_SUPPORTED, name
        assert parse_status(twin, progressive=False) == Status.SUCCESS, name


def test_parse_header_of_every_pin(L):
    from oracle import oracle

    colors = {"pgray": ColorSpace.GRAY, "pcmyk": ColorSpace.CMYK, "pycck": ColorSpace.YCCK, "prgb": ColorSpace.RGB}
    for name, (prog, twin, rgb) in pc.pins().items():
        o = oracle.decode(twin)
        dec = jpeggpu_amd.Decoder()
        try:
            dec.set_progressive(True)
            dec.set_device_scan(True)  # ignored for a progressive image
            info = dec.parse_header(prog)
            assert info.num_components == o.ncomp
            for c in range(o.ncomp):
                assert (info.sizes_y[c], info.sizes_x[c]) == o.planes[c].shape, (name, c)
            assert dec.color_space() == colors.get(name, ColorSpace.YCBCR), name
            pi = dec.progressive_info()
            assert pi.progressive == 1
            assert pi.num_scans == {1: 6, 3: 10, 4: 18}[o.ncomp], name
            assert pi.num_levels == 3, name
            lay = dec.layout()
            assert lay.num_scans == o.ncomp
            size = dec.get_buffer_size()
            for c in range(o.ncomp):
                sl = lay.scans[c]
                assert (sl.num_components, sl.component_idx[0], sl.num_subsequences, sl.num_segments, sl.num_chunks, sl.device_scan) == (1, c, 0, 0, 0, 0)
                assert sl.data_units_per_mcu == 1 and sl.num_data_units == pi.visible_blocks_x[c] * pi.visible_blocks_y[c]
                assert (pi.visible_blocks_y[c], pi.visible_blocks_x[c]) == (-(-o.planes[c].shape[0] // 8), -(-o.planes[c].shape[1] // 8))
                assert pi.blocks_x[c] >= pi.visible_blocks_x[c] and pi.blocks_y[c] >= pi.visible_blocks_y[c]
                assert pi.off_coefficients[c] % 256 == 0
                assert pi.off_coefficients[c] + pi.blocks_x[c] * pi.blocks_y[c] * 128 <= size
                assert sl.off_du_table + sl.num_data_units * 8 <= size
            # a baseline file parsed next is a baseline file again
            dec.parse_header(twin)
            assert dec.progressive_info().progressive == 0 and dec.progressive_info().num_scans == 0
        finally:
            dec.cleanup()
    hs = oracle.decode(pc.pins()["p420"][1])
    assert hs.hs[0] == 2  # (the padded grid is larger than the visible one for 4:2:0 of 40 x 24: 6 x 4 against 5 x 3 blocks)


def tiny(script, nc=3, restart=0):
    """A 17 x 9 4:2:0 (or grey) progressive file with this scan script; the coefficients do not matter."""
    sampling = [(2, 2), (1, 1), (1, 1)][:nc]
    coef = [np.ones((2, 4, 64), np.int64) * 3 for _ in range(nc)]
    q = {0: np.ones(64, np.int64) * 2}
    return pr.encode(17, 9, sampling, q, [0] * nc, coef, script, restart=restart)


ALL = (0, 1, 2)
DC = (ALL, 0, 0, 0, 0)


def too_many_scans():
    return tiny([((0,), 0, 0, 0, 0)] + [((0,), k, k, 0, 0) for k in range(1, 64)] + [((1,), 0, 0, 0, 0), ((2,), 0, 0, 0, 0)])


def one_restart_marker_less():
    f = tiny([DC, ((0,), 1, 63, 0, 0), ((1,), 1, 63, 0, 0), ((2,), 1, 63, 0, 0)], restart=1)
    i = f.rindex(b"\xff\xd0")  # a restart marker of the last scans
    return f[:i] + f[i + 2:]


REFUSALS = (
    ("Ss = 0 with Se != 0", lambda: tiny([(ALL, 0, 5, 0, 0)]), Status.INVALID_JPEG),
    ("an AC scan with two components", lambda: tiny([DC, ((1, 2), 1, 63, 0, 0)]), Status.INVALID_JPEG),
    ("Al = 14", lambda: tiny([(ALL, 0, 0, 0, 14)]), Status.INVALID_JPEG),
    ("Ah != Al + 1", lambda: tiny([(ALL, 0, 0, 0, 3), (ALL, 0, 0, 3, 1)]), Status.INVALID_JPEG),
    ("a refinement before its first scan", lambda: tiny([(ALL, 0, 0, 1, 0)]), Status.NOT_SUPPORTED),
    ("a refinement of the wrong bit", lambda: tiny([(ALL, 0, 0, 0, 3), (ALL, 0, 0, 2, 1)]), Status.NOT_SUPPORTED),
    ("an AC scan before the component's DC scan", lambda: tiny([((0,), 1, 63, 0, 0), DC]), Status.NOT_SUPPORTED),
    ("a first scan repeated", lambda: tiny([DC, DC]), Status.NOT_SUPPORTED),
    ("a component without a DC scan", lambda: tiny([((0,), 0, 0, 0, 0), ((0,), 1, 63, 0, 0)]), Status.INVALID_JPEG),
    ("more than 64 scans", too_many_scans, Status.NOT_SUPPORTED),
    ("a wrong restart-marker count in one scan", one_restart_marker_less, Status.INVALID_JPEG),
    ("SOF10", lambda: tiny([DC]).replace(b"\xff\xc2", b"\xff\xca", 1), Status.NOT_SUPPORTED),
)


@pytest.mark.parametrize("what,make,status", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(L, what, make, status):
    assert parse_status(make()) == status
    assert prog_twin.parse(make())[0] == status  # (the twin compiles the same parser)


def test_accepted_neighbours_of_the_refusals(L):
    """The same files one step inside the rules parse: the refusals above are about what they say they are about."""
    assert parse_status(tiny([DC])) == Status.SUCCESS
    assert parse_status(tiny([(ALL, 0, 0, 0, 13)])) == Status.SUCCESS
    assert parse_status(tiny([(ALL, 0, 0, 0, 3), (ALL, 0, 0, 3, 2)])) == Status.SUCCESS
    sixty_four = tiny([DC] + [((0,), k, k, 0, 0) for k in range(1, 64)])
    assert parse_status(sixty_four) == Status.SUCCESS
    dec = jpeggpu_amd.Decoder()
    try:
        dec.set_progressive(True)
        dec.parse_header(sixty_four)
        assert dec.progressive_info().num_scans == 64 and dec.progressive_info().num_levels == 1
    finally:
        dec.cleanup()


def test_segment_shard_is_refused(L):
    prog = pc.pins()["p420_rst1"][0]
    assert parse_status(prog, shard=(0, 2)) == Status.NOT_SUPPORTED
    assert parse_status(prog, shard=(0, 1)) == Status.SUCCESS


def twin_cases():
    out = {n: p for n, (p, _, _) in pc.pins().items()}
    out.update({n: f for n, (f, _) in pc.crafted().items()})
    return out


def test_host_twin_equals_the_restatement():
    """Every (scan, segment) in level order through jg_prog_core.h: the coefficient buffers, padded blocks included, equal
    the restatement's on every pin and every crafted case, the scripts that stop early included; so do the levels."""
    cases = twin_cases()
    assert len(cases) == 10 + len(pc.CRAFTED)
    for name, data in cases.items():
        want = pr.decode(data)
        st, info, coef, back = prog_twin.decode(data)
        assert st == 0, name
        assert list(info.scan_level[:info.num_scans]) == want.levels, name
        assert info.num_levels == max(want.levels) + 1
        assert [info.scan_segments[k] for k in range(info.num_scans)] == [s["segments"] for s in want.scans], name
        for c in range(info.num_comp):
            assert coef[c].shape == want.coef[c].shape, (name, c)
            bad = np.argwhere(coef[c] != want.coef[c])
            assert len(bad) == 0, (name, c, bad[:4].tolist())


def test_pack_round_trip():
    """The hand-over's symbol stream read back by jg_defs.h's rules returns the visible blocks, escapes included."""
    escapes = 0
    for name, data in twin_cases().items():
        st, info, coef, back = prog_twin.decode(data)
        assert st == 0
        for c in range(info.num_comp):
            vis = coef[c][:info.vis_y[c], :info.vis_x[c]]
            assert np.array_equal(back[c], vis), (name, c)
            escapes += int((np.abs(vis[:, :, 1:].astype(np.int32)) >= 512).sum())
    assert escapes > 1000  # the dense_escapes coefficients reach the escape entries
