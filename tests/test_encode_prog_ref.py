"""The restatement of progressive encoding (tests/encode_prog_ref.py) against Pillow's pinned progressive=True files
(tests/golden/encode_prog_pins.npz), what its edge images reach, and a live Pillow where one on libjpeg-turbo is importable.
No GPU needed."""
import io

import numpy as np
import pytest

from tests import encode_cases as K
from tests import encode_prog_ref as R
from tests import encode_ref as E

CASES = K.cases()
EDGES = R.edge_cases()


@pytest.fixture(scope="module")
def edge_files():
    """The restatement's file and statistics of every edge image, made once."""
    out = {}
    for c, img in EDGES:
        stats = {}
        out[c["name"]] = (R.encode(img, c["quality"], c["subsampling"], c["restart_interval"], stats), stats)
    return out


def test_restatement_equals_every_pin(edge_files):
    """All cases of encode_cases.cases() and the edge images, none left out."""
    pins = R.pins()[0]
    assert len(pins) == len(CASES) + len(EDGES) and len(EDGES) == 11
    wrong = [c["name"] for c in CASES if not R.equals_pin(c["name"], R.encode(K.image(c), c["quality"], c["subsampling"], c["restart_interval"]))]
    wrong += [name for name, (data, _) in edge_files.items() if not R.equals_pin(name, data)]
    assert not wrong, wrong
    assert R.pins()[1] == K.pins()[1], "both pin files come from the same Pillow and libjpeg-turbo"


def test_single_symbol_tables(edge_files):
    """8 x 8 zeros: every AC scan is one run of one block, and every table has one symbol."""
    stats = edge_files["prog_zero_8x8_grey"][1]
    assert stats["max_run"] == 1
    assert [len(s) for s in stats["scans"]] == [1, 1, 1, 1, 0, 1]
    assert all(sym == 0x00 for s in stats["scans"][1:] for (_, _, sym) in s)


def test_luma_scans_walk_real_blocks_only():
    c, img = EDGES[2]
    assert c["name"] == "prog_37x53_rgb_420" and img.shape == (37, 53, 3)
    co = E.coefficients(img, 2, 2, c["quality"])
    assert len(R.scan_blocks(co, (0,))[0]) == 7 * 5 and co["mcus_x"] * 2 * co["mcus_y"] * 2 == 8 * 6
    assert len(R.scan_blocks(co, (1,))[0]) == 4 * 3 and len(R.scan_blocks(co, (0, 1, 2))[0]) == 4 * 3 * 6


def test_flat_image_runs_end_at_the_cap(edge_files):
    data, stats = edge_files["prog_flat_1456_grey"]
    assert len(data) == 8584 and stats["cap_flushes"] == 4 and stats["max_run"] == 0x7FFF and stats["be_flushes"] == 0


def test_a_block_ends_a_long_run(edge_files):
    """Behind the last block the noise touches, 17 070 blocks make one run; no run reaches the cap."""
    data, stats = edge_files["prog_flat_1456_grey_one_block"]
    assert stats["max_run"] == 17070 and stats["cap_flushes"] == 0


def test_pending_correction_bits_end_runs(edge_files):
    data, stats = edge_files["prog_binary_256_grey_q100"]
    assert len(data) == 75909 and stats["be_flushes"] == 3 and stats["cap_flushes"] == 0
    assert edge_files["prog_binary_256_grey_q100_r40"][1]["be_flushes"] >= 1


def test_segments_end_runs(edge_files):
    stats = edge_files["prog_flat_400_grey_r100"][1]
    assert stats["max_run"] == 100 and stats["cap_flushes"] == stats["be_flushes"] == 0


def test_refinement_zrl_and_long_tail_in_one_file(edge_files):
    stats = edge_files["prog_long_tail_32_grey_q100"][1]
    assert stats["refine_zrl"] >= 1 and stats["refine_long_tail"] >= 1


def test_live_pillow_on_a_seeded_sweep():
    Image = pytest.importorskip("PIL.Image")
    from PIL import ImageFile, features

    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("this Pillow is not built on libjpeg-turbo")
    rng = np.random.default_rng(4321)
    saved = ImageFile.MAXBLOCK
    ImageFile.MAXBLOCK = 1 << 24
    try:
        for _ in range(40):
            h, w = (int(v) for v in rng.integers(1, 60, 2))
            grey = bool(rng.integers(0, 2))
            img = rng.integers(0, 256, (h, w) if grey else (h, w, 3), dtype=np.uint8)
            kind = int(rng.integers(0, 3))
            if kind == 1:
                img = (img // 64 * 64).astype(np.uint8)
            elif kind == 2:  # nearly flat: long end-of-band runs
                img = (120 + (img > 250) * 60).astype(np.uint8)
            q, s, r = int(rng.integers(1, 101)), ["4:4:4", "4:2:2", "4:2:0"][int(rng.integers(0, 3))], [0, 1, 2, 3][int(rng.integers(0, 4))]
            f = io.BytesIO()
            Image.fromarray(img).save(f, "JPEG", quality=q, subsampling=E.PILLOW_SUBSAMPLING[E.SUBSAMPLINGS[s]], restart_marker_blocks=r, progressive=True)
            assert R.encode(img, q, s, r) == f.getvalue(), (h, w, grey, kind, q, s, r)
    finally:
        ImageFile.MAXBLOCK = saved
