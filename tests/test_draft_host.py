"""libjpeg's scale mode on the host (jpeggpu_ext_set_scale_mode): the sizes, effective sampling factors and block sizes
parse_header reports, crop geometry, shard rows and refusals against tests/draft_ref.py; draft_scale against Pillow. No GPU
needed."""
import os

import numpy as np
import pytest

import jpeggpu_amd
from jpeggpu_amd import JpegGpuError, Status
from jpeggpu_amd import build as jbuild
from tests import cases, draft_ref
from tests.conftest import GOLDEN

SCALES = (1, 2, 4, 8)


@pytest.fixture(scope="module")
def L():
    jbuild.build()
    return jpeggpu_amd.lib()


@pytest.fixture(scope="module")
def files():
    return {k: v for k, v in draft_ref.inputs().items() if k != "photo"}


@pytest.fixture(scope="module")
def decoded(files):
    from oracle import oracle

    return {name: oracle.decode(data) for name, data in files.items()}


def parse(data, scale=1, mode="libjpeg", crop=None, shard=None, device_scan=False, shard_rows=False):
    """(info, scale_info, crop_info, layout, buffer size[, shard rows per component]) of one parse_header."""
    dec = jpeggpu_amd.Decoder()
    try:
        dec.set_scale(scale)
        if mode is not None:
            dec.set_scale_mode(mode)
        if crop is not None:
            dec.set_crop(*crop)
        if shard is not None:
            dec.set_segment_shard(*shard)
        if device_scan:
            dec.set_device_scan(True)
        info = dec.parse_header(data)
        out = (info, dec.scale_info(), dec.crop_info(), dec.layout(), dec.get_buffer_size())
        if shard_rows:
            out += ([dec.shard_rows(c) for c in range(info.num_components)],)
        return out
    finally:
        dec.cleanup()


def test_scale_mode_arguments(L, files):
    dec = jpeggpu_amd.Decoder()
    try:
        for bad in (-1, 2, 7):
            assert L.jpeggpu_ext_set_scale_mode(dec._h, bad) == Status.INVALID_ARGUMENT
        assert L.jpeggpu_ext_set_scale_mode(None, 1) == Status.INVALID_ARGUMENT
        with pytest.raises(ValueError):
            dec.set_scale_mode("draft")
        with pytest.raises(JpegGpuError) as e:  # nothing parsed yet
            dec.scale_info()
        assert e.value.status == Status.INVALID_ARGUMENT
        assert L.jpeggpu_ext_get_scale_info(dec._h, None) == Status.INVALID_ARGUMENT
        # takes effect at the next parse_header, like the scale
        dec.set_scale(2)
        a = dec.parse_header(files["ss_2x2"])
        dec.set_scale_mode("libjpeg")
        assert dec.scale_info().mode == 0 and list(dec.scale_info().block_size[:3]) == [4, 4, 4]
        b = dec.parse_header(files["ss_2x2"])
        assert dec.scale_info().mode == 1 and list(dec.scale_info().block_size[:3]) == [4, 8, 8]
        assert [a.sizes_x[c] for c in range(3)] == [100, 50, 50] and [b.sizes_x[c] for c in range(3)] == [100, 100, 100]
        dec.set_scale_mode("uniform")
        c = dec.parse_header(files["ss_2x2"])
        assert [c.sizes_x[k] for k in range(3)] == [100, 50, 50] and list(c.subsampling.x[:3]) == [2, 1, 1]
    finally:
        dec.cleanup()


def test_sizes_factors_and_block_sizes_of_every_file(L, files, decoded):
    n = 0
    for name, data in files.items():
        dec = decoded[name]
        hs, vs = draft_ref.factors_of(dec)
        for d in SCALES:
            info, si, ci, _, _ = parse(data, d)
            nc = info.num_components
            assert nc == dec.ncomp and si.scale_denom == d and si.mode == 1
            if d == 1:  # the mode changes nothing at scale 1
                want_sizes = [(p.shape[1], p.shape[0]) for p in dec.planes]
                want_blk, eh, ev = [8] * nc, hs, vs
            else:
                want_sizes = draft_ref.plane_sizes(dec.width, dec.height, hs, vs, d)
                want_blk = draft_ref.block_sizes(hs, vs, d)
                eh, ev = draft_ref.effective_factors(hs, vs, d)
            assert [(info.sizes_x[c], info.sizes_y[c]) for c in range(nc)] == want_sizes, (name, d)
            assert list(si.block_size[:nc]) == want_blk, (name, d)
            assert (list(info.subsampling.x[:nc]), list(info.subsampling.y[:nc])) == (eh, ev), (name, d)
            assert si.fancy_upsampling == (0 if d == 8 else 1), (name, d)
            assert [(ci.full_x[c], ci.full_y[c]) for c in range(nc)] == want_sizes
            assert (ci.width, ci.height) == (draft_ref.ceil_div(dec.width, d), draft_ref.ceil_div(dec.height, d))
            n += 1
    assert n >= 4 * 100


def test_uniform_mode_reports_what_it_did(L, files, decoded):
    from tests import scaled_ref

    for name, data in files.items():
        dec = decoded[name]
        hs, vs = draft_ref.factors_of(dec)
        for d in SCALES:
            for mode in (None, "uniform"):
                info, si, ci, _, _ = parse(data, d, mode=mode)
                nc = info.num_components
                want = [(scaled_ref.scaled_size(p.shape[1], d), scaled_ref.scaled_size(p.shape[0], d)) for p in dec.planes]
                assert [(info.sizes_x[c], info.sizes_y[c]) for c in range(nc)] == want, (name, d)
                assert (list(info.subsampling.x[:nc]), list(info.subsampling.y[:nc])) == (hs, vs), (name, d)
                assert si.mode == 0 and list(si.block_size[:nc]) == [8 // d] * nc and si.fancy_upsampling == 1


def test_buffer_size_and_layout_do_not_depend_on_the_mode(L, files):
    for name, data in files.items():
        for d in (2, 8):
            _, _, _, la, na = parse(data, d, mode="uniform")
            _, _, _, lb, nb = parse(data, d, mode="libjpeg")
            assert na == nb and la.transferred_bytes == lb.transferred_bytes and la.num_scans == lb.num_scans, (name, d)
            for i in range(la.num_scans):
                assert la.scans[i].num_subsequences == lb.scans[i].num_subsequences
                assert la.scans[i].num_data_units == lb.scans[i].num_data_units


def rectangles(rng, W, H):
    """Rectangles that touch every edge and corner, the whole image, single pixels, and seeded ones."""
    out = {(0, 0, W, H), (0, 0, 1, 1), (W - 1, 0, 1, 1), (0, H - 1, 1, 1), (W - 1, H - 1, 1, 1), (0, 0, W, 1), (0, H - 1, W, 1),
           (0, 0, 1, H), (W - 1, 0, 1, H), (0, H // 3, W, max(1, H // 3)), (W // 2, 0, max(1, W // 4), H)}
    for _ in range(12):
        w, h = int(rng.integers(1, W + 1)), int(rng.integers(1, H + 1))
        out.add((int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), w, h))
    return sorted(out)


def test_crop_windows_match_the_restatement(L, files, decoded):
    rng = np.random.default_rng(20261016)
    n = 0
    for name, data in files.items():
        dec = decoded[name]
        hs, vs = draft_ref.factors_of(dec)
        for d in SCALES:
            W, H = draft_ref.ceil_div(dec.width, d), draft_ref.ceil_div(dec.height, d)
            full, _, _, _, _ = parse(data, d)
            for rect in rectangles(rng, W, H):
                info, si, ci, _, _ = parse(data, d, crop=rect)
                win, _ = draft_ref.crop_windows(dec.width, dec.height, hs, vs, d, rect)
                assert (ci.x, ci.y, ci.width, ci.height) == rect
                for c in range(dec.ncomp):
                    got = (ci.origin_x[c], ci.origin_y[c], info.sizes_x[c], info.sizes_y[c])
                    assert got == win[c], (name, d, rect, c, got, win[c])
                    assert (ci.full_x[c], ci.full_y[c]) == (full.sizes_x[c], full.sizes_y[c])
                    assert (info.subsampling.x[c], info.subsampling.y[c]) == (full.subsampling.x[c], full.subsampling.y[c])
                if rect == (0, 0, W, H):
                    assert [(info.sizes_x[c], info.sizes_y[c]) for c in range(dec.ncomp)] == [(full.sizes_x[c], full.sizes_y[c]) for c in range(dec.ncomp)]
                n += 1
    assert n > 5000


@pytest.mark.parametrize("rect", [(0, 0, 101, 1), (0, 0, 1, 77), (100, 0, 1, 1), (0, 76, 1, 1), (90, 70, 11, 6)])
def test_rectangle_outside_the_scaled_image(L, files, rect):
    parse(files["ss_2x2"], 2, crop=(0, 0, 100, 76))  # 200 x 152 at 1/2
    with pytest.raises(JpegGpuError) as e:
        parse(files["ss_2x2"], 2, crop=rect)
    assert e.value.status == Status.INVALID_ARGUMENT


def test_band_crop_keeps_its_segments_as_in_uniform_mode(L, files, photo_bytes):
    """The restart-segment selection is unchanged: a rectangle covers the same MCUs whichever mode sizes the blocks."""
    for data in (files["dri_row"], files["dri_7"], photo_bytes):
        for d in (2, 4, 8):
            _, _, ci, lay_full, _ = parse(data, d)
            W, H = ci.width, ci.height
            rect = (W // 3, H // 3, max(1, W // 3), max(1, H // 9))
            _, _, _, la, _ = parse(data, d, mode="uniform", crop=rect)
            _, _, _, lb, _ = parse(data, d, mode="libjpeg", crop=rect)
            assert lb.scans[0].num_segments < lay_full.scans[0].num_segments
            # the halo is one sample of each component's own plane, so the window's MCU range can differ by the MCUs that
            # one chroma sample reaches in the uniform mode: never more segments than that mode keeps, plus none
            assert lb.scans[0].num_segments <= la.scans[0].num_segments


def test_segment_shards_work_and_report_rows_of_each_components_plane(L, files, decoded):
    """Shards are supported in this mode: a band is whole MCU rows, v_c S_c rows of component c each."""
    from tools import jpegsynth

    inputs = {"dri_row": files["dri_row"], "sweep:y2x4_rowdri": files["sweep:y2x4_rowdri"],
              "two_rows": jpegsynth.encode(333, 251, cases.S420, restart_interval=42, seed=78)}
    from oracle import oracle

    for name, data in inputs.items():
        dec = oracle.decode(data)
        hs, vs = draft_ref.factors_of(dec)
        for d in (2, 4, 8):
            sizes = draft_ref.plane_sizes(dec.width, dec.height, hs, vs, d)
            blk = draft_ref.block_sizes(hs, vs, d)
            for world in (2, 3):
                ends = [0] * dec.ncomp
                for rank in range(world):
                    info, _, _, lay, _, rows = parse(data, d, shard=(rank, world), shard_rows=True)
                    assert [(info.sizes_x[c], info.sizes_y[c]) for c in range(dec.ncomp)] == sizes
                    for c, (first, count) in enumerate(rows):
                        assert first == ends[c], (name, d, world, rank, c)  # the bands tile the plane
                        if rank + 1 < world:
                            assert (first + count) % (blk[c] * vs[c]) == 0 or first + count == sizes[c][1]
                        ends[c] = first + count
                assert ends == [s[1] for s in sizes], (name, d, world)


def test_shard_and_crop_still_do_not_go_together(L, files):
    with pytest.raises(JpegGpuError) as e:
        parse(files["dri_row"], 2, crop=(0, 0, 16, 16), shard=(0, 2))
    assert e.value.status == Status.NOT_SUPPORTED


def test_environment_switch(L, files, monkeypatch):
    monkeypatch.setenv("JPEGGPU_SCALE_MODE", "libjpeg")
    dec = jpeggpu_amd.Decoder()
    try:
        dec.set_scale(2)
        info = dec.parse_header(files["ss_2x2"])
        assert dec.scale_info().mode == 1 and [info.sizes_x[c] for c in range(3)] == [100] * 3
    finally:
        dec.cleanup()
    monkeypatch.setenv("JPEGGPU_SCALE_MODE", "uniform")
    dec = jpeggpu_amd.Decoder()
    try:
        dec.set_scale(2)
        info = dec.parse_header(files["ss_2x2"])
        assert dec.scale_info().mode == 0 and [info.sizes_x[c] for c in range(3)] == [100, 50, 50]
    finally:
        dec.cleanup()


def test_draft_scale_against_the_pinned_table():
    table = np.load(os.path.join(GOLDEN, "draft_pins.npz"))["draft_scale"]
    assert len(table) > 300 and set(table[:, 4].tolist()) == {1, 2, 4, 8}
    for w, h, rw, rh, s in table.tolist():
        assert jpeggpu_amd.draft_scale(w, h, (rw, rh)) == s, (w, h, rw, rh, s)
    with pytest.raises(ValueError):
        jpeggpu_amd.draft_scale(10, 10, (0, 5))


def test_draft_scale_against_pillow(files, decoded):
    pytest.importorskip("PIL")
    import io

    from PIL import Image

    rng = np.random.default_rng(99)
    n = 0
    for name, data in files.items():
        dec = decoded[name]
        if not draft_ref.has_rgb(dec):
            continue
        for _ in range(6):
            req = (int(rng.integers(1, 2 * dec.width + 2)), int(rng.integers(1, 2 * dec.height + 2)))
            if n % 3 == 0:
                req = (max(1, dec.width // int(rng.integers(1, 12))), max(1, dec.height // int(rng.integers(1, 12))))
            im = Image.open(io.BytesIO(data))
            got = im.draft("RGB", req)
            s = jpeggpu_amd.draft_scale(dec.width, dec.height, req)
            assert im.size == (draft_ref.ceil_div(dec.width, s), draft_ref.ceil_div(dec.height, s)), (name, req, s, got)
            n += 1
    assert n > 500


def test_draft_kernels_use_no_scratch(L):
    meta = jbuild.kernel_metadata(jbuild.device_assembly(source="jg_idct.hip"))
    draft = {k: v for k, v in meta.items() if "DraftJobs" in k}
    assert sum("idct_kernel" in k for k in draft) == 4 and sum("idct_scaled_kernel" in k for k in draft) == 12, sorted(draft)
    for k, v in draft.items():
        assert v.get("private_seg_size", 1) == 0 and v.get("uses_dynamic_stack", 0) == 0, (k, v)
        assert v["num_vgpr"] <= (256 if "idct_scaled_kernel" in k else 128), (k, v)  # the bounds of the other instantiations
