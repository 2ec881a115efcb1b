"""Every legal sampling layout (tests/cases.sampling_sweep) on the host: the files are what Pillow decodes
(tests/golden/sampling_pins.json, written by tools/make_sampling_pins.py), the emulation twin of the device pipeline is
exact on every scan, parse_header's plane sizes and crop windows follow their stated formulas, every crop window holds
the samples libjpeg's upsampler reads, and the one illegal MCU is refused."""
import hashlib
import json
import os

import numpy as np
import pytest

import jpeggpu_amd
from jpeggpu_amd import JpegGpuError, Status
from jpeggpu_amd import build as jbuild
from oracle import oracle
from tests import cases, libjpeg_ref
from tests.conftest import GOLDEN
from tests.emu import emu
from tests.test_crop_host import expected_window, parse, rectangles

SCALES = (1, 2, 4, 8)


@pytest.fixture(scope="module")
def L():
    jbuild.build()
    return jpeggpu_amd.lib()


@pytest.fixture(scope="module")
def corpus():
    return cases.sampling_sweep()


@pytest.fixture(scope="module")
def refs(corpus):
    return {k: oracle.decode(d) for k, d in corpus.items() if not cases.sweep_is_refused(k)}


def _sha(b):
    return hashlib.sha256(np.ascontiguousarray(b).tobytes() if isinstance(b, np.ndarray) else b).hexdigest()


def test_corpus_covers_what_it_claims(corpus, refs):
    """Every layout at two sizes whose last MCU is partial on both axes with wholly invisible blocks; 7 to 10 units per
    MCU; vertical factors 3 and 4; the variants."""
    units = set()
    for name, samp in cases.SWEEP_LAYOUTS.items():
        hmax, vmax = max(h for h, _ in samp), max(v for _, v in samp)
        units.add(sum(h * v for h, v in samp))
        for kind in ("a", "b"):
            dec = refs["%s_%s" % (name, kind)]
            assert (dec.hs, dec.vs) == ([h for h, _ in samp], [v for _, v in samp]), name
            for size, f in ((dec.width, hmax), (dec.height, vmax)):
                last = size % (8 * f)
                assert last != 0, (name, kind)
                if f > 1:
                    assert last <= 8 * (f - 1), (name, kind, "no wholly invisible block in the last MCU")
    assert set(range(3, 11)) <= units
    assert len(cases.SWEEP_LAYOUTS) == 22
    for name in cases.SWEEP_VARIANTS:
        assert refs[name + "_ni"].nscans == 3 and refs[name + "_dri"].restart_interval > 0
        mcus_x = -(-refs[name + "_dri"].width // (8 * max(refs[name + "_dri"].hs)))
        assert mcus_x % refs[name + "_dri"].restart_interval != 0, name
    for name in cases.SWEEP_TINY:  # an upsampled plane at most 2 samples wide (h2v1 / h2v2: replication)
        dec = refs[name + "_tiny"]
        assert any(max(dec.hs) // h >= 2 and p.shape[1] <= 2 for h, p in zip(dec.hs, dec.planes)), name
    assert sum(cases.sweep_is_planes_only(k) for k in corpus) == 4 and sum(cases.sweep_is_refused(k) for k in corpus) == 1


def _pins():
    with open(os.path.join(GOLDEN, "sampling_pins.json")) as f:
        return json.load(f)


def test_corpus_is_pinned_and_equals_pillow(corpus, refs):
    """The files are the pinned ones, and what Pillow (libjpeg-turbo) decoded from them at authoring time is what the
    numpy restatement of libjpeg (tests/libjpeg_ref.py) gives from the oracle's coefficients: the RGB of the integral
    files, the ISLOW planes of the others. Where Pillow is importable, also against Pillow itself."""
    pins = _pins()
    assert sorted(pins) == sorted(corpus)
    try:
        import PIL  # noqa: F401
        from tools.make_sampling_pins import pillow_image
    except ImportError:  # no Pillow: the pins carry the check
        pillow_image = None
    for name, data in corpus.items():
        pin = pins[name]
        assert _sha(data) == pin["jpeg_sha256"], name
        assert ("pillow" in pin) == (cases.sweep_is_refused(name) or name.startswith("po_y3") or name.startswith("po_two")), name
        if cases.sweep_is_refused(name):
            continue
        dec = refs[name]
        if cases.sweep_is_planes_only(name):
            assert "rgb_sha256" not in pin
            assert [_sha(p) for p in libjpeg_ref.islow_planes_of(dec)] == pin["planes_sha256"], name
        else:
            want = libjpeg_ref.libjpeg_rgb_of(dec)
            assert _sha(want) == pin["rgb_sha256"], name
        if pillow_image is not None:
            im = pillow_image(data)
            assert (im is None) == ("pillow" in pin), name
            if "rgb_sha256" in pin:
                assert np.array_equal(np.asarray(im.convert("RGB")), want), name


@pytest.mark.parametrize("subseq_bytes,max_intra_iters", [(128, 256), (32, 256), (256, 1), (32, 1), (64, 2), (64, 255)])
def test_emulated_pipeline_is_exact(corpus, refs, subseq_bytes, max_intra_iters):
    """tests/emu against oracle.scan_stages on every scan of every file: the sync state's unit counter cycles over 1 to
    10 units per MCU, the DC sums are per component; with the multi-hypothesis tables at 64 / 32 bytes too."""
    for name, data in corpus.items():
        if cases.sweep_is_refused(name):
            continue
        for s in range(refs[name].nscans):
            tw = oracle.scan_stages(data, s, subseq_bytes)
            ok = tw.p >= 0
            for mh in (False, True) if max_intra_iters == 256 else (False,):
                rc, r = emu.decode_scan(data, s, subseq_bytes, max_intra_iters, multi_hypothesis=mh)
                what = (name, s, subseq_bytes, max_intra_iters, mh)
                assert rc == 0, what
                assert np.array_equal(r.destuffed, tw.destuffed) and np.array_equal(r.seg_index, tw.seg_index), what
                assert np.array_equal(r.p[ok], tw.p[ok]) and np.array_equal(r.n[ok], tw.n[ok]), what
                assert np.array_equal(r.cz[ok], tw.cz[ok]), what
                for k in range(4):
                    assert np.array_equal(r.dc[k][ok].astype(np.int16), tw.dc[k][ok].astype(np.int16)), what
                assert np.array_equal(r.coef, tw.stream_coef), what


def test_plane_sizes_at_every_scale(L, corpus, refs):
    """sizes_x[c] = ceil(X h_c / (h_max d)), likewise sizes_y; a single component's factors are ignored."""
    for name, data in corpus.items():
        if cases.sweep_is_refused(name):
            continue
        dec = refs[name]
        hs, vs = (dec.hs, dec.vs) if dec.ncomp > 1 else ([1], [1])
        for d in SCALES:
            info, ci, _, _ = parse(data, d)
            assert info.num_components == dec.ncomp, name
            for c in range(dec.ncomp):
                want = (-(-dec.width * hs[c] // (max(hs) * d)), -(-dec.height * vs[c] // (max(vs) * d)))
                assert (info.sizes_x[c], info.sizes_y[c]) == want, (name, d, c)
                assert (info.subsampling.x[c], info.subsampling.y[c]) == (dec.hs[c], dec.vs[c]), (name, c)
            assert (ci.width, ci.height) == (-(-dec.width // d), -(-dec.height // d)), (name, d)


def _needed(lo, hi, r, fancy, size):
    """The samples libjpeg's upsampler reads for output pixels lo..hi of one axis at ratio r: floor(x / r) for
    replication (and a copy), one more on each side for the fancy modes, clipped to the plane."""
    a, b = lo // r, hi // r
    if fancy:
        a, b = a - 1, b + 1
    return max(a, 0), min(b, size - 1)


def _modes(full, c):
    """(horizontal fancy, vertical fancy) of component c as jdsample.c picks them from the full plane's width."""
    n = full.num_components
    hs, vs = list(full.subsampling.x[:n]), list(full.subsampling.y[:n])
    if n == 1:
        return False, False
    hr, vr = max(hs) // hs[c], max(vs) // vs[c]
    if (hr, vr) in ((2, 1), (2, 2)) and full.sizes_x[c] > 2:
        return True, vr == 2
    return False, (hr, vr) == (1, 2)


def _seeded_rectangles(rng, width, height, count):
    out = []
    for _ in range(count):
        w = int(rng.integers(1, width + 1))
        h = int(rng.integers(1, height + 1))
        out.append((int(rng.integers(0, width - w + 1)), int(rng.integers(0, height - h + 1)), w, h))
    return out


def test_crop_windows(L, corpus, refs):
    """For many rectangles per file and scale: get_crop equals the restatement of jpeggpu_ext.h
    (test_crop_host.expected_window); independently of it, every window holds each sample the upsampler reads for the
    rectangle and starts on the MCU grid (the block grid for a scan of one component)."""
    rng = np.random.default_rng(11)
    checked = 0
    for name, data in corpus.items():
        if cases.sweep_is_refused(name):
            continue
        dec = refs[name]
        n = dec.ncomp
        for d in SCALES:
            full, full_ci, _, _ = parse(data, d)
            width, height = full_ci.width, full_ci.height
            hs, vs = list(full.subsampling.x[:n]), list(full.subsampling.y[:n])
            if n == 1:
                hs, vs = [1], [1]
            blk = 8 // d
            rects = rectangles(width, height) + _seeded_rectangles(rng, width, height, 24)
            for rx, ry in ((1, 1), (max(hs), max(vs))):  # starting at x = hr - 1, y = vr - 1 (mod the ratio)
                x, y = min(rx * 3 - 1, width - 1), min(ry * 3 - 1, height - 1)
                rects.append((x, y, min(7, width - x), min(5, height - y)))
            mw, mh = 8 * max(hs) // d, 8 * max(vs) // d  # the last partial MCU alone
            lx, ly = (width - 1) // mw * mw, (height - 1) // mh * mh
            rects.append((lx, ly, width - lx, height - ly))
            for rect in rects:
                x, y, w, h = rect
                info, ci, _, _ = parse(data, d, crop=rect)
                win, _ = expected_window(full, d, rect)
                mcu_x = set()
                for c in range(n):
                    ox, oy, sx, sy = ci.origin_x[c], ci.origin_y[c], info.sizes_x[c], info.sizes_y[c]
                    what = (name, d, rect, c)
                    assert (ox, oy, sx, sy) == win[c], what
                    hr, vr = max(hs) // hs[c], max(vs) // vs[c]
                    fx, fy = _modes(full, c)
                    if max(hs) % hs[c] == 0 and max(vs) % vs[c] == 0:  # libjpeg's upsampler takes integral ratios only
                        ax, bx = _needed(x, x + w - 1, hr, fx, full.sizes_x[c])
                        ay, by = _needed(y, y + h - 1, vr, fy, full.sizes_y[c])
                        assert ox <= ax and bx < ox + sx and oy <= ay and by < oy + sy, what
                    assert ox + sx <= full.sizes_x[c] and oy + sy <= full.sizes_y[c], what
                    if dec.nscans == 1 and n > 1:
                        assert ox % (blk * hs[c]) == 0 and oy % (blk * vs[c]) == 0, what
                        mcu_x.add((ox // (blk * hs[c]), oy // (blk * vs[c])))
                    else:
                        assert ox % blk == 0 and oy % blk == 0, what
                assert len(mcu_x) <= 1, (name, d, rect, mcu_x)
                checked += 1
    assert checked > 12000


def test_the_11_unit_mcu_is_refused_and_the_non_integral_ratio_parses(L, corpus, refs):
    for name, data in corpus.items():
        if not cases.sweep_is_refused(name):
            continue
        with pytest.raises(JpegGpuError) as e:
            parse(data)
        assert e.value.status == Status.INVALID_JPEG, name
    for name in ("po_y3x1_cb2x1", "po_y3x1_cb2x1_dri"):
        info, _, lay, _ = parse(corpus[name])
        assert [info.sizes_x[c] for c in range(3)] == [p.shape[1] for p in refs[name].planes], name
        assert lay.scans[0].data_units_per_mcu == 6
    _, _, lay, _ = parse(corpus["po_two_1x1_3x3"])
    assert lay.scans[0].data_units_per_mcu == 10
