"""Every legal sampling layout (tests/cases.sampling_sweep) on the GPU, bit-exact against the CPU references: the stage
buffers of the Huffman path (the sync state's unit counter cycles over 1 to 10 units per MCU), the placement of every
IDCT (reference, ISLOW, 1/2, 1/4, 1/8, cropped) with partial MCUs that hold wholly invisible blocks, fancy and legacy RGB
(a per-component choice of upsampler, luma included), crops, batches on every plan, the batched resize and segment
shards of 24- and 32-line MCU rows. Every plane and every RGB output lies inside guard bytes."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

from tests import cases, libjpeg_ref, scaled_ref
from tests import pillow_resample_ref as R
from tests.conftest import GOLDEN
from tests.test_crop_host import rectangles
from tests.test_gpu_crop import _batch_decode as crop_batch_decode
from tests.test_gpu_crop import assert_window
from tests.test_gpu_scaled import GUARD, Guarded, _tmp
from tests.test_gpu_slow_sync import _assert_planes, _batch, check_stages

pytestmark = pytest.mark.gpu

KINDS = ((1, "reference"), (1, "islow"), (2, "reference"), (4, "reference"), (8, "reference"))


@pytest.fixture(scope="module")
def torch_cuda(gpu_lib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def corpus():
    return {k: v for k, v in cases.sampling_sweep().items() if not cases.sweep_is_refused(k)}


@pytest.fixture(scope="module")
def refs(corpus):
    from oracle import oracle

    return {k: oracle.decode(d) for k, d in corpus.items()}


@pytest.fixture(scope="module")
def pins():
    with open(os.path.join(GOLDEN, "sampling_pins.json")) as f:
        return json.load(f)


def _rgb_names(corpus):
    return [k for k in corpus if not cases.sweep_is_planes_only(k)]


def want_planes(ref, scale, method):
    if scale != 1:
        return scaled_ref.scaled_planes_of(ref, scale)
    return libjpeg_ref.islow_planes_of(ref) if method == "islow" else ref.planes


class Tight:
    """Planes with pitch = width in one buffer each, two guard rows above and below: a write past a row's end lands in
    the next row (and shows as a wrong sample), a write past the plane in the guards."""

    def __init__(self, torch, info):
        self.bufs, self.ptrs, self.pitches, self.shape = [], [], [], []
        for c in range(info.num_components):
            w, h = info.sizes_x[c], info.sizes_y[c]
            buf = torch.full(((h + 4) * w,), GUARD, dtype=torch.uint8, device="cuda:0")
            self.bufs.append(buf)
            self.ptrs.append(buf.data_ptr() + 2 * w)
            self.pitches.append(w)
            self.shape.append((h, w))

    def planes(self):
        out = []
        for buf, (h, w) in zip(self.bufs, self.shape):
            a = buf.cpu().numpy()
            assert (a[:2 * w] == GUARD).all() and (a[(h + 2) * w:] == GUARD).all(), "a guard row around the plane was written"
            out.append(a[2 * w:(h + 2) * w].reshape(h, w).copy())
        return out


def rgb_fancy(torch, planes, info, width, height, expect=0):
    """jpeggpu_ext_planes_to_rgbi_fancy into rows of 3 width + 5 bytes (unaligned) with a guard row below: (H, W, 3)."""
    import jpeggpu_amd
    from jpeggpu_amd.api import Img

    src = Img()
    for c in range(info.num_components):
        src.image[c], src.pitch[c] = planes[c].data_ptr(), planes[c].stride(0)
    pitch = 3 * width + 5
    out = torch.full((height + 1, pitch), GUARD, dtype=torch.uint8, device="cuda:0")
    st = jpeggpu_amd.lib().jpeggpu_ext_planes_to_rgbi_fancy(C.byref(info), C.byref(src), out.data_ptr(), pitch, width, height, None)
    assert st == expect, jpeggpu_amd.status_string(st)
    torch.cuda.synchronize()
    a = out.cpu().numpy()
    if expect != 0:
        assert (a == GUARD).all(), "a refused call wrote"
        return None
    assert (a[:, 3 * width:] == GUARD).all() and (a[height] == GUARD).all(), "wrote past the image"
    return a[:height, :3 * width].reshape(height, width, 3).copy()


def crop_rgb(torch, g, info, ci, expect=0):
    """jpeggpu_ext_crop_to_rgbi_fancy of guarded window planes into a guarded output: (h, w, 3)."""
    import jpeggpu_amd
    from jpeggpu_amd.api import Img

    w, h = ci.width, ci.height
    buf = torch.full((h + 2, 3 * w + 24), GUARD, dtype=torch.uint8, device="cuda:0")
    src = Img()
    for c in range(info.num_components):
        src.image[c], src.pitch[c] = g.ptrs[c], g.pitches[c]
    st = jpeggpu_amd.lib().jpeggpu_ext_crop_to_rgbi_fancy(C.byref(info), C.byref(ci), C.byref(src), buf[1:, 8:].data_ptr(), buf.stride(0), None)
    assert st == expect, jpeggpu_amd.status_string(st)
    torch.cuda.synchronize()
    a = buf.cpu().numpy()
    if expect != 0:
        assert (a == GUARD).all(), "a refused call wrote"
        return None
    out = a[1:1 + h, 8:8 + 3 * w].copy()
    a[1:1 + h, 8:8 + 3 * w] = GUARD
    assert (a == GUARD).all(), "a guard byte around the RGB output was written"
    return out.reshape(h, w, 3)


def decode(torch, data, scale=1, method="reference", crop=None, device_scan=False, subseq_bytes=None, tight=False, rgb=False):
    """One lone decode into guarded planes: (planes, info, crop_info, layout, rgb of the rectangle or None)."""
    import jpeggpu_amd

    dec = jpeggpu_amd.Decoder(subseq_bytes)
    try:
        dec.set_scale(scale)
        dec.set_idct(method)
        dec.set_device_scan(device_scan)
        if crop is not None:
            dec.set_crop(*crop)
        info = dec.parse_header(data)
        ci = dec.crop_info()
        lay = dec.layout()
        n = dec.get_buffer_size()
        tmp, base = _tmp(torch, n)
        g = (Tight if tight else Guarded)(torch, info)
        dec.transfer(base, n, 0)
        dec.decode(g.ptrs, g.pitches, base, n, 0)
        torch.cuda.synchronize()
        if device_scan:
            assert dec.device_status(base, 0) == jpeggpu_amd.Status.SUCCESS
        out = crop_rgb(torch, g, info, ci) if rgb else None
        return g.planes(), info, ci, lay, out
    finally:
        dec.cleanup()


def image_size(info):
    n = info.num_components
    hs, vs = list(info.subsampling.x[:n]), list(info.subsampling.y[:n])
    return info.sizes_x[hs.index(max(hs))], info.sizes_y[vs.index(max(vs))]


@pytest.mark.parametrize("subseq_bytes", [None, 32])
@pytest.mark.parametrize("device_scan", [False, True])
def test_stage_parity(torch_cuda, corpus, refs, subseq_bytes, device_scan):
    """Every stage buffer of every scan against its CPU twin: destuffed bytes, segment index, the sync states (p, n,
    (c, z)) and DC sums per component, the symbol stream; then the planes."""
    import jpeggpu_amd

    for name, data in corpus.items():
        planes, info, tmp, base, lay = jpeggpu_amd.decode_to_planes(data, subseq_bytes=subseq_bytes, return_tmp=True,
                                                                    device_scan=device_scan)
        what = (name, subseq_bytes, device_scan)
        check_stages(torch_cuda, data, tmp, base, lay, lay.subsequence_bytes, what)
        _assert_planes([p.cpu().numpy() for p in planes], refs[name].planes, what)


def test_lone_decodes_guarded(torch_cuda, corpus, refs):
    """The reference IDCT, the ISLOW IDCT and the reduced IDCTs: each with pitch = width and with slack columns of guard
    bytes, against the oracle, libjpeg_ref and scaled_ref."""
    for name, data in corpus.items():
        for scale, method in KINDS:
            want = want_planes(refs[name], scale, method)
            for tight in (True, False):
                got, info, _, _, _ = decode(torch_cuda, data, scale, method, tight=tight)
                _assert_planes(got, want, (name, scale, method, "pitch = width" if tight else "slack"))


def test_fancy_rgb_equals_the_restatement_and_pillow(torch_cuda, corpus, refs, pins):
    """jpeggpu_ext_planes_to_rgbi_fancy on ISLOW planes: libjpeg_ref.planes_to_rgb_fancy and the Pillow pin."""
    import jpeggpu_amd

    for name in _rgb_names(corpus):
        planes, info = jpeggpu_amd.decode_to_planes(corpus[name], idct="islow")
        W, H = image_size(info)
        dec = refs[name]
        assert (W, H) == (dec.width, dec.height), name
        got = rgb_fancy(torch_cuda, planes, info, W, H)
        n = info.num_components
        want = libjpeg_ref.planes_to_rgb_fancy([p.cpu().numpy() for p in planes], list(info.subsampling.x[:n]),
                                               list(info.subsampling.y[:n]), W, H)
        bad = np.argwhere(got != want)
        assert len(bad) == 0, (name, len(bad), bad[:4].tolist())
        assert hashlib.sha256(got.tobytes()).hexdigest() == pins[name]["rgb_sha256"], name


def test_rgb_calls_refuse_what_libjpeg_refuses(torch_cuda, corpus):
    """A non-integral ratio (and 2 or 4 components): NOT_SUPPORTED from the three RGB calls, and nothing written."""
    import jpeggpu_amd
    from tests.test_gpu_resize import run

    status = int(jpeggpu_amd.Status.NOT_SUPPORTED)
    good = jpeggpu_amd.decode_to_planes(corpus["y2x2_a"])
    for name in [k for k in corpus if cases.sweep_is_planes_only(k)]:
        planes, info = jpeggpu_amd.decode_to_planes(corpus[name])
        W, H = max(p.shape[1] for p in planes), max(p.shape[0] for p in planes)
        rgb_fancy(torch_cuda, planes, info, W, H, expect=status)
        cw, ch = min(W, 20), min(H, 9)
        _, cinfo, ci, _, _ = decode(torch_cuda, corpus[name], crop=(W - cw, 3, cw, ch))
        g = Guarded(torch_cuda, cinfo)
        crop_rgb(torch_cuda, g, cinfo, ci, expect=status)
        run(torch_cuda, [(good[0], good[1], None), (planes, info, None)], 16, 12, expect=status)


def test_legacy_rgb_and_upsample(torch_cuda, corpus):
    """jpeggpu_ext_upsample_planes: dst[y][x] = src[min(y v_c / v_max, h - 1)][min(x h_c / h_max, w - 1)], exact;
    jpeggpu_ext_planes_to_rgbi: the oracle's restatement of the reference's helper within 1 LSB (float, maybe FMA)."""
    import jpeggpu_amd
    from jpeggpu_amd.api import Img
    from oracle import oracle

    torch = torch_cuda
    L = jpeggpu_amd.lib()
    for name in _rgb_names(corpus):
        planes, info = jpeggpu_amd.decode_to_planes(corpus[name])
        n = info.num_components
        hs, vs = list(info.subsampling.x[:n]), list(info.subsampling.y[:n])
        W, H = image_size(info)
        src, dst = Img(), Img()
        outs = []
        for c in range(n):
            src.image[c], src.pitch[c] = planes[c].data_ptr(), planes[c].stride(0)
            o = torch.full((H + 1, W + 3), GUARD, dtype=torch.uint8, device="cuda:0")
            outs.append(o)
            dst.image[c], dst.pitch[c] = o.data_ptr(), o.stride(0)
        assert L.jpeggpu_ext_upsample_planes(C.byref(info), C.byref(src), C.byref(dst), W, H, None) == 0, name
        torch.cuda.synchronize()
        for c in range(n):
            p = planes[c].cpu().numpy()
            ys = np.minimum(np.arange(H) * vs[c] // max(vs), p.shape[0] - 1)
            xs = np.minimum(np.arange(W) * hs[c] // max(hs), p.shape[1] - 1)
            o = outs[c].cpu().numpy()
            assert (o[:, W:] == GUARD).all() and (o[H] == GUARD).all(), (name, c, "wrote past the plane")
            assert np.array_equal(o[:H, :W], p[ys][:, xs]), (name, c)
        pitch = 3 * W + 5
        out = torch.full((H + 1, pitch), GUARD, dtype=torch.uint8, device="cuda:0")
        assert L.jpeggpu_ext_planes_to_rgbi(C.byref(info), C.byref(src), out.data_ptr(), pitch, W, H, None) == 0, name
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert (got[:, 3 * W:] == GUARD).all() and (got[H] == GUARD).all(), (name, "wrote past the image")
        got = got[:H, :3 * W].reshape(H, W, 3).astype(np.int32)
        ref = oracle.planes_to_rgbi([p.cpu().numpy() for p in planes], hs, vs, W, H).astype(np.int32)
        diff = np.abs(got - ref)
        assert diff.max() <= 1, (name, int(diff.max()))
        assert (diff == 0).mean() > 0.999, (name, float((diff == 0).mean()))


def crop_rectangles(width, height, hr, vr, mcu_w, mcu_h):
    """test_crop_host.rectangles, rectangles that start at x = hr - 1, y = vr - 1 (mod the ratio) and the last partial
    MCU alone."""
    out = list(rectangles(width, height))
    for k in (1, 3):
        x, y = min(k * hr - 1, width - 1), min(k * vr - 1, height - 1)
        out.append((x, y, min(2 * hr + 1, width - x), min(2 * vr + 1, height - y)))
    lx, ly = (width - 1) // mcu_w * mcu_w, (height - 1) // mcu_h * mcu_h
    out.append((lx, ly, width - lx, height - ly))
    return sorted(set(out))


def test_crops_at_every_kind(torch_cuda, corpus, refs):
    """Cropped decodes at every kind: the window planes equal the uncropped planes' windows, and (integral files) the
    rectangle's RGB equals the full fancy RGB sliced. On the restart-marker files parse_header drops segments outside
    the rectangle, and the windows stay right."""
    import jpeggpu_amd

    n_rects = dropped = 0
    for name, data in corpus.items():
        ref = refs[name]
        has_rgb = not cases.sweep_is_planes_only(name)
        hr = max(ref.hs) // min(ref.hs) if max(ref.hs) % min(ref.hs) == 0 else 1
        vr = max(ref.vs) // min(ref.vs) if max(ref.vs) % min(ref.vs) == 0 else 1
        for scale, method in KINDS:
            full, finfo, fci, flay, _ = decode(torch_cuda, data, scale, method)
            _assert_planes(full, want_planes(ref, scale, method), (name, scale, method))
            if has_rgb:
                fp, fi = jpeggpu_amd.decode_to_planes(data, scale=scale, idct=method)
                W, H = image_size(fi)
                full_rgb = rgb_fancy(torch_cuda, fp, fi, W, H)
            mw, mh = -(-8 * max(ref.hs) // scale), -(-8 * max(ref.vs) // scale)
            for rect in crop_rectangles(fci.width, fci.height, hr, vr, mw, mh):
                planes, info, ci, lay, rgb = decode(torch_cuda, data, scale, method, crop=rect, rgb=has_rgb)
                what = (name, scale, method, rect)
                assert_window(planes, full, info, ci, what)
                if has_rgb:
                    x, y, w, h = rect
                    assert np.array_equal(rgb, full_rgb[y:y + h, x:x + w]), what
                if ref.restart_interval and lay.scans[0].num_segments < flay.scans[0].num_segments:
                    dropped += 1
                n_rects += 1
    assert n_rects > 3000 and dropped > 100, (n_rects, dropped)


def test_full_batch_plan(torch_cuda, corpus, refs, monkeypatch):
    """All sweep files in one jpeggpu_ext_decode_batch on the full batch's plan: the fused tail + write launch on and
    off, and a caller's cap of 1 and 3 flow iterations; every item stage by stage and its planes."""
    import jpeggpu_amd

    monkeypatch.setenv("JPEGGPU_EXP_KEEP_FLOWS_BELOW", "0")  # read at jpeggpu_ext_batch_create
    names = list(corpus)
    for iters, fused in ((None, True), (None, False), (1, None), (3, None)):
        got, _ = _batch(torch_cuda, [corpus[k] for k in names], iters=iters, fused=fused, device_scan_every=3)
        for name, planes in zip(names, got):
            _assert_planes(planes, refs[name].planes, (name, iters, fused))
    assert jpeggpu_amd.fused_tail_timeouts() == 0


def test_small_call_plans(torch_cuda, corpus, refs, monkeypatch):
    """Calls of 1 to 8 images told their size (jpeggpu_ext_set_batch_hint): the small-call plans, every file in one of
    them."""
    import jpeggpu_amd

    monkeypatch.setenv("JPEGGPU_EXP_KEEP_FLOWS_BELOW", "220000")  # the library's own choice, whatever an earlier test set
    names = list(corpus)
    k, hint = 0, 1
    while k < len(names):
        group = names[k:k + hint]
        got, lays = _batch(torch_cuda, [corpus[n] for n in group], hint=len(group))
        assert [l.subsequences_per_sequence for l in lays] == [240] * len(group), group
        for name, planes in zip(group, got):
            _assert_planes(planes, refs[name].planes, (name, len(group)))
        k += hint
        hint = hint % 8 + 1
    assert jpeggpu_amd.fused_tail_timeouts() == 0


def test_batch_mixes_scales_methods_and_crops(torch_cuda, corpus, refs):
    import jpeggpu_amd

    pattern = [(1, "islow", True), (1, "reference", False), (2, "reference", True), (8, "reference", False),
               (4, "reference", True), (1, "islow", False), (1, "reference", True)]
    items, keys = [], []
    fulls = {}
    for k, name in enumerate(corpus):
        d, method, cropped = pattern[k % len(pattern)]
        if (name, d, method) not in fulls:
            fulls[(name, d, method)] = decode(torch_cuda, corpus[name], d, method)
        ci = fulls[(name, d, method)][2]
        rects = rectangles(ci.width, ci.height)
        items.append((corpus[name], d, method, rects[k % len(rects)] if cropped else None, k % 3 == 1))
        keys.append((name, d, method))
    for hint in (0, 64):
        got = crop_batch_decode(torch_cuda, items, hint)
        for (data, d, method, rect, dscan), (planes, info, ci), key in zip(items, got, keys):
            full = fulls[key][0]
            _assert_planes(full, want_planes(refs[key[0]], d, method), key)
            assert_window(planes, full, info, ci, (key, rect, dscan, hint))
    assert jpeggpu_amd.fused_tail_timeouts() == 0


def resize_entries(corpus):
    """Whole "_a" files and cropped "_b" and "_tiny" files of every integral layout, ISLOW, and a few reference / 1/2
    decodes: (planes, info, crop_info or None)."""
    import jpeggpu_amd

    out = []
    for k, name in enumerate(_rgb_names(corpus)):
        data = corpus[name]
        if name.endswith("_a"):
            planes, info = jpeggpu_amd.decode_to_planes(data, idct="islow" if k % 4 else "reference", scale=2 if k % 7 == 3 else 1)
            out.append((planes, info, None))
        elif name.endswith("_b") or name.endswith("_tiny"):
            planes, info = jpeggpu_amd.decode_to_planes(data, idct="islow")
            W, H = image_size(info)
            rect = (W // 5, H // 4, max(1, W - W // 5 - W // 7), max(1, H - H // 4 - 1)) if W > 3 else (1, 1, W - 1, H - 2)
            out.append(jpeggpu_amd.decode_to_planes(data, idct="islow", crop=rect))
    return out


@pytest.mark.parametrize("layout", ("NHWC", "NCHW"))
@pytest.mark.parametrize("filt", R.FILTERS)
def test_resize_mixed_batch(torch_cuda, corpus, layout, filt):
    """One jpeggpu_ext_resize_to_rgb call of all of them to a smaller and to a larger size: each item equals Pillow's
    resampling (restated) of the item's RGB."""
    from tests.test_gpu_resize import assert_items, run

    entries = resize_entries(corpus)
    assert len(entries) > 40
    for w, h in ((23, 17), (97, 83)):
        got = run(torch_cuda, entries, w, h, filt, layout)
        assert_items(got, entries, w, h, filt, layout, "sweep")


def test_segment_shard_bands(torch_cuda, corpus, refs):
    """Restart intervals of one MCU row with v_max 3 and 4 (24- and 32-line MCU rows), at scale 1 and 1/2: `world`
    decoders each write only their band of every plane, and the bands make the image."""
    import jpeggpu_amd

    torch = torch_cuda
    names = [n for n in corpus if n.endswith("_rowdri")]
    assert {max(refs[n].vs) for n in names} == {3, 4}
    for name in names:
        data = corpus[name]
        for scale in (1, 2):
            want = want_planes(refs[name], scale, "reference")
            for world in (2, 3):
                planes = [torch.full(p.shape, 0xAB, dtype=torch.uint8, device="cuda:0") for p in want]
                for rank in range(world):
                    dec = jpeggpu_amd.Decoder(32 if rank % 2 else 64)
                    try:
                        dec.set_scale(scale)
                        dec.set_segment_shard(rank, world)
                        info = dec.parse_header(data)
                        n = dec.get_buffer_size()
                        tmp, base = _tmp(torch, n)
                        before = [p.clone() for p in planes]
                        dec.transfer(base, n, 0)
                        dec.decode([p.data_ptr() for p in planes], [p.stride(0) for p in planes], base, n, 0)
                        torch.cuda.synchronize()
                        for c in range(info.num_components):
                            a, cnt = dec.shard_rows(c)
                            what = (name, scale, world, rank, c)
                            assert torch.equal(planes[c][:a], before[c][:a]) and torch.equal(planes[c][a + cnt:], before[c][a + cnt:]), what
                            assert np.array_equal(planes[c][a:a + cnt].cpu().numpy(), want[c][a:a + cnt]), what
                    finally:
                        dec.cleanup()
                for c in range(len(want)):
                    assert np.array_equal(planes[c].cpu().numpy(), want[c]), (name, scale, world, c)
