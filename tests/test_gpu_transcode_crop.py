"""The cropped transcode on the device (jpeggpu_ext_set_transcode_crop; gather_blocks<true> of jg_encode.hip behind an offset):
every pinned Pillow file of cropped pixels, source kinds, windows with dummy columns, rows and corners, two tiles, every
orientation with a crop off the centre, the decode narrowed to the window's restart segments (jpeggpu_ext_set_crop) against
the same call on a whole decode, calls that mix item kinds, the DC limit across a crop's left edge, the Python layer and a
decode of the result. Byte for byte against tests/transcode_crop_ref.transform; every output slot lies between guard bytes."""
import numpy as np
import pytest

import jpeggpu_amd
from jpeggpu_amd import JpegGpuError, Status
from tests import exif_ref
from tests import transcode_cases as T
from tests import transcode_crop_cases as W
from tests import transcode_crop_ref as Z
from tests import transcode_orient_cases as K
from tests import transcode_ref as R
from tests.test_gpu_transcode import DEV, G, GUARD, torch, transcode_guarded  # noqa: F401 (torch is a fixture)

pytestmark = pytest.mark.gpu

KIND_OPTIONS = [dict(), dict(optimize=True), dict(progressive=True)]


def _options(plan):
    return dict(crops=[p[1] for p in plan], orientation=[p[2] for p in plan], trim=[p[3] for p in plan], optimize=[bool(p[4].get("optimize")) for p in plan],
                progressive=[bool(p[4].get("progressive")) for p in plan], restart_interval=[p[4].get("restart_interval") for p in plan])


def run(torch, plan):
    """plan: (source, rect or None, orientation, trim, options) per item, in ONE call on whole decodes. (files, sizes, status)."""
    return transcode_guarded(torch, [p[0] for p in plan], **_options(plan))


def run_narrowed(torch, plan, windows):
    """The same call on decodes that keep only `windows[i]`, a STORED rectangle of source pixels (Decoder.set_crop), where
    it is not None. Returns (files, sizes, status, bytes transferred)."""
    datas = [p[0] for p in plan]
    caps = [2 * len(d) + 2048 for d in datas]
    offsets, total = [], G
    for cap in caps:
        offsets.append(total)
        total += cap + G
    buf = torch.full((total,), GUARD, dtype=torch.uint8, device=DEV)
    with jpeggpu_amd.BatchDecode(datas, DEV, coefficients_only=True, crops=windows) as bd:
        bd.decode()
        sizes, status = jpeggpu_amd.transcode_into(bd, [buf[o:o + cap] for o, cap in zip(offsets, caps)], **_options(plan))
        sizes, status, moved = sizes.cpu().tolist(), status.cpu().tolist(), bd.transferred_bytes
    host = buf.cpu().numpy()
    untouched = np.ones(total, bool)
    files = []
    for o, size, st in zip(offsets, sizes, status):
        if st == 0:
            untouched[o:o + size] = False
        files.append(host[o:o + size].tobytes() if st == 0 else None)
    assert (host[untouched] == GUARD).all(), "bytes outside the files were written"
    return files, sizes, status, moved


def check(torch, plan, what=None):
    got, _, status = run(torch, plan)
    assert status == [0] * len(plan)
    wrong = [(i if what is None else what[i]) for i, (p, g) in enumerate(zip(plan, got)) if g != Z.transform(p[0], p[1], p[2], p[3], **p[4])]
    assert not wrong, wrong[:10]
    return got


def test_every_pin(torch):
    """Pillow's file of the cropped pixels (and of the rectangle of the transposed cell image), byte for byte, in one call."""
    sources, want, _ = W.pins()
    plan, keys = [], []
    for ci, case in enumerate(W.pin_cases()):
        for wi, (window, rect) in enumerate(W.windows(case["w"], case["h"], *W.imcu(case["sampling"])).items()):
            kind = W.pin_kind(ci, wi)
            plan.append((sources[case["name"]], rect, 1, False, W.KINDS[kind]))
            keys.append((case["name"], window, kind))
    for name, o, trim, rect in W.oriented_pin_cases():
        kind = next(k for k in "ABC" if (name, o, trim, rect, k) in want)
        plan.append((K.pins()[0][name], rect, o, trim, W.KINDS[kind]))
        keys.append((name, o, trim, rect, kind))
    assert len(plan) == len(want) >= 88
    got, _, status = run(torch, plan)
    assert status == [0] * len(plan)
    wrong = [k for k, g in zip(keys, got) if g != want[k]]
    assert not wrong, wrong[:10]


@pytest.mark.parametrize("sampling", ["grey", "4:4:4", "4:2:0", "4:2:2"])
@pytest.mark.parametrize("kind", K.SOURCE_KINDS)
def test_source_kinds(torch, kind, sampling):
    """A 75 x 53 source of each kind and layout, without and with restart markers: the six windows and ragged ones, the
    output kinds in turn, restart intervals 0, 1, the source's and one MCU row of the target."""
    ux, uy = W.imcu(sampling)
    rects = list(W.windows(75, 53, ux, uy).values()) + [(x // ux * ux, y // uy * uy, w, h) for x, y, w, h in W.ragged(75, 53, 8, 8)]
    plan = []
    for restart in (0, 2):
        src = W.source_of_kind(kind, sampling, 75, 53, ["noise", "photo"][restart // 2], 3 + restart, restart)
        for n, rect in enumerate(rects):
            r = [0, 1, None, -(-rect[2] // ux)][(n + restart) % 4]
            plan.append((src, rect, 1, False, dict(KIND_OPTIONS[n % 3], restart_interval=r)))
    check(torch, plan)


@pytest.mark.parametrize("sampling", ["4:2:0", "4:2:2"])
def test_dummy_column_row_and_corner(torch, sampling):
    """Windows whose target has luma blocks beyond its real grid: inside the image (the source has real blocks there, the
    target the encoder's dummies) and at the source's ragged edges."""
    hs, vs = K.FACTORS[sampling]
    src = {kind: W.source_of_kind(kind, sampling, 88, 72, "noise", 5, 0) for kind in ("interleaved", "progressive")}
    rects = [(16, 16, 40, 32), (16, 16, 32, 40), (16, 16, 40, 40), (32, 32, 56, 40), (0, 0, 33, 17), (48, 48, 40, 24), (0, 0, 88, 72)]
    dummies = [(-(-w // 8) % hs != 0, -(-h // 8) % vs != 0) for _, _, w, h in rects]
    assert (True, False) in dummies and ((True, True) in dummies) == (vs == 2) and ((False, True) in dummies) == (vs == 2)
    plan = [(src[kind], rect, 1, False, dict(KIND_OPTIONS[(n + k) % 3], restart_interval=[0, 2][n % 2])) for k, kind in enumerate(src) for n, rect in enumerate(rects)]
    check(torch, plan)


def test_two_tiles(torch):
    """128 x 112 out of 160 x 144 in 4:2:0: 336 blocks, two gather tiles."""
    assert T.blocks_of(128, 112, "4:2:0") == (336, 2)
    plan = []
    for k, kind in enumerate(K.SOURCE_KINDS):
        src = W.source_of_kind(kind, "4:2:0", 160, 144, "photo", 7, 0)
        plan += [(src, (16, 16, 128, 112), 1, False, KIND_OPTIONS[k]), (src, (32, 32, 128, 112), 3, False, KIND_OPTIONS[(k + 1) % 3])]
    check(torch, plan)


@pytest.mark.parametrize("sampling", ["grey", "4:4:4", "4:2:0", "4:2:2"])
def test_orientations_with_a_crop_off_the_centre(torch, sampling):
    """Each orientation with rectangles that a mirror does not map onto themselves: offset, mirror and exchange in another
    order give other blocks. 75 x 53 needs the trim where an axis is mirrored; 80 x 64 does not."""
    hs, vs = K.FACTORS[sampling]
    plan, what = [], []
    for w, h in W.SIZES:
        srcs = [W.source_of_kind(kind, sampling, w, h, "noise", 9, [0, 3][k % 2]) for k, kind in enumerate(K.SOURCE_KINDS)]
        for o in range(1, 9):
            try:
                tw, th, ths, tvs = Z.target_geometry(w, h, hs, vs, o, True)
            except Z.Unsupported:
                assert sampling == "4:2:2" and o >= 5
                continue
            ux, uy = 8 * ths, 8 * tvs
            for n, rect in enumerate(((ux, 0, 2 * ux, 3 * uy), (0, 2 * uy, tw - ux, th - 2 * uy), (2 * ux, uy, tw - 2 * ux - 3, 11))):
                assert rect[0] + rect[2] <= tw and rect[1] + rect[3] <= th
                assert n < 2 or (rect[0] != tw - rect[0] - rect[2] and rect[1] != th - rect[1] - rect[3])  # off the centre on both axes
                plan.append((srcs[(o + n) % 3], rect, o, True, dict(KIND_OPTIONS[(o + n) % 3], restart_interval=[None, 0, 2][n])))
                what.append((w, h, o, rect))
    assert len(plan) >= (24 if sampling == "4:2:2" else 48)
    check(torch, plan, what)


def _restart_sources():
    """Sources of the project's encoder with a restart interval of one MCU row, and of 3 MCUs (so that the first kept MCU
    is no row start): 4:2:0 and 4:4:4 of 5 x 6 MCUs of 16 x 16 and 10 x 12 of 8 x 8, and a grey file."""
    out = []
    for sampling, (w, h), row in (("4:2:0", (80, 96), 5), ("4:4:4", (80, 96), 10), ("grey", (77, 93), 10), ("4:2:2", (80, 48), 5)):
        for restart in (row, 3):
            out.append((sampling, w, h, restart, W.source_of_kind("interleaved", sampling, w, h, "noise", restart, restart)))
    return out


def test_narrowed_decode(torch):
    """The decode keeps only the restart segments that hold the rectangle's source pixels: the files are those of the same
    call on whole decodes, byte for byte, for windows in the middle, at the bottom, at the top right and the whole image,
    at orientation 1 and turned, and less is transferred."""
    plan, windows = [], []
    for sampling, w, h, restart, src in _restart_sources():
        hs, vs = K.FACTORS[sampling]
        for o in (1, 3, 6, 8):
            if sampling == "4:2:2" and o >= 5:
                continue
            tw, th, ths, tvs = Z.target_geometry(w, h, hs, vs, o, True)
            ux, uy = 8 * ths, 8 * tvs
            for n, rect in enumerate(((2 * ux, 2 * uy, 2 * ux, uy), (ux, th // uy * uy - uy, 2 * ux, th - (th // uy * uy - uy)), (tw // ux * ux - ux, 0, ux, uy + 3), (0, 0, tw, th))):
                rect = tuple(int(v) for v in rect)
                target, stored = jpeggpu_amd.transcode_crop_rects(w, h, hs, vs, rect, o, True)
                assert target == rect
                plan.append((src, rect, o, True, dict(KIND_OPTIONS[(n + o) % 3], restart_interval=[None, 0][n % 2])))
                windows.append(stored)
    narrow, _, status, moved = run_narrowed(torch, plan, windows)
    assert status == [0] * len(plan)
    whole, _, status, moved_whole = run_narrowed(torch, plan, [None] * len(plan))
    assert status == [0] * len(plan)
    assert [i for i, (a, b) in enumerate(zip(narrow, whole)) if a != b] == []
    assert [i for i, (p, g) in enumerate(zip(plan, whole)) if g != Z.transform(p[0], p[1], p[2], p[3], **p[4])] == []
    print("transferred: %d bytes narrowed, %d whole" % (moved, moved_whole))
    assert moved < moved_whole


def test_narrowed_decode_of_other_sources(torch):
    """A decode window on files it does not narrow -- no restart markers, a scan per component, progressive -- changes nothing."""
    plan, windows = [], []
    for k, kind in enumerate(K.SOURCE_KINDS):
        src = W.source_of_kind(kind, "4:2:0", 80, 64, "photo", k, 0 if kind == "interleaved" else 2)
        for o, rect in ((1, (32, 16, 32, 32)), (6, (16, 32, 33, 20))):
            plan.append((src, rect, o, False, KIND_OPTIONS[(k + o) % 3]))
            windows.append(jpeggpu_amd.transcode_crop_rects(80, 64, 2, 2, rect, o)[1])
    narrow, _, status, _ = run_narrowed(torch, plan, windows)
    assert status == [0] * len(plan)
    assert [i for i, (p, g) in enumerate(zip(plan, narrow)) if g != Z.transform(p[0], p[1], p[2], p[3], **p[4])] == []


def test_a_window_that_does_not_cover_the_crop_is_refused(torch):
    _, w, h, _, src = _restart_sources()[0]
    plan = [(src, (16, 32, 32, 32), 1, False, dict())]
    for window in ((48, 32, 16, 32), (16, 64, 32, 16), (16, 32, 32, 8)):  # (a window keeps a sample of halo: 47 and 63 lie an MCU on)
        with pytest.raises(JpegGpuError, match="item 0") as e:
            run_narrowed(torch, plan, [window])
        assert e.value.status == Status.NOT_SUPPORTED
    with pytest.raises(JpegGpuError, match="item 0"):  # a decode window without a transcode crop
        run_narrowed(torch, [(src, None, 1, False, dict())], [(16, 32, 32, 32)])
    got, _, status, _ = run_narrowed(torch, plan, [(16, 32, 32, 32)])
    assert status == [0] and got[0] == Z.transform(src, (16, 32, 32, 32))


def test_mixed_call(torch):
    """Cropped, oriented, cropped-and-oriented and plain items in one call; the plain ones are the files of a call of their
    own (which launches the other instantiation of the gather) and keep the source's dummy blocks."""
    srcs = [W.source_of_kind(kind, "4:2:0", 75, 53, "noise", 20 + k, k) for k, kind in enumerate(K.SOURCE_KINDS)]
    grey = W.source_of_kind("interleaved", "grey", 75, 53, "photo", 4, 0)
    plan = []
    for k, src in enumerate(srcs + [grey]):
        u = 8 if src is grey else 16
        plan += [(src, None, 1, False, KIND_OPTIONS[k % 3]), (src, (u, u, 2 * u, u + 5), 1, False, KIND_OPTIONS[(k + 1) % 3]), (src, None, 5, False, KIND_OPTIONS[(k + 2) % 3]),
                 (src, (u, 0, u + 1, 3 * u), 7, True, KIND_OPTIONS[k % 3]), (src, None, 1, False, dict(KIND_OPTIONS[(k + 1) % 3], restart_interval=2))]
    got = check(torch, plan)
    plain = [i for i, p in enumerate(plan) if p[1] is None and p[2] == 1]
    alone, _, status = run(torch, [plan[i] for i in plain])
    assert status == [0] * len(plain) and alone == [got[i] for i in plain]
    assert alone == [R.transcode(plan[i][0], **plan[i][4]) for i in plain]


def test_dc_limit_across_the_left_edge(torch):
    """The left edge of a crop is predicted from the right edge of its row above. A source with a DC difference of 2048
    between the first two blocks of a row is uncodable whole and codable from the second column on; one whose second row's
    second block lies 2048 from the first row's last is codable whole and uncodable from the second column on. Status 4, size
    0 and an untouched slot for that item only, on both branches of the gather."""
    rng = np.random.default_rng(31)

    def grid():
        g = np.zeros((2, 3, 64), np.int16)
        g[..., 0] = rng.integers(-20, 21, (2, 3))
        g[..., 1] = rng.integers(-3, 4, (2, 3))
        return g

    a, b = grid(), grid()
    a[0, 0, 0], a[0, 1, 0] = -1024, 1024
    b[0, 2, 0], b[1, 1, 0] = -1024, 1024
    rect = (8, 0, 16, 16)
    good = K.pins()[0]["32x32_grey_q100"]
    for route in ("baseline", "progressive"):
        whole_bad, crop_bad = (T._limit_file(route, 24, 16, T.FACTOR_LISTS["grey"], [g]) for g in (a, b))
        with pytest.raises(Z.Unsupported):
            Z.transform(whole_bad, None, restart_interval=0)
        with pytest.raises(Z.Unsupported):
            Z.transform(crop_bad, rect, restart_interval=0)
        for options in KIND_OPTIONS:
            options = dict(options, restart_interval=0)
            plan = [(good, (8, 8, 16, 16), 1, False, options), (whole_bad, None, 1, False, options), (whole_bad, rect, 1, False, options),
                    (crop_bad, None, 1, False, options), (crop_bad, rect, 1, False, options), (good, None, 1, False, options)]
            got, sizes, status = run(torch, plan)
            assert status == [0, 4, 0, 0, 4, 0] and sizes[1] == 0 and sizes[4] == 0, (route, options)
            assert [g for g, p in zip(got, plan) if g is not None] == [Z.transform(p[0], p[1], **p[4]) for p, s in zip(plan, status) if s == 0]
        # a restart marker at the row's start takes the prediction away, and the crop is codable again
        got, _, status = run(torch, [(crop_bad, rect, 1, False, dict(restart_interval=2))])
        assert status == [0] and got[0] == Z.transform(crop_bad, rect, restart_interval=2)


def test_python_layer():
    """transcode_jpeg(crops=): one rectangle for all, a list with None, `expand`, displayed rectangles under
    exif_transpose=True; the decode is narrowed without the caller asking, and the files do not change for it; refusals name
    the item before anything is enqueued."""
    sources = K.pins()[0]
    base = [sources["48x32_420_q100"], sources["32x32_grey_q100"], sources["64x48_444_q100"], sources["16x64_420_q100"]]
    plain = [base[o % len(base)] for o in range(1, 9)]
    tagged = [exif_ref.with_orientation(p, o) for p, o in zip(plain, range(1, 9))]
    shown = []  # the displayed geometry of each file
    for p, o in zip(plain, range(1, 9)):
        info = R._checked(p)
        shown.append(Z.target_geometry(info["w"], info["h"], info["hs"], info["vs"], o))
    rects = [(tw - 16, th - 16, 16, 16) for tw, th, _, _ in shown]
    for options in KIND_OPTIONS:
        got = jpeggpu_amd.transcode_jpeg(tagged, exif_transpose=True, crops=rects, **options)
        assert got == jpeggpu_amd.transcode_jpeg(plain, orientation=list(range(1, 9)), crops=rects, **options)
        assert got == [Z.transform(p, rect, o, **options) for p, rect, o in zip(plain, rects, range(1, 9))]
    one = (0, 0, 16, 9)  # one rectangle for every file
    assert jpeggpu_amd.transcode_jpeg(tagged, exif_transpose=True, crops=one) == [Z.transform(p, one, o) for p, o in zip(plain, range(1, 9))]
    ragged = [(tw - 11, th - 7, 10, 6) for tw, th, _, _ in shown]
    got = jpeggpu_amd.transcode_jpeg(tagged, exif_transpose=True, crops=ragged, expand=True)
    assert got == [Z.transform(p, Z.expanded(r, g[2], g[3]), o) for p, r, g, o in zip(plain, ragged, shown, range(1, 9))]
    ragged = (21, 9, 10, 20)
    with pytest.raises(JpegGpuError, match="item 0") as e:  # 4:2:0: 21 is no multiple of 16
        jpeggpu_amd.transcode_jpeg(plain[:2], crops=ragged)
    assert e.value.status == Status.NOT_SUPPORTED
    with pytest.raises(JpegGpuError, match="item 1") as e:
        jpeggpu_amd.transcode_jpeg(plain[:2], crops=[None, (0, 0, 64, 64)])
    assert e.value.status == Status.INVALID_ARGUMENT
    mixed = jpeggpu_amd.transcode_jpeg(plain[:3], crops=[None, (8, 8, 9, 9), (5, 19, 9, 30)], expand=[False, False, True], orientation=[None, 4, None])
    assert mixed == [R.transcode(plain[0]), Z.transform(plain[1], (8, 8, 9, 9), 4), Z.transform(plain[2], (0, 16, 14, 33))]
    assert jpeggpu_amd.transcode_jpeg(plain[:1]) == [R.transcode(plain[0])]  # new decoders: nothing is left of the crop
    # sources with restart markers: the decode is narrowed (transcode_crop_rects -> Decoder.set_crop)
    rs = _restart_sources()
    crops = [(16, 32, 40, 9), (32, 16, 48, 80), (8, 64, 69, 13), (0, 0, 80, 48), (16, 32, 40, 9), (35, 19, 45, 47), (19, 9, 34, 32), (0, 0, 80, 48)]
    ors = [3, 1, 6, 2, 1, 8, 1, 4]
    datas = [r[4] for r in rs]
    got = jpeggpu_amd.transcode_jpeg(datas, crops=crops, orientation=ors, trim=True, expand=True, optimize=True)
    want = []
    for (sampling, w, h, _, src), rect, o in zip(rs, crops, ors):
        _, _, ths, tvs = Z.target_geometry(w, h, *K.FACTORS[sampling], o, True)
        want.append(Z.transform(src, Z.expanded(rect, ths, tvs), o, True, optimize=True))
    assert got == want
    buf, offsets, sizes = jpeggpu_amd.transcode_jpeg_to_device(datas[:1], crops=[(16, 32, 32, 32)], progressive=True)
    assert buf[offsets[0]:offsets[0] + sizes[0]].cpu().numpy().tobytes() == Z.transform(datas[0], (16, 32, 32, 32), progressive=True)


def test_decode_of_the_result(torch):
    """4:4:4: decode_to_rgb of the cropped file is decode_to_rgb(source, crop=) on the device, also where the rectangle ends
    inside a block (the file keeps the source's samples there)."""
    for kind in K.SOURCE_KINDS[::2]:
        src = W.source_of_kind(kind, "4:4:4", 75, 53, "photo", 2, 0)
        rects = [(8, 8, 32, 24), (16, 0, 59, 53), (24, 16, 13, 21), (0, 0, 75, 53)]
        files = jpeggpu_amd.transcode_jpeg([src] * len(rects), crops=rects, optimize=True)
        for f, rect in zip(files, rects):
            got, want = jpeggpu_amd.decode_to_rgb(f), jpeggpu_amd.decode_to_rgb(src, crop=rect)
            assert got.shape == want.shape == (rect[3], rect[2], 3) and bool((got == want).all()), (kind, rect)
