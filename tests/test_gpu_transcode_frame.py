"""The transcode that keeps its source's frame, on the device (jpeggpu_amd.transcode_jpeg(..., frame="source");
jpeggpu_ext_set_transcode_frame): Pillow's pinned files byte for byte, every sampling layout the decoder reads against
tests/transcode_frame_ref.py, against the oracle's coefficients and against Pillow's decode, orientations and crops on general
layouts, tiles whose edge lies inside an MCU of ten blocks, calls that mix the modes, and the identity on the files the
default takes. Every source is at most 140 x 120 pixels."""
import io

import numpy as np
import pytest

import jpeggpu_amd
from jpeggpu_amd import JpegGpuError
from oracle import oracle
from tests import cases, color_ref
from tests import transcode_cases as T
from tests import transcode_frame_cases as K
from tests import transcode_frame_ref as F
from tests.test_gpu_transcode import transcode_guarded
from tools import jpegsynth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def torch(gpu_lib):
    import torch

    assert torch.cuda.is_available()
    assert hasattr(jpeggpu_amd.lib(), "jpeggpu_ext_set_transcode_frame"), "the library lacks jpeggpu_ext_set_transcode_frame"
    return torch


@pytest.fixture(scope="module")
def sweep():
    """name -> bytes: every file of the sampling sweep that parse_header accepts, the matrix's two- and four-component files
    and its 16-bit tables."""
    out = {k: v for k, v in cases.sampling_sweep().items() if not k.startswith("refuse_")}
    matrix = cases.matrix()
    out.update({k: matrix[k] for k in ("two_comp", "four_comp_opt", "four_comp_444", "q16_tables")})
    return out


def keep(torch, datas, **options):
    files, _, status = transcode_guarded(torch, datas, capacities=[4 * len(d) + 4096 for d in datas], frame="source", **options)
    assert status == [0] * len(datas), status
    return files


def real_blocks(data, progressive=False):
    """Per component the coefficients of its real blocks [by, bx, 64], by the oracle (a progressive file: by
    tests/progressive_ref.py, the decoder's reference for such files)."""
    info = F.parse(data)
    hmax, vmax = max(f[0] for f in info["factors"]), max(f[1] for f in info["factors"])
    grids = F.P.decode(data).coef if progressive else oracle.decode(data).coef
    return [np.asarray(g)[:F.comp_blocks(info["h"], fv, vmax), :F.comp_blocks(info["w"], fh, hmax)] for g, (fh, fv) in zip(grids, info["factors"])]


def test_pillows_pins(torch):
    pins = K.pins()
    names = sorted(K.sources())
    for kind, options in K.OPTIONS.items():
        got = keep(torch, [pins["S_%s-A" % n] for n in names], **options)
        assert [n for n, g in zip(names, got) if g != pins["S_%s-%s" % (n, kind)]] == [], kind
    got = keep(torch, [pins["S_%s-Br" % n] for n in names], restart_interval=0)
    assert [n for n, g in zip(names, got) if g != pins["S_%s-A" % n]] == []
    for name in sorted(K.oriented()):
        for o in range(2, 9):
            assert keep(torch, [pins["O_%s-1" % name]], orientation=o)[0] == pins["O_%s-%d" % (name, o)], (name, o)


KIND = {"plain": dict(), "optimize": dict(optimize=True), "progressive": dict(progressive=True)}


@pytest.mark.parametrize("kind", list(KIND))
def test_every_sampling_layout(torch, sweep, kind):
    """Against the restatement; and, resting on neither restatement, the oracle's coefficients of the output are the
    source's on every real block, and Pillow decodes both files to the same pixels."""
    from PIL import Image

    names = sorted(sweep)
    got = keep(torch, [sweep[n] for n in names], **KIND[kind])
    assert [n for n, g in zip(names, got) if g != F.transcode(sweep[n], **KIND[kind])] == []
    opened = 0
    for n, g in zip(names, got):
        for a, b in zip(real_blocks(sweep[n]), real_blocks(g, kind == "progressive")):
            assert np.array_equal(a, b), n
        try:
            want = np.asarray(Image.open(io.BytesIO(sweep[n])))
        except Exception:
            continue
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(g))), want), n
        opened += 1
    assert opened > len(names) // 2


def test_progressive_sources(torch):
    """A progressive source of a general layout: Pillow's progressive CMYK and three-table files back to the pinned plain file."""
    from PIL import Image

    pins = K.pins()
    for name, (img, mode, params) in list(K.sources().items())[:8]:
        f = io.BytesIO()
        Image.fromarray(img, mode).save(f, "JPEG", progressive=True, **params)
        assert keep(torch, [f.getvalue()], restart_interval=0)[0] == pins["S_%s-A" % name], name
        assert keep(torch, [f.getvalue()], optimize=True, restart_interval=3)[0] == pins["S_%s-Br" % name], name
        assert keep(torch, [f.getvalue()], progressive=True)[0] == f.getvalue(), name


def test_the_default_still_refuses(torch, sweep):
    for options in KIND.values():
        with pytest.raises(JpegGpuError) as e:
            jpeggpu_amd.transcode_jpeg([sweep["y4x1_a"]], **options)
        assert e.value.status == jpeggpu_amd.Status.NOT_SUPPORTED


def oriented_sources(sweep):
    colour = color_ref.cases()
    out = {k: sweep[k] for k in ("y2x1_a", "y1x2_a", "y4x1_a", "y4x2_a", "y2x2_c2x1_a", "po_four_8du")}
    out["cmyk"] = next(d for d, m in colour.values() if m == color_ref.CMYK)
    return out


@pytest.mark.parametrize("trim", [False, True])
def test_orientations(torch, sweep, trim):
    datas, wants, what = [], [], []
    for name, data in oriented_sources(sweep).items():
        for o in range(2, 9):
            try:
                want = F.transcode(data, orientation=o, trim=trim, optimize=(o % 2 == 0), progressive=(o % 3 == 0))
            except F.Unsupported:
                with pytest.raises(JpegGpuError):
                    jpeggpu_amd.transcode_jpeg([data], orientation=o, trim=trim, frame="source")
                continue
            datas.append(data), wants.append(want), what.append((name, o))
    assert len(datas) > (30 if trim else 5)
    got = keep(torch, datas, orientation=[o for _, o in what], trim=trim, optimize=[o % 2 == 0 for _, o in what], progressive=[o % 3 == 0 for _, o in what])
    assert [w for w, g, want in zip(what, got, wants) if g != want] == []


def test_422_turned_and_turned_back(torch):
    data = jpegsynth.encode(96, 64, ((2, 1), (1, 1), (1, 1)), seed=11)
    turned = keep(torch, [data], orientation=6)[0]
    info = F.parse(turned)
    assert (info["w"], info["h"], [c["sampling"] for c in info["comps"]]) == (64, 96, [0x12, 0x11, 0x11])
    assert turned == F.transcode(data, orientation=6)
    assert keep(torch, [turned], orientation=8)[0] == keep(torch, [data])[0] == F.transcode(data)
    with pytest.raises(JpegGpuError):
        jpeggpu_amd.transcode_jpeg([data], orientation=6)


@pytest.mark.parametrize("layout,w,h,interval", [("y4x2", 136, 120, 2), ("y1x2", 75, 100, 3)])
def test_crops(torch, layout, w, h, interval):
    """iMCU-aligned and expanded origins, ragged sizes; transcode_jpeg narrows the decode to the restart segments needed."""
    samp = cases.SWEEP_LAYOUTS[layout]
    hmax, vmax = max(f[0] for f in samp), max(f[1] for f in samp)
    data = jpegsynth.encode(w, h, samp, restart_interval=interval, seed=12)
    for o, rect, expand in ((1, (8 * hmax, 8 * vmax, 37, 29), False), (1, (8 * hmax + 3, 16 * vmax + 5, 30, 21), True), (1, (0, 0, w, h), False),
                            (1, (0, 8 * vmax, w, 16 * vmax), False), (5, (8 * vmax, 8 * hmax, 19, 40), False), (5, (8 * vmax + 1, 2, 22, 33), True)):
        ux, uy = (8 * vmax, 8 * hmax) if o >= 5 else (8 * hmax, 8 * vmax)
        for options in (dict(optimize=expand), dict(progressive=True)):
            want = F.transcode(data, orientation=o, crop=F.C.expanded(rect, ux // 8, uy // 8) if expand else rect, **options)
            got = jpeggpu_amd.transcode_jpeg([data], orientation=o, crops=[rect], expand=expand, frame="source", **options)[0]
            assert got == want, (layout, o, rect, expand, options)
    # the decode really is narrowed: the hook transcode_jpeg installs sets a window, and less than the file is transferred
    rect = (0, 8 * vmax, w, 16 * vmax)
    hooks = jpeggpu_amd.api._transcode_windows(1, 1, False, False, [rect], False, "source")
    assert hooks is not None and hooks[0] is not None
    with jpeggpu_amd.BatchDecode([data], DEV, coefficients_only=True, crop_hooks=hooks) as bd:
        bd.decode()
        out = torch.empty(4 * len(data) + 4096, dtype=torch.uint8, device=DEV)
        sizes, status = jpeggpu_amd.transcode_into(bd, [out], crops=[rect], frame="source")
        assert status.cpu().tolist() == [0] and bd.transferred_bytes < len(data), (bd.transferred_bytes, len(data))
        assert out[:int(sizes[0])].cpu().numpy().tobytes() == F.transcode(data, crop=rect)
    with pytest.raises(JpegGpuError):
        jpeggpu_amd.transcode_jpeg([data], crops=[(8, 8, 20, 20)], frame="source")


@pytest.mark.parametrize("interval", [0, 3])
def test_a_tile_edge_inside_an_mcu(torch, interval):
    """40 MCUs of 10 blocks: two tiles of 256 blocks, the edge inside MCU 25; and four components of 1 x 1 in more than 256 blocks."""
    data = jpegsynth.encode(136, 120, cases.SWEEP_LAYOUTS["y4x2"], restart_interval=interval, seed=13)
    four = jpegsynth.encode(72, 64, ((1, 1),) * 4, restart_interval=interval, seed=14)
    assert len(F.parse(four)["comps"]) == 4
    for options in KIND.values():
        got = keep(torch, [data, four], **options)
        assert got[0] == F.transcode(data, **options) and got[1] == F.transcode(four, **options), (interval, options)
        got = keep(torch, [data, four], restart_interval=5, orientation=3, trim=True, **options)  # (136 is cut to 128)
        assert got[0] == F.transcode(data, restart_interval=5, orientation=3, trim=True, **options), (interval, options)
        assert got[1] == F.transcode(four, restart_interval=5, orientation=3, trim=True, **options), (interval, options)


def test_one_call_mixes_the_modes(torch, sweep):
    pins, plain = K.pins(), T.pins()[0]
    case = T.cases()[3]
    s422 = jpegsynth.encode(96, 64, ((2, 1), (1, 1), (1, 1)), seed=11)
    datas = [plain[case["name"]]["A"], sweep["y4x1_a"], pins["S_cmyk_80x64-A"], s422, plain[case["name"]]["A"]]
    frames = ["encoder", "source", "source", "source", "source"]
    options = dict(optimize=[True, False, False, False, False], progressive=[False, False, True, False, True], orientation=[1, 1, 1, 6, 1])
    files, _, status = transcode_guarded(torch, datas, capacities=[4 * len(d) + 4096 for d in datas], frame=frames, **options)
    assert status == [0] * 5
    assert files[0] == plain[case["name"]]["B"] and files[4] == plain[case["name"]]["C"]
    assert files[1] == F.transcode(datas[1]) and files[2] == pins["S_cmyk_80x64-C"] and files[3] == F.transcode(s422, orientation=6)


def test_files_the_default_takes_are_the_same_bytes(torch):
    files = T.pins()[0]
    datas = [files[c["name"]]["A"] for c in T.cases()]
    datas += [K.renumbered(d, 2) for d in datas[:6]]  # (the default writes tables 0 and 1 whatever the source calls them)
    for options in (dict(), dict(optimize=True), dict(progressive=True), dict(restart_interval=2)):
        a, _, sa = transcode_guarded(torch, datas, **options)
        b, _, sb = transcode_guarded(torch, datas, frame="source", **options)
        assert sa == sb == [0] * len(datas) and a == b, options
