"""BatchDecode, the front half of decode_resized, decode_center_cropped and decode_batch_to_rgb: its planes and records
against decode_to_planes of every file alone, a second round of transfers and decodes, close(), a construction that fails
part-way, and the C calls the three pipelines make through it. Every comparison is exact. Four small files: a grey one, a
4:2:0 one with restart markers (decoded as a stored crop), a 4:4:4 one (at 1/2, with EXIF orientation 6) and a progressive
one."""
import pytest

from tests import cases, exif_ref
from tests import progressive_cases as pc

pytestmark = pytest.mark.gpu

SCALES = [1, 1, 2, 1]
CROPS = [None, (37, 21, 101, 77), None, None]
ORIENTATIONS = [1, 1, 6, 1]


@pytest.fixture(scope="module")
def torch_cuda(gpu_lib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def datas():
    m = cases.matrix()
    return [m["gray"], m["dri_7"], exif_ref.with_orientation(m["ss_1x1"], 6), pc.pins()["p420_rst1"][0]]


@pytest.fixture(scope="module")
def lone(torch_cuda, datas):
    """decode_to_planes of every file alone with BatchDecode's settings: (planes, info, crop_info or None, colour, orientation),
    computed once and left unchanged."""
    import jpeggpu_amd

    out = []
    for data, scale, crop in zip(datas, SCALES, CROPS):
        r = jpeggpu_amd.decode_to_planes(data, idct="islow", scale=scale, scale_mode="libjpeg", progressive=True, crop=crop,
                                         return_color=True, return_orientation=True)
        out.append((r[0], r[1], r[2] if crop is not None else None, r[-2], r[-1]))
    return out


def struct_bytes(s):
    return None if s is None else bytes(s)


def assert_planes(torch, bd, lone):
    for i, (got, want) in enumerate(zip(bd.planes, lone)):
        assert len(got) == len(want[0]), i
        for c, (g, w) in enumerate(zip(got, want[0])):
            assert g.shape == w.shape and torch.equal(g, w), (i, c)


def test_planes_and_records_equal_the_lone_decodes(torch_cuda, datas, lone):
    import jpeggpu_amd

    with jpeggpu_amd.BatchDecode(datas, scales=SCALES, crops=CROPS) as bd:
        bd.decode()
        torch_cuda.cuda.synchronize()
        assert_planes(torch_cuda, bd, lone)
        assert [struct_bytes(i) for i in bd.infos] == [struct_bytes(w[1]) for w in lone]
        assert [struct_bytes(ci) for ci in bd.crop_infos] == [struct_bytes(w[2]) for w in lone]
        assert bd.colors == [w[3] for w in lone]
        assert bd.orientations == [w[4] for w in lone] == ORIENTATIONS
        assert bd.replicates == [False] * 4 and len(bd.decoders) == 4
        assert bd.transferred_bytes == sum(d.layout().transferred_bytes for d in bd.decoders) > 0
        for planes in bd.planes:  # and again, after new transfers: the object serves any number of rounds
            for p in planes:
                p.zero_()
        bd.transfer()
        bd.decode()
        torch_cuda.cuda.synchronize()
        assert_planes(torch_cuda, bd, lone)


def test_close_twice(torch_cuda, datas):
    import jpeggpu_amd

    bd = jpeggpu_amd.BatchDecode(datas, scales=SCALES, crops=CROPS)
    bd.decode()
    torch_cuda.cuda.synchronize()
    bd.close()
    bd.close()
    assert len(bd.decoders) == 4 and all(not d._h for d in bd.decoders) and not bd.batch._h
    for again in (bd.decode, bd.transfer):  # a closed object says so instead of handing null handles to the library
        with pytest.raises(RuntimeError, match="closed"):
            again()


def test_a_failing_construction_cleans_up(torch_cuda, datas, monkeypatch):
    """The third file cut to its first 64 bytes: its two predecessors' decoders and its own are cleaned up before the
    exception leaves the constructor."""
    import jpeggpu_amd

    cleaned = []
    cleanup = jpeggpu_amd.Decoder.cleanup

    def counting(self):
        if self._h:  # (a decoder's __del__ calls cleanup once more, on a handle that is null by then)
            cleaned.append(self)
        cleanup(self)

    monkeypatch.setattr(jpeggpu_amd.Decoder, "cleanup", counting)
    with pytest.raises(jpeggpu_amd.JpegGpuError, match="jpeggpu_decoder_parse_header") as e:
        jpeggpu_amd.BatchDecode(datas[:2] + [datas[2][:64]] + datas[3:], scales=SCALES, crops=CROPS)
    assert len(cleaned) == 3 and all(not d._h for d in cleaned)
    assert e.value.status != jpeggpu_amd.Status.SUCCESS
    torch_cuda.cuda.synchronize()


class Recorder:
    """api.lib()'s library with every call of a jpeggpu function noted by name."""

    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def call(*args):
            self.calls.append(name)
            return fn(*args)

        return call


OUTPUT_CALLS = ("jpeggpu_ext_resize_to_rgb", "jpeggpu_ext_resize_to_rgb_cs", "jpeggpu_ext_resize_to_rgb_oriented", "jpeggpu_ext_resize_to_tensor",
                "jpeggpu_ext_resize_view_to_tensor", "jpeggpu_ext_batch_to_rgb")
SIZERS = ("jpeggpu_ext_resize_scratch_size", "jpeggpu_ext_resize_scratch_size_cs", "jpeggpu_ext_resize_scratch_size_oriented",
          "jpeggpu_ext_resize_view_scratch_size", "jpeggpu_ext_batch_rgb_scratch_size")


@pytest.mark.parametrize("exif_transpose", [False, True])
def test_the_pipelines_calls(torch_cuda, datas, monkeypatch, exif_transpose):
    """Each pipeline makes one jpeggpu_ext_decode_batch call and one output call, the one its docstring names, with the
    scratch size from that call's own function; a header is parsed once, and once more only for what must see the header
    before the rectangle is chosen: with exif_transpose an item with a crop, in decode_center_cropped every item."""
    import jpeggpu_amd
    from jpeggpu_amd import api

    rec = Recorder(api.lib())
    monkeypatch.setattr(api, "lib", lambda: rec)
    crops = [None, CROPS[1], (3, 5, 40, 30), None]  # displayed pixels at the scale where exif_transpose is on
    with_crop = sum(c is not None for c in crops)
    want = {
        "decode_resized": ("jpeggpu_ext_resize_to_rgb_oriented" if exif_transpose else "jpeggpu_ext_resize_to_rgb_cs",
                           "jpeggpu_ext_resize_scratch_size_oriented" if exif_transpose else "jpeggpu_ext_resize_scratch_size_cs",
                           4 + (with_crop if exif_transpose else 0)),
        "decode_center_cropped": ("jpeggpu_ext_resize_view_to_tensor", "jpeggpu_ext_resize_view_scratch_size", 8),
        "decode_batch_to_rgb": ("jpeggpu_ext_batch_to_rgb", "jpeggpu_ext_batch_rgb_scratch_size", 4 + (with_crop if exif_transpose else 0)),
    }
    runs = {
        "decode_resized": lambda: jpeggpu_amd.decode_resized(datas, 16, crops=crops, scales=SCALES, exif_transpose=exif_transpose),
        "decode_center_cropped": lambda: jpeggpu_amd.decode_center_cropped(datas, 32, 24, scales=SCALES, exif_transpose=exif_transpose),
        "decode_batch_to_rgb": lambda: jpeggpu_amd.decode_batch_to_rgb(datas, crops=crops, scales=SCALES, exif_transpose=exif_transpose),
    }
    for name, run in runs.items():
        del rec.calls[:]
        out = run()
        assert len(out) == 4, name
        output, sizer, parses = want[name]
        assert [c for c in rec.calls if c in OUTPUT_CALLS] == [output], name
        assert [c for c in rec.calls if c in SIZERS] == [sizer], name
        assert rec.calls.count("jpeggpu_ext_decode_batch") == 1, name
        assert rec.calls.count("jpeggpu_decoder_parse_header") == parses, name
        assert rec.calls.count("jpeggpu_decoder_startup") == rec.calls.count("jpeggpu_decoder_cleanup") == 4, name
        assert rec.calls.count("jpeggpu_ext_batch_create") == rec.calls.count("jpeggpu_ext_batch_destroy") == 1, name
        assert rec.calls.index(sizer) < rec.calls.index(output) and rec.calls.index("jpeggpu_ext_decode_batch") < rec.calls.index(output), name
    # with a dtype the resize of decode_resized is the tensor call, its scratch the uint8 call's
    del rec.calls[:]
    jpeggpu_amd.decode_resized(datas, 16, scales=SCALES, exif_transpose=exif_transpose, dtype=torch_cuda.float16)
    assert [c for c in rec.calls if c in OUTPUT_CALLS] == ["jpeggpu_ext_resize_to_tensor"]
    assert [c for c in rec.calls if c in SIZERS] == [want["decode_resized"][1]]
