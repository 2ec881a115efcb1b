"""Lossless transcoding on the device (jpeggpu_amd.transcode_jpeg; gather_blocks of jg_encode.hip behind a batched decode
that stops in front of the IDCT): every direction between Pillow's pinned files byte for byte, calls that mix output kinds,
slots that are too small, sources Pillow cannot write against tests/transcode_ref.py and the oracle's coefficients, a source
the target cannot code, and the decode's coefficients-only flag. Every output slot lies between guard bytes."""
import numpy as np
import pytest

import jpeggpu_amd
from jpeggpu_amd import JpegGpuError
from oracle import oracle
from tests import cases
from tests import transcode_cases as T
from tests import transcode_ref as R

pytestmark = pytest.mark.gpu

GUARD, G = 0xA5, 64
CASES = T.cases()
DIRECTIONS = T.DIRECTIONS
DEV = "cuda:0"


@pytest.fixture(scope="module")
def torch(gpu_lib):
    import torch

    assert torch.cuda.is_available()
    return torch


def transcode_guarded(torch, datas, capacities=None, **options):
    """One batched decode (coefficients only) and one jpeggpu_ext_transcode_batch call into guarded slots. Returns (files,
    sizes, status): files[i] the slot's bytes up to its reported size, None where status is not 0. Asserts that nothing
    outside the files was written."""
    capacities = [2 * len(d) + 2048 for d in datas] if capacities is None else capacities
    offsets, total = [], G
    for cap in capacities:
        offsets.append(total)
        total += cap + G
    buf = torch.full((total,), GUARD, dtype=torch.uint8, device=DEV)
    with jpeggpu_amd.BatchDecode(datas, DEV, coefficients_only=True) as bd:
        bd.decode()
        sizes, status = jpeggpu_amd.transcode_into(bd, [buf[o:o + cap] for o, cap in zip(offsets, capacities)], **options)
        sizes, status = sizes.cpu().tolist(), status.cpu().tolist()
    host = buf.cpu().numpy()
    untouched = np.ones(total, bool)
    files = []
    for o, size, st in zip(offsets, sizes, status):
        if st == 0:
            untouched[o:o + size] = False
        files.append(host[o:o + size].tobytes() if st == 0 else None)
    assert (host[untouched] == GUARD).all(), "bytes outside the files were written"
    return files, sizes, status


def test_every_pinned_direction(torch):
    """One call per direction over all the cases: A -> B, A -> C, C -> A, B -> A, A -> A, C -> C, B -> B, C -> B."""
    files = T.pins()[0]
    for src, options, want in DIRECTIONS:
        got, _, status = transcode_guarded(torch, [files[c["name"]][src] for c in CASES], **options)
        assert status == [0] * len(CASES), (src, options)
        wrong = [c["name"] for c, g in zip(CASES, got) if g != files[c["name"]][want]]
        assert not wrong, (src, options, want, wrong)


def test_restart_intervals(torch):
    """A with another interval is Pillow's file with that interval, from the plain and from the progressive source; and back."""
    files = T.pins()[0]
    some = [c for c in CASES if c["restart_to"] is not None]
    for src in "AC":
        got, _, status = transcode_guarded(torch, [files[c["name"]][src] for c in some], restart_interval=[c["restart_to"] for c in some])
        assert status == [0] * len(some)
        assert [c["name"] for c, g in zip(some, got) if g != files[c["name"]]["R"]] == []
    got, _, _ = transcode_guarded(torch, [files[c["name"]]["R"] for c in some], restart_interval=[c["restart_interval"] for c in some])
    assert [c["name"] for c, g in zip(some, got) if g != files[c["name"]]["A"]] == []
    got, _, _ = transcode_guarded(torch, [files[c["name"]]["R"] for c in some], restart_interval=None)  # the source's own
    assert [c["name"] for c, g in zip(some, got) if g != files[c["name"]]["R"]] == []


def test_one_call_mixing_everything(torch):
    """Sources of all three kinds, all sizes, grey and colour, each to another kind: the pinned files, and the same items
    done one by one."""
    files = T.pins()[0]
    plan = [(c, *DIRECTIONS[i % len(DIRECTIONS)]) for i, c in enumerate(CASES)]
    datas = [files[c["name"]][src] for c, src, _, _ in plan]
    optimize = [bool(o.get("optimize")) for _, _, o, _ in plan]
    progressive = [bool(o.get("progressive")) for _, _, o, _ in plan]
    got, _, status = transcode_guarded(torch, datas, optimize=optimize, progressive=progressive)
    assert status == [0] * len(plan)
    assert [c["name"] for (c, _, _, want), g in zip(plan, got) if g != files[c["name"]][want]] == []
    for k in range(len(plan)):
        alone, _, _ = transcode_guarded(torch, [datas[k]], optimize=optimize[k], progressive=progressive[k])
        assert alone[0] == got[k], plan[k][0]["name"]
    assert jpeggpu_amd.transcode_jpeg(datas, optimize=optimize, progressive=progressive) == got


def test_too_small(torch):
    """d_sizes is the capacity the item needs, its slot stays as it was, its neighbours are written."""
    files = T.pins()[0]
    names = ["136x120_420_q75_r0_smooth", "17x13_420_q100_r1_noise", "33x17_grey_q100_r3_noise", "136x120_grey_q75_r0_smooth"]
    datas = [files[n]["A"] for n in names]
    for options, want in ((dict(), "A"), (dict(optimize=True), "B"), (dict(progressive=True), "C")):
        need = [len(files[n][want]) for n in names]
        caps = [need[0], need[1] - 1, need[2], 0]
        got, sizes, status = transcode_guarded(torch, datas, caps, **options)  # (the guard check covers the two slots)
        assert status == [0, 1, 0, 1] and sizes == need
        assert got[0] == files[names[0]][want] and got[2] == files[names[2]][want]


def _uncoded_dummies(src_coef, out_coef):
    """The oracle's arrays of source and output: equal on every block the source has; beyond them the output is zero."""
    for s, o in zip(src_coef, out_coef):
        assert o.shape[0] >= s.shape[0] and o.shape[1] >= s.shape[1]
        assert (o[:s.shape[0], :s.shape[1]] == s).all()
        rest = o.copy()
        rest[:s.shape[0], :s.shape[1]] = 0
        assert not rest.any()


def test_sources_pillow_cannot_write(torch):
    """Escapes in every unit, scans of one component each (whose dummy blocks no scan codes), restart markers."""
    matrix = cases.matrix()
    sources = {"dense_escapes": cases.dense_escape_case(), "ni_444": matrix["ni_444"], "ni_420": matrix["ni_420"], "ni_420_dri": matrix["ni_420_dri"],
               "odd_17x9": matrix["odd_17x9"], "gray_hdr_2x2": matrix["gray_hdr_2x2"], "q100_noisy": matrix["q100_noisy"], "dri_nondiv": matrix["dri_nondiv"]}
    names = list(sources)
    for options in (dict(), dict(optimize=True), dict(progressive=True), dict(restart_interval=2)):
        got, _, status = transcode_guarded(torch, [sources[n] for n in names], **options)
        assert status == [0] * len(names), options
        for n, g in zip(names, got):
            assert g == R.transcode(sources[n], **options), (n, options)
    got, _, _ = transcode_guarded(torch, [sources[n] for n in names])
    for n, g in zip(names, got):
        _uncoded_dummies(oracle.decode(sources[n]).coef, oracle.decode(g).coef)
    assert oracle.decode(sources["ni_420"]).coef[0].shape[1] % 2 == 1, "the case has a dummy column no scan codes"


def test_empty_segment_source():
    """The decoder refuses this file at parse time (both walks do: tests/cases.py), so there is nothing to transcode."""
    with pytest.raises(JpegGpuError):
        jpeggpu_amd.transcode_jpeg([cases.empty_segment_case()])


def test_uncodable(torch):
    """One AC coefficient of category 11, which no baseline or progressive AC code expresses, and a DC difference of category
    12: status 4 and size 0, the slot untouched, the other item of the call fine."""
    from tools import jpegsynth

    coef = np.zeros((4, 64), np.int16)
    coef[:, 0] = [5, -3, 7, 0]
    coef[:, 1] = [1, -1, 2, 3]
    ac = coef.copy()
    ac[2, 5] = 1500
    dc = coef.copy()
    dc[:, 0] = [1023, -1025, 0, 0]
    good = jpegsynth.encode_blocks(coef, 2, np.ones(64, np.uint8), optimize=True)
    for bad in (jpegsynth.encode_blocks(ac, 2, np.ones(64, np.uint8), optimize=True), jpegsynth.encode_blocks(dc, 2, np.ones(64, np.uint8), optimize=True)):
        for options in (dict(), dict(optimize=True), dict(progressive=True)):
            got, sizes, status = transcode_guarded(torch, [good, bad, good], **options)
            assert status == [0, 4, 0] and sizes[1] == 0, options
            assert got[0] == got[2] == R.transcode(good, **options)
            with pytest.raises(JpegGpuError, match="item 1"):
                jpeggpu_amd.transcode_jpeg([good, bad], **options)


def test_coefficients_only_leaves_the_planes(torch):
    files = T.pins()[0]
    datas = [files["136x120_420_q75_r0_smooth"]["A"], files["33x17_444_q100_r0_noise"]["C"], files["136x120_grey_q75_r0_smooth"]["B"]]
    with jpeggpu_amd.BatchDecode(datas, DEV) as bd:
        for planes in bd.planes:
            for p in planes:
                p.fill_(0x5A)
        bd.batch.set_coefficients_only(True)
        bd.decode()
        torch.cuda.synchronize()
        assert all(bool((p == 0x5A).all()) for planes in bd.planes for p in planes)
        bd.batch.set_coefficients_only(False)
        bd.transfer()
        bd.decode()
        torch.cuda.synchronize()
        again = [[p.cpu() for p in planes] for planes in bd.planes]
    with jpeggpu_amd.BatchDecode(datas, DEV) as fresh:
        fresh.decode()
        torch.cuda.synchronize()
        for a, b in zip(again, fresh.planes):
            assert all(bool((x == y.cpu()).all()) for x, y in zip(a, b))
    assert not bool((again[0][0] == 0x5A).all())


def test_round_trip_through_the_decoder(torch):
    src = T.pins()[0]["136x120_420_q75_r0_smooth"]["A"]
    out = jpeggpu_amd.transcode_jpeg([src], progressive=True)[0]
    assert out != src
    assert bool((jpeggpu_amd.decode_to_rgb(out) == jpeggpu_amd.decode_to_rgb(src)).all())
