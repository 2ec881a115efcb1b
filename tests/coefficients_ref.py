"""CPU reference of DCT-domain access (jpeggpu_amd.read_coefficients / write_coefficients), on the earlier restatements,
which it imports and does not change.

    read(data) -> Coef: per component the quantised coefficients over its REAL block grid, int16 [blocks_y, blocks_x, 64]
                  in natural order with the DC absolute -- oracle.decode(data).coef for a baseline file,
                  tests/progressive_ref.decode(data).coef for a progressive one, each cut to the real grid --; the tables
                  (uint16 [64], natural order) and the frame from tests/transcode_frame_ref.parse
    write(co, optimize=False, progressive=False, restart_interval=0) -> bytes: the file of those arrays. The MCU stream is
                  transcode_frame_ref.mcu_stream's for a MAPPED item -- the arrays hold no dummy blocks; a dummy block is 63
                  zeros and the DC of the block in front of it in the MCU --, coded by encode_ref / encode_opt_ref /
                  encode_prog_ref behind patched `coefficients` / `quant_table` for the layouts the pixel encoder writes (as
                  transcode_ref.transcode does), and by transcode_frame_ref's header, entropy and progressive_file for every
                  other layout, its tables numbered by first appearance. Unsupported: an AC magnitude of 1024 or more, a DC
                  difference of 2048 or more in the file's prediction order.
    sources(): name -> bytes, the small files of every layout and coding the reader takes (tools/jpegsynth.py,
                  tests/progressive_ref.encode, a crafted file of tests/idct_cases.py's escape ladder)
    cases() / pins(): the Pillow-written sources of tests/golden/coefficients_pins.npz (tools/make_coefficients_pins.py)
    rgb(co) -> libjpeg's RGB of the arrays: tests/libjpeg_ref's ISLOW IDCT, fancy upsampling and colour conversion"""
import functools
import hashlib
import json
import os

import numpy as np

from tests import encode_opt_ref as O
from tests import encode_prog_ref as G
from tests import encode_ref as E
from tests import libjpeg_ref as L
from tests import transcode_frame_ref as F
from tests import transcode_ref as R

Unsupported = R.Unsupported
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "coefficients_pins.npz")
COLORS = ["unknown", "grey", "ycbcr", "rgb", "cmyk", "ycck"]  # by enum jpeggpu_ext_color_space
INVERSE = np.argsort(E.ZIGZAG)  # a zigzag-ordered table [INVERSE] is in natural order


class Coef:
    """coef[c] int16 [blocks_y, blocks_x, 64]; qtables[c] uint16 [64] natural order; sampling [(h, v)] as the frame header
    holds them; color: an index of COLORS."""

    def __init__(self, coef, qtables, w, h, sampling, color, progressive=False, restart=0):
        self.coef, self.qtables, self.w, self.h = coef, qtables, w, h
        self.sampling, self.color, self.progressive, self.restart = [tuple(f) for f in sampling], color, progressive, restart

    def factors(self):
        return [(1, 1)] if len(self.sampling) == 1 else list(self.sampling)

    def copy(self):
        return Coef([c.copy() for c in self.coef], [q.copy() for q in self.qtables], self.w, self.h, self.sampling, self.color, self.progressive, self.restart)


def grids(w, h, factors):
    hmax, vmax = max(f[0] for f in factors), max(f[1] for f in factors)
    return [(F.comp_blocks(h, fv, vmax), F.comp_blocks(w, fh, hmax)) for fh, fv in factors]


def read(data):
    data = bytes(data)
    info = F.parse(data)
    out = Coef([], [], info["w"], info["h"], [(c["sampling"] >> 4, c["sampling"] & 15) for c in info["comps"]], COLORS.index(info["color"]),
               info["progressive"], info["restart"])
    for g, c, (gh, gw) in zip(F.source_grids(data, info), info["comps"], grids(info["w"], info["h"], info["factors"])):
        assert g.shape[0] >= gh and g.shape[1] >= gw
        out.coef.append(np.ascontiguousarray(g[:gh, :gw]).astype(np.int16))
        out.qtables.append(np.array(info["qtabs"][c["q"]], np.uint16)[INVERSE])
    return out


def encoder_layout(co):
    """The subsampling name if the pixel encoder writes this layout (then the file has its header), else None."""
    nc = len(co.coef)
    if any(int(q.max()) > 255 for q in co.qtables[:2]):
        return None
    if nc == 1:
        return R.GREY_SUBSAMPLING.get(co.sampling[0][0] << 4 | co.sampling[0][1])  # (the restatements write three sampling bytes for grey)
    if nc != 3 or COLORS[co.color] != "ycbcr" or co.sampling[1] != (1, 1) or co.sampling[2] != (1, 1) or not np.array_equal(co.qtables[1], co.qtables[2]):
        return None
    return R.COLOUR_SUBSAMPLING.get(co.sampling[0])


def write(co, optimize=False, progressive=False, restart_interval=0):
    nc, factors, r = len(co.coef), co.factors(), restart_interval
    for g, shape in zip(co.coef, grids(co.w, co.h, factors)):
        assert g.shape == shape + (64,), "a grid that does not fit the frame"
    stream = F.mcu_stream([np.asarray(g, np.int64) for g in co.coef], factors, co.w, co.h, True)
    if np.abs(stream["coefs"][:, 1:].astype(np.int64)).max(initial=0) >= 1024:
        raise Unsupported("an AC coefficient of category above 10")
    if np.abs(R.dc_differences(stream, r)).max(initial=0) >= 2048:
        raise Unsupported("a DC difference of category above 11")
    subsampling = encoder_layout(co)
    if subsampling is not None:
        stream["hs"], stream["vs"] = factors[0]
        tabs = [np.asarray(q, np.int64) for q in co.qtables[:2]]
        saved = E.coefficients, E.quant_table
        try:  # the three encoders read both through the module when they are called (transcode_ref.transcode)
            E.coefficients = lambda *a, **k: stream
            E.quant_table = lambda base, quality: tabs[0] if base is E.BASE_LUMA else tabs[-1]
            return (G if progressive else O if optimize else E).encode(None, None, subsampling, r)
        finally:
            E.coefficients, E.quant_table = saved
    numbers, tables = [], {}
    for q in co.qtables:  # numbered by first appearance: components with equal tables share one
        t = next((k for k, v in tables.items() if np.array_equal(v, np.asarray(q)[E.ZIGZAG])), len(tables))
        tables.setdefault(t, np.asarray(q)[E.ZIGZAG])
        numbers.append(t)
    info = dict(color=COLORS[co.color], comps=[dict(q=t) for t in numbers])
    bytes_ = [f[0] << 4 | f[1] for f in co.sampling]
    if progressive:
        return F.progressive_file(info, stream, factors, co.w, co.h, bytes_, tables, r)
    dhts, data = F.entropy(stream, F.selectors(info["color"], nc), r, optimize)
    return F.header(info, co.w, co.h, bytes_, tables, r, dhts) + data + b"\xff\xd9"


def planes(co):
    """Each component's samples by jpeg_idct_islow, cut to the component's size."""
    factors = co.factors()
    hmax, vmax = max(f[0] for f in factors), max(f[1] for f in factors)
    out = []
    for g, q, (fh, fv) in zip(co.coef, co.qtables, factors):
        bh, bw = g.shape[:2]
        full = L.idct_islow(g.reshape(-1, 64), np.asarray(q)).reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)
        out.append(np.ascontiguousarray(full[:-(-co.h * fv // vmax), :-(-co.w * fh // hmax)]))
    return out


def rgb(co):
    """What Pillow's convert("RGB") shows of a grey or YCbCr file with these coefficients."""
    factors = co.factors()
    return L.planes_to_rgb_fancy(planes(co), [f[0] for f in factors], [f[1] for f in factors], co.w, co.h)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ---- the Pillow-written pins ----

SIZES = ((17, 9), (75, 53))
QUALITIES = (30, 75, 95)
SAMPLINGS = ("grey", "4:4:4", "4:2:2", "4:2:0")
KINDS = {"A": dict(), "B": dict(optimize=True), "C": dict(progressive=True)}


def cases():
    return [dict(name="%dx%d_%s_q%d" % (w, h, s.replace(":", ""), q), w=w, h=h, sampling=s, quality=q) for w, h in SIZES for s in SAMPLINGS for q in QUALITIES]


def image(case):
    """Smooth with a little noise: every frequency band is used and the files stay small."""
    w, h = case["w"], case["h"]
    rng = np.random.default_rng([w, h, SAMPLINGS.index(case["sampling"]), case["quality"]])
    y, x = np.mgrid[0:h, 0:w]
    base = 128 + 90 * np.sin(x / 9.0) * np.cos(y / 6.0)
    if case["sampling"] != "grey":
        base = np.stack([base, np.roll(base, 5, 1), 255 - base], -1)
    return np.clip(base + rng.normal(0, 3, base.shape), 0, 255).astype(np.uint8)


_pins = None


def pins():
    """name -> dict(A=, B=, C=: Pillow's plain, optimize=True and progressive=True file of the case's pixels; sha: the SHA-256
    of each component's expected int16 tensor), and the versions that wrote them."""
    global _pins
    if _pins is None:
        with np.load(GOLDEN) as z:
            meta = json.loads(z["meta"].tobytes().decode())
            blob = z["files"].tobytes()
        files = {}
        for name, entry in meta["cases"].items():
            files[name] = {k: blob[a:b] for k, (a, b) in entry["files"].items()}
            files[name]["sha"] = entry["sha"]
        _pins = files, meta["versions"]
    return _pins


# ---- sources beyond Pillow's files: every layout and coding the reader takes, at the smallest sizes that reach every path ----

LAYOUTS = {"420": ((2, 2), (1, 1), (1, 1)), "422": ((2, 1), (1, 1), (1, 1)), "444": ((1, 1), (1, 1), (1, 1)), "440": ((1, 2), (1, 1), (1, 1)),
           "411": ((4, 1), (1, 1), (1, 1))}
SMALL_SIZES = ((8, 8), (9, 9), (17, 9))
READ_TILE = 256  # kReadTile: the blocks of one component that a workgroup of the read kernel stores


def crafted_units():
    """tests/idct_cases.escape_ladder -- 1 to 63 escaped coefficients a unit (the last: 63 coded coefficients, 127 entries), an
    escape at every entry position and zigzag index, both signs -- and two units of 63 coefficients of +1023 and of -1023,
    padded with empty units to whole rows of 32 blocks."""
    from tests import idct_cases as I

    units, _ = I.escape_ladder(np.random.default_rng(20261120))
    for sign in (1, -1):
        u = np.full(64, sign * 1023, np.int64)
        u[0] = 7 * sign
        units.append(u)
    units += [np.zeros(64, np.int64)] * (-len(units) % I.BLOCKS_X)
    return np.stack(units).astype(np.int16)


@functools.lru_cache(maxsize=1)
def sources():
    from oracle import oracle
    from tests import idct_cases as I
    from tests import progressive_ref as P
    from tools import jpegsynth

    e = jpegsynth.encode
    out = {"grey_1x1": e(1, 1, ((1, 1),), seed=501)}  # one block, one tile, 63 idle lanes in its only busy wave
    for k, (w, h) in enumerate(SMALL_SIZES):  # dummy blocks to the right, below and both; chroma grids of one block
        for j, (name, sampling) in enumerate(LAYOUTS.items()):
            out["%dx%d_%s" % (w, h, name)] = e(w, h, sampling, seed=510 + 10 * k + j)
    out["264x200_420"] = e(264, 200, LAYOUTS["420"], quality=60, seed=541)  # 825 luma blocks: 4 tiles, the last of 57 blocks
    out["ni_420"] = e(75, 53, LAYOUTS["420"], interleaved=False, seed=542)  # a component's own scan: the real blocks only
    o = oracle.decode(out["ni_420"])
    out["prog_of_ni_420"] = P.encode(o.width, o.height, list(zip(o.hs, o.vs)), {q: o.qtab[q] for q in set(o.qidx)}, o.qidx, o.coef,
                                     P.script_pillow_like(o.ncomp))
    out["dri1_420"] = e(40, 24, LAYOUTS["420"], restart_interval=1, seed=543)
    out["dri3_422"] = e(75, 53, LAYOUTS["422"], restart_interval=3, seed=544)
    out["crafted"] = jpegsynth.encode_blocks(crafted_units(), I.BLOCKS_X, I.COUNTS_Q.astype(np.uint8))
    # ... under a 16-bit table that reaches 65521: products of up to 1023 x 65521 round in float32 and overflow float16
    out["crafted_q16"] = I.with_qtables16(out["crafted"], {0: 1 + 1040 * np.arange(64)})
    out["cmyk"] = e(33, 17, ((1, 1),) * 4, seed=545)
    out["two_comp"] = e(24, 17, ((2, 1), (1, 1)), seed=546)
    out["q16"] = e(40, 24, LAYOUTS["420"], restart_interval=2, quality=3, noise=30, seed=547, qmax=65535)  # 16-bit DQT (Pq = 1)
    return out
