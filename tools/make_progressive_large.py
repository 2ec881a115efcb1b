"""Writes tests/golden/progressive_large.npz: the progressive JPEGs that are too slow to build at test time -- two crafted
grey files of 32 942 blocks whose scans hold end-of-band runs of every category and the run of 32 767 blocks, written by
tests/progressive_ref.encode, and two photo-like files that Pillow (libjpeg-turbo) writes, with their baseline twins.

    python tools/make_progressive_large.py          (needs Pillow; written with Pillow 12.2)

Deterministic: fixed seeds, no time stamps, the arrays stored in a fixed order; a second run writes the same bytes.
The file stays below 1 000 000 bytes and the generator refuses to write more.

eob_ladder  grey 1456 x 1448, 182 x 181 = 32 942 blocks, no restart markers. Script: DC Al = 1; AC 1..5 Al = 1;
            AC 6..63 Al = 1; then the three refinements to Al = 0. Sixteen separator blocks enclose gaps of 2^r blocks,
            r = 0 .. 14 (32 767 + 16 blocks; the 159 behind the last separator are one more gap). Band 1..5 holds a
            coefficient in the separators only (zig-zag 5, magnitude 2 or 3), so its first scan and its refinement hold one
            run symbol of every category 0 .. 14 (category 7 twice). Band 6..63 holds a coefficient of magnitude 4 or 5 at
            zig-zag 6 in EVERY block, and the separators get a new +-1 at zig-zag 63 in the refinement: that scan holds a
            run of every category in which every block takes a correction bit, of both values.
eob_cap     the same geometry and script. Blocks 0, 100 and the last one hold AC coefficients, every other block has
            none: behind block 100 lie 32 840 empty blocks, which is a run of 0x7FFF -- the longest the format can say --
            and a run of 73 right behind it, in every AC scan.
photo       1024 x 768, 4:2:0, quality 85, progressive=True against progressive=False, optimize=True: smooth shapes plus
            Gaussian texture (sigma 14), no restart markers: scans of tens of KB on one lane, stuffed FF 00 pairs by the
            hundred, optimised tables with codes longer than the look-up's 9 bits.
photo_rst   512 x 384, the same with restart_marker_blocks=1: 768 segments in the DC scans, 3 072 in luma's AC scans.

libjpeg's progressive mode changes the entropy coding only, so a photo and its twin hold the same coefficients: the
generator ASSERTS that Pillow decodes both to the same pixels at full size and after draft() to 1/2, 1/4, 1/8, and fails
otherwise. Pillow's RGB is pinned as SHA-256 and shape only (the pixels would be 3 MB).

Arrays: names; prog/<name> for all four; twin/<name>, rgb_sha256/<name>/<d> (32 bytes), rgb_shape/<name>/<d> for the photos.
"""
import hashlib
import io
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import progressive_ref as pr  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "progressive_large.npz")
LIMIT = 1000 * 1000
SCALES = (1, 2, 4, 8)
GRID = (181, 182)  # block rows, block columns of the crafted files
NAT = pr.ZIGZAG     # zig-zag index -> natural index


def script_ladder():
    return [((0,), 0, 0, 0, 1), ((0,), 1, 5, 0, 1), ((0,), 6, 63, 0, 1), ((0,), 0, 0, 1, 0), ((0,), 1, 5, 1, 0), ((0,), 6, 63, 1, 0)]


def separators():
    """Block numbers (raster order) of the sixteen separators: block 0, then one behind a gap of 2^r blocks, r = 0 .. 14."""
    at, out = 0, [0]
    for r in range(15):
        at += (1 << r) + 1
        out.append(at)
    return out


def dc_walk(rng, n):
    """DC values whose differences stay small (the DC scan is most of such a file's bytes), odd and even ones alike."""
    return np.clip(np.cumsum(rng.integers(-3, 4, n)), -900, 900)


def encode_grey(coef):
    q = {0: np.full(64, 2, np.int64)}
    return pr.encode(GRID[1] * 8, GRID[0] * 8, [(1, 1)], q, [0], [coef.reshape(GRID[0], GRID[1], 64)], script_ladder())


def eob_ladder():
    rng = np.random.default_rng(20261019)
    n = GRID[0] * GRID[1]
    coef = np.zeros((n, 64), np.int64)
    coef[:, 0] = dc_walk(rng, n)
    coef[:, NAT[6]] = rng.choice([4, 5, -4, -5], n)
    seps = separators()
    assert len(seps) == 16 and seps[-1] == 32767 + 15 and n - 1 - seps[-1] == 159
    coef[seps, NAT[5]] = rng.choice([2, 3, -2, -3], len(seps))
    coef[seps, NAT[63]] = rng.choice([1, -1], len(seps))
    return encode_grey(coef)


def eob_cap():
    rng = np.random.default_rng(20261020)
    n = GRID[0] * GRID[1]
    coef = np.zeros((n, 64), np.int64)
    coef[:, 0] = dc_walk(rng, n)
    for b in (0, 100, n - 1):  # first scans, correction bits of both values and new coefficients in the refinements
        coef[b, NAT[2]], coef[b, NAT[5]], coef[b, NAT[3]] = 3, -2, 1
        coef[b, NAT[6]], coef[b, NAT[40]], coef[b, NAT[63]] = -5, 4, -1
    assert n - 1 - 101 == 0x7FFF + 73
    return encode_grey(coef)


def picture(width, height, seed):
    """Smooth shapes plus Gaussian texture."""
    from PIL import Image

    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:height, 0:width].astype(np.float64)
    planes = []
    for c in range(3):
        p = 128 + 60 * np.sin(x / (41.0 + 9 * c) + c) + 45 * np.cos(y / (33.0 + 11 * c)) + 25 * ((x // 96 + y // 80) % 2)
        p += 30 * np.exp(-((x - width * (0.3 + 0.2 * c)) ** 2 + (y - height * 0.5) ** 2) / (2 * (height / 5.0) ** 2))
        planes.append(p + rng.normal(0, 14, (height, width)))
    return Image.fromarray(np.clip(np.stack(planes, -1), 0, 255).astype(np.uint8), "RGB")


def save(im, **kw):
    b = io.BytesIO()
    im.save(b, "JPEG", quality=85, optimize=True, subsampling=2, **kw)
    return b.getvalue()


def pillow_rgb(data, d):
    from PIL import Image

    im = Image.open(io.BytesIO(data))
    w, h = im.size
    if d > 1:
        im.draft("RGB", (max(w // d, 1), max(h // d, 1)))
    out = np.asarray(im.convert("RGB"))
    assert out.shape[:2] == (-(-h // d), -(-w // d)), (out.shape, w, h, d)
    return out


def main():
    arrays = {"names": np.array(["eob_cap", "eob_ladder", "photo", "photo_rst"])}
    arrays["prog/eob_ladder"] = np.frombuffer(eob_ladder(), np.uint8)
    arrays["prog/eob_cap"] = np.frombuffer(eob_cap(), np.uint8)
    for name, w, h, seed, kw in (("photo", 1024, 768, 700, {}), ("photo_rst", 512, 384, 701, dict(restart_marker_blocks=1))):
        im = picture(w, h, seed)
        prog, twin = save(im, progressive=True, **kw), save(im, progressive=False, **kw)
        assert b"\xff\xc2" in prog[:700] and b"\xff\xc2" not in twin[:700]
        arrays["prog/" + name] = np.frombuffer(prog, np.uint8)
        arrays["twin/" + name] = np.frombuffer(twin, np.uint8)
        for d in SCALES:
            a, b = pillow_rgb(prog, d), pillow_rgb(twin, d)
            assert np.array_equal(a, b), "Pillow decodes %s and its twin differently at 1/%d" % (name, d)
            arrays["rgb_sha256/%s/%d" % (name, d)] = np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)
            arrays["rgb_shape/%s/%d" % (name, d)] = np.array(a.shape, np.int64)
    for k in sorted(arrays):
        if k.startswith(("prog/", "twin/")):
            print("%-16s %7d bytes" % (k, arrays[k].size))
    b = io.BytesIO()
    with zipfile.ZipFile(b, "w", zipfile.ZIP_DEFLATED) as z:  # np.savez_compressed's format without its time stamps
        for k, a in arrays.items():
            member = io.BytesIO()
            np.lib.format.write_array(member, np.asanyarray(a), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), member.getvalue(), zipfile.ZIP_DEFLATED)
    assert len(b.getvalue()) < LIMIT, "%d bytes: more than a committed fixture may have" % len(b.getvalue())
    with open(OUT, "wb") as f:
        f.write(b.getvalue())
    print("%d bytes" % len(b.getvalue()))


if __name__ == "__main__":
    main()
