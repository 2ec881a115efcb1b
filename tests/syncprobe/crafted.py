"""A file whose sync-pack multi-symbol entries end in long magnitudes (jg_defs.h: the last symbol of an entry needs only
its code inside the index bits)."""
import numpy as np

from tools import jpegsynth

S420 = ((2, 2), (1, 1), (1, 1))
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13,
                   6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45,
                   38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


def _blocks(n, rng):
    """n coefficient blocks (natural order) whose two most frequent AC symbols are (run 0, category 1) and (run 0,
    category 10): runs of +-1 closed by a coefficient of magnitude 512..1023, a few other symbols in between, an end of
    block behind 20 to 50 coefficients. DC values are small, so that any order of the blocks needs the same few DC
    categories."""
    zz = np.zeros((n, 64), np.int16)
    zz[:, 0] = rng.integers(-24, 25, n)
    for b in range(n):
        k, last = 1, int(rng.integers(20, 51))
        while k < last:
            r = rng.random()
            if r < 0.60:
                zz[b, k] = rng.choice((-1, 1))
            elif r < 0.90:
                zz[b, k] = rng.choice((-1, 1)) * int(rng.integers(512, 1024))
            elif r < 0.95:
                zz[b, k] = rng.choice((-1, 1)) * int(rng.integers(2, 64))
            # else: a zero, i.e. a run
            k += 1
        zz[b, last] = 1  # no run of zeros in front of the end of block
    nat = np.zeros_like(zz)
    nat[:, ZIGZAG] = zz
    return nat


def long_magnitude_case(seed=77):
    """128 x 128, 4:2:0, one restart interval per MCU row. The Huffman tables are the ones jpegsynth.encode_blocks fits
    (optimize=True) to the file's own blocks -- encode_blocks writes grayscale files only, so its tables are taken from
    the file it writes and the 4:2:0 file is coded with them for every component (encode_custom)."""
    from tests.syncprobe import syncprobe

    rng = np.random.default_rng(seed)
    mx = my = 8
    luma = _blocks(4 * mx * my, rng).reshape(2 * my, 2 * mx, 64)
    cb = _blocks(mx * my, rng).reshape(my, mx, 64)
    cr = _blocks(mx * my, rng).reshape(my, mx, 64)
    every = np.concatenate([luma.reshape(-1, 64), cb.reshape(-1, 64), cr.reshape(-1, 64)])
    q = np.ones(64, np.uint8)
    fitted = syncprobe.dht_tables(jpegsynth.encode_blocks(every, 24, q, optimize=True))
    dc = [(b, v) for tc, _, b, v in fitted if tc == 0]
    ac = [(b, v) for tc, _, b, v in fitted if tc == 1]
    assert len(dc) == 1 and len(ac) == 1
    return jpegsynth.encode_custom(16 * mx, 16 * my, S420, [luma, cb, cr], dc, ac, tables=[(0, 0)] * 3, qtables=[q],
                                   restart_interval=mx)
