"""Inputs of the run-schedule tests (CPU: tests/test_sync_runs_host.py, GPU: tests/test_gpu_sync_runs.py): scans whose
restart segments have a given number of subsequences, scans of an exact number of subsequences, and the layouts a
batched call meets. All from tools/jpegsynth, a few hundred KB at the most."""
import functools

import numpy as np

from tests.syncruns import syncruns
from tools import jpegsynth

GRAY = ((1, 1),)
S420 = ((2, 2), (1, 1), (1, 1))
SEQ = 255  # subsequences per write-pass sequence of a batched call (jg_defs.h, kSeqSubseqBatch)


@functools.lru_cache(maxsize=None)
def segments_of(k, subseq_bytes):
    """A grayscale scan most of whose restart segments are k subsequences of `subseq_bytes` long: the first restart
    interval (in MCUs) at which at least 4 in 5 are."""
    for ri in range(1, 400):
        data = jpegsynth.encode(1024, 48, GRAY, True, ri, quality=88, noise=9, seed=5)
        x = syncruns.run(data, subseq_bytes, 1)
        if x.segments_of[k] * 5 >= x.segments * 4 and x.segments >= 8:
            return data
    raise AssertionError("no restart interval gives segments of %d subsequences" % k)


def _column(n, seed=11):
    """n coefficient blocks of 35 to 60 bytes each: the image is one block wide, so a file of n blocks is a prefix, block by
    block, of the file of n + 1, and the subsequence count grows by at most one per block."""
    rng = np.random.default_rng(seed)
    coef = np.zeros((n, 64), np.int16)
    coef[:, 0] = rng.integers(-60, 61, n)
    coef[:, 1:41] = rng.integers(-31, 32, (n, 40))
    return coef


@functools.lru_cache(maxsize=None)
def exactly(subsequences, subseq_bytes):
    """A grayscale scan without restart markers of exactly that many subsequences (bisection over the block count)."""
    coef, q = _column(8000), np.ones(64, np.uint8)
    count = lambda n: syncruns.num_subseq(jpegsynth.encode_blocks(coef[:n], 1, q), subseq_bytes)
    lo, hi = 1, len(coef)
    assert count(hi) >= subsequences
    while lo < hi:  # the smallest n with count(n) >= subsequences; the count grows in steps of at most one
        mid = (lo + hi) // 2
        if count(mid) >= subsequences:
            hi = mid
        else:
            lo = mid + 1
    data = jpegsynth.encode_blocks(coef[:lo], 1, q)
    assert syncruns.num_subseq(data, subseq_bytes) == subsequences
    return data


def no_restart():
    return jpegsynth.encode(333, 251, S420, True, 0, quality=85, noise=8, seed=21)


def layouts():
    """A 4:2:0 interleaved file with restart intervals, a three-scan non-interleaved file, a 4-component file."""
    return {"420_dri": jpegsynth.encode(333, 251, S420, True, 7, quality=88, noise=9, seed=22),
            "three_scans": jpegsynth.encode(200, 152, ((1, 1), (1, 1), (1, 1)), False, 0, quality=85, noise=8, seed=23),
            "four_comp": jpegsynth.encode(168, 120, ((2, 1), (1, 1), (1, 1), (2, 1)), True, 0, quality=85, optimize=True, noise=6, seed=24)}


def files(r, subseq_bytes):
    """name -> bytes: the cases of one run length at one subsequence size."""
    out = {"segments_of_%d" % k: segments_of(k, subseq_bytes) for k in sorted({1, 2, 3, r + 1})}
    out["no_restart"] = no_restart()
    out["fewer_than_r"] = exactly(max(r - 1, 1), subseq_bytes)
    out["one_subsequence"] = exactly(1, subseq_bytes)
    out["255r"] = exactly(SEQ * r, subseq_bytes)
    out["255r_plus_1"] = exactly(SEQ * r + 1, subseq_bytes)
    out.update(layouts())
    return out
