"""What DCT-domain access costs, in one process, the variants alternating inside every round (the method of
tools/thumbnail_rate.py): 64 files of bench.py's default configuration (BASELINE.json configs[2]: 4032 x 3024, 4:2:0, a
restart interval of one MCU row; tools/jpegsynth), parsed and transferred once.

  * "decode_coefficients_only" (a): the decode batch that stops in front of the IDCT, alone.
  * "read_int16" (b): jpeggpu_ext_read_coefficients_batch on that decoded batch -- the output allocation, one copy of
    descriptors and the ONE launch of read_blocks; "read_float32" and "read_float16": the same, dequantised.
  * "transcode_plain": jpeggpu_ext_transcode_batch on the same decoded batch, whose first launch is gather_blocks (c): the
    gather reads the entries read_blocks reads and stores the same 128 bytes a block, but there is no call that launches it
    alone, so its own time comes from a kernel trace (below).
  * "decode_batch_to_rgb" (d): parse, transfer, the full decode batch and the RGB conversion: what a caller spends who
    wants pixels.
  * "read_coefficients": the public call from bytes on the host -- parse, transfer, (a) and (b).
Medians of the rounds with their spread (max - min), in milliseconds per call over all 64 files, from device events. Before
anything is timed the tensors of the first and last file are compared with the oracle's coefficients.

`--once` makes `--iters` rounds of (a), (b) and the transcode call and nothing else: the process to put under a kernel trace
(`rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/coefficients_rate.py --once`), which gives read_blocks
and gather_blocks their own durations in the same run. `--trace FILE` then reads that trace's kernel CSV and prints the
median and spread of both kernels' durations.
Not bench.py: that one measures the flagship workload and stays as it is.

    python tools/coefficients_rate.py [--rounds 7] [--iters 3] [--images 64] [--out coefficients_rate.json] [--once] [--trace FILE]
"""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.crop_rate import _time  # noqa: E402
from tools.draft_rate import _spread  # noqa: E402


def _sources(n):
    from tools import jpegsynth

    cfg = [jpegsynth.config(2, seed=100 + s) for s in range(8)]
    return [cfg[i % 8] for i in range(n)]


def _check(jpeggpu_amd, datas, cs):
    import numpy as np

    from oracle import oracle

    for i in (0, len(datas) - 1):
        want = oracle.decode(datas[i]).coef
        for t, w in zip(cs[i].coefficients, want):
            got = t.cpu().numpy().reshape(t.shape[0], t.shape[1], 64)
            assert np.array_equal(got, w[:got.shape[0], :got.shape[1]]), "a coefficient tensor differs from the oracle's"


def run(rounds, iters, n, once=False):
    import torch

    import jpeggpu_amd

    datas = _sources(n)
    with jpeggpu_amd.BatchDecode(datas, "cuda:0", coefficients_only=True) as bd:
        slots = [torch.empty(2 * len(d) + 4096, dtype=torch.uint8, device="cuda:0") for d in datas]
        bd.decode()
        _check(jpeggpu_amd, datas, jpeggpu_amd.read_coefficients_into(bd))
        items = jpeggpu_amd.api._transcode_items(bd, False, False, None)
        variants = {
            "decode_coefficients_only": bd.decode,
            "read_int16": lambda: jpeggpu_amd.read_coefficients_into(bd),
            "read_float32": lambda: jpeggpu_amd.read_coefficients_into(bd, torch.float32, True),
            "read_float16": lambda: jpeggpu_amd.read_coefficients_into(bd, torch.float16, True),
            "transcode_plain": lambda: jpeggpu_amd.transcode_into(bd, slots, items=items),
        }
        if once:
            for _ in range(iters):
                for k in ("decode_coefficients_only", "read_int16", "transcode_plain"):
                    variants[k]()
            torch.cuda.synchronize()
            return [dict(once=True, iters=iters, images=n)]
        variants["decode_batch_to_rgb"] = lambda: jpeggpu_amd.decode_batch_to_rgb(datas)
        variants["read_coefficients"] = lambda: jpeggpu_amd.read_coefficients(datas)
        for fn in variants.values():  # warm up: allocator, staging ring, code objects
            fn()
        torch.cuda.synchronize()
        res = {k: [] for k in variants}
        for _ in range(rounds):
            for k, fn in variants.items():  # the variants alternate inside every round
                res[k].append(_time(torch, fn, iters))
    blocks = sum(t.shape[0] * t.shape[1] for x in jpeggpu_amd.read_coefficients(datas[:1]) for t in x.coefficients) * n
    out = [dict(variant=k, ms=_spread(v), images_per_s=round(n * 1e3 / _spread(v)["median"], 1)) for k, v in res.items()]
    out.append(dict(workload="configs[2] 4032x3024 4:2:0", images=n, blocks=blocks, int16_bytes=128 * blocks, rounds=rounds, iters=iters))
    return out


def trace(path):
    """Median and spread of read_blocks' and gather_blocks' durations in a rocprofv3 kernel-trace CSV, in milliseconds."""
    ms = {"read_blocks": [], "gather_blocks": []}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            for k in ms:
                if k in row["Kernel_Name"]:
                    ms[k].append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-6)
    return [dict(kernel=k, launches=len(v), ms=_spread(v)) for k, v in ms.items() if v]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--out", default=None)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--trace", default=None)
    a = ap.parse_args()
    res = trace(a.trace) if a.trace else run(a.rounds, a.iters, a.images, a.once)
    for r in res:
        print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
