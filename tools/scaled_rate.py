"""Decode rate at every scale (jpeggpu_ext_set_scale): the reference photo decoded on its own, and a 64-image batch of
BASELINE.json configs[2] (4032 x 3024 4:2:0, tools/jpegsynth) through jpeggpu_ext_decode_batch, at d = 1, 2, 4, 8 in
one process, the scales alternating round by round. Per scale: images/s from device events, the `idct` stage's ms from
the batch's stage timing, the bytes that stage moves (symbol stream + data-unit table read, planes written) and their
share of HBM peak. Not bench.py: that one measures the flagship workload at full size and stays as it is.

    python tools/scaled_rate.py [--rounds 7] [--iters 10] [--out scaled_rate.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E peak, GB/s
SCALES = (1, 2, 4, 8)


def _setup(torch, datas, d, hint):
    import jpeggpu_amd

    return jpeggpu_amd.BatchDecode(datas, hint=hint, idct="reference", progressive=False, scales=[d] * len(datas), scale_mode="uniform")


def _idct_bytes(bd):
    """Bytes the IDCT stage moves: data-unit records (8 B), symbol entries (2 B each, all of a unit's at d < 8, the DC one
    at d = 8 -- approximated by the write pass's counts read back) and the plane bytes written."""
    total = 0
    for dec, planes in zip(bd.decoders, bd.planes):
        lay = dec.layout()
        for s in range(lay.num_scans):
            sl = lay.scans[s]
            total += 8 * sl.num_data_units
        total += sum(p.numel() for p in planes)
    return total


def _sym_bytes(torch, bd, d):
    import numpy as np

    from tests import gpu_util

    total = 0
    for dec, tmp in zip(bd.decoders[:1], bd.tmps):
        lay = dec.layout()
        base = (tmp.data_ptr() + 255) // 256 * 256
        for s in range(lay.num_scans):
            sl = lay.scans[s]
            tab = gpu_util.tmp_view(torch, tmp, base, sl.off_du_table, sl.num_data_units * 2, torch.int32).view(np.uint32).reshape(-1, 2)
            total += 2 * (sl.num_data_units if d == 8 else int((tab[:, 1] & 127).sum()))
    return total * len(bd.decoders)


def run(rounds, iters):
    import torch

    from tools import jpegsynth

    photo = open(os.path.join(ROOT, "tests", "golden", "IMG_6510.JPG"), "rb").read()
    cfg = [jpegsynth.config(2, seed=100 + s) for s in range(8)]
    setups = {}
    for d in SCALES:
        setups[("photo", d)] = _setup(torch, [photo], d, 0)
        setups[("batch64", d)] = _setup(torch, [cfg[i % 8] for i in range(64)], d, 64)
    results = {k: {"img_s": [], "idct_ms": []} for k in setups}
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for bd in setups.values():  # warm-up, and the symbol-stream bytes of each setup
        bd.decode()
    torch.cuda.synchronize()
    sym = {k: _sym_bytes(torch, v, k[1]) for k, v in setups.items()}
    for r in range(rounds):
        for name in ("photo", "batch64"):
            for d in SCALES:  # the scales alternate inside every round
                bd = setups[(name, d)]
                torch.cuda.synchronize()
                ev0.record()
                for _ in range(iters):
                    bd.decode()
                ev1.record()
                torch.cuda.synchronize()
                ms = ev0.elapsed_time(ev1) / iters
                results[(name, d)]["img_s"].append(len(bd.decoders) * 1000.0 / ms)
                bd.batch.set_profiling(True)  # (a new measurement window)
                for _ in range(3):
                    bd.decode()
                torch.cuda.synchronize()
                results[(name, d)]["idct_ms"].append(bd.batch.stage_ms()["idct"])
                bd.batch.set_profiling(False)
    out = []
    for (name, d), v in results.items():
        bd = setups[(name, d)]
        nbytes = _idct_bytes(bd) + sym[(name, d)]
        idct = statistics.median(v["idct_ms"])
        out.append({
            "workload": name, "scale": d, "images": len(bd.decoders),
            "img_s_median": round(statistics.median(v["img_s"]), 1), "img_s_min": round(min(v["img_s"]), 1), "img_s_max": round(max(v["img_s"]), 1),
            "idct_ms_median": round(idct, 4), "idct_ms_min": round(min(v["idct_ms"]), 4), "idct_ms_max": round(max(v["idct_ms"]), 4),
            "idct_bytes": nbytes, "idct_gb_s": round(nbytes / (idct * 1e6), 1) if idct > 0 else None,
            "idct_hbm_share": round(nbytes / (idct * 1e6) / HBM_PEAK_GBS, 4) if idct > 0 else None,
        })
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = run(a.rounds, a.iters)
    for r in res:
        print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
