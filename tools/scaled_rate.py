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

    keep, entries = [], []
    for data in datas:
        dec = jpeggpu_amd.Decoder()
        dec.set_batch_hint(hint)
        dec.set_scale(d)
        info = dec.parse_header(data)
        n = dec.get_buffer_size()
        tmp = torch.empty(n + 256, dtype=torch.uint8, device="cuda:0")
        base = (tmp.data_ptr() + 255) // 256 * 256
        planes = [torch.empty((info.sizes_y[c], info.sizes_x[c]), dtype=torch.uint8, device="cuda:0") for c in range(info.num_components)]
        dec.transfer(base, n, 0)
        keep.append((dec, tmp, planes, info))
        entries.append((dec, [p.data_ptr() for p in planes], [p.stride(0) for p in planes], base, n))
    batch = jpeggpu_amd.Batch(len(datas) * 3)
    scratch = torch.empty(batch.scratch_size, dtype=torch.uint8, device="cuda:0")
    batch.set_items(entries)
    return batch, scratch, keep


def _idct_bytes(keep):
    """Bytes the IDCT stage moves: data-unit records (8 B), symbol entries (2 B each, all of a unit's at d < 8, the DC one
    at d = 8 -- approximated by the write pass's counts read back) and the plane bytes written."""
    total = 0
    for dec, tmp, planes, info in keep:
        lay = dec.layout()
        for s in range(lay.num_scans):
            sl = lay.scans[s]
            total += 8 * sl.num_data_units
        total += sum(p.numel() for p in planes)
    return total


def _sym_bytes(torch, keep, d):
    import numpy as np

    from tests import gpu_util

    total = 0
    for dec, tmp, planes, info in keep[:1]:
        lay = dec.layout()
        base = (tmp.data_ptr() + 255) // 256 * 256
        for s in range(lay.num_scans):
            sl = lay.scans[s]
            tab = gpu_util.tmp_view(torch, tmp, base, sl.off_du_table, sl.num_data_units * 2, torch.int32).view(np.uint32).reshape(-1, 2)
            total += 2 * (sl.num_data_units if d == 8 else int((tab[:, 1] & 127).sum()))
    return total * len(keep)


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
    for (name, d), (batch, scratch, keep) in setups.items():  # warm-up, and the symbol-stream bytes of each setup
        batch.decode(scratch.data_ptr(), 0)
    torch.cuda.synchronize()
    sym = {k: _sym_bytes(torch, v[2], k[1]) for k, v in setups.items()}
    for r in range(rounds):
        for name in ("photo", "batch64"):
            for d in SCALES:  # the scales alternate inside every round
                batch, scratch, keep = setups[(name, d)]
                torch.cuda.synchronize()
                ev0.record()
                for _ in range(iters):
                    batch.decode(scratch.data_ptr(), 0)
                ev1.record()
                torch.cuda.synchronize()
                ms = ev0.elapsed_time(ev1) / iters
                results[(name, d)]["img_s"].append(len(keep) * 1000.0 / ms)
                batch.set_profiling(True)  # (a new measurement window)
                for _ in range(3):
                    batch.decode(scratch.data_ptr(), 0)
                torch.cuda.synchronize()
                results[(name, d)]["idct_ms"].append(batch.stage_ms()["idct"])
                batch.set_profiling(False)
    out = []
    for (name, d), v in results.items():
        keep = setups[(name, d)][2]
        nbytes = _idct_bytes(keep) + sym[(name, d)]
        idct = statistics.median(v["idct_ms"])
        out.append({
            "workload": name, "scale": d, "images": len(keep),
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
