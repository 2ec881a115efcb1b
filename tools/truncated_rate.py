"""What a truncated file costs on the device, in one process: one 12 MP file (BASELINE.json configs[2]: 4032 x 3024 4:2:0, a
restart interval per MCU row; and the same picture without restart markers), whole and cut at half its scan, decoded on
its own with the flag set (jpeggpu_ext_set_truncated) and stage timing on: the stage times of the lone decode, whole and cut
alternating round by round. The three launches of jg_trunc.hip are counted in the stages they follow: the destuff stage
(trunc_prepare) and the write pass (trunc_find, trunc_fill). Nothing is asserted.

    python tools/truncated_rate.py [--rounds 5] [--iters 10] [--out truncated_rate.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def run(rounds, iters):
    import torch

    import jpeggpu_amd
    from tools import jpegsynth

    def scan_begin(d):
        i = 2
        while True:
            m, n = d[i + 1], d[i + 2] << 8 | d[i + 3]
            i += 2 + n
            if m == 0xDA:
                return i

    files = {"rst": jpegsynth.config(2, seed=0), "plain": jpegsynth.encode(4032, 3024, ((2, 2), (1, 1), (1, 1)), True, 0, quality=88, noise=9, seed=0)}
    stream = torch.cuda.Stream()
    out = {}
    for name, data in files.items():
        b = scan_begin(data)
        inputs = {"whole": data, "cut": data[:b + (len(data) - b) // 2]}
        state = {}
        for kind, d in inputs.items():
            dec = jpeggpu_amd.Decoder()
            dec.set_truncated(True)
            info = dec.parse_header(d)
            n = dec.get_buffer_size()
            tmp = torch.empty(n + 256, dtype=torch.uint8, device="cuda")
            base = (tmp.data_ptr() + 255) // 256 * 256
            planes = [torch.zeros((info.sizes_y[c], info.sizes_x[c]), dtype=torch.uint8, device="cuda") for c in range(info.num_components)]
            dec.transfer(base, n, stream.cuda_stream)
            dec.set_profiling(True)
            state[kind] = (dec, [p.data_ptr() for p in planes], [p.stride(0) for p in planes], base, n, tmp, planes)
        samples = {kind: [] for kind in inputs}
        for _ in range(rounds):
            for kind, (dec, ptrs, pitches, base, n, _, _) in state.items():
                for _ in range(iters):
                    dec.decode(ptrs, pitches, base, n, stream.cuda_stream)
                stream.synchronize()
                samples[kind].append(dec.stage_ms())
        for kind in inputs:
            stages = samples[kind][0].keys()
            out["%s_%s" % (name, kind)] = {"bytes": len(inputs[kind]), "subsequence_bytes": state[kind][0].layout().subsequence_bytes,
                                           "stage_us": {s: round(1e3 * statistics.median(r[s] for r in samples[kind]), 1) for s in stages}}
            out["%s_%s" % (name, kind)]["total_us"] = round(sum(out["%s_%s" % (name, kind)]["stage_us"].values()), 1)
        for dec, *_ in state.values():
            dec.cleanup()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = run(a.rounds, a.iters)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
