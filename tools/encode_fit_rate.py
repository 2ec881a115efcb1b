"""What encoding to a byte budget costs on the device against the route a caller had without it, in one process, the variants
alternating inside every round (the method of tools/tensor_rate.py), timed with device events around each variant's calls.
Two workloads, both over the range 1..95 with each image's budget at half of its size at quality 75:

  * "resized": 64 RGB images of 224 x 224, 4:2:0
  * "photos":  8 RGB images of 4032 x 3024 (12 MP), 4:2:0

  * "fit":  jpeggpu_amd.encode_fit_into -- ONE jpeggpu_ext_encode_fit_batch call: the pixel stage once, every evaluation on the
    device, no synchronisation before the results are read;
  * "host": the same bisection driven from the host through encode_into with outs=None (sizes only), one synchronisation and
    one read-back per evaluation, every evaluation with its own pixel stage, then the final encode_into into the slots --
    what a caller could do before.
Both end with the sizes, statuses and qualities on the host. Before anything is timed the two routes' qualities and files are
compared. The bar: "fit" is not slower than "host" on either workload (medians of the rounds; the spreads are max - min).

`--parent-lib PATH` adds the plain call: jpeggpu_ext_encode_batch at quality 75 on the same images through this build's
library ("plain") and through the library at PATH, built from the parent commit ("plain_parent"), alternating as above: the
kernels of an existing call were recompiled from shared code, and the two must agree within the spread of the rounds.
Not bench.py: that one measures the flagship workload and stays as it is.

`--once WORKLOAD` runs a single budget call and nothing else: the process to put under a kernel trace.

    python tools/encode_fit_rate.py [--rounds 7] [--iters 5] [--parent-lib PATH] [--out encode_fit_rate.json] [--once photos|resized]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.draft_rate import _spread  # noqa: E402

LO, HI, REFERENCE_QUALITY = 1, 95, 75
PARAMS = dict(subsampling="4:2:0", restart_interval=0)


def _workload(torch, name):
    import jpeggpu_amd
    from tools import jpegsynth

    cfg = [jpegsynth.config(2, seed=100 + s) for s in range(8)]
    if name == "photos":
        return [x.clone() for x in jpeggpu_amd.decode_batch_to_rgb(cfg)]
    return list(jpeggpu_amd.decode_resized([cfg[i % 8] for i in range(64)], 224).contiguous())


def _events(torch, fn, iters):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    ev0.record()
    for _ in range(iters):
        fn()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) / iters


def _slots(torch, images, budgets):
    offsets, total = [], 0
    for b in budgets:
        offsets.append(total)
        total = (total + b + 15) // 16 * 16
    buf = torch.empty(max(total, 1), dtype=torch.uint8, device=images[0].device)
    return buf, [buf[o:o + b] for o, b in zip(offsets, budgets)]


def fit_route(torch, images, budgets, outs):
    import jpeggpu_amd

    sizes, status, qualities = jpeggpu_amd.encode_fit_into(images, outs, budgets, HI, LO, **PARAMS)
    raw = torch.cat([sizes.view(torch.uint8), status.view(torch.uint8), qualities.view(torch.uint8)]).cpu()  # one synchronisation
    n = len(images)
    return raw[:8 * n].view(torch.int64).tolist(), raw[8 * n:12 * n].view(torch.int32).tolist(), raw[12 * n:].view(torch.int32).tolist()


def host_route(torch, images, budgets, outs):
    """The rule of jpeggpu_ext_encode_fit_batch with the host in the loop: the items in lockstep, one sizes-only call per evaluation
    over the items still searching."""
    import jpeggpu_amd

    n = len(images)

    def sizes_at(which, qs):
        """{i: size(qs[i])} of the items still searching, in one call."""
        s, _ = jpeggpu_amd.encode_into([images[i] for i in which], [None] * len(which), quality=[qs[i] for i in which], **PARAMS)
        return dict(zip(which, s.cpu().tolist()))  # the synchronisation and the read-back of this evaluation

    chosen, over = [None] * n, [False] * n
    s = sizes_at(list(range(n)), [HI] * n)
    for i in range(n):
        if s[i] <= budgets[i]:
            chosen[i] = HI
    todo = [i for i in range(n) if chosen[i] is None]
    if todo:
        s = sizes_at(todo, [LO] * n)
        for i in todo:
            if s[i] > budgets[i]:
                chosen[i], over[i] = LO, True
    best, a, b = [LO] * n, [LO + 1] * n, [HI - 1] * n
    while True:
        for i in range(n):
            if chosen[i] is None and a[i] > b[i]:
                chosen[i] = best[i]
        todo = [i for i in range(n) if chosen[i] is None]
        if not todo:
            break
        m = [(a[i] + b[i]) // 2 for i in range(n)]
        s = sizes_at(todo, m)
        for i in todo:
            if s[i] <= budgets[i]:
                best[i], a[i] = m[i], m[i] + 1
            else:
                b[i] = m[i] - 1
    sizes, status = jpeggpu_amd.encode_into(images, [None if o else out for o, out in zip(over, outs)], quality=chosen, **PARAMS)
    raw = torch.cat([sizes.view(torch.uint8), status.view(torch.uint8)]).cpu()
    status = [5 if o else st for o, st in zip(over, raw[8 * n:].view(torch.int32).tolist())]
    return raw[:8 * n].view(torch.int64).tolist(), status, chosen


def _plain_call(torch, L, images):
    """jpeggpu_ext_encode_batch through the library handle L, sizes only read back: the existing call as a caller makes it."""
    from jpeggpu_amd import api

    _, items = api._encode_items(images, REFERENCE_QUALITY, PARAMS["subsampling"], 0, "HWC")
    n = len(images)
    caps = [x.numel() for x in images]
    buf, outs = _slots(torch, images, caps)
    for i, o in enumerate(outs):
        items[i].out, items[i].capacity = o.data_ptr(), o.numel()
    need = L.jpeggpu_ext_encode_scratch_size(items, n)
    scratch = torch.empty(need, dtype=torch.uint8, device=images[0].device)
    result = torch.empty(12 * n, dtype=torch.uint8, device=images[0].device)
    stream = torch.cuda.current_stream(images[0].device).cuda_stream

    def call():
        assert L.jpeggpu_ext_encode_batch(items, n, scratch.data_ptr(), need, result.data_ptr(), result.data_ptr() + 8 * n, stream) == 0

    def files():
        call()
        sizes = result[:8 * n].view(torch.int64).cpu().tolist()
        assert not result[8 * n:].view(torch.int32).cpu().any()
        return [o[:s].cpu().numpy().tobytes() for o, s in zip(outs, sizes)]

    return call, files, (buf, scratch, result, items)


def _load(path):
    from jpeggpu_amd.api import EncodeItem

    L = C.CDLL(path)
    L.jpeggpu_ext_encode_scratch_size.argtypes = [C.POINTER(EncodeItem), C.c_int]
    L.jpeggpu_ext_encode_scratch_size.restype = C.c_size_t
    L.jpeggpu_ext_encode_batch.argtypes = [C.POINTER(EncodeItem), C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def run(rounds, iters, parent_lib=None):
    import torch

    import jpeggpu_amd

    out = []
    for name in ("resized", "photos"):
        images = _workload(torch, name)
        n = len(images)
        budgets = [len(f) // 2 for f in jpeggpu_amd.encode_jpeg(images, quality=REFERENCE_QUALITY, **PARAMS)]
        buf_a, outs_a = _slots(torch, images, budgets)
        buf_b, outs_b = _slots(torch, images, budgets)
        fit = lambda: fit_route(torch, images, budgets, outs_a)  # noqa: E731
        host = lambda: host_route(torch, images, budgets, outs_b)  # noqa: E731
        a, b = fit(), host()
        assert a == b, "the two routes disagree: %r / %r" % (a, b)
        assert all(torch.equal(x[:s], y[:s]) for x, y, s, st in zip(outs_a, outs_b, a[0], a[1]) if st == 0), "the two routes' files differ"
        variants = {"fit": fit, "host": host}
        keep = []
        if parent_lib:
            call, files, hold = _plain_call(torch, jpeggpu_amd.lib(), images)
            call_p, files_p, hold_p = _plain_call(torch, _load(parent_lib), images)
            assert files() == files_p(), "the plain call's files differ from the parent's"
            keep += [hold, hold_p]
            variants.update(plain=call, plain_parent=call_p)
        res = {k: [] for k in variants}
        for _ in range(rounds):
            for k, fn in variants.items():  # the variants alternate inside every round
                res[k].append(_events(torch, fn, iters))
        r = {k: _spread(v) for k, v in res.items()}
        entry = dict(workload=name, images=n, range=[LO, HI], budgets="size(%d) / 2" % REFERENCE_QUALITY, qualities=a[2], over_budget=sum(st == 5 for st in a[1]),
                     launches=jpeggpu_amd.encode_fit_launches(images[0].shape[1], images[0].shape[0], 3, 0, HI, LO), ms=r, rounds=rounds, iters=iters)
        entry["bar"] = {"fit_over_host": round(r["fit"]["median"] / r["host"]["median"], 4), "holds": bool(r["fit"]["median"] <= r["host"]["median"])}
        if parent_lib:
            p, q = r["plain"], r["plain_parent"]
            entry["plain"] = {"over_parent": round(p["median"] / q["median"], 4),
                              "within_spread": bool(abs(p["median"] - q["median"]) <= max(p["spread"], q["spread"]))}
        out.append(entry)
        del images, buf_a, buf_b, outs_a, outs_b, keep
        torch.cuda.empty_cache()
    return out


def once(name):
    """One budget call and nothing else: the process to put under a kernel trace."""
    import torch

    import jpeggpu_amd

    images = _workload(torch, name)
    budgets = [len(f) // 2 for f in jpeggpu_amd.encode_jpeg(images, quality=REFERENCE_QUALITY, **PARAMS)]
    buf, outs = _slots(torch, images, budgets)
    sizes, status, qualities = fit_route(torch, images, budgets, outs)
    print(json.dumps(dict(workload=name, images=len(images), file_bytes=sum(sizes), qualities=qualities)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--once", default=None, choices=("photos", "resized"))
    a = ap.parse_args()
    if a.once:
        return once(a.once)
    res = run(a.rounds, a.iters, a.parent_lib)
    for r in res:
        print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
