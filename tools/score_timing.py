#!/usr/bin/env python3
"""score_timing.py -- gear_token_logprobs against the PyTorch formulation on the same fp16 logits.

Per shape [N, V]: the kernel with lp only and with every output (lse, rank, kl, agree, top-8; the second matrix doubles the mandatory
read), and torch.log_softmax(x.float(), -1).gather(...) (+ topk 8).  Warm, median of repeated passes (device events around `inner`
calls), bytes/s against the one mandatory read of the logits (N V 2 bytes per matrix), peak extra memory of each path.

    python tools/score_timing.py [--json] [--shapes 16x32000,2048x32000,16x128256,2048x128256]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed(fn, reps, inner):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3 / inner)
    return statistics.median(ts), min(ts), max(ts)


def peak_extra(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="16x32000,2048x32000,16x128256,2048x128256")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("score_timing.py measures on the GPU; there is none")
    from gear_amd.scoring import token_logprobs
    rows = []
    for shape in args.shapes.split(","):
        N, V = (int(t) for t in shape.split("x"))
        g = torch.Generator(device="cuda").manual_seed(N + V)
        x = (torch.rand((N, V), device="cuda", generator=g) * 60 - 30).half()
        r = (x.float() + 0.05 * torch.randn((N, V), device="cuda", generator=g)).half()
        ids = torch.randint(0, V, (N,), device="cuda", generator=g)
        inner = 200 if N * V < 4e6 else 20

        def k_lp():
            return token_logprobs(x, ids).logprobs

        def k_all():
            return token_logprobs(x, ids, r, 8)

        def t_lp():
            return torch.log_softmax(x.float(), -1).gather(1, ids[:, None])

        def t_all():
            ls = torch.log_softmax(x.float(), -1)
            lr = torch.log_softmax(r.float(), -1)
            return (ls.gather(1, ids[:, None]), ls.topk(8, -1), (lr.exp() * (lr - ls)).sum(-1),
                    ls.argmax(-1) == lr.argmax(-1), (x > x.gather(1, ids[:, None])).sum(-1))

        err = float((k_lp() - t_lp()[:, 0]).abs().max())
        row = dict(N=N, V=V, max_abs_diff_vs_torch=err)
        for name, fn, mats in (("kernel_lp", k_lp, 1), ("kernel_all", k_all, 2), ("torch_lp", t_lp, 1), ("torch_all", t_all, 2)):
            med, lo, hi = timed(fn, args.reps, inner)
            row[name] = dict(us=med * 1e6, us_min=lo * 1e6, us_max=hi * 1e6, read_GBps=mats * N * V * 2 / med / 1e9,
                             peak_extra_bytes=peak_extra(fn))
        rows.append(row)
        if not args.json:
            print(f"[{N} x {V}]  (|kernel - torch| lp max {err:.2e})")
            for name in ("kernel_lp", "torch_lp", "kernel_all", "torch_all"):
                d = row[name]
                print(f"  {name:11s} {d['us']:10.1f} us  (min {d['us_min']:.1f}, max {d['us_max']:.1f})  {d['read_GBps']:8.1f} GB/s of "
                      f"mandatory read   peak extra {d['peak_extra_bytes'] / 2 ** 20:9.2f} MiB")
    if args.json:
        print(json.dumps(rows))


if __name__ == "__main__":
    main()
