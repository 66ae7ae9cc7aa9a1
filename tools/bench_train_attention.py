#!/usr/bin/env python
"""Forward + backward of the heads' linear attention: train_attention.LinearAttention against the plain-torch formula
(train_attention.linear_attention_formula: the reference's Attention.forward_linear, att_layers/attention.py:46-64) in fp32, on the
same GPU.

At 8 and at 24 images of 38 x 51 = 1938 tokens (the two training batch sizes of the reference's configs), L = S = 1938, 8 heads of
16.  One step = forward, then backward from a fixed gradient into q, k and v.  The two implementations are timed alternately,
A/B/A/B, `--rounds` times each (device events around `--iters` steps after a warm-up of both); the report gives the median and
min / max over the rounds, the bytes the algorithm has to move over the HIP time, and torch.cuda.max_memory_allocated of one step
of each (above what is allocated before it).  Writes profiles/train_attention_bench.txt (or --out).

    python tools/bench_train_attention.py [--rounds 7] [--iters 200] [--batches 8,24] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L = S = 38 * 51
H, D = 8, 16
EPS = 1e-6


def bytes_moved(N):
    """What forward + backward must read and write once: forward q, k, v in, out out; backward q, k, v, gO in, gQ, gK, gV out
    (the [N H, 272] blocks and the chunk partials are under 1 % of it)."""
    return 4.0 * H * D * N * (2 * L + 2 * S + 3 * L + 4 * S)


def make_step(fn, x, go):
    def step():
        for t in x:
            t.grad = None
        fn(*x).backward(go)
    return step


def time_ms(step, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        step()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def peak_mib(step):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    step()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--batches", default="8,24")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_attention_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_train_attention: needs a GPU (nothing is measured on the CPU)")
    from mickey_amd import build as mk_build
    from mickey_amd.train_attention import LinearAttention, linear_attention_formula
    lines = ["# tools/bench_train_attention.py: forward + backward of the heads' linear attention, train_attention.LinearAttention (hip) vs "
             "the plain-torch formula in fp32 (torch)",
             "# %s, torch %s, kernels %s; L = S = %d, %d heads of %d; %d alternating rounds of %d steps, ms per step: median [min .. max]"
             % (torch.cuda.get_device_name(0), torch.__version__, mk_build.source_hash(), L, H, D, args.rounds, args.iters),
             "# peak MiB: torch.cuda.max_memory_allocated of one step above the inputs; GB/s: the bytes forward + backward must move / hip time",
             "", "%-4s %-28s %-28s %7s %9s %10s %10s" % ("N", "hip ms", "torch ms", "t/h", "hip GB/s", "hip MiB", "torch MiB")]
    hip = LinearAttention(EPS)
    for N in [int(b) for b in args.batches.split(",")]:
        g = torch.Generator().manual_seed(N)
        x = [(1.5 * torch.randn((N, T, H, D), generator=g)).cuda().requires_grad_(True) for T in (L, S)] + \
            [torch.randn((N, S, H, D), generator=g).cuda().requires_grad_(True)]
        go = torch.randn((N, L, H, D), generator=g).cuda()
        steps = {"hip": make_step(hip, x, go), "torch": make_step(lambda q, k, v: linear_attention_formula(q, k, v, EPS), x, go)}
        for k in ("hip", "torch"):   # warm-up: code objects, the vendor library's algorithm search
            for _ in range(5):
                steps[k]()
        torch.cuda.synchronize()
        t = {"hip": [], "torch": []}
        for _ in range(args.rounds):
            for k in ("hip", "torch"):
                t[k].append(time_ms(steps[k], args.iters))
        for t_ in x:
            t_.grad = None
        mem = {k: peak_mib(steps[k]) for k in ("hip", "torch")}
        med = {k: statistics.median(v) for k, v in t.items()}
        fmt = {k: "%8.3f [%8.3f .. %8.3f]" % (med[k], min(t[k]), max(t[k])) for k in t}
        lines.append("%-4d %-28s %-28s %7.2f %9.1f %10.1f %10.1f" % (N, fmt["hip"], fmt["torch"], med["torch"] / med["hip"],
                                                                 bytes_moved(N) / med["hip"] * 1e-6, mem["hip"], mem["torch"]))
        sep = min(t["torch"]) > max(t["hip"]) or min(t["hip"]) > max(t["torch"])
        verdict = ("hip is FASTER" if med["hip"] < med["torch"] else "hip is NOT faster") if sep else "no difference beyond the spread"
        lines.append("# N = %d: torch / hip = %.2f (median); the min-max ranges of the two %s: %s"
                     % (N, med["torch"] / med["hip"], "do not overlap" if sep else "OVERLAP", verdict))
        print("\n".join(lines[-2:]), flush=True)
        del x, go, steps
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
