#!/usr/bin/env python
"""Forward + backward of the heads' BasicBlocks (utils/extractor_utils.py:12-35), fp32, two contenders on the same GPU:

    convs    a reference-style block after use_hip_convs alone: the 3x3 convolutions on the HIP kernels, BatchNorm / ReLU / the residual
             add / the 1x1 shortcut as the small torch ops a reference model runs
    blocks   the same block after use_hip_convs AND use_hip_blocks: BatchNorm + residual + ReLU as one node (mickey_amd.train_block),
             the shortcut on the Linear kernels

At 8 and at 24 images of 38 x 51 (the two training batch sizes of the reference's configs), for the five block shapes of a head
(1024->512, 512->256, 256->128, 128->64 with a shortcut, 128->128 without) and for the four blocks of one head in a row
(1024->512->256->128->64).  The input is a contiguous NCHW tensor without a gradient, as the frozen encoder hands it over.  One step =
forward in training mode, then backward from a fixed gradient into every Parameter.  The contenders are timed alternately, `--rounds`
times each (device events around `--iters` steps after half a second of alternating steps of both); the report gives the median and
min / max over the rounds, whether the ranges overlap, and torch.cuda.max_memory_allocated of one step (above what is allocated
before it).  Every batch size runs in a child process of its own under a time limit; the first one that fails or runs out of time
ends the run (the parent process itself never opens the GPU).  Writes profiles/train_block_bench.txt (or --out).

    python tools/bench_train_blocks.py [--rounds 7] [--iters 10] [--batches 8,24] [--limit 300] [--out FILE]
"""
import argparse
import copy
import os
import statistics
import subprocess
import sys
import time

import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W = 38, 51
SHAPES = ((1024, 512), (512, 256), (256, 128), (128, 64), (128, 128))
HEAD = (1024, 512, 256, 128, 64)
ORDER = ("convs", "blocks")
WARMUP_S = 0.5   # of alternating steps of both contenders before a case is timed


class Block(nn.Module):
    """A BasicBlock in plain torch modules and ops, launch for launch what a reference-style head runs."""

    def __init__(self, cin, cout):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, cout, kernel_size=3, stride=1, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(cout)
        self.conv2 = nn.Conv2d(cout, cout, kernel_size=3, stride=1, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(cout)
        if cin != cout:
            self.shortcut = nn.Sequential(nn.Conv2d(cin, cout, kernel_size=1, stride=1, bias=False))

    def forward(self, x, relu=True):
        shortcut = self.shortcut(x) if hasattr(self, "shortcut") else x
        out = torch.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        out += shortcut
        if relu:
            out = torch.relu(out)
        return out


def make_step(model, x, go):
    params = list(model.parameters())

    def step():
        for p in params:
            p.grad = None
        model(x).backward(go)
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


def child(N, rounds, iters):
    """One batch size: prints the report lines of every case."""
    from mickey_amd import train_block as tb, train_heads as th
    torch.manual_seed(0)
    print("# N = %d on %s" % (N, torch.cuda.get_device_name(0)))
    cases = [("%d->%d" % s, s) for s in SHAPES] + [("head:" + "-".join(str(c) for c in HEAD), HEAD)]
    for label, widths in cases:
        g = torch.Generator().manual_seed(N)
        x = torch.randn((N, widths[0], H, W), generator=g).cuda()
        go = torch.randn((N, widths[-1], H, W), generator=g).cuda()
        base = nn.Sequential(*[Block(a, b) for a, b in zip(widths[:-1], widths[1:])]).cuda().train()
        models = {"convs": base, "blocks": copy.deepcopy(base)}
        nblk = len(widths) - 1
        assert th.use_hip_convs(models["convs"]) == 2 * nblk
        assert th.use_hip_convs(models["blocks"]) == 2 * nblk and tb.use_hip_blocks(models["blocks"]) == nblk
        steps = {k: make_step(models[k], x, go) for k in ORDER}
        t0 = time.perf_counter()   # warm-up: code objects, the allocator, and the clocks
        while time.perf_counter() - t0 < WARMUP_S:
            for k in ORDER:
                for _ in range(iters):
                    steps[k]()
            torch.cuda.synchronize()
        t = {k: [] for k in ORDER}
        for _ in range(rounds):
            for k in ORDER:
                t[k].append(time_ms(steps[k], iters))
        for m in models.values():
            for p in m.parameters():
                p.grad = None
        mem = {k: peak_mib(steps[k]) for k in ORDER}
        med = {k: statistics.median(v) for k, v in t.items()}
        fmt = {k: "%7.3f [%7.3f .. %7.3f]" % (med[k], min(t[k]), max(t[k])) for k in t}
        print("%-4d %-26s %-28s %-28s %9.1f %9.1f" % (N, label, fmt["convs"], fmt["blocks"], mem["convs"], mem["blocks"]))
        sep = min(t["convs"]) > max(t["blocks"]) or min(t["blocks"]) > max(t["convs"])
        verdict = (("blocks is FASTER" if med["blocks"] < med["convs"] else "blocks is SLOWER") if sep else "no difference beyond the spread")
        print("# N = %d %s: convs / blocks = %.2f (median); the min-max ranges %s: %s"
              % (N, label, med["convs"] / med["blocks"], "do not overlap" if sep else "OVERLAP", verdict), flush=True)
        del models, steps, base, x, go
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batches", default="8,24")
    ap.add_argument("--limit", type=int, default=300, help="seconds each batch size may take")
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_block_bench.txt"))
    args = ap.parse_args()
    if args.child:
        if not torch.cuda.is_available():
            sys.exit("bench_train_blocks: needs a GPU (nothing is measured on the CPU)")
        child(args.child, args.rounds, args.iters)
        return
    from mickey_amd import build as mk_build
    lines = ["# tools/bench_train_blocks.py: forward (training mode) + backward of the heads' BasicBlocks (fp32) into every Parameter",
             "# convs: use_hip_convs alone (BatchNorm / ReLU / add / 1x1 shortcut in torch); blocks: use_hip_convs + use_hip_blocks",
             "# torch %s, kernels %s; images of %d x %d, NCHW input; %d alternating rounds of %d steps, ms per step: median [min .. max]"
             % (torch.__version__, mk_build.source_hash(), H, W, args.rounds, args.iters),
             "# peak MiB: torch.cuda.max_memory_allocated of one step above the inputs and parameters",
             "", "%-4s %-26s %-28s %-28s %9s %9s" % ("N", "block", "convs ms", "blocks ms", "convs MiB", "block MiB")]
    for N in [int(b) for b in args.batches.split(",")]:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(N), "--rounds", str(args.rounds), "--iters", str(args.iters)]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired as e:
            sys.exit("bench_train_blocks: %d images ran past %d s; stopping\n%s" % (N, args.limit, e.stdout or ""))
        print(r.stdout, end="", flush=True)
        if r.returncode != 0:
            sys.exit("bench_train_blocks: %d images ended with status %d; stopping" % (N, r.returncode))
        lines += r.stdout.splitlines()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
