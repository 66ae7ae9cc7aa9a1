#!/usr/bin/env python
"""Forward + backward of the four head tails (mickey_extractor.py:98-124,134-140,172-176,211-216,248-249), fp32, two contenders on
the same GPU:

    torch   the tails as a reference-style model runs them: a bias-free 1x1 nn.Conv2d and the same sequence of small torch ops
            (mean / sub / exp / ones_like + four slice assignments / mul / sum / sum / div; sigmoid; pow / sum / add / pow / div)
    hip     mickey_amd.train_tails: one autograd node per tail

At 8 and at 24 images of 38 x 51 (the two training batch sizes of the reference's configs), features channels_last as the preceding
ReLU leaves them (64 channels, 128 for the descriptors).  One step = forward, then backward from a fixed gradient into the features
and the weight.  `desc+view` adds what the matcher asks of the descriptors, a contiguous [B, C, n] tensor: a copy for torch, a view
for hip.  The contenders are timed alternately, `--rounds` times each (device events around `--iters` steps after half a second of alternating steps of both);
the report gives the median and min / max over the rounds, whether the ranges overlap, and torch.cuda.max_memory_allocated of one
step (above what is allocated before it).  Every batch size runs in a child process of its own under a time limit; the first one
that fails or runs out of time ends the run (the parent process itself never opens the GPU).  Writes profiles/train_tails_bench.txt (or --out).

    python tools/bench_train_tails.py [--rounds 7] [--iters 20] [--batches 8,24] [--limit 240] [--out FILE]
"""
import argparse
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
TAILS = ("score", "offset", "depth", "desc", "desc+view")
ORDER = ("torch", "hip")
WARMUP_S = 0.5   # of alternating steps of both contenders before a tail is timed


class TorchTail(nn.Module):
    """One tail in plain torch ops, launch for launch what a reference-style head runs after resblock4."""

    def __init__(self, kind):
        super().__init__()
        self.kind = kind
        if kind in ("score", "offset", "depth"):
            self.conv = nn.Conv2d(64, 2 if kind == "offset" else 1, kernel_size=1, bias=False)
        self.eps = nn.Parameter(torch.tensor(1e-16), requires_grad=False)

    def borders_off(self, t, b):
        mask = torch.ones_like(t)
        mask[:, :, :b, :] = 0
        mask[:, :, :, :b] = 0
        mask[:, :, t.shape[2] - b:, :] = 0
        mask[:, :, :, t.shape[3] - b:] = 0
        return mask * t

    def forward(self, x):
        if self.kind == "score":
            s = self.conv(x)
            B = s.shape[0]
            s = s - (s.view(B, -1).mean(-1).view(B, 1, 1, 1) + self.eps).detach()
            e = self.borders_off(torch.exp(s / 100), 3)
            return e / (e.sum(-1).sum(-1).view(B, 1, 1, 1) + self.eps)
        if self.kind == "offset":
            return torch.sigmoid(self.conv(x))
        if self.kind == "depth":
            return self.conv(x)
        y = x / x.pow(2).sum(dim=1, keepdim=True).add(1e-10).pow(0.5)
        return y.reshape(y.shape[0], y.shape[1], -1).contiguous() if self.kind == "desc+view" else y


class HipTail(nn.Module):
    def __init__(self, ref):
        super().__init__()
        self.kind = ref.kind
        if hasattr(ref, "conv"):
            self.conv = ref.conv

    def forward(self, x):
        from mickey_amd import train_tails as tt
        if self.kind == "score":
            return tt.score_tail_train(x, self.conv.weight)
        if self.kind == "offset":
            return tt.offset_tail_train(x, self.conv.weight)
        if self.kind == "depth":
            return tt.depth_tail_train(x, self.conv.weight)
        y = tt.desc_l2norm_train(x)
        return y.view(y.shape[0], y.shape[1], -1) if self.kind == "desc+view" else y


def make_step(model, x, go):
    def step():
        x.grad = None
        for p in model.parameters():
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
    """One batch size: prints the report lines of every tail."""
    torch.manual_seed(0)
    print("# N = %d on %s" % (N, torch.cuda.get_device_name(0)))
    for kind in TAILS:
        C = 128 if kind.startswith("desc") else 64
        g = torch.Generator().manual_seed(N)
        x = torch.relu(torch.randn((N, C, H, W), generator=g)).cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
        ref = TorchTail(kind).cuda()
        models = {"torch": ref, "hip": HipTail(ref)}
        with torch.no_grad():
            shape = ref(x).shape
        go = torch.randn(tuple(shape), generator=g).cuda()
        steps = {k: make_step(models[k], x, go) for k in ORDER}
        t0 = time.perf_counter()   # warm-up: code objects, the allocator, and the clocks -- a round is a few ms, far shorter than their ramp
        while time.perf_counter() - t0 < WARMUP_S:
            for k in ORDER:
                for _ in range(iters):
                    steps[k]()
            torch.cuda.synchronize()
        t = {k: [] for k in ORDER}
        for _ in range(rounds):
            for k in ORDER:
                t[k].append(time_ms(steps[k], iters))
        x.grad = None
        for p in ref.parameters():
            p.grad = None
        mem = {k: peak_mib(steps[k]) for k in ORDER}
        med = {k: statistics.median(v) for k, v in t.items()}
        fmt = {k: "%7.3f [%7.3f .. %7.3f]" % (med[k], min(t[k]), max(t[k])) for k in t}
        print("%-4d %-10s %-28s %-28s %9.1f %9.1f" % (N, kind, fmt["torch"], fmt["hip"], mem["torch"], mem["hip"]))
        sep = min(t["torch"]) > max(t["hip"]) or min(t["hip"]) > max(t["torch"])
        verdict = (("hip is FASTER" if med["hip"] < med["torch"] else "hip is SLOWER") if sep else "no difference beyond the spread")
        print("# N = %d %s: torch / hip = %.2f (median); the min-max ranges %s: %s"
              % (N, kind, med["torch"] / med["hip"], "do not overlap" if sep else "OVERLAP", verdict), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batches", default="8,24")
    ap.add_argument("--limit", type=int, default=240, help="seconds each batch size may take")
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_tails_bench.txt"))
    args = ap.parse_args()
    if args.child:
        if not torch.cuda.is_available():
            sys.exit("bench_train_tails: needs a GPU (nothing is measured on the CPU)")
        child(args.child, args.rounds, args.iters)
        return
    from mickey_amd import build as mk_build
    lines = ["# tools/bench_train_tails.py: forward + backward of the head tails (fp32) into the features and the 1x1 weight",
             "# torch: a 1x1 nn.Conv2d and the small torch ops of a reference-style head; hip: mickey_amd.train_tails (one node per tail)",
             "# torch %s, kernels %s; images of %d x %d, channels_last; %d alternating rounds of %d steps, ms per step: median [min .. max]"
             % (torch.__version__, mk_build.source_hash(), H, W, args.rounds, args.iters),
             "# peak MiB: torch.cuda.max_memory_allocated of one step above the inputs and parameters",
             "", "%-4s %-10s %-28s %-28s %9s %9s" % ("N", "tail", "torch ms", "hip ms", "torch MiB", "hip MiB")]
    for N in [int(b) for b in args.batches.split(",")]:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(N), "--rounds", str(args.rounds), "--iters", str(args.iters)]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired as e:
            sys.exit("bench_train_tails: %d images ran past %d s; stopping\n%s" % (N, args.limit, e.stdout or ""))
        print(r.stdout, end="", flush=True)
        if r.returncode != 0:
            sys.exit("bench_train_tails: %d images ended with status %d; stopping" % (N, r.returncode))
        lines += r.stdout.splitlines()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
