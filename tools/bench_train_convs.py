#!/usr/bin/env python
"""Forward + backward of the heads' trainable 3x3 convolutions: train_heads.Conv3x3 against nn.Conv2d in fp32, on the same GPU.

The eight distinct 3x3 shapes of the default configuration (resblock1-4 of a head, mickey_extractor.py:67-251) plus the descriptor
head's 128 -> 128 twice more, at 8 and at 24 images of 38 x 51 (the two training batch sizes of the reference's configs).  Per shape
one step = forward, then backward from a fixed gradient: weight gradient always, input gradient except for 1024 -> 512, whose
input is the frozen encoder's feature map.  The two implementations are timed alternately, A/B/A/B, `--rounds` times each (device
events around `--iters` steps after a warm-up of both); per shape and in total the report gives the median and min / max over the
rounds.  Writes profiles/train_conv_bench.txt (or --out).

    python tools/bench_train_convs.py [--rounds 5] [--iters 10] [--batches 8,24] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (Cin, Cout, how often a head stack runs it, input requires grad)
SHAPES = [(1024, 512, 1, False), (512, 512, 1, True), (512, 256, 1, True), (256, 256, 1, True), (256, 128, 1, True),
          (128, 128, 3, True), (128, 64, 1, True), (64, 64, 1, True)]
H, W = 38, 51


def flops(cin, cout, B, x_grad):
    return 2.0 * B * H * W * 9 * cin * cout * (3 if x_grad else 2)


def make_step(conv, x, gy):
    def step():
        conv.weight.grad = None
        if x.requires_grad:
            x.grad = None
        conv(x).backward(gy)
    return step


def time_ms(step, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        step()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batches", default="8,24")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_conv_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_train_convs: needs a GPU (nothing is measured on the CPU)")
    from mickey_amd import build as mk_build
    from mickey_amd.train_heads import Conv3x3
    lines = ["# tools/bench_train_convs.py: forward + backward of the heads' 3x3 convs, train_heads.Conv3x3 (hip) vs nn.Conv2d fp32 (torch)",
             "# %s, torch %s, kernels %s; %d alternating rounds of %d steps, ms per step: median [min .. max]"
             % (torch.cuda.get_device_name(0), torch.__version__, mk_build.source_hash(), args.rounds, args.iters)]
    for B in [int(b) for b in args.batches.split(",")]:
        lines.append("")
        lines.append("## %d images of %d x %d" % (B, H, W))
        lines.append("%-12s %2s %5s  %-28s %-28s %7s %9s" % ("shape", "x", "dgrad", "hip ms", "torch ms", "t/h", "hip TF/s"))
        tot = {"hip": [0.0] * args.rounds, "torch": [0.0] * args.rounds}
        for cin, cout, count, x_grad in SHAPES:
            g = torch.Generator().manual_seed(cin + cout)
            x = torch.randn((B, cin, H, W), generator=g).cuda().requires_grad_(x_grad)
            gy = torch.randn((B, cout, H, W), generator=g).cuda()
            ref = nn.Conv2d(cin, cout, 3, padding=1, bias=False).cuda()
            hip = Conv3x3(cin, cout).cuda()
            with torch.no_grad():
                hip.weight.copy_(ref.weight)
            steps = {"hip": make_step(hip, x, gy), "torch": make_step(ref, x, gy)}
            for k in ("hip", "torch"):   # warm-up: code objects, the vendor library's algorithm search
                for _ in range(3):
                    steps[k]()
            torch.cuda.synchronize()
            t = {"hip": [], "torch": []}
            for _ in range(args.rounds):
                for k in ("hip", "torch"):
                    t[k].append(time_ms(steps[k], args.iters))
            for k in t:
                for r in range(args.rounds):
                    tot[k][r] += count * t[k][r]
            med = {k: statistics.median(v) for k, v in t.items()}
            fmt = {k: "%8.3f [%8.3f .. %8.3f]" % (med[k], min(t[k]), max(t[k])) for k in t}
            lines.append("%4d->%-6d %2d %5s  %-28s %-28s %7.2f %9.1f" % (cin, cout, count, "yes" if x_grad else "no", fmt["hip"], fmt["torch"],
                                                                   med["torch"] / med["hip"], flops(cin, cout, B, x_grad) / med["hip"] * 1e-9))
            print(lines[-1], flush=True)
            del x, gy, ref, hip, steps
            torch.cuda.empty_cache()
        med = {k: statistics.median(v) for k, v in tot.items()}
        lines.append("%-12s %2s %5s  %-28s %-28s %7.2f" % ("total", "", "", "%8.3f [%8.3f .. %8.3f]" % (med["hip"], min(tot["hip"]), max(tot["hip"])),
                                                    "%8.3f [%8.3f .. %8.3f]" % (med["torch"], min(tot["torch"]), max(tot["torch"])),
                                                    med["torch"] / med["hip"]))
        sep = min(tot["torch"]) > max(tot["hip"]) or min(tot["hip"]) > max(tot["torch"])
        lines.append("# total: torch / hip = %.2f (median); the min-max ranges of the two %s"
                     % (med["torch"] / med["hip"], "do not overlap" if sep else "OVERLAP: no difference beyond the spread"))
        print("\n".join(lines[-2:]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
