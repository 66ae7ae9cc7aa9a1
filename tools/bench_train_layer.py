#!/usr/bin/env python
"""Forward + backward of one EncoderLayer of the heads' transformer (att_layers/transformer_utils.py:40-66), self attention, fp32,
three contenders on the same GPU:

    torch       a stand-in layer with the reference's structure in plain torch (its attention is linear_attention_formula)
    hip-attn    the same layer after use_hip_attention: the attention core on the HIP kernels, the Linears / LayerNorms / concat /
                ReLU / residual in torch -- what the project had before train_layer, the baseline that counts
    hip-layer   train_layer.HipEncoderLayer (use_hip_encoder_layers): the whole layer as one autograd node

At 8 and at 24 images of 38 x 51 = 1938 tokens (the two training batch sizes of the reference's configs).  One step = forward, then
backward from a fixed gradient into x and all ten parameters.  The contenders are timed alternately, A/B/C/A/B/C, `--rounds` times
each (device events around `--iters` steps after a warm-up of all); the report gives the median and min / max over the rounds,
whether the ranges overlap, and torch.cuda.max_memory_allocated of one step of each (above what is allocated before it).  Writes
profiles/train_layer_bench.txt (or --out).

    python tools/bench_train_layer.py [--rounds 7] [--iters 20] [--batches 8,24] [--out FILE]
    python tools/bench_train_layer.py --trace-steps 5 [--batches 8]     a few hip-layer steps and nothing else (for a kernel trace)
"""
import argparse
import copy
import os
import statistics
import sys

import torch
import torch.nn.functional as F
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L = 38 * 51
ORDER = ("torch", "hip-attn", "hip-layer")


class Att(nn.Module):
    def __init__(self):
        super().__init__()
        self.feature_map = lambda t: F.elu(t) + 1
        self.eps = 1e-6
        self.attention = "linear"

    def forward(self, q, k, v):
        from mickey_amd.train_attention import linear_attention_formula
        return linear_attention_formula(q, k, v, self.eps)


class Layer(nn.Module):
    def __init__(self, d=128, nhead=8):
        super().__init__()
        self.dim, self.nhead = d // nhead, nhead
        self.q_proj = nn.Linear(d, d, bias=False)
        self.k_proj = nn.Linear(d, d, bias=False)
        self.v_proj = nn.Linear(d, d, bias=False)
        self.attention = Att()
        self.merge = nn.Linear(d, d, bias=False)
        self.mlp = nn.Sequential(nn.Linear(2 * d, 2 * d, bias=False), nn.ReLU(True), nn.Linear(2 * d, d, bias=False))
        self.norm1 = nn.LayerNorm(d)
        self.norm2 = nn.LayerNorm(d)

    def forward(self, x, source):
        N, T, C = x.shape
        q = self.q_proj(x).view(N, T, self.nhead, self.dim)
        k = self.k_proj(source).view(N, -1, self.nhead, self.dim)
        v = self.v_proj(source).view(N, -1, self.nhead, self.dim)
        m = self.norm1(self.merge(self.attention(q, k, v).reshape(N, T, C)))
        return x + self.norm2(self.mlp(torch.cat([x, m], dim=2)))


def make_step(model, x, go):
    layer = model[0]

    def step():
        x.grad = None
        for p in layer.parameters():
            p.grad = None
        layer(x, x).backward(go)
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


def contenders():
    from mickey_amd.train_attention import use_hip_attention
    from mickey_amd.train_layer import use_hip_encoder_layers
    torch.manual_seed(0)
    base = nn.Sequential(Layer()).cuda()
    models = {k: copy.deepcopy(base) for k in ORDER}
    assert use_hip_attention(models["hip-attn"]) == 1
    assert use_hip_encoder_layers(models["hip-layer"]) == 1
    return models


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batches", default="8,24")
    ap.add_argument("--trace-steps", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_layer_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_train_layer: needs a GPU (nothing is measured on the CPU)")
    from mickey_amd import build as mk_build
    models = contenders()
    batches = [int(b) for b in args.batches.split(",")]
    if args.trace_steps:
        g = torch.Generator().manual_seed(batches[0])
        x = torch.randn((batches[0], L, 128), generator=g).cuda().requires_grad_(True)
        go = torch.randn((batches[0], L, 128), generator=g).cuda()
        step = make_step(models["hip-layer"], x, go)
        for _ in range(args.trace_steps):
            step()
        torch.cuda.synchronize()
        print("ran %d hip-layer steps at %d images" % (args.trace_steps, batches[0]))
        return
    lines = ["# tools/bench_train_layer.py: forward + backward of one EncoderLayer (self attention, fp32) into x and all ten parameters",
             "# torch: plain torch; hip-attn: use_hip_attention only (the baseline that counts); hip-layer: train_layer.HipEncoderLayer",
             "# %s, torch %s, kernels %s; %d tokens per image; %d alternating rounds of %d steps, ms per step: median [min .. max]"
             % (torch.cuda.get_device_name(0), torch.__version__, mk_build.source_hash(), L, args.rounds, args.iters),
             "# peak MiB: torch.cuda.max_memory_allocated of one step above the inputs and parameters",
             "", "%-4s %-30s %-30s %-30s %9s %9s %9s" % (("N",) + tuple(k + " ms" for k in ORDER) + tuple(k + " MiB" for k in ORDER))]
    for N in batches:
        g = torch.Generator().manual_seed(N)
        x = torch.randn((N, L, 128), generator=g).cuda().requires_grad_(True)
        go = torch.randn((N, L, 128), generator=g).cuda()
        steps = {k: make_step(models[k], x, go) for k in ORDER}
        for k in ORDER:   # warm-up: code objects, the vendor library's algorithm search
            for _ in range(5):
                steps[k]()
        torch.cuda.synchronize()
        t = {k: [] for k in ORDER}
        for _ in range(args.rounds):
            for k in ORDER:
                t[k].append(time_ms(steps[k], args.iters))
        x.grad = None
        for m in models.values():
            for p in m.parameters():
                p.grad = None
        mem = {k: peak_mib(steps[k]) for k in ORDER}
        med = {k: statistics.median(v) for k, v in t.items()}
        fmt = {k: "%8.3f [%8.3f .. %8.3f]" % (med[k], min(t[k]), max(t[k])) for k in t}
        lines.append("%-4d %-30s %-30s %-30s %9.1f %9.1f %9.1f" % ((N,) + tuple(fmt[k] for k in ORDER) + tuple(mem[k] for k in ORDER)))
        for other in ("hip-attn", "torch"):
            sep = min(t[other]) > max(t["hip-layer"]) or min(t["hip-layer"]) > max(t[other])
            verdict = (("hip-layer is FASTER" if med["hip-layer"] < med[other] else "hip-layer is NOT faster") if sep
                       else "no difference beyond the spread")
            lines.append("# N = %d: %s / hip-layer = %.2f (median); the min-max ranges of the two %s: %s"
                         % (N, other, med[other] / med["hip-layer"], "do not overlap" if sep else "OVERLAP", verdict))
        print("\n".join(lines[-3:]), flush=True)
        del x, go, steps
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
