#!/usr/bin/env python
"""The tail of a training step (reference model.py:104-145) over the trainable parameters of the default model -- the four heads of
mickey_amd/configs/mickey_default.yaml and the dustbin score, fp32 -- five contenders on the same GPU, each on its own copy:

    torch          what the trainer does today: five isnan / isinf `.any()` checks read by the host (on stand-ins of probs_grad[0]
                   and the keypoint / depth gradients), clip_grad_norm_(5), the per-parameter isnan scan with its `if`, and
                   torch.optim.Adam(eps=1e-6).step() in torch's default (foreach) form
    torch-bare     the same without the five checks and without the scan: clip_grad_norm_ and step() only (no host synchronisation)
    fused          as torch, with torch.optim.Adam(fused=True): the strongest torch baseline
    fused-bare     as torch-bare, with fused=True
    hip            HipAdam.step_guarded(max_norm=5, also_finite=the stand-ins): three launches, no host synchronisation

The gradients are fixed and their norm lies below max_norm (no contender rewrites them; torch multiplies them by 1 all the same).
The contenders are timed alternately, `--rounds` times each: a round is `--iters` steps with ONE device synchronisation at its end;
wall = the host clock around the round including that synchronisation, device = HIP events around the same steps, both per step,
as median [min .. max] over the rounds.  Then mk_optim_adam alone: `--iters` launches back to back on the table of the last step,
HIP events around them, against the 28 bytes per parameter it must move (p, g, m, v read; p, m, v written).  The measurement runs
in a child process under a time limit (the parent never opens the GPU).  Writes profiles/train_optim_bench.txt (or --out).

    python tools/bench_train_optim.py [--rounds 7] [--iters 20] [--images 8] [--limit 300] [--out FILE]
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ORDER = ("torch", "torch-bare", "fused", "fused-bare", "hip")
WARMUP_S = 0.5
MAX_NORM = 5.0
NOT_TRAINED = ("running_mean", "running_var", "num_batches_tracked", ".eps", "offset_par1", "offset_par2", "ones_kernel")


def parameter_shapes():
    """the shapes of every trainable tensor of the four default heads (mickey_extractor.py:67-251) and the dustbin score"""
    from mickey_amd import synthetic
    from mickey_amd.config import default_cfg
    sd = synthetic.heads_state_dict(default_cfg())
    shapes = [tuple(v.shape) for k, v in sd.items() if not k.endswith(NOT_TRAINED)]
    return shapes + [()]


def make_step(kind, params, watched):
    if kind == "hip":
        from mickey_amd.train_optim import HipAdam
        opt = HipAdam(params, lr=1e-4, eps=1e-6)
        return opt, lambda: opt.step_guarded(max_norm=MAX_NORM, also_finite=watched)
    opt = torch.optim.Adam(params, lr=1e-4, eps=1e-6, fused=True if kind.startswith("fused") else None)
    bare = kind.endswith("bare")

    def step():
        if not bare:   # model.py:104-116
            invalid = [torch.isnan(watched[0]).any()] + [torch.isnan(t).any() or torch.isinf(t).any() for t in watched[1:]]
            if any(bool(i) for i in invalid):
                return False
        torch.nn.utils.clip_grad_norm_(params, max_norm=MAX_NORM)
        if not bare:   # model.py:140-143
            nans = sum([torch.isnan(p.grad).any() for p in params if p.grad is not None])
            if nans != 0:
                return False
        opt.step()
        return True
    return opt, step


def time_round(step, iters):
    """-> (wall ms per step, device ms per step): one synchronisation, at the end"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    for _ in range(iters):
        step()
    b.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3 / iters
    return wall, a.elapsed_time(b) / iters


def child(images, rounds, iters):
    dev = torch.device("cuda")
    shapes = parameter_shapes()
    count = sum(int(torch.Size(s).numel()) for s in shapes)
    print("# %s: %d trainable tensors, %d elements (%.1f MB per fp32 copy); stand-ins for %d images of 38 x 51"
          % (torch.cuda.get_device_name(0), len(shapes), count, count * 4 / 1e6, images))
    g = torch.Generator().manual_seed(0)
    base = [torch.randn(s, generator=g) * 0.02 for s in shapes]
    grads = [torch.randn(s, generator=g) for s in shapes]
    scale = 0.5 * MAX_NORM / float(torch.sqrt(sum(t.double().pow(2).sum() for t in grads)))
    n = 38 * 51
    watched = tuple(torch.randn(s, generator=g).to(dev) for s in ((images, n, n), (images, 2, n), (images, 2, n), (images, 1, n), (images, 1, n)))
    steps, opts = {}, {}
    for kind in ORDER:
        params = [torch.nn.Parameter(t.to(dev)) for t in base]
        for p, gr in zip(params, grads):
            p.grad = (gr * scale).to(dev)
        opts[kind], steps[kind] = make_step(kind, params, watched)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < WARMUP_S:
        for kind in ORDER:
            for _ in range(iters):
                steps[kind]()
        torch.cuda.synchronize()
    status = steps["hip"]()
    print("# gradient norm %.4f (max_norm %g: not clipped), hip status ok = %d" % (float(status[1]), MAX_NORM, int(status[0])))
    wall, devt = {k: [] for k in ORDER}, {k: [] for k in ORDER}
    for _ in range(rounds):
        for kind in ORDER:
            w, d = time_round(steps[kind], iters)
            wall[kind].append(w)
            devt[kind].append(d)
    fmt = lambda v: "%7.3f [%7.3f .. %7.3f]" % (statistics.median(v), min(v), max(v))
    print("%-11s %-28s %-28s" % ("contender", "wall ms per step", "device ms per step"))
    for kind in ORDER:
        print("%-11s %-28s %-28s" % (kind, fmt(wall[kind]), fmt(devt[kind])))
    med = {k: statistics.median(v) for k, v in wall.items()}
    for other in ("torch", "fused", "fused-bare"):
        sep = min(wall[other]) > max(wall["hip"]) or min(wall["hip"]) > max(wall[other])
        verdict = (("hip is FASTER" if med["hip"] < med[other] else "hip LOSES") if sep else "no difference beyond the spread")
        print("# wall, %s / hip = %.2f (median); the min-max ranges %s: %s"
              % (other, med[other] / med["hip"], "do not overlap" if sep else "OVERLAP", verdict))
    for full, bare in (("torch", "torch-bare"), ("fused", "fused-bare")):
        print("# the host synchronisations of %s (five checks + the scan): %.3f ms of wall time per step (%s - %s, medians)"
              % (full, med[full] - med[bare], full, bare))
    # mk_optim_adam alone, on the table of the step above
    from mickey_amd import _native
    opt = opts["hip"]
    opt.step()
    table, cmap, go = opt._table[1], opt._map[1], opt._go
    chunks = sum(-(-int(torch.Size(s).numel()) // _native.query("mk_optim_chunk_elems")) for s in shapes)
    launch = lambda: _native.call("mk_optim_adam", table.data_ptr(), len(shapes), cmap.data_ptr(), chunks, go.data_ptr(), _native.stream())
    t = [time_round(launch, iters)[1] for _ in range(rounds)]
    rate = lambda ms: 28.0 * count / (ms * 1e-3) / 1e12
    print("# mk_optim_adam alone, %d workgroups, %d launches back to back: %s ms per launch = %.2f TB/s [%.2f .. %.2f] of the %.2f GB it must move"
          % (chunks, iters, fmt(t), rate(statistics.median(t)), rate(max(t)), rate(min(t)), 28.0 * count / 1e9), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--limit", type=int, default=300, help="seconds the measurement may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_optim_bench.txt"))
    args = ap.parse_args()
    if args.child:
        if not torch.cuda.is_available():
            sys.exit("bench_train_optim: needs a GPU (nothing is measured on the CPU)")
        child(args.images, args.rounds, args.iters)
        return
    from mickey_amd import build as mk_build
    lines = ["# tools/bench_train_optim.py: the tail of a training step (finite checks, clip_grad_norm_, NaN scan, Adam) over the default model's trainable parameters, fp32",
             "# torch / fused: the reference trainer's sequence with torch.optim.Adam (default / fused=True); -bare: without its host checks; hip: HipAdam.step_guarded",
             "# torch %s, kernels %s; %d alternating rounds of %d steps, one synchronisation per round, ms per step: median [min .. max]"
             % (torch.__version__, mk_build.source_hash(), args.rounds, args.iters), ""]
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--rounds", str(args.rounds), "--iters", str(args.iters),
           "--images", str(args.images)]
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=args.limit)
    except subprocess.TimeoutExpired as e:
        sys.exit("bench_train_optim: ran past %d s; stopping\n%s" % (args.limit, e.stdout or ""))
    print(r.stdout, end="", flush=True)
    if r.returncode != 0:
        sys.exit("bench_train_optim: the measurement ended with status %d\n%s" % (r.returncode, r.stderr))
    lines += r.stdout.splitlines()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
