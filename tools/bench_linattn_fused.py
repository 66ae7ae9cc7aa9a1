"""Layer-level A/B of the heads' linear attention: the separate launches against the fused kernels, one layer at the benchmark
geometry (G = 4, nimg = 64, 51 x 38 tokens, C = 128), interleaved in one process, medians of event timings.

    python tools/bench_linattn_fused.py [--dtype fp16|bf16] [--iters 30] [--nimg 64]

  old        gemm_grouped (q | k | v, fp32) -> linattn_kv -> linattn_apply -> gemm_ln128 (merge -> norm1)
  new        linattn_kv_fused -> linattn_apply_fused (with merge -> norm1)
  new-msg    linattn_kv_fused -> linattn_apply_fused (msg only) -> gemm_ln128        (the simpler form of the second fusion)
Each fusion is also set against what it replaces on its own, the one qkv GEMM counted 2/3 (k | v) under the first and 1/3 (q) under
the second.  All three sequences must give the same bits (asserted).  Prints one JSON line; the exit status is 1 when the new sequence is not at
least twice as fast as the old one."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mickey_amd import ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="fp16", choices=["fp16", "bf16"])
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--nimg", type=int, default=64)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    dtype = torch.float16 if args.dtype == "fp16" else torch.bfloat16
    G, nimg, gh, gw, C = 4, args.nimg, 51, 38, 128
    L = gh * gw
    M = nimg * L
    gen = torch.Generator(device="cuda").manual_seed(1)
    rn = lambda *shape, s=1.0: torch.randn(shape, device=dev, generator=gen) * s  # noqa: E731
    cat_a = rn(G, M, 2 * C).to(dtype)
    cat_b = cat_a.clone()
    cat_c = cat_a.clone()
    qkv_w = rn(G, 3 * C, C, s=2.0 / math.sqrt(C)).to(dtype)
    merge_w = rn(G, C, C, s=1.5 / math.sqrt(C)).to(dtype)
    lw, lb = 1.0 + 0.3 * rn(G, C), 0.2 * rn(G, C)
    qkv = torch.empty((G, M, 3 * C), device=dev, dtype=torch.float32)
    kv_a, kv_b = (torch.empty((G * nimg * (C // 16), 272), device=dev) for _ in range(2))
    work_a, work_b = (torch.empty((ops.linattn_work_floats(G, nimg, L, C),), device=dev) for _ in range(2))
    msg_a = torch.empty((G, M, C), device=dev, dtype=dtype)
    msg_c = torch.empty((G, M, C), device=dev, dtype=dtype)

    def old_gemm():
        ops.gemm_grouped(cat_a, qkv_w, None, qkv, G, M, 3 * C, C, 2 * C, C, 3 * C, M * 2 * C, 3 * C * C, 0, M * 3 * C)

    def old_kv():
        ops.linattn_kv(qkv, kv_a, work_a, G, nimg, L, C)

    def old_apply():
        ops.linattn_apply(qkv, kv_a, msg_a, C, G, nimg, L, C)

    def old_merge():
        ops.gemm_ln128(msg_a, merge_w, lw, lb, 1e-5, cat_a[:, :, C:], G, M, C, ldo=2 * C)

    def new_kv():
        ops.linattn_kv_fused(cat_b, qkv_w, kv_b, work_b, G, nimg, L, C)

    def new_apply():
        ops.linattn_apply_fused(cat_b, qkv_w, kv_b, cat_b[:, :, C:], G, nimg, L, C, merge_w=merge_w, ln_w=lw, ln_b=lb)

    def new_apply_msg():
        ops.linattn_apply_fused(cat_c, qkv_w, kv_b, msg_c, G, nimg, L, C)

    def new_merge():
        ops.gemm_ln128(msg_c, merge_w, lw, lb, 1e-5, cat_c[:, :, C:], G, M, C, ldo=2 * C)

    steps = [("old_gemm", old_gemm), ("old_kv", old_kv), ("old_apply", old_apply), ("old_merge", old_merge),
             ("new_kv", new_kv), ("new_apply", new_apply), ("new_apply_msg", new_apply_msg), ("new_merge", new_merge)]
    times = {n: [] for n, _ in steps}
    for it in range(args.iters + 3):   # the sequences alternate launch by launch group: same clocks, same thermal state
        evs = []
        for n, f in steps:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            evs.append((n, e0, e1))
        torch.cuda.synchronize()
        if it >= 3:
            for n, e0, e1 in evs:
                times[n].append(e0.elapsed_time(e1) * 1e3)
    assert torch.equal(kv_a, kv_b) and torch.equal(cat_a, cat_b) and torch.equal(cat_a, cat_c) and torch.equal(msg_a, msg_c)
    med = {n: statistics.median(v) for n, v in times.items()}
    old = med["old_gemm"] + med["old_kv"] + med["old_apply"] + med["old_merge"]
    new = med["new_kv"] + med["new_apply"]
    new_msg = med["new_kv"] + med["new_apply_msg"] + med["new_merge"]
    res = {"device": torch.cuda.get_device_name(0), "dtype": args.dtype, "G": G, "nimg": nimg, "L": L, "iters": args.iters,
           "median_us": {k: round(v, 1) for k, v in med.items()},
           "old_us": round(old, 1), "new_us": round(new, 1), "new_msg_form_us": round(new_msg, 1),
           "speedup": round(old / new, 2), "speedup_msg_form": round(old / new_msg, 2),
           "kv_fusion": {"old_us": round(med["old_gemm"] * 2 / 3 + med["old_kv"], 1), "new_us": round(med["new_kv"], 1)},
           "apply_fusion": {"old_us": round(med["old_gemm"] / 3 + med["old_apply"] + med["old_merge"], 1), "new_us": round(med["new_apply"], 1),
                            "new_msg_form_us": round(med["new_apply_msg"] + med["new_merge"], 1)},
           "bit_identical": True}
    print(json.dumps(res))
    return 0 if old >= 2.0 * new else 1


if __name__ == "__main__":
    sys.exit(main())
