"""Training matcher alone: forward + backward of final_scores = dualSoftmax(dsc0, dsc1) * (scr0^T scr1) at the reference's training
batch (8 pairs, n = 1938, curriculum_learning.yaml:37), HIP (mickey_amd.train_matcher, split-fp16 and exact fp32 correlation)
against torch fp32 autograd of the same formula in the same process.  HIP-event medians after warm-up, peak memory of each step
(torch.cuda.max_memory_allocated above what was allocated before it), and the shares of the governing roofs derived from the shapes.

    python tools/bench_matcher_grad.py [B] [n]
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mickey_amd.train_matcher import dual_softmax_train  # noqa: E402

F32_MATRIX_PEAK = 157e12     # v_mfma_f32_32x32x2_f32, MI355X
F16_MATRIX_PEAK = 2.5e15     # 16-bit matrix cores (dense)
HBM_BW = 6.0e12              # what HBM sustains for streaming access (6.1-6.9 TB/s measured)


def timed(fn, reps=10, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return sorted(ts)[len(ts) // 2]


def peak_bytes(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def torch_final(d0, d1, s0, s1, dustbin, temperature):
    """the reference's formula as the reference writes it (feature_matcher.py:64-83, compute_correspondences.py:46-50)"""
    S = torch.matmul(d0.transpose(1, 2).contiguous(), d1) / temperature
    B, m, n = S.shape
    Z = torch.cat([torch.cat([S, dustbin.expand(B, m, 1)], -1), torch.cat([dustbin.expand(B, 1, n), dustbin.expand(B, 1, 1)], -1)], 1)
    P = (torch.softmax(Z, 1) * torch.softmax(Z, 2))[:, :-1, :-1]
    return P * torch.matmul(s0.transpose(2, 1).contiguous(), s1)


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 1938
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    d0 = torch.nn.functional.normalize(torch.randn((B, 128, n), generator=g), dim=1).to(dev).requires_grad_()
    d1 = torch.nn.functional.normalize(torch.randn((B, 128, n), generator=g), dim=1).to(dev).requires_grad_()
    s0 = torch.softmax(torch.randn((B, 1, n), generator=g), -1).to(dev).requires_grad_()
    s1 = torch.softmax(torch.randn((B, 1, n), generator=g), -1).to(dev).requires_grad_()
    db = torch.nn.Parameter(torch.tensor(1.0, device=dev))
    G = torch.randn((B, n, n), generator=g).to(dev)
    params = (d0, d1, s0, s1, db)

    def step(make):
        for p in params:
            p.grad = None
        make().backward(G)

    runs = {"hip_split": lambda: dual_softmax_train(d0, d1, s0, s1, 0.1, db, split=True),
            "hip_exact": lambda: dual_softmax_train(d0, d1, s0, s1, 0.1, db, split=False),
            "torch_fp32_autograd": lambda: torch_final(d0, d1, s0, s1, db, 0.1)}
    res = {}
    for name, make in runs.items():
        fwd = timed(lambda: make().detach())
        t = timed(lambda: step(make))
        mem = peak_bytes(lambda: step(make))
        res[name] = {"fwd_ms": round(fwd, 3), "fwd_bwd_ms": round(t, 3), "peak_mib": round(mem / 2 ** 20, 1)}
    # shares of the roofs: one correlation = 2 C n0 n1 FLOP per pair; HIP forward 2 (split: statistics + outputs) or 1 (exact: stored
    # and re-read) correlations, backward 3 correlations + 2 gradient GEMMs of the same size on the fp32 matrix cores; the split
    # correlation is 3 16-bit MFMA passes (lo.hi + hi.lo + hi.hi).  Bytes: G read three times (sweep 1 and both sweep-2 kernels),
    # final_scores written once, the sweep-2 partials written and read once (4 chunks x C x n per side).
    corr = 2.0 * 128 * n * n * B
    mb = 4.0 * B * n * n
    parts = 2 * 2 * 4.0 * B * 4 * 128 * n
    bytes_ = 3 * mb + mb + parts
    t_mem = bytes_ / HBM_BW
    roofs = {"hip_split": max(5 * 3 * corr / F16_MATRIX_PEAK + 2 * corr / F32_MATRIX_PEAK, t_mem),
             "hip_exact": max(6 * corr / F32_MATRIX_PEAK, t_mem)}
    for k, r in roofs.items():
        res[k]["roof_ms"] = round(r * 1e3, 3)
        res[k]["share_of_roof"] = round(r * 1e3 / res[k]["fwd_bwd_ms"], 3)
    tt = res["torch_fp32_autograd"]
    for k in ("hip_split", "hip_exact"):
        res[k]["speedup_vs_torch"] = round(tt["fwd_bwd_ms"] / res[k]["fwd_bwd_ms"], 2)
        res[k]["memory_vs_torch"] = round(res[k]["peak_mib"] / tt["peak_mib"], 3)
    line = {"what": "dual-softmax fwd+bwd", "B": B, "n": n, "C": 128, "gflop_per_correlation_per_pair": round(corr / B / 1e9, 3),
            "G_mb_per_pair_per_read": round(mb / B / 1e6, 1), "hbm_bytes_hip_gb": round(bytes_ / 1e9, 3), **res}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
