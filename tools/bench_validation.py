#!/usr/bin/env python
"""The validation tail of the trainer (reference lib/models/MicKey/model.py:66-89, 205-280) after the loss, two contenders on the same
GPU and the same inputs:

    torch      the metrics and the summary as the trainer computes them, restated in plain torch / numpy from the formulas:
               pose_error_torch and vcre_torch step by step (lib/utils/metrics.py:12-53, 83-125: the eye grid uploaded per call, 4 x 4
               homogeneous matrices, torch.linalg.inv), the records kept as a list of per-step tensors, and at the end of the epoch
               torch.stack, a copy to the host and a sort-based average precision in numpy, three times (benchmarks/utils.py:138-188)
    hip        pose_metrics into a ValidationAccumulator (one launch per step) and summary() (two launches, one read-back)

Both use HipProcrustesSolver for the poses: the reference's torch solver (probabilisticProcrustes.py:183-348) is not restated here, so
the figures show the metric and summary part only, on top of the same solver time.  Two measurements:

    tail       one validation step of `--pairs` pairs on the planted problem of mickey_amd.synthetic (n = 51 x 38 = 1938): solver,
               metrics, and ONE summary over the records so far, per step
    summary    the summary alone over N = `--records` random records

The contenders are timed alternately, `--rounds` times each: a round is `--iters` repetitions with one device synchronisation at its
end (the torch contender's summary synchronises by itself); wall ms per repetition as median [min .. max].  The measurement runs in a
child process under a time limit (the parent never opens the GPU).  Writes profiles/validation_bench.txt (or --out).

    python tools/bench_validation.py [--rounds 7] [--iters 10] [--pairs 8] [--records 32768] [--limit 300] [--out FILE]
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ORDER = ("torch", "hip")
WARMUP_S = 0.5
THRESHOLDS = (0.25, 5, 0.5, 10, 90)


def eye_grid_host():
    x = (np.arange(7) - 3.0) * 0.3
    y = (np.arange(4) - 1.5) * 0.3
    z = np.arange(7) * 0.3 + 1.8
    xx, yy, zz = np.meshgrid(x, y, z)
    return np.stack([xx.reshape(-1), yy.reshape(-1), zz.reshape(-1), np.ones(196)], -1)


EYE = eye_grid_host()


def torch_metrics(R, t, T, K, W=540, H=720):
    """the launches of pose_error_torch + vcre_torch, from their formulas"""
    B = R.shape[0]
    Rgt, tgt = T[:, :3, :3], T[:, :3, 3:].transpose(1, 2)
    st, sg = torch.linalg.norm(t, dim=-1), torch.linalg.norm(tgt, dim=-1)
    cos = torch.clip((t @ tgt.transpose(1, 2)).squeeze(-1) / (st * sg + 1e-9), -1.0, 1.0)
    ang = torch.rad2deg(torch.acos(cos))
    ang = torch.minimum(ang, 180 - ang)
    euc = torch.linalg.norm(t - tgt, dim=-1)
    trace = torch.diagonal(R.transpose(1, 2) @ Rgt, dim1=-2, dim2=-1).sum(-1)
    r_err = torch.rad2deg(torch.acos(torch.clip((trace - 1) / 2, -1.0, 1.0)))
    eye = torch.tile(torch.from_numpy(EYE).unsqueeze(0).to(R.device).float(), [B, 1, 1])

    def proj(P):
        q = (K @ P.transpose(2, 1)).transpose(2, 1)
        return q[:, :, :2] / (q[:, :, 2:] + 1e-16)

    uv_gt = proj(eye[:, :, :3])
    est = torch.tile(torch.eye(4).view(1, 4, 4), [B, 1, 1]).to(R.device).float()
    est[:, :3, :3], est[:, :3, -1] = R, t[:, 0]
    gt = torch.tile(torch.eye(4).view(1, 4, 4), [B, 1, 1]).to(R.device).float()
    gt[:, :3, :3], gt[:, :3, -1] = Rgt, tgt[:, 0]
    uv = proj((torch.linalg.inv(gt) @ est @ eye.transpose(2, 1)).transpose(2, 1)[:, :, :3])
    hi = torch.tensor([float(W), float(H)], device=R.device)
    d = torch.minimum(torch.clip(uv_gt, min=0), hi) - torch.minimum(torch.clip(uv, min=0), hi)
    vcre = (((d ** 2.0).sum(-1) + 1e-6) ** 0.5).mean(-1).view(B, 1)
    return ang, euc, r_err, vcre


def host_ap(conf, tp):
    """sort by confidence, one (precision, recall) point per group of ties, recall-weighted sum of precisions"""
    order = np.argsort(conf)[::-1]
    conf, tp = conf[order], tp[order]
    idx = np.r_[np.where(np.diff(conf))[0], conf.size - 1]
    prec = np.cumsum(tp)[idx] / (idx + 1.0)
    rec = (idx + 1.0) / conf.size
    return float(np.sum(np.diff(np.r_[0.0, rec]) * prec))


def torch_summary(steps):
    """on_validation_epoch_end over [(ang, euc, r_err, vcre, inliers)] per step"""
    ang, euc, r_err, vcre, inl = (torch.cat([s[k].reshape(-1) for s in steps]) for k in range(5))
    means = torch.stack([v.mean() for v in (ang, euc, r_err, vcre)])
    conf = inl.detach().cpu().numpy()
    out = []
    for acc in ((euc < THRESHOLDS[0]) * (r_err < THRESHOLDS[1]), (euc < THRESHOLDS[2]) * (r_err < THRESHOLDS[3]), vcre < THRESHOLDS[4]):
        out += [float(acc.sum() / len(acc)), host_ap(conf, acc.detach().cpu().numpy())]
    return means.tolist() + out


def time_round(fn, iters):
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def alternate(fns, rounds, iters):
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < WARMUP_S:
        for kind in ORDER:
            fns[kind]()
        torch.cuda.synchronize()
    wall = {k: [] for k in ORDER}
    for _ in range(rounds):
        for kind in ORDER:
            wall[kind].append(time_round(fns[kind], iters))
    return wall


def report(title, wall):
    fmt = lambda v: "%8.3f [%8.3f .. %8.3f]" % (statistics.median(v), min(v), max(v))  # noqa: E731
    print("%-10s %-12s %s" % (title, "contender", "wall ms"))
    for kind in ORDER:
        print("%-10s %-12s %s" % ("", kind, fmt(wall[kind])))
    sep = min(wall["torch"]) > max(wall["hip"]) or min(wall["hip"]) > max(wall["torch"])
    med = {k: statistics.median(v) for k, v in wall.items()}
    verdict = ("hip is FASTER" if med["hip"] < med["torch"] else "hip LOSES") if sep else "no difference beyond the spread"
    print("# %s: torch / hip = %.2f (medians); the min-max ranges %s: %s" % (title, med["torch"] / med["hip"],
                                                                          "do not overlap" if sep else "OVERLAP", verdict), flush=True)


def child(pairs, records, rounds, iters):
    from mickey_amd import synthetic as syn
    from mickey_amd import train_eval as te
    from mickey_amd.config import default_cfg
    dev = torch.device("cuda")
    cfg = default_cfg()
    data, Rgt, tgt = syn.planted_pose_problem(B=pairs, h=51, w=38, seed=4321)
    batch = {k: v.to(dev) for k, v in data.items()}
    T = torch.eye(4).repeat(pairs, 1, 1)
    T[:, :3, :3], T[:, :3, 3] = Rgt, tgt[:, 0]
    batch["T_0to1"] = T.to(dev)
    batch["Kori_color0"] = torch.tensor([[590.0, 0, 270], [0, 590, 360], [0, 0, 1]]).repeat(pairs, 1, 1).to(dev)
    print("# %s; %d pairs of n = %d" % (torch.cuda.get_device_name(0), pairs, 51 * 38))
    solver = te.HipProcrustesSolver(cfg, seed=1)
    acc = te.ValidationAccumulator(pairs, dev, steps=1)

    def tail_hip():
        acc.reset()
        R, t, inl = solver.estimate_pose_vectorized(batch)
        acc.add(R, t, inl, batch)
        return acc.summary()

    def tail_torch():
        R, t, inl = solver.estimate_pose_vectorized(batch)
        return torch_summary([torch_metrics(R, t, batch["T_0to1"], batch["Kori_color0"]) + (inl,)])

    report("tail", alternate({"torch": tail_torch, "hip": tail_hip}, rounds, iters))

    rng = np.random.default_rng(0)
    rec = np.zeros((records, 8), np.float32)
    rec[:, 0], rec[:, 3], rec[:, 4] = rng.uniform(0, 90, records), rng.uniform(0, 0.8, records), rng.uniform(0, 16, records)
    rec[:, 5], rec[:, 6] = rng.uniform(0, 200, records), rng.integers(3, 2048, records)
    big = te.ValidationAccumulator(records, dev, steps=1)
    big.records.copy_(torch.from_numpy(rec))
    big.n = records
    step = 8
    listed = [tuple(big.records[i:i + step, c] for c in (0, 3, 4, 5, 6)) for i in range(0, records, step)]   # the trainer's list of step outputs
    a, b = big.summary(), torch_summary(listed)
    names = ("val_metric_pose/ours_t_err_ang", "val_metric_pose/ours_t_err_euc", "val_metric_pose/ours_R_err", "val_vcre/metric_ours_vcre",
             "val_AUC_pose/prec_pose_ours", "val_AUC_pose/auc_pose", "val_AUC_pose/prec_pose_ours_10", "val_AUC_pose/auc_pose_10",
             "val_vcre/prec_vcre_ours", "val_vcre/auc_vcre")
    print("# summary over N = %d records in steps of %d: largest |hip - torch| / |torch| over the ten figures = %.2e"
          % (records, step, max(abs(a[n] - v) / max(abs(v), 1e-30) for n, v in zip(names, b))))
    report("summary", alternate({"torch": lambda: torch_summary(listed), "hip": big.summary}, rounds, max(1, iters // 2)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--records", type=int, default=32768)
    ap.add_argument("--limit", type=int, default=300, help="seconds the measurement may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "validation_bench.txt"))
    args = ap.parse_args()
    if args.child:
        if not torch.cuda.is_available():
            sys.exit("bench_validation: needs a GPU (nothing is measured on the CPU)")
        child(args.pairs, args.records, args.rounds, args.iters)
        return
    from mickey_amd import build as mk_build
    lines = ["# tools/bench_validation.py: the validation tail after the loss (solver + pose / VCRE metrics + epoch summary) and the summary alone",
             "# torch: the trainer's metric and summary sequence restated in torch / numpy; hip: mickey_amd.train_eval; both on HipProcrustesSolver",
             "# torch %s, kernels %s; %d alternating rounds of %d repetitions, one synchronisation per round, wall ms per repetition: median [min .. max]"
             % (torch.__version__, mk_build.source_hash(), args.rounds, args.iters), ""]
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--rounds", str(args.rounds), "--iters", str(args.iters),
           "--pairs", str(args.pairs), "--records", str(args.records)]
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=args.limit)
    except subprocess.TimeoutExpired as e:
        sys.exit("bench_validation: ran past %d s; stopping\n%s" % (args.limit, e.stdout or ""))
    print(r.stdout, end="", flush=True)
    if r.returncode != 0:
        sys.exit("bench_validation: the measurement ended with status %d\n%s" % (r.returncode, r.stderr))
    lines += r.stdout.splitlines()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
