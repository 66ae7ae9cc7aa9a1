"""Pair-list mode against the standard forward on the same pairs (README "Pair-list mode"): ViT-L in the bench configuration
(bf16 encoder, heads auto, synthetic checkpoint), 540x720, 32 pairs per step, two pair structures:

    sequence   33 frames -> the 32 consecutive pairs (i, i + 1): 33 images encoded instead of 64
    kf_x_q     4 keyframes x 8 queries -> 32 pairs from 12 frames: 12 images encoded instead of 64

The standard forward gets the materialised batch (images[pair_index[:, 0]], images[pair_index[:, 1]]), the pair-list forward the
image set and the list.  The two alternate step by step after a warm-up of each; HIP events around every step; median and
min-max per case.  Prints one JSON line.

    python tools/bench_pairlist.py [--steps 10] [--warmup 2]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    from mickey_amd import synthetic as syn
    from mickey_amd.config import default_cfg
    from mickey_amd.model import MickeyRelativePose
    dev = torch.device("cuda:0")
    cfg = default_cfg()
    cfg["AMD"]["ENCODER_DTYPE"] = "bf16"   # bench.py's defaults: --dtype bf16, --heads-dtype auto, --graph auto (eager at B = 32)
    cfg["AMD"]["HEADS_DTYPE"] = "auto"
    model = MickeyRelativePose(cfg)
    model.load_state_dict(syn.mickey_state_dict(cfg, seed=0))
    model = model.to(dev)
    H, W = 720, 540
    cases = {"sequence": (33, [[i, i + 1] for i in range(32)]),
             "kf_x_q": (12, [[k, 4 + q] for k in range(4) for q in range(8)])}

    def step(d):
        data = dict(d)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        model(data)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), data

    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    out = {"metric": "pairlist_forward_pairs_per_s", "size": [H, W], "steps": args.steps, "warmup": args.warmup, "cases": {},
           "device": torch.cuda.get_device_name(dev)}
    for name, (N, pairs) in cases.items():
        batch = syn.synthetic_batch(B=N, H=H, W=W, seed=1234)
        images, K = batch["image0"].to(dev), batch["K_color0"].to(dev)
        idx = torch.tensor(pairs, device=dev, dtype=torch.long)
        P = len(pairs)
        std = {"image0": images[idx[:, 0]], "image1": images[idx[:, 1]], "K_color0": K[idx[:, 0]], "K_color1": K[idx[:, 1]]}
        pl = {"images": images, "K_color": K, "pair_index": torch.tensor(pairs, dtype=torch.int32)}
        for _ in range(args.warmup):
            step(std)
            step(pl)
        t_std, t_pl, same = [], [], True
        for i in range(args.steps):
            model.reseed(calls=0)
            a, ds = step(std)
            model.reseed(calls=0)
            b, dp = step(pl)
            t_std.append(a)
            t_pl.append(b)
            if i == 0:
                same = all(torch.equal(ds[k], dp[k]) for k in ("R", "t", "inliers"))
        ms_std, ms_pl = med(t_std), med(t_pl)
        out["cases"][name] = {
            "images": N, "pairs": P, "images_encoded_standard": 2 * P,
            "standard_ms_per_step": round(ms_std, 2), "standard_ms_min_max": [round(min(t_std), 2), round(max(t_std), 2)],
            "pairlist_ms_per_step": round(ms_pl, 2), "pairlist_ms_min_max": [round(min(t_pl), 2), round(max(t_pl), 2)],
            "standard_pairs_per_s": round(P / ms_std * 1e3, 1), "pairlist_pairs_per_s": round(P / ms_pl * 1e3, 1),
            "ratio": round(ms_std / ms_pl, 3), "ranges_overlap": bool(min(t_std) <= max(t_pl)), "outputs_equal": bool(same)}
        del std, pl, images
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
