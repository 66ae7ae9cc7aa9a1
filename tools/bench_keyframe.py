"""Keyframe mode against the standard forward on the same pairs (README "Keyframe mode"): ViT-L in the bench configuration
(bf16 encoder, heads auto, synthetic checkpoint), 540x720, B = 32 pairs that share K = 1 keyframe.  The standard forward gets
image0 expanded to 32 copies (64 images encoded), the keyframe forward image0 once (33 images).  The two alternate step by step
after a warm-up of each; HIP events around every step; medians.  Prints one JSON line.

    python tools/bench_keyframe.py [--steps 10] [--warmup 2] [--batch 32]
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
    ap.add_argument("--batch", type=int, default=32)
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
    B, H, W = args.batch, 720, 540
    batch = {k: v.to(dev) for k, v in syn.synthetic_batch(B=B, H=H, W=W, seed=1234).items()}
    key = batch["image0"][:1].contiguous()
    std = dict(batch, image0=key.expand(B, -1, -1, -1).contiguous())
    kf = dict(batch, image0=key, keyframe_index=torch.zeros((B,), dtype=torch.int32))

    def step(d):
        data = dict(d)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        model(data)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), data

    for _ in range(args.warmup):
        step(std)
        step(kf)
    t_std, t_kf = [], []
    same = True
    for i in range(args.steps):
        model.reseed(calls=0)
        a, ds = step(std)
        model.reseed(calls=0)
        b, dk = step(kf)
        t_std.append(a)
        t_kf.append(b)
        if i == 0:
            same = all(torch.equal(ds[k], dk[k]) for k in ("final_scores", "R", "t", "inliers"))
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    ms_std, ms_kf = med(t_std), med(t_kf)
    print(json.dumps({"metric": "keyframe_forward_pairs_per_s", "batch": B, "keyframes": 1, "size": [H, W], "steps": args.steps,
                      "warmup": args.warmup, "standard_pairs_per_s": round(B / ms_std * 1e3, 1),
                      "keyframe_pairs_per_s": round(B / ms_kf * 1e3, 1), "ratio": round(ms_std / ms_kf, 3),
                      "standard_ms_per_step": round(ms_std, 2), "keyframe_ms_per_step": round(ms_kf, 2),
                      "outputs_equal": bool(same), "device": torch.cuda.get_device_name(dev)}))


if __name__ == "__main__":
    main()
