"""The frozen encoder of a training step: what it costs on the HIP kernels, and what the channel-major final norm saves.
(dev tool, not product code; needs a GPU -- there is no CPU path and no fallback)

    python tools/bench_train_encoder.py [--pairs 8] [--reps 20] [--warmup 3] [--out profiles/train_encoder_bench.txt]

ViT-L, 540x720, the reference's training batch of 8 pairs.  Every time is a median over --reps repetitions, each repetition
between two device events on the current stream after --warmup untimed ones; the legs are ALTERNATED repetition by repetition in
one process, so that whatever else the machine is doing meets all of them alike.
  (a) FrozenDinoV2 in fp16 and bf16: two calls of 8 images (the reference's two forward_features calls) and one call of 16
      (encode_frozen on both image sets);
  (b) baseline: the torch restatement oracle.mickey_oracle.vit_forward_features on the GPU in fp16 under no_grad (two calls of 8
      images, then .permute / .reshape / .float() as mickey_extractor.py:49-52).  It is a STAND-IN for the reference's torch
      encoder, which is not available where this runs: plain torch ops of the same mathematics, attention matrix materialised;
  (c) mk_layernorm_nchw against the path it replaces -- mk_layernorm dense fp32, then torch's permute + contiguous copy -- on the
      same rows (16 images' tokens).
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mickey_amd import build, ops, synthetic as syn, train_encoder as te  # noqa: E402
from oracle import mickey_oracle as O  # noqa: E402


def alternate(legs, reps, warmup):
    """legs: {name: callable}.  -> {name: sorted times in ms}; repetition r runs every leg once, in order."""
    times = {k: [] for k in legs}
    for r in range(warmup + reps):
        for name, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= warmup:
                times[name].append(e0.elapsed_time(e1))
    return {k: sorted(v) for k, v in times.items()}


def fmt(name, t):
    n = len(t)
    return "%-58s median %8.3f ms   min %8.3f   max %8.3f   (%d repetitions)" % (name, t[n // 2], t[0], t[-1], n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--height", type=int, default=540)
    ap.add_argument("--width", type=int, default=720)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "train_encoder_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_train_encoder.py measures on a GPU; none is visible (nothing was measured)")
    dev = torch.device("cuda:0")
    B, H, Wd = a.pairs, a.height, a.width
    gh, gw = H // 14, Wd // 14
    npix, D = gh * gw, 1024
    lines = ["train_encoder_bench: measured on %s (device events, medians; kernel sources %s)" %
             (torch.cuda.get_device_name(0), build.source_hash()),
             "ViT-L/14, %d pairs of %dx%d (%d patch tokens per image), synthetic weights and images" % (B, H, Wd, npix), ""]
    sd = syn.dinov2_state_dict("vit_large", seed=0)
    g = torch.Generator().manual_seed(1)
    im0, im1 = (torch.rand((B, 3, H, Wd), generator=g).to(dev) for _ in range(2))

    # ---- (a) + (b), alternated ----------------------------------------------------------------------------------------
    enc = {dt: te.FrozenDinoV2(sd, dtype=dt).to(dev) for dt in ("fp16", "bf16")}
    sd16 = {k: v.to(dev).half() for k, v in sd.items()}
    im0h, im1h = im0.half(), im1.half()

    # the oracle resamples the position table in fp32 and returns it so; the reference casts it back to the tokens' type
    # (dinov2.py:189 .to(previous_dtype)) -- without that the fp16 stand-in would silently run in fp32
    interp = O.interp_pos_embed

    def torch_leg():
        O.interp_pos_embed = lambda pe, h, w_: interp(pe, h, w_).to(pe.dtype)
        try:
            with torch.no_grad():
                return [O.vit_forward_features(sd16, "", x, 16).permute(0, 2, 1).reshape(B, D, gh, gw).float() for x in (im0h, im1h)]
        finally:
            O.interp_pos_embed = interp

    legs = {}
    for dt, m in enc.items():
        legs["(a) FrozenDinoV2 %s, two calls of %d images" % (dt, B)] = lambda m=m: (m(im0), m(im1))
        legs["(a) FrozenDinoV2 %s, one call of %d images" % (dt, 2 * B)] = lambda m=m: te.encode_frozen(m, [im0, im1])
    legs["(b) torch fp16 restatement (stand-in), two calls of %d" % B] = torch_leg
    t = alternate(legs, a.reps, a.warmup)
    lines.append("(a) the frozen encoder on the HIP kernels / (b) the torch stand-in for the reference's fp16 encoder, alternated:")
    lines += ["  " + fmt(k, v) for k, v in t.items()]
    base = t["(b) torch fp16 restatement (stand-in), two calls of %d" % B]
    for k, v in t.items():
        if k.startswith("(a)"):
            lines.append("  measured ratio (b) / %s: %.2f" % (k, base[len(base) // 2] / v[len(v) // 2]))
    ref = torch_leg()
    got = enc["fp16"](im0)
    err = float((got.double() - ref[0].double()).norm() / ref[0].double().norm())
    lines += ["  FrozenDinoV2 fp16 vs the stand-in on image set 0: relative difference %.2e (two fp16 evaluations of one model)" % err, ""]
    del ref, got, sd16, legs
    torch.cuda.empty_cache()

    # ---- (c) the new output stage against the two steps it replaces ------------------------------------------------------------
    nimg = 2 * B
    ntok = npix + 1
    x = torch.randn((nimg * ntok, D), generator=g).to(dev)
    w = (1 + 0.1 * torch.randn((D,), generator=g)).to(dev)
    b = (0.1 * torch.randn((D,), generator=g)).to(dev)
    dense = torch.empty((nimg * npix, D), device=dev, dtype=torch.float32)

    def old_path():
        ops.layernorm(x, w, b, 1e-6, out=dense, rows_out=nimg * npix, rows_per_img=ntok, skip=1)
        return dense.view(nimg, npix, D).permute(0, 2, 1).contiguous()

    def old_ln_only():
        ops.layernorm(x, w, b, 1e-6, out=dense, rows_out=nimg * npix, rows_per_img=ntok, skip=1)

    def new_path():
        return ops.layernorm_nchw(x, w, b, 1e-6, nimg, npix, ntok, skip=1)

    same = torch.equal(old_path(), new_path())
    t = alternate({"(c) mk_layernorm_nchw (allocates its output)": new_path,
                   "(c) mk_layernorm dense fp32 + permute().contiguous()": old_path,
                   "(c) mk_layernorm dense fp32 alone": old_ln_only}, max(a.reps, 50), a.warmup)
    byt = 8.0 * nimg * npix * D
    lines.append("(c) the final norm of %d images, channel-major fp32 output (%.0f MB to move: 4 B read + 4 B written per element):" %
                 (nimg, byt / 1e6))
    lines += ["  " + fmt(k, v) for k, v in t.items()]
    lines.append("  (allocations inside the timed span: mk_layernorm_nchw's torch.empty of its %.0f MB output; the old path's dense buffer is"
                 " allocated beforehand, its contiguous() allocates the %.0f MB result; both come from torch's caching allocator)" %
                 (byt / 2e6, byt / 2e6))
    tn, to = t["(c) mk_layernorm_nchw (allocates its output)"], t["(c) mk_layernorm dense fp32 + permute().contiguous()"]
    mn, mo = tn[len(tn) // 2], to[len(to) // 2]
    lines.append("  mk_layernorm_nchw: %.0f GB/s of its %.0f MB; outputs of the two paths torch.equal: %s" % (byt / mn / 1e6, byt / 1e6, same))
    lines.append("  condition (new kernel faster than the two steps it replaces, measured alternately): %s (%.3f ms vs %.3f ms, %.2fx)" %
                 ("MET" if mn < mo else "NOT MET", mn, mo, mo / mn))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
