#!/usr/bin/env python
"""Bit fingerprints of every linear-attention entry point: one line per case with the SHA-256 of each output's raw bytes (chunk
partials, kv, out, and for training gq, gk, gv, gkv).  Inputs come from CPU generators with fixed seeds.  Run it on two builds on
the same machine and compare the outputs line for line: a refactor of the kernels must not change a single bit.  The bits depend
on the installed math library (expf), so the output is a proof for one machine and one software stack, not a golden file.

    python tools/linattn_bits.py [--out FILE]
"""
import argparse
import hashlib
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mickey_amd import ops  # noqa: E402

DEV = torch.device("cuda:0")
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def sha(t):
    if t is None:
        return "-"
    torch.cuda.synchronize()
    return hashlib.sha256(t.contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def line(name, **outs):
    return name + " " + " ".join("%s=%s" % (k, sha(v)) for k, v in outs.items())


def zeros(*shape, dtype=torch.float32):
    return torch.zeros(shape, device=DEV, dtype=dtype)


def unfused(L, C, out_dtype, seed):
    G, nimg = 2, 2
    qkv = torch.randn((G, nimg * L, 3 * C), generator=torch.Generator().manual_seed(seed)).to(DEV)
    kv = zeros(G * nimg * (C // 16), 272)
    work = zeros(ops.linattn_work_floats(G, nimg, L, C))
    ops.linattn_kv(qkv, kv, work, G, nimg, L, C)
    out = zeros(G, nimg * L, C, dtype=DTYPES[out_dtype])
    ops.linattn_apply(qkv, kv, out, C, G, nimg, L, C)
    return line("unfused L=%d C=%d out=%s" % (L, C, out_dtype), work=work, kv=kv, out=out)


def fused(G, nimg, gh, gw, dtype, merge, seed):
    C, L = 128, gh * gw
    M = nimg * L
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *shape, s=1.0: (torch.randn(shape, generator=gen) * s).to(DEV)  # noqa: E731
    cat = rn(G, M, 2 * C).to(DTYPES[dtype])
    qkv_w = rn(G, 3 * C, C, s=2.0 / math.sqrt(C)).to(DTYPES[dtype])
    merge_w = rn(G, C, C, s=1.5 / math.sqrt(C)).to(DTYPES[dtype])
    lw, lb = 1.0 + 0.3 * rn(G, C), 0.2 * rn(G, C)
    kv = zeros(G * nimg * (C // 16), 272)
    work = zeros(ops.linattn_work_floats(G, nimg, L, C))
    ops.linattn_kv_fused(cat, qkv_w, kv, work, G, nimg, L, C)
    if merge:   # the normalised rows go to the other column half of the same rows, as in the heads
        out = ops.linattn_apply_fused(cat, qkv_w, kv, cat[:, :, C:], G, nimg, L, C, merge_w=merge_w, ln_w=lw, ln_b=lb)
    else:
        out = ops.linattn_apply_fused(cat, qkv_w, kv, zeros(G, M, C, dtype=DTYPES[dtype]), G, nimg, L, C)
    return line("fused G=%d nimg=%d %dx%d %s merge=%d" % (G, nimg, gh, gw, dtype, merge), work=work, kv=kv, out=out)


def training(N, L, S, C, seed):
    """forward once, then the backward for each `need` mask; the C entry points directly, so that work and gkv can be read"""
    H = C // 16
    gen = torch.Generator().manual_seed(seed)
    if L == S:   # thirds of one packed [N, L, 3C] buffer
        packed = (1.5 * torch.randn((N, L, 3 * C), generator=gen)).to(DEV)
        q, k, v = (packed[:, :, i * C:(i + 1) * C].view(N, L, H, 16) for i in range(3))
    else:        # separate views: q with padded rows, k | v as halves of one buffer
        qb = (1.5 * torch.randn((N, L, C + 32), generator=gen)).to(DEV)
        kvb = (1.5 * torch.randn((N, S, 2 * C), generator=gen)).to(DEV)
        q, k, v = qb[:, :, :C].view(N, L, H, 16), kvb[:, :, :C].view(N, S, H, 16), kvb[:, :, C:].view(N, S, H, 16)
    go = torch.randn((N, L, H, 16), generator=gen).to(DEV)
    eps = 1e-6
    rows = ops._attn_rows(q) + ops._attn_rows(k) + ops._attn_rows(v)
    nwork = int(ops.query("mk_linattn_train_work_floats", N, L, S, C))
    out, kv, work = zeros(N, L, H, 16), zeros(N * H, 272), zeros(nwork)
    ops.call("mk_linattn_train_fwd", *rows, eps, ops.ptr(out), ops.ptr(kv), ops.ptr(work), N, L, S, C, ops.stream())
    name = "train N=%d L=%d S=%d C=%d" % (N, L, S, C)
    lines = [line(name + " fwd", work=work, kv=kv, out=out)]
    for need in ((1, 1, 1), (1, 0, 0), (0, 1, 1)):
        gq = zeros(N, L, H, 16) if need[0] else None
        gk = zeros(N, S, H, 16) if need[1] else None
        gv = zeros(N, S, H, 16) if need[2] else None
        gkv, work = zeros(N * H, 272), zeros(nwork)
        ops.call("mk_linattn_train_bwd", *rows, ops.ptr(kv), ops.ptr(go), eps, ops.ptr(work), ops.ptr(gkv), ops.ptr(gq), ops.ptr(gk),
                 ops.ptr(gv), N, L, S, C, ops.stream())
        lines.append(line(name + " bwd need=%d%d%d" % need, work=work, gkv=gkv, gq=gq, gk=gk, gv=gv))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("linattn_bits: needs a GPU")
    lines = ["# %s, torch %s, hip %s" % (torch.cuda.get_device_name(0), torch.__version__, torch.version.hip)]
    seed = 100
    for L in (1, 63, 64, 65, 130):
        for dt in ("fp32", "bf16", "fp16"):
            seed += 1
            lines.append(unfused(L, 128, dt, seed))
    lines.append(unfused(65, 64, "fp16", 150))
    seed = 200
    for dt in ("bf16", "fp16"):
        for geom in ((4, 3, 5, 7), (4, 2, 9, 11), (1, 1, 8, 8)):
            for merge in (0, 1):
                seed += 1
                lines.append(fused(*geom, dt, merge, seed))
    for i, shape in enumerate(((1, 1, 1, 16), (2, 37, 29, 128), (3, 200, 333, 64), (2, 65, 64, 128))):
        lines += training(*shape, 300 + i)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
