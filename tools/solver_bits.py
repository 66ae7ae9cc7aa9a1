#!/usr/bin/env python
"""Bit fingerprints of the sampler, the pose solver and the training-time RANSAC: one line per case (an entry point at one size)
with a SHA-256 per output (its first 128 bits) over the raw bytes of that output in every variant of the case, in a fixed order:
injected noise / injected indices / Philox, 0 and 4 refinement rounds, VCRE / POSE_ERR with the soft clip off and on.  Inputs come from CPU generators with fixed seeds; the sizes cross every loop edge of the shared rigid-fit
code (k, S = 3, 64, 65, 130, and 1024 matches per lane slot table; 1, 5, 33 hypotheses per set: one wave, the 4-wave stride, more
than one pass of 8 parked hypotheses; 0 and 4 refinement rounds) and the inputs take its rare branches (collinear, coincident,
mirrored sets, masks with fewer than three ones, fractional weights).  Run it on two builds on the same machine
(MICKEY_HIP_LIB selects the library) and compare: a refactor of mk_sampler.hip, mk_solver.hip, mk_train_tail.hip or
mk_procrustes.hpp must not change a single bit.  Lines that start with `~` hold sums of fp32 atomics, whose order is not fixed:
they are printed, not compared.  The bits depend on the installed math library: a proof for one machine and one software
stack, not a golden file.

    python tools/solver_bits.py [--out FILE]
    python tools/solver_bits.py --compare FILE_A FILE_B      (no GPU: exit status 1 if a comparable line differs)
"""
import argparse
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = (3, 64, 65, 130)
ITS = (1, 5, 33)
TH = 0.15


class Case:
    """one output line: add() the outputs of every variant of the case, then str()"""

    def __init__(self, name):
        self.name, self.h = name, {}

    def add(self, **outs):
        torch.cuda.synchronize()
        for k, v in outs.items():
            self.h.setdefault(k, hashlib.sha256()).update(v.contiguous().cpu().view(torch.uint8).numpy().tobytes())
        return self

    def __str__(self):
        return self.name + " " + " ".join("%s=%s" % (k, h.hexdigest()[:32]) for k, h in self.h.items())


def rotation(gen):
    q, r = torch.linalg.qr(torch.randn((3, 3), generator=gen, dtype=torch.float64))
    q = q * torch.sign(torch.diagonal(r))
    return (q * torch.linalg.det(q)).float()


def match_sets(nsets, S, seed, mirror=False):
    """X, Y [nsets, S, 3], w [nsets, S]: Y = R X + t + noise, every fifth match an outlier; rows 0..2 of set 0 collinear,
    rows 3, 4 equal and rows 5..7 equal when S allows (the degenerate triples index them)"""
    gen = torch.Generator().manual_seed(seed)
    X = torch.randn((nsets, S, 3), generator=gen) * torch.tensor([3.0, 2.0, 1.0])
    if S >= 8:
        X[0, 2] = 2.0 * X[0, 1] - X[0, 0]
        X[0, 4] = X[0, 3]
        X[0, 6] = X[0, 7] = X[0, 5]
    Y = torch.empty_like(X)
    for s in range(nsets):
        R = rotation(gen)
        if mirror:
            R = R @ torch.diag(torch.tensor([1.0, 1.0, -1.0]))
        Y[s] = X[s] @ R.T + torch.randn((1, 3), generator=gen)
    Y += 0.01 * torch.randn(Y.shape, generator=gen)
    out = torch.arange(S) % 5 == 4
    Y[:, out] += torch.randn((nsets, int(out.sum()), 3), generator=gen)
    w = torch.rand((nsets, S), generator=gen) + 0.05
    return X, Y, w, gen


def exp1(shape, gen):
    return -torch.log(torch.rand(shape, generator=gen).clamp_min(1e-7))


def intrinsics(B):
    return torch.tensor([[600.0, 0.0, 360.0], [0.0, 590.0, 270.0], [0.0, 0.0, 1.0]]).repeat(B, 1, 1)


def sampler(ops, dev):
    lines = []
    B, rows = 2, 3
    for ncell in (4096, 4099):     # the 16-byte and the 4-byte histogram reads
        for k in SIZES:
            gen = torch.Generator().manual_seed(1000 + k + ncell)
            p = torch.rand((B, ncell), generator=gen) ** 4
            p[:, ::7] = 0.0
            noise = exp1((B * rows, ncell), gen)
            c = Case("exprace_topk ncell=%d k=%d" % (ncell, k))
            idx, cnt = ops.exprace_topk(p.to(dev), rows, k, noise=noise.to(dev))
            c.add(idx_noise=idx, cnt_noise=cnt)
            idx, cnt = ops.exprace_topk(p.to(dev), rows, k, seed=77, offset=5)
            lines.append(str(c.add(idx_philox=idx, cnt_philox=cnt)))
    return lines


def gather(ops, dev):
    lines = []
    B, rows, n0, n1 = 2, 3, 37, 41
    K0, K1 = intrinsics(B).to(dev), (intrinsics(B) * torch.tensor([1.1, 0.9, 1.0]).view(1, 3, 1)).to(dev)
    for k in SIZES:
        gen = torch.Generator().manual_seed(2000 + k)
        fs = torch.rand((B, n0, n1), generator=gen).to(dev)
        kps0, kps1 = (torch.rand((B, 2, n0), generator=gen) * 500).to(dev), (torch.rand((B, 2, n1), generator=gen) * 500).to(dev)
        dep0, dep1 = (torch.rand((B, 1, n0), generator=gen) * 4 + 0.5).to(dev), (torch.rand((B, 1, n1), generator=gen) * 4 + 0.5).to(dev)
        idx = torch.randint(0, n0 * n1, (B * rows, k), generator=gen, dtype=torch.int32).to(dev)
        X, Y, wts, corr = ops.gather_backproject(idx, fs, kps0, dep0, kps1, dep1, K0, K1, rows)
        lines.append(str(Case("gather_backproject k=%d" % k).add(X=X, Y=Y, wts=wts, corr=corr)))
        gX, gY = torch.randn(X.shape, generator=gen).to(dev), torch.randn(Y.shape, generator=gen).to(dev)
        g = ops.gather_backproject_bwd(idx, corr, gX, gY, K0, K1, B, rows, n0, n1)
        lines.append("~" + str(Case("gather_backproject_bwd k=%d (fp32 atomics: not comparable)" % k).add(gkps0=g[0], gdep0=g[1], gkps1=g[2], gdep1=g[3])))
    return lines


def inference(ops, dev):
    lines = []
    B, itm = 2, 2
    nsets = B * itm
    for k in SIZES:
        for itr in ITS:
            X, Y, w, gen = match_sets(nsets, k, 3000 + 10 * k + itr)
            Xd, Yd, wd = X.to(dev), Y.to(dev), w.to(dev)
            name = "k=%d it_ransac=%d" % (k, itr)
            noise3 = exp1((nsets * itr, k), gen).to(dev)
            idx3 = torch.stack([torch.randperm(k, generator=gen)[:3] for _ in range(nsets * itr)]).to(torch.int32).to(dev)
            hyp, ref = Case("ransac_hypotheses " + name), Case("refine_pose " + name)
            for tag, kw in (("noise", dict(noise3=noise3)), ("idx3", dict(idx3_in=idx3)), ("philox", dict(seed=11, offset=3, set_base=7))):
                Rh, th, score, sel = ops.ransac_hypotheses(Xd, Yd, wd, itr, TH, **kw)
                hyp.add(Rh=Rh, th=th, score=score, idx3=sel)
                if tag == "philox":
                    continue
                for num_ref in (0, 4):
                    r = ops.refine_pose(Xd, Yd, Rh, th, score, B, itm, itr, TH, num_ref, 3)
                    ref.add(R=r[0], t=r[1], conf=r[2], best=r[3], mask=r[4], rounds=r[5], invalid=r[6])
            lines += [str(hyp), str(ref)]
    # the rare branches of the 3 x 3 Kabsch: generic, collinear, two coincident, three coincident triples; a mirrored set
    for mirror in (False, True):
        X, Y, w, gen = match_sets(1, 8, 3900 + mirror, mirror)
        idx3 = torch.tensor([[0, 3, 5], [0, 1, 2], [3, 4, 0], [5, 6, 7]], dtype=torch.int32).to(dev)
        Rh, th, score, sel = ops.ransac_hypotheses(X.to(dev), Y.to(dev), w.to(dev), 4, TH, idx3_in=idx3)
        lines.append(str(Case("ransac_hypotheses degenerate triples mirror=%d" % mirror).add(Rh=Rh, th=th, score=score, idx3=sel)))
        r = ops.refine_pose(X.to(dev), Y.to(dev), Rh, th, score, 1, 1, 4, 10.0, 4, 3)   # every match an inlier of the mirrored fit too
        lines.append(str(Case("refine_pose degenerate triples mirror=%d" % mirror).add(R=r[0], t=r[1], conf=r[2], best=r[3], mask=r[4], rounds=r[5])))
    return lines


def rare_masks(mask, S, itr):
    """hypotheses 0.. of set 0: two ones, one, none, the collinear triple, coincident points, fractional weights"""
    rows = [[0, 1], [0], [], [0, 1, 2], [3, 4, 5, 6, 7]]
    for h, ones in enumerate(rows[:itr]):
        mask[h] = 0.0
        mask[h, [j for j in ones if j < S]] = 1.0
    if itr > len(rows):
        mask[len(rows)] *= torch.linspace(0.25, 1.75, S)
    return mask


def training(ops, dev):
    lines = []
    B, itm = 2, 2
    nsets = B * itm
    K0, K1 = intrinsics(B).to(dev), (intrinsics(B) * torch.tensor([1.1, 0.9, 1.0]).view(1, 3, 1)).to(dev)
    for S in SIZES + (1024,):
        nc = 3 if S == 3 else 8
        for itr in ITS:
            X, Y, w, gen = match_sets(nsets, S, 4000 + 10 * S + itr, mirror=(S == 65))
            Xd, Yd, wd = X.to(dev), Y.to(dev), w.to(dev)
            name = "S=%d it_ransac=%d" % (S, itr)
            noise = exp1((nsets * itr, S), gen).to(dev)
            idx_in = torch.stack([torch.randperm(S, generator=gen)[:nc] for _ in range(nsets * itr)]).to(torch.int32).to(dev)
            cases = [Case(f + " " + name) for f in ("train_ransac_masks", "train_tail_fwd", "train_aggregate_fwd", "train_aggregate_bwd",
                                                    "train_tail_bwd")]
            for num_ref in (0, 4):
                for tag, kw in (("noise", dict(noise=noise)), ("idx", dict(idx_in=idx_in)), ("philox", dict(seed=21, offset=9, set_base=5))):
                    mask, idx, rounds = ops.train_ransac_masks(Xd, Yd, wd, itr, TH, num_ref, nc, **kw)
                    cases[0].add(mask=mask, idx=idx, rounds=rounds)
            mask = rare_masks(mask.cpu(), S, itr).to(dev)
            Rgt = torch.stack([rotation(gen) for _ in range(B)]).to(dev)
            tgt = torch.randn((B, 3), generator=gen).to(dev)
            for loss_type in (0, 1):   # VCRE, POSE_ERR
                for clip in (0, 1):
                    out, Rt, saved = ops.train_tail_fwd(Xd, Yd, mask, Rgt, tgt, K0, K1, itr, itm, TH, loss_type, clip)
                    cases[1].add(loss=out[:, 0], rot=out[:, 1], trans=out[:, 2], score=out[:, 3], R=Rt[:, :9], t=Rt[:, 9:], saved=saved)
                    lv, per_pair, coef, flags = ops.train_aggregate_fwd(out, Rt, saved, B, itm, itr, 0.3, clip, 1.5, 2.0)
                    cases[2].add(loss_value=lv, per_pair=per_pair, coef=coef, flags=flags)
                    g = ops.train_aggregate_bwd(coef, torch.randn((B,), generator=gen).to(dev), B, itm, itr)
                    cases[3].add(g=g)
                    gX, gY = ops.train_tail_bwd(Xd, Yd, mask, Rgt, tgt, K0, K1, itr, itm, TH, loss_type, clip, Rt, saved, g)
                    cases[4].add(gX=gX, gY=gY)
            lines += [str(c) for c in cases]
    return lines


def compare(a, b):
    la, lb = ([l for l in open(f).read().splitlines() if l and l[0] not in "#~"] for f in (a, b))
    bad = [x for x, y in zip(la, lb) if x != y]
    print("%d comparable lines in %s, %d in %s, %d differ" % (len(la), a, len(lb), b, len(bad) + abs(len(la) - len(lb))))
    for x in bad:
        print("  differs: " + x[:100])
    return 1 if bad or len(la) != len(lb) or not la else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--compare", nargs=2, default=None)
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    if not torch.cuda.is_available():
        sys.exit("solver_bits: needs a GPU")
    from mickey_amd import ops
    dev = torch.device("cuda:0")
    lines = ["# %s, torch %s, hip %s" % (torch.cuda.get_device_name(0), torch.__version__, torch.version.hip)]
    lines += sampler(ops, dev) + gather(ops, dev) + inference(ops, dev) + training(ops, dev)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
