"""Write tests/golden/linattn_grad.npz from THE REFERENCE's own autograd (CPU only).

    python tools/make_golden_linattn.py          (needs the reference checkout: MICKEY_REFERENCE_ROOT, oracle/ref_shim.py)

Feeds seeded q, k, v and an incoming gradient gO -- fp32-representable values, scaled so that both branches of elu occur -- through
the reference's Attention(attention='linear') (att_layers/attention.py:14-21,46-64) in fp64 under autograd and stores the inputs,
out and the three gradients, for two small cases (one with L != S).  tests/test_train_attention_cpu.py checks the in-repo formulas
(mickey_amd.train_attention.linear_attention_formula / _grads) against the file, tests/test_train_attention_gpu.py the kernels.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "linattn_grad.npz")
CASES = {"a": (2, 11, 7, 8), "b": (1, 12, 12, 4)}   # (N, L, S, H), heads of 16 channels; fp64 results: about 150 KB in all
EPS = 1e-6


def inputs(N, L, S, H, seed):
    g = torch.Generator().manual_seed(seed)
    q = 1.5 * torch.randn((N, L, H, 16), generator=g)   # fp32 values: about half of them on each branch of elu
    k = 1.5 * torch.randn((N, S, H, 16), generator=g)
    v = torch.randn((N, S, H, 16), generator=g)
    go = torch.randn((N, L, H, 16), generator=g)
    return q, k, v, go


def main():
    ref_shim.install()
    from lib.models.MicKey.modules.att_layers.attention import Attention
    att = Attention(eps=EPS, attention="linear")
    out = {"eps": np.float64(EPS)}
    for i, (tag, (N, L, S, H)) in enumerate(CASES.items()):
        q, k, v, go = inputs(N, L, S, H, 20261017 + i)
        assert bool((q > 0).any()) and bool((q < 0).any()) and bool((k > 0).any()) and bool((k < 0).any())
        x = [t.double().requires_grad_() for t in (q, k, v)]
        y = att(*x)
        gq, gk, gv = torch.autograd.grad(y, x, go.double())
        y = y.detach()
        for name, t in (("q", q), ("k", k), ("v", v), ("go", go)):
            out["%s_%s" % (name, tag)] = t.numpy()                      # float32
        for name, t in (("out", y.detach()), ("gq", gq), ("gk", gk), ("gv", gv)):
            out["%s_%s" % (name, tag)] = t.numpy()                      # float64
        print("  %s %s: |out| %.3e |gq| %.3e |gk| %.3e |gv| %.3e" % (tag, (N, L, S, H), float(y.norm()), float(gq.norm()), float(gk.norm()),
                                                                     float(gv.norm())))
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
