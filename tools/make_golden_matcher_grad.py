"""Write tests/golden/matcher_grad.npz from THE REFERENCE's own autograd (CPU only).

    python tools/make_golden_matcher_grad.py          (needs the reference checkout: MICKEY_REFERENCE_ROOT, oracle/ref_shim.py)

The reference trainer back-propagates d loss / d log(final_scores + 1e-16) through the matcher (lib/models/MicKey/model.py:124-134).
This runs exactly that on the reference's modules -- dualSoftmax (feature_matcher.py:54-83), with and without its dustbin, times
ComputeCorrespondences.kp_matrix_scores (compute_correspondences.py:46-50), log(. + 1e-16), backward of a seeded G -- in fp32
(the reference's dtype) on B = 2 ragged pairs of unit-norm descriptors whose keypoint scores have exact zeros (the border,
remove_brd_and_softmax), and stores the inputs, G and every gradient.  tests/test_matcher_grad_gpu.py reproduces the gradients
with mickey_amd.train_matcher; tests/test_matcher_grad_cpu.py checks the file against the fp64 formulas.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "matcher_grad.npz")
B, C, N0, N1, TEMPERATURE = 2, 128, 150, 131, 0.1


def inputs():
    g = torch.Generator().manual_seed(20261015)
    d0 = torch.randn((B, C, N0), generator=g)
    d1 = torch.randn((B, C, N1), generator=g)
    d0 = d0 / d0.norm(dim=1, keepdim=True)
    d1 = d1 / d1.norm(dim=1, keepdim=True)
    s0 = torch.softmax(torch.randn((B, 1, N0), generator=g), -1)
    s1 = torch.softmax(torch.randn((B, 1, N1), generator=g), -1)
    s0[:, :, :7] = 0.0   # border keypoints: exactly zero scores
    s1[:, :, -5:] = 0.0
    G = torch.randn((B, N0, N1), generator=g)
    return d0, d1, s0, s1, G


def main():
    ref_shim.install()
    from lib.models.MicKey.modules.compute_correspondences import ComputeCorrespondences
    from lib.models.MicKey.modules.utils.feature_matcher import dualSoftmax
    d0, d1, s0, s1, G = inputs()
    out = {"dsc0": d0, "dsc1": d1, "scr0": s0, "scr1": s1, "G": G, "temperature": np.float32(TEMPERATURE)}
    for tag, use_dustbin in (("nodb", False), ("db", True)):
        m = dualSoftmax({"TEMPERATURE": TEMPERATURE, "USE_DUSTBIN": use_dustbin})
        x = [t.clone().requires_grad_() for t in (d0, d1, s0, s1)]
        scores = m(x[0], x[1])
        final = scores * ComputeCorrespondences.kp_matrix_scores(None, x[2], x[3])
        torch.autograd.backward(torch.log(final + 1e-16), G)
        for k, t in zip(("g_dsc0", "g_dsc1", "g_scr0", "g_scr1"), x):
            out["%s_%s" % (k, tag)] = t.grad
        if use_dustbin:
            out["dustbin"] = np.float32(m.dustbin_score.item())
            out["g_dustbin_db"] = m.dustbin_score.grad
        print("  %s: |g_dsc0| %.3e |g_dsc1| %.3e |g_scr0| %.3e |g_scr1| %.3e" %
              ((tag,) + tuple(float(t.grad.norm()) for t in x)))
    arrs = {k: (v.detach().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in out.items()}
    np.savez_compressed(OUT, **arrs)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
