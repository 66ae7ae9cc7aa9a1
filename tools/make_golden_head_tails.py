"""Write tests/golden/head_tails_grad.npz from THE REFERENCE's own head modules under fp64 autograd (CPU only).

    python tools/make_golden_head_tails.py    (needs the reference checkout: MICKEY_REFERENCE_ROOT, oracle/ref_shim.py)

Builds the reference's DeepResBlock_det / _offset / _depth / _desc (mickey_extractor.py:67-251) with the default configuration, puts
pass-through modules in the place of resblock1..4 and att_layer, and calls each head's own forward on seeded relu(randn) features of
[2, 64, 8, 9] ([2, 128, 8, 9] for the descriptors) in fp64: what runs is exactly the head's tail -- `score` + remove_brd_and_softmax,
`score` + sigmoid + remove_borders, `xy_offset` + sigmoid, `depth` with both settings of use_depth_sigmoid, desc_l2norm.  The 1x1
weights are seeded randn / sqrt(C).  Stored: the inputs and the incoming gradients (fp32-representable values, as fp32), the outputs
and every gradient (fp64), and the constants the tails read (temperature, eps, border, max_depth).  Data only, a few tens of KB.
tests/test_train_tails_cpu.py checks the in-repo restatements (mickey_amd.train_tails.*_formula) against the file and, where the
reference is present, that generate() reproduces it bit for bit.
"""
import os
import sys

import numpy as np
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "head_tails_grad.npz")
SHAPE = (2, 64, 8, 9)
SHAPE_DESC = (2, 128, 8, 9)
SEED = 20261019
# case -> (head class, the 1x1 conv's attribute or None, attributes set on the head before the call)
CASES = {
    "score_softmax": ("DeepResBlock_det", "score", {"use_softmax": True}),
    "score_sigmoid": ("DeepResBlock_det", "score", {"use_softmax": False}),
    "offset": ("DeepResBlock_offset", "xy_offset", {}),
    "depth": ("DeepResBlock_depth", "depth", {"use_depth_sigmoid": False}),
    "depth_sigmoid": ("DeepResBlock_depth", "depth", {"use_depth_sigmoid": True}),
    "desc": ("DeepResBlock_desc", None, {"norm_desc": True}),
}


class _Pass(nn.Module):
    def forward(self, x, relu=True):
        return x


def generate():
    """{name: array}: everything the fixture holds, from the reference's own modules."""
    from mickey_amd.config import default_cfg
    ref_shim.install()
    try:
        import lib.models.MicKey.modules.mickey_extractor as ext
        cfg = default_cfg()["MICKEY"]
        out = {}
        g = torch.Generator().manual_seed(SEED)
        for case, (cls, conv, attrs) in CASES.items():
            head = getattr(ext, cls)(cfg)
            for name in ("resblock1", "resblock2", "resblock3", "resblock4", "att_layer"):
                setattr(head, name, _Pass())
            for k, v in attrs.items():
                setattr(head, k, v)
            shape = SHAPE if conv else SHAPE_DESC
            x = torch.relu(torch.randn(shape, generator=g))
            ins = [x.double().requires_grad_()]
            if conv:
                w = torch.randn(getattr(head, conv).weight.shape, generator=g) / shape[1] ** 0.5
                with torch.no_grad():
                    getattr(head, conv).weight.copy_(w)
                out["w_" + case] = w.numpy()
            head = head.double()
            if conv:
                ins.append(getattr(head, conv).weight)
            y = head(ins[0])
            go = torch.randn(y.shape, generator=g)
            grads = torch.autograd.grad(y, ins, go.double())
            out["x_" + case], out["go_" + case] = x.numpy(), go.numpy()            # float32
            out["out_" + case] = y.detach().numpy()                                # float64
            out["gx_" + case] = grads[0].numpy()
            if conv:
                out["gw_" + case] = grads[1].numpy()
            if cls == "DeepResBlock_det":
                out["temperature"] = np.float64(head.tmp_softmax)
                out["eps"] = np.float64(float(head.eps))                           # the fp32 Parameter's value
                out["border"] = np.int64(3)                                        # mickey_extractor.py:138,140
            if cls == "DeepResBlock_depth":
                out["max_depth"] = np.float64(head.max_depth)
        out["eps_l2norm"] = np.float64(1e-10)                                      # utils/extractor_utils.py:8
        return out
    finally:
        ref_shim.uninstall()


def main():
    out = generate()
    np.savez_compressed(OUT, **out)
    for k in sorted(out):
        print("  %-22s %-8s %s" % (k, out[k].dtype, out[k].shape))
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))
    assert os.path.getsize(OUT) < 1 << 20


if __name__ == "__main__":
    main()
