"""Write tests/golden/encoder_layer_grad*.npz from THE REFERENCE's own EncoderLayer under fp64 autograd (CPU only).

    python tools/make_golden_encoder_layer.py    (needs the reference checkout: MICKEY_REFERENCE_ROOT, oracle/ref_shim.py)

Builds the reference's EncoderLayer(d_model=128, nhead=8, attention='linear') (att_layers/transformer_utils.py:14-66) with seeded
xavier weights and a non-trivial LayerNorm affine, feeds it seeded x, source and an incoming gradient in fp64 and stores the inputs
(fp32-representable values, as fp32), the output and all twelve gradients (fp64) for a self-attention case (N, L) = (2, 11) and a
cross-attention case (N, L, S) = (1, 12, 7).  A seed is taken only if every pre-activation of the MLP's ReLU is at least 1e-5
away from zero, so that the mask is the same in every precision.  The six weight matrices are 164k values and their fp64 gradients
1.3 MB per case, so the fixture is five files, each below 1 MiB: encoder_layer_grad.npz (inputs, outputs, the gradients of x, source
and the LayerNorm parameters), encoder_layer_grad_<case>_proj.npz (gradients of wq, wk, wv, wm) and encoder_layer_grad_<case>_mlp.npz
(gradients of w1, w2); load_golden() below puts them together again.  tests/test_train_layer_cpu.py checks the in-repo restatement
(mickey_amd.train_layer.encoder_layer_formula) against the file, tests/test_train_layer_gpu.py the kernels.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
OUT = os.path.join(GOLDEN, "encoder_layer_grad.npz")
PARTS = {"proj": ("gwq", "gwk", "gwv", "gwm"), "mlp": ("gw1", "gw2")}
CASES = {"self": (2, 11, None), "cross": (1, 12, 7)}   # (N, L, S)
PARAMS = ("q_proj.weight", "k_proj.weight", "v_proj.weight", "merge.weight", "mlp.0.weight", "mlp.2.weight", "norm1.weight",
          "norm1.bias", "norm2.weight", "norm2.bias")
NAMES = ("wq", "wk", "wv", "wm", "w1", "w2", "ln1_w", "ln1_b", "ln2_w", "ln2_b")
MARGIN = 1e-5


def draw(layer_cls, N, L, S, seed):
    g = torch.Generator().manual_seed(20261017)   # the same weights in both cases (stored once)
    layer = layer_cls(128, 8, attention="linear")
    sd = {}
    for name, p in layer.named_parameters():
        if p.dim() == 2:
            bound = (6.0 / (p.shape[0] + p.shape[1])) ** 0.5   # xavier uniform
            sd[name] = (torch.rand(p.shape, generator=g) * 2 - 1) * bound
        elif name.endswith("weight"):
            sd[name] = 1 + 0.1 * torch.randn(p.shape, generator=g)
        else:
            sd[name] = 0.1 * torch.randn(p.shape, generator=g)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((N, L, 128), generator=g)
    source = None if S is None else torch.randn((N, S, 128), generator=g)
    go = torch.randn((N, L, 128), generator=g)
    layer.load_state_dict(sd, strict=True)
    return layer.double(), sd, x, source, go


def load_golden(golden_dir=GOLDEN):
    """All five files as one {name: array}."""
    z = dict(np.load(os.path.join(golden_dir, "encoder_layer_grad.npz")))
    for tag in CASES:
        for part in PARTS:
            z.update(np.load(os.path.join(golden_dir, "encoder_layer_grad_%s_%s.npz" % (tag, part))))
    return z


def main():
    ref_shim.install()
    from lib.models.MicKey.modules.att_layers.transformer_utils import EncoderLayer
    out = {}
    for i, (tag, (N, L, S)) in enumerate(CASES.items()):
        for seed in range(20261017 + 100 * i, 20261017 + 100 * i + 64):
            layer, sd, x, source, go = draw(EncoderLayer, N, L, S, seed)
            pre = []
            hook = layer.mlp[0].register_forward_hook(lambda mod, inp, res: pre.append(res.detach().abs().min()))
            xd = x.double().requires_grad_()
            sdd = None if source is None else source.double().requires_grad_()
            y = layer(xd, xd if sdd is None else sdd)
            hook.remove()
            if float(pre[0]) >= MARGIN:
                break
        else:
            raise SystemExit("no seed keeps the ReLU's pre-activations %g away from zero for case %s" % (MARGIN, tag))
        params = [dict(layer.named_parameters())[n] for n in PARAMS]
        grads = torch.autograd.grad(y, [xd] + ([] if sdd is None else [sdd]) + params, go.double())
        out["x_" + tag], out["go_" + tag] = x.numpy(), go.numpy()                       # float32
        out["out_" + tag] = y.detach().numpy()                                          # float64
        out["gx_" + tag] = grads[0].numpy()
        if sdd is not None:
            out["source_" + tag] = source.numpy()
            out["gsource_" + tag] = grads[1].numpy()
        for n, pn, gr in zip(NAMES, PARAMS, grads[-len(PARAMS):]):
            out[n] = sd[pn].numpy()                                                     # float32, the same in both cases
            out["g%s_%s" % (n, tag)] = gr.numpy()
        out["margin_" + tag] = np.float64(float(pre[0]))
        print("  %s %s seed %d: min |pre-activation| %.3e  |out| %.3e |gx| %.3e" % (tag, (N, L, S), seed, float(pre[0]), float(y.norm()),
                                                                                   float(grads[0].norm())))
    out["attn_eps"], out["ln_eps"] = np.float64(1e-6), np.float64(1e-5)
    files = {OUT: out}
    for tag in CASES:
        for part, names in PARTS.items():
            files[os.path.join(GOLDEN, "encoder_layer_grad_%s_%s.npz" % (tag, part))] = {"%s_%s" % (n, tag): out.pop("%s_%s" % (n, tag))
                                                                                          for n in names}
    for path, arrays in files.items():
        np.savez_compressed(path, **arrays)
        print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
        assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
