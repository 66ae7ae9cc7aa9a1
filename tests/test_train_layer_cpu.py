"""mickey_amd.train_layer without a GPU: the plain-torch restatement of the layer against the reference's own fp64 autograd
(tests/golden/encoder_layer_grad*.npz, written by tools/make_golden_encoder_layer.py), the argument checks of the ops, the swap
contract of use_hip_encoder_layers and the C ABI of the new entry points."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
WEIGHTS = ("wq", "wk", "wv", "wm", "w1", "w2", "ln1_w", "ln1_b", "ln2_w", "ln2_b")
NEW_SYMBOLS = ("mk_train_rows_per_chunk", "mk_train_chunks", "mk_train_ln_steps", "mk_train_linear_fwd", "mk_train_linear_ln128_fwd", "mk_train_linear_dgrad",
               "mk_train_linear_wgrad", "mk_train_tail", "mk_train_ln128_fwd", "mk_train_ln128_bwd")


def load_golden():
    z = dict(np.load(os.path.join(GOLDEN, "encoder_layer_grad.npz")))
    for tag in ("self", "cross"):
        for part in ("proj", "mlp"):
            z.update(np.load(os.path.join(GOLDEN, "encoder_layer_grad_%s_%s.npz" % (tag, part))))
    return z


@pytest.fixture(scope="module")
def nv():
    from mickey_amd import build, _native
    if not os.path.exists(build.lib_path()):
        build.build(verbose=False)
    _native.load()
    return _native


def test_golden_fixture_is_data_of_the_two_cases():
    for f in os.listdir(GOLDEN):
        if f.startswith("encoder_layer_grad"):
            assert os.path.getsize(os.path.join(GOLDEN, f)) < 1 << 20, f
    z = load_golden()
    assert z["x_self"].shape == (2, 11, 128) and z["x_cross"].shape == (1, 12, 128) and z["source_cross"].shape == (1, 7, 128)
    assert "source_self" not in z
    for tag in ("self", "cross"):
        assert z["x_" + tag].dtype == np.float32 and z["go_" + tag].dtype == np.float32
        assert z["out_" + tag].dtype == np.float64 and z["out_" + tag].shape == z["x_" + tag].shape
        assert z["gx_" + tag].dtype == np.float64 and z["gx_" + tag].shape == z["x_" + tag].shape
        assert float(z["margin_" + tag]) >= 1e-5
        for n in WEIGHTS:
            assert z[n].dtype == np.float32 and z["g%s_%s" % (n, tag)].dtype == np.float64 and z["g%s_%s" % (n, tag)].shape == z[n].shape
    assert z["gsource_cross"].shape == (1, 7, 128)


@pytest.mark.parametrize("tag", ["self", "cross"])
def test_formula_reproduces_the_reference_autograd(tag):
    from mickey_amd import train_layer as tl
    z = load_golden()
    x = torch.from_numpy(z["x_" + tag]).double().requires_grad_()
    src = x if tag == "self" else torch.from_numpy(z["source_" + tag]).double().requires_grad_()
    w = [torch.from_numpy(z[n]).double().requires_grad_() for n in WEIGHTS]
    out = tl.encoder_layer_formula(x, src, *w, attn_eps=float(z["attn_eps"]), ln1_eps=float(z["ln_eps"]), ln2_eps=float(z["ln_eps"]))
    ins = [x] + ([] if tag == "self" else [src]) + w
    names = ["gx"] + ([] if tag == "self" else ["gsource"]) + ["g" + n for n in WEIGHTS]
    grads = torch.autograd.grad(out, ins, torch.from_numpy(z["go_" + tag]).double())
    got = dict(zip(names, grads), out=out.detach())
    assert len(got) == (12 if tag == "self" else 13)   # out + the gradients of x (, source) and the ten parameters
    for name, g in got.items():
        want = torch.from_numpy(z["%s_%s" % (name, tag)])
        assert g.dtype == torch.float64 and g.shape == want.shape
        e = float((g - want).abs().max() / want.abs().max())
        print("%s %s: %.3e" % (tag, name, e))
        assert e <= 1e-12, (tag, name, e)


def test_bad_arguments_raise_before_any_launch():
    from mickey_amd import _native, train_layer as tl
    z = load_golden()
    w = [torch.from_numpy(z[n]) for n in WEIGHTS]
    x, s = torch.zeros(2, 5, 128), torch.zeros(2, 7, 128)
    with pytest.raises(_native.MickeyHipError):          # well-formed CPU tensors: no CPU fallback
        tl.encoder_layer_train(x, s, *w)
    with pytest.raises(_native.MickeyHipError):
        tl.encoder_layer_train(x, x, *w)
    with pytest.raises(_native.MickeyHipError):
        tl.HipEncoderLayer()(x, x)
    with pytest.raises(_native.MickeyHipError):
        tl.linear_train(x, w[0])
    with pytest.raises(_native.MickeyHipError):
        tl.layernorm_train(x, w[6], w[7])
    bad_inputs = [
        (x.half(), s), (x, s.double()), (x.bfloat16(), s.bfloat16()),       # dtype (autocast is not covered)
        (x.reshape(10, 128), s), (x, s.reshape(2, 7, 8, 16)),               # rank
        (torch.zeros(2, 5, 64), torch.zeros(2, 7, 64)), (x, torch.zeros(2, 7, 256)),   # width
        (x, torch.zeros(3, 7, 128)),                                        # N
        (torch.zeros(2, 0, 128), s), (x, torch.zeros(2, 0, 128)), (torch.zeros(0, 5, 128), torch.zeros(0, 7, 128)),   # empty
        (x.numpy(), s),                                                     # not a tensor
    ]
    for a, b in bad_inputs:
        with pytest.raises(ValueError):
            tl.encoder_layer_train(a, b, *w)
    for i, n in enumerate(WEIGHTS):
        for wrong in (w[i].double(), torch.zeros(64, 64), w[i][None]):
            with pytest.raises(ValueError):
                tl.encoder_layer_train(x, s, *(w[:i] + [wrong] + w[i + 1:]))
    for eps in (float("nan"), float("inf"), -1e-6, "1e-6", None, True):
        for kw in ("attn_eps", "ln1_eps", "ln2_eps"):
            with pytest.raises(ValueError):
                tl.encoder_layer_train(x, s, *w, **{kw: eps})
        with pytest.raises(ValueError):
            tl.layernorm_train(x, w[6], w[7], eps)
    for a, ww in ((x.half(), w[0]), (x, w[0].double()), (x, torch.zeros(128, 64)), (x, torch.zeros(120, 128)), (x, torch.zeros(128)),
                  (torch.zeros(0, 128), w[0])):
        with pytest.raises(ValueError):
            tl.linear_train(a, ww)
    for a, g, b in ((x.double(), w[6], w[7]), (torch.zeros(2, 5, 64), w[6], w[7]), (x, torch.zeros(64), w[7]), (x, w[6], w[7].double()),
                    (torch.zeros(0, 128), w[6], w[7])):
        with pytest.raises(ValueError):
            tl.layernorm_train(a, g, b)
    for kw in (dict(d_model=64), dict(nhead=4), dict(attention="full")):
        with pytest.raises(ValueError):
            tl.HipEncoderLayer(**kw)


# ---- a stand-in for the reference's att_layers: the attribute names of Attention / EncoderLayer, none of its code --------------
def _elu1(x):
    return F.elu(x) + 1


class _Att(nn.Module):
    def __init__(self, attention="linear", eps=1e-6):
        super().__init__()
        self.feature_map = _elu1
        self.eps = eps
        self.attention = attention

    def forward(self, queries, keys, values):
        raise NotImplementedError


class _Layer(nn.Module):
    def __init__(self, d=128, nhead=8, attention="linear", bias=False, affine=True):
        super().__init__()
        self.dim, self.nhead = d // nhead, nhead
        self.q_proj = nn.Linear(d, d, bias=bias)
        self.k_proj = nn.Linear(d, d, bias=False)
        self.v_proj = nn.Linear(d, d, bias=False)
        self.attention = _Att(attention)
        self.merge = nn.Linear(d, d, bias=False)
        self.mlp = nn.Sequential(nn.Linear(2 * d, 2 * d, bias=False), nn.ReLU(True), nn.Linear(2 * d, d, bias=False))
        self.norm1 = nn.LayerNorm(d, elementwise_affine=affine)
        self.norm2 = nn.LayerNorm(d)


class _Gelu(_Layer):
    def __init__(self):
        super().__init__()
        self.mlp[1] = nn.GELU()


class _Model(nn.Module):
    def __init__(self):
        super().__init__()
        self.layers = nn.ModuleList([_Layer(), _Layer(), _Layer()])
        self.shared = self.layers[0]                   # one module under two parents
        self.full = _Layer(attention="full")
        self.narrow = _Layer(d=64)
        self.heads4 = _Layer(nhead=4)
        self.biased = _Layer(bias=True)
        self.plain_norm = _Layer(affine=False)
        self.gelu = _Gelu()
        self.fp16 = _Layer().half()
        self.conv = nn.Conv2d(32, 32, 3, padding=1, bias=False)


def test_swap_contract():
    from mickey_amd import train_layer as tl
    m = _Model()
    m.layers[2].eval()
    keys = list(m.state_dict().keys())
    params = {n: p for n, p in m.named_parameters()}
    children = {i: dict(m.layers[i]._modules) for i in range(3)}
    assert tl.use_hip_encoder_layers(m) == 4   # three layers + the second registration of the shared one
    for i in range(3):
        lay = m.layers[i]
        assert type(lay) is tl.HipEncoderLayer and lay.nhead == 8 and lay.dim == 16
        assert list(lay._modules) == list(children[i])
        for name, child in children[i].items():
            assert lay._modules[name] is child, name
    assert m.shared is m.layers[0]
    assert m.layers[0].training and not m.layers[2].training
    for name in ("full", "narrow", "heads4", "biased", "plain_norm", "gelu", "fp16"):
        assert type(getattr(m, name)) in (_Layer, _Gelu), name
    assert type(m.conv) is nn.Conv2d
    assert list(m.state_dict().keys()) == keys
    for n, p in m.named_parameters():
        assert p is params[n], n
    assert tl.use_hip_encoder_layers(m) == 0   # idempotent
    m.load_state_dict(_Model().state_dict(), strict=True)
    assert tl.use_hip_encoder_layers(nn.Sequential(_Layer(), nn.ReLU(), _Layer(attention="full"))) == 1
    # a freshly built module has the reference's state-dict keys
    assert list(tl.HipEncoderLayer().state_dict().keys()) == list(_Layer().state_dict().keys())


def test_swap_composes_with_the_other_use_hip_calls():
    from mickey_amd import train_attention as ta, train_heads as th, train_layer as tl, train_matcher as tm
    calls = (tl.use_hip_encoder_layers, ta.use_hip_attention, th.use_hip_convs, tm.use_hip_matcher)
    for order in ((0, 1, 2, 3), (3, 2, 1, 0), (1, 0, 3, 2)):
        m = _Model()
        m.conv3 = nn.Conv2d(64, 32, 3, padding=1, bias=False)
        keys = list(m.state_dict().keys())
        counts = {}
        for i in order:
            counts[i] = calls[i](m)
        # attention modules with the linear contract: the 3 layers (the shared one is reached once more through its second parent when
        # the layers are still plain modules), narrow, heads4, biased, plain_norm, gelu, fp16
        assert counts[0] == 4 and counts[2] == 2 and counts[3] == 0 and counts[1] == 9, counts
        assert list(m.state_dict().keys()) == keys
        for lay in m.layers:
            assert type(lay) is tl.HipEncoderLayer and isinstance(lay.attention, ta.LinearAttention)
        assert isinstance(m.conv3, th.Conv3x3)
        assert tl.use_hip_encoder_layers(m) == 0


def test_abi_of_the_new_entry_points(nv):
    lib = nv.load()
    raw = open(os.path.join(ROOT, "include", "mickey_hip.h")).read()
    declared = set(re.findall(r"\b(mk_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", raw, flags=re.S)))
    for name in NEW_SYMBOLS:
        assert name in declared and name in nv.SIGNATURES and hasattr(lib, name), name
    assert nv.missing_symbols() == []
    decl = raw.index("int mk_train_rows_per_chunk(")
    assert "att_layers/transformer_utils.py:40-66" in raw[raw.rfind("/*", 0, decl):decl]
    from mickey_amd import ops
    for name in ("train_linear_fwd", "train_linear_ln128_fwd", "train_linear_dgrad", "train_linear_wgrad", "train_tail", "train_ln128_fwd", "train_ln128_bwd"):
        assert callable(getattr(ops, name))
    # the chunking of a weight gradient: whole steps of 128 rows, at most 32 chunks, a function of the row count alone
    q = nv.query
    for M, rpc, chunks in ((1, 128, 1), (128, 128, 1), (129, 128, 2), (600, 128, 5), (3876, 128, 31), (4096, 128, 32), (4097, 256, 17),
                           (15504, 512, 31), (46512, 1536, 31)):
        assert (q("mk_train_rows_per_chunk", M), q("mk_train_chunks", M)) == (rpc, chunks), M
        assert q("mk_train_ln_steps", M) == (M + 127) // 128
    assert q("mk_train_chunks", 0) == 0 and q("mk_train_rows_per_chunk", -3) == 0 and q("mk_train_ln_steps", 0) == 0
    one = 16   # any non-null, aligned address: argument checks come before every launch and never touch it

    def fwd(**kw):
        a = dict(dict(a1=one, lda1=128, K1=128, a2=None, lda2=0, K2=0, w=one, w2=None, w3=None, ws=0, out=one, ldo=128, M=5, N=128), **kw)
        return lib.mk_train_linear_fwd(a["a1"], a["lda1"], a["K1"], a["a2"], a["lda2"], a["K2"], a["w"], a["w2"], a["w3"], a["ws"], a["out"],
                                       a["ldo"], a["M"], a["N"], 0, None)
    for bad in (dict(a1=None), dict(a1=8), dict(w=None), dict(out=4), dict(lda1=64), dict(lda1=130), dict(K1=120), dict(K2=128), dict(M=0),
                dict(N=0), dict(N=126), dict(ldo=64), dict(ws=128), dict(ws=128, N=384, w2=one), dict(ws=100, N=300, w2=one, w3=one)):
        assert fwd(**bad) == 1, bad
        assert b"mk_train_linear_fwd" in lib.mk_last_error()

    def dgrad(**kw):
        a = dict(dict(g=one, ldg=128, gp=0, gs=0, w=one, mask=None, ldm=0, o1=one, ldo1=128, K1=128, o2=None, ldo2=0, K2=0, M=5, N=128), **kw)
        return lib.mk_train_linear_dgrad(a["g"], a["ldg"], a["gp"], a["gs"], a["w"], None, None, 0, a["mask"], a["ldm"], a["o1"], a["ldo1"],
                                         a["K1"], a["o2"], a["ldo2"], a["K2"], 0, a["M"], a["N"], None)
    for bad in (dict(g=None), dict(w=None), dict(o1=None), dict(o1=4), dict(ldg=64), dict(N=120), dict(K2=128), dict(mask=one, ldm=64),
                dict(M=0), dict(gs=100), dict(gs=64, ldg=32), dict(gs=64, gp=6)):
        assert dgrad(**bad) == 1, bad
        assert b"mk_train_linear_dgrad" in lib.mk_last_error()

    def wgrad(**kw):
        a = dict(dict(g=one, ldg=128, a1=one, lda1=128, K1=128, part=one, cs=16384, rpc=128, chunks=1, M=5, N=128), **kw)
        return lib.mk_train_linear_wgrad(a["g"], a["ldg"], 0, 0, a["a1"], a["lda1"], a["K1"], None, 0, 0, a["part"], a["cs"], a["rpc"],
                                         a["chunks"], a["M"], a["N"], None)
    for bad in (dict(g=None), dict(a1=None), dict(part=None), dict(part=8), dict(cs=100), dict(cs=16386), dict(rpc=0), dict(rpc=100),
                dict(chunks=0), dict(M=129), dict(M=0), dict(lda1=64)):
        assert wgrad(**bad) == 1, bad
        assert b"mk_train_linear_wgrad" in lib.mk_last_error()
    assert lib.mk_train_tail(None, 0, 0, 0, None, 0, 0, 0, one, None) == 1
    assert lib.mk_train_tail(one, 4, 1, 8, None, 0, 0, 0, one, None) == 1      # stride below the width
    assert lib.mk_train_tail(None, 0, 0, 0, one, 512, 0, 512, one, None) == 1  # no steps
    assert lib.mk_train_ln128_fwd(None, one, one, 1e-5, None, 0, one, None, None, 5, None) == 1
    assert lib.mk_train_ln128_fwd(one, one, one, -1.0, None, 0, one, None, None, 5, None) == 1
    assert lib.mk_train_ln128_fwd(one, one, one, 1e-5, one, 64, one, None, None, 5, None) == 1
    assert lib.mk_train_ln128_fwd(one, one, one, 1e-5, None, 0, one, None, None, 0, None) == 1
    ln = lambda **kw: (lambda a: lib.mk_train_linear_ln128_fwd(a["a1"], a["lda1"], a["K1"], None, 0, 0, a["w"], one, one, a["eps"], a["resid"],   # noqa: E731
                                                               a["ldr"], a["out"], None, None, a["M"], None))(
        dict(dict(a1=one, lda1=128, K1=128, w=one, eps=1e-5, resid=None, ldr=0, out=one, M=5), **kw))
    for bad in (dict(a1=None), dict(w=None), dict(out=8), dict(lda1=64), dict(K1=100), dict(eps=-1.0), dict(resid=one, ldr=64), dict(M=0)):
        assert ln(**bad) == 1, bad
        assert b"mk_train_linear_ln128_fwd" in lib.mk_last_error()
    assert lib.mk_train_ln128_bwd(one, one, None, one, one, None, 0, 5, None) == 1
    assert lib.mk_train_ln128_bwd(one, one, one, one, one, one, 128, 5, None) == 1
    assert lib.mk_train_ln128_bwd(one, one, one, one, None, None, 0, 5, None) == 0   # nothing wanted: nothing launched
