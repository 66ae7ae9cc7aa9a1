"""mickey_amd.train_attention without a GPU: the formulas the kernels implement against the reference's own fp64 autograd
(tests/golden/linattn_grad.npz, written by tools/make_golden_linattn.py), the argument checks of the op, the swap contract of
use_hip_attention and the C ABI of the new entry points."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "linattn_grad.npz")
NEW_SYMBOLS = ("mk_linattn_train_work_floats", "mk_linattn_train_fwd", "mk_linattn_train_bwd")


@pytest.fixture(scope="module")
def nv():
    from mickey_amd import build, _native
    if not os.path.exists(build.lib_path()):
        build.build(verbose=False)
    _native.load()
    return _native


def test_golden_fixture_is_small_and_has_both_elu_branches():
    assert os.path.getsize(GOLDEN) < 256 * 1024
    z = np.load(GOLDEN)
    shapes = set()
    for tag in ("a", "b"):
        q, k, v, go = (z["%s_%s" % (n, tag)] for n in ("q", "k", "v", "go"))
        assert q.dtype == np.float32 and k.dtype == np.float32 and v.dtype == np.float32 and go.dtype == np.float32
        assert (q > 0).any() and (q < 0).any() and (k > 0).any() and (k < 0).any()
        assert z["out_" + tag].dtype == np.float64 and z["out_" + tag].shape == q.shape
        assert z["gq_" + tag].shape == q.shape and z["gk_" + tag].shape == k.shape and z["gv_" + tag].shape == v.shape
        shapes.add((q.shape[1] == k.shape[1], q.shape[2]))
    assert (False, 8) in shapes   # one case with L != S


@pytest.mark.parametrize("tag", ["a", "b"])
def test_formulas_reproduce_the_reference_autograd(tag):
    from mickey_amd import train_attention as ta
    z = np.load(GOLDEN)
    eps = float(z["eps"])
    q, k, v, go = (torch.from_numpy(z["%s_%s" % (n, tag)]).double() for n in ("q", "k", "v", "go"))
    want = {n: torch.from_numpy(z["%s_%s" % (n, tag)]) for n in ("out", "gq", "gk", "gv")}
    got = dict(zip(("gq", "gk", "gv"), ta.linear_attention_grads(q, k, v, go, eps)))
    got["out"] = ta.linear_attention_formula(q, k, v, eps)
    # and the forward formula under autograd
    x = [t.clone().requires_grad_() for t in (q, k, v)]
    auto = dict(zip(("gq", "gk", "gv"), torch.autograd.grad(ta.linear_attention_formula(*x, eps), x, go)))
    for name, w in want.items():
        assert got[name].dtype == torch.float64 and got[name].shape == w.shape
        e = float((got[name] - w).abs().max() / w.abs().max())
        print("%s %s: %.3e" % (tag, name, e))
        assert e <= 1e-12, (tag, name, e)
        if name in auto:
            assert float((auto[name] - w).abs().max() / w.abs().max()) <= 1e-12, (tag, name)


def test_feature_map_is_elu_plus_one():
    from mickey_amd import train_attention as ta
    x = torch.linspace(-20, 20, 4001, dtype=torch.float64)
    assert float((ta.feature_map(x) - (F.elu(x) + 1)).abs().max()) <= 1e-15
    big = torch.tensor([200.0], requires_grad=True)   # exp(200) overflows fp32: neither the value nor the gradient may see it
    y = ta.feature_map(big)
    y.backward()
    assert float(y.detach()) == 201.0 and float(big.grad) == 1.0


def test_bad_arguments_raise_before_any_launch():
    from mickey_amd import _native, train_attention as ta
    ok = lambda *s: torch.zeros(s)   # noqa: E731
    q, k, v = ok(2, 5, 8, 16), ok(2, 7, 8, 16), ok(2, 7, 8, 16)
    with pytest.raises(_native.MickeyHipError):          # well-formed CPU tensors: no CPU fallback
        ta.linear_attention_train(q, k, v)
    with pytest.raises(_native.MickeyHipError):
        ta.LinearAttention()(q, k, v)
    bad = [
        (q.half(), k.half(), v.half()),                  # half precision (autocast) is not covered
        (q.double(), k, v), (q, k.double(), v), (q, k, v.bfloat16()),
        (q.reshape(2, 5, 128), k, v),                    # rank
        (q, k.reshape(2, 7, 128), v.reshape(2, 7, 128)),
        (ok(2, 5, 4, 32), ok(2, 7, 4, 32), ok(2, 7, 4, 32)),   # head size
        (ok(2, 5, 16, 8), ok(2, 7, 16, 8), ok(2, 7, 16, 8)),
        (ok(1, 5, 9, 16), ok(1, 7, 9, 16), ok(1, 7, 9, 16)),   # C = 144 > 128
        (q, ok(3, 7, 8, 16), ok(3, 7, 8, 16)),           # N
        (q, ok(2, 7, 4, 16), ok(2, 7, 4, 16)),           # H
        (q, k, ok(2, 6, 8, 16)),                         # S of k and v
        (q, k, ok(2, 7, 4, 16)),
        (ok(2, 0, 8, 16), k, v), (q, ok(2, 0, 8, 16), ok(2, 0, 8, 16)), (ok(0, 5, 8, 16), ok(0, 7, 8, 16), ok(0, 7, 8, 16)),   # empty
        (q.numpy(), k, v),                               # not a tensor
    ]
    for args in bad:
        with pytest.raises(ValueError):
            ta.linear_attention_train(*args)
    for eps in (float("nan"), float("inf"), -1e-6, "1e-6", None, True):
        with pytest.raises(ValueError):
            ta.linear_attention_train(q, k, v, eps)
        with pytest.raises(ValueError):
            ta.LinearAttention(eps)


# ---- a stand-in for the reference's att_layers: the attribute names of Attention / EncoderLayer, none of its code --------------
def _elu1(x):
    return F.elu(x) + 1


class _Att(nn.Module):
    def __init__(self, attention="linear", eps=1e-6, feature_map=_elu1):
        super().__init__()
        self.feature_map = feature_map
        self.eps = eps
        self.use_dropout = False
        self.dropout = nn.Dropout(0.1)
        self.attention = attention

    def forward(self, queries, keys, values):
        raise NotImplementedError


class _Layer(nn.Module):
    def __init__(self, d=32, **kw):
        super().__init__()
        self.q_proj, self.k_proj, self.v_proj = (nn.Linear(d, d, bias=False) for _ in range(3))
        self.attention = _Att(**kw)
        self.merge = nn.Linear(d, d, bias=False)
        self.norm1 = nn.LayerNorm(d)


class _WithParam(_Att):
    def __init__(self):
        super().__init__()
        self.scale = nn.Parameter(torch.ones(1))


class _Model(nn.Module):
    def __init__(self):
        super().__init__()
        self.layers = nn.ModuleList([_Layer(), _Layer(eps=1e-5), _Layer()])
        self.full = _Layer(attention="full")
        self.flash = _Layer(attention="flash")
        self.relu_map = _Layer(feature_map=lambda x: F.relu(x) + 1)   # another kernel feature map: not ours
        self.exp_map = _Layer(feature_map=torch.exp)
        self.no_map = _Layer(feature_map=None)
        self.bool_eps = _Layer(eps=True)
        self.text_eps = _Layer(eps="1e-6")
        self.with_param = _WithParam()
        self.shared = self.layers[0].attention                       # one module under two parents
        self.conv = nn.Conv2d(32, 32, 3, padding=1, bias=False)


def test_swap_contract():
    from mickey_amd import train_attention as ta
    m = _Model()
    m.layers[2].eval()
    keys = list(m.state_dict().keys())
    params = {n: p for n, p in m.named_parameters()}
    assert ta.use_hip_attention(m) == 4   # three layers + the second registration of the shared one
    for i, eps in enumerate((1e-6, 1e-5, 1e-6)):
        a = m.layers[i].attention
        assert isinstance(a, ta.LinearAttention) and a.eps == eps and a.attention == "linear"
        assert list(a.parameters()) == [] and list(a.buffers()) == []
    assert m.shared is m.layers[0].attention
    assert m.layers[0].attention.training and not m.layers[2].attention.training
    for name in ("full", "flash", "relu_map", "exp_map", "no_map", "bool_eps", "text_eps"):
        assert type(getattr(m, name).attention) is _Att, name
    assert type(m.with_param) is _WithParam and type(m.conv) is nn.Conv2d
    assert type(m.layers[0].q_proj) is nn.Linear and type(m.layers[0].norm1) is nn.LayerNorm
    assert list(m.state_dict().keys()) == keys
    for n, p in m.named_parameters():
        assert p is params[n], n
    assert ta.use_hip_attention(m) == 0   # idempotent
    m.load_state_dict(_Model().state_dict(), strict=True)
    # the bare module, and a model that is itself the attention module's parent only
    assert ta.use_hip_attention(nn.Sequential(_Att(), nn.ReLU(), _Att("full"))) == 1


def test_swap_composes_with_the_other_use_hip_calls():
    from mickey_amd import train_attention as ta, train_heads as th, train_matcher as tm
    for order in ((0, 1, 2), (2, 1, 0), (1, 2, 0)):
        m = _Model()
        m.conv3 = nn.Conv2d(64, 32, 3, padding=1, bias=False)
        keys = list(m.state_dict().keys())
        calls = (ta.use_hip_attention, th.use_hip_convs, tm.use_hip_matcher)
        counts = {}
        for i in order:
            counts[i] = calls[i](m)
        assert counts == {0: 4, 1: 2, 2: 0}
        assert list(m.state_dict().keys()) == keys
        assert isinstance(m.layers[1].attention, ta.LinearAttention) and isinstance(m.conv3, th.Conv3x3)


def test_abi_of_the_new_entry_points(nv):
    lib = nv.load()
    raw = open(os.path.join(ROOT, "include", "mickey_hip.h")).read()
    declared = set(re.findall(r"\b(mk_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", raw, flags=re.S)))
    for name in NEW_SYMBOLS:
        assert name in declared and name in nv.SIGNATURES and hasattr(lib, name), name
    assert nv.missing_symbols() == []
    decl = raw.index("long long mk_linattn_train_work_floats(")
    assert "att_layers/attention.py:46-64" in raw[raw.rfind("/*", 0, decl):decl]
    # the partial-sum buffer: one 272-float slab per (image, head, chunk of 64 tokens of the longer side)
    q = nv.query
    assert q("mk_linattn_train_work_floats", 8, 1938, 1938, 128) == 8 * 8 * 31 * 272
    assert q("mk_linattn_train_work_floats", 1, 1, 1, 16) == 272
    assert q("mk_linattn_train_work_floats", 2, 37, 129, 64) == 2 * 4 * 3 * 272 == q("mk_linattn_train_work_floats", 2, 129, 37, 64)
    for bad in ((0, 5, 5, 128), (1, 0, 5, 128), (1, 5, 0, 128), (1, 5, 5, 144), (1, 5, 5, 24), (1, 5, 5, 0)):
        assert q("mk_linattn_train_work_floats", *bad) == 0, bad
    one = 16   # any non-null, aligned address: argument checks come before every launch and never touch it
    ok = dict(q=one, ldq=128, sq=640, k=one, ldk=128, sk=640, v=one, ldv=128, sv=640, eps=1e-6, out=one, kv=one, work=one, go=one,
              gkv=one, gq=one, gk=one, gv=one, nimg=1, L=5, S=5, C=128)

    def fwd(**kw):
        a = dict(ok, **kw)
        return lib.mk_linattn_train_fwd(a["q"], a["ldq"], a["sq"], a["k"], a["ldk"], a["sk"], a["v"], a["ldv"], a["sv"], a["eps"], a["out"],
                                        a["kv"], a["work"], a["nimg"], a["L"], a["S"], a["C"], None)

    def bwd(**kw):
        a = dict(ok, **kw)
        return lib.mk_linattn_train_bwd(a["q"], a["ldq"], a["sq"], a["k"], a["ldk"], a["sk"], a["v"], a["ldv"], a["sv"], a["kv"], a["go"],
                                        a["eps"], a["work"], a["gkv"], a["gq"], a["gk"], a["gv"], a["nimg"], a["L"], a["S"], a["C"], None)
    common = (dict(q=None), dict(k=None), dict(v=None), dict(kv=None), dict(q=8), dict(v=20), dict(ldq=64), dict(ldk=130), dict(ldv=0),
              dict(sq=6), dict(sk=-128), dict(nimg=0), dict(nimg=70000), dict(L=0), dict(S=-1), dict(C=144), dict(C=24), dict(C=0))
    for bad in common + (dict(out=None), dict(work=None), dict(out=4)):
        assert fwd(**bad) == 1, bad
        assert b"mk_linattn_train_fwd" in lib.mk_last_error()
    for bad in common + (dict(go=None), dict(work=None), dict(gkv=None), dict(gq=4), dict(gk=8), dict(gv=12),
                         dict(work=None, gkv=None, gk=None)):   # (gv still wanted)
        assert bwd(**bad) == 1, bad
        assert b"mk_linattn_train_bwd" in lib.mk_last_error()
    assert bwd(gq=None, gk=None, gv=None, work=None, gkv=None) == 0   # nothing wanted: nothing launched
