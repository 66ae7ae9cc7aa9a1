"""mickey_amd.train_tails without a GPU: the plain-torch restatements of the four head tails against the reference's own fp64 autograd
(tests/golden/head_tails_grad.npz, written by tools/make_golden_head_tails.py), the softmax backward identity the kernel implements,
the argument checks of the ops, the swap contract of use_hip_tails / use_hip_training and the C ABI of the new entry points."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "head_tails_grad.npz")
NEW_SYMBOLS = ("mk_train_headtail_chunk_rows", "mk_train_headtail_chunks", "mk_train_headtail_fwd", "mk_train_headtail_bwd",
               "mk_train_desc_l2norm_fwd", "mk_train_desc_l2norm_bwd")
CASES = ("score_softmax", "score_sigmoid", "offset", "depth", "depth_sigmoid", "desc")


@pytest.fixture(scope="module")
def nv():
    from mickey_amd import build, _native
    if not os.path.exists(build.lib_path()):
        build.build(verbose=False)
    _native.load()
    return _native


def _formula(tt, z, case, x, w):
    if case == "score_softmax":
        return tt.score_tail_formula(x, w, int(z["border"]), True, float(z["temperature"]), float(z["eps"]))
    if case == "score_sigmoid":
        return tt.score_tail_formula(x, w, int(z["border"]), False)
    if case == "offset":
        return tt.offset_tail_formula(x, w)
    if case == "depth":
        return tt.depth_tail_formula(x, w, False)
    if case == "depth_sigmoid":
        return tt.depth_tail_formula(x, w, True, float(z["max_depth"]))
    return tt.desc_l2norm_formula(x, float(z["eps_l2norm"]))


def test_golden_fixture_is_data_of_the_six_cases():
    assert os.path.getsize(GOLDEN) < 1 << 20
    z = np.load(GOLDEN)
    for case in CASES:
        C = 128 if case == "desc" else 64
        cout = {"offset": 2, "desc": C}.get(case, 1)
        assert z["x_" + case].shape == (2, C, 8, 9) and z["x_" + case].dtype == np.float32 and float(z["x_" + case].min()) == 0.0
        assert z["go_" + case].shape == (2, cout, 8, 9) and z["go_" + case].dtype == np.float32
        assert z["out_" + case].shape == (2, cout, 8, 9) and z["out_" + case].dtype == np.float64
        assert z["gx_" + case].shape == (2, C, 8, 9) and z["gx_" + case].dtype == np.float64
        if case != "desc":
            assert z["w_" + case].shape == (cout, 64, 1, 1) and z["w_" + case].dtype == np.float32
            assert z["gw_" + case].shape == (cout, 64, 1, 1) and z["gw_" + case].dtype == np.float64
    assert float(z["temperature"]) == 100.0 and int(z["border"]) == 3 and float(z["max_depth"]) == 60.0
    assert float(z["eps"]) == float(np.float32(1e-16)) and float(z["eps_l2norm"]) == 1e-10
    assert len(z.files) == 6 * 4 + 5 * 2 + 5


@pytest.mark.parametrize("case", CASES)
def test_formula_reproduces_the_reference_autograd(case):
    from mickey_amd import train_tails as tt
    z = np.load(GOLDEN)
    x = torch.from_numpy(z["x_" + case]).double().requires_grad_()
    w = None if case == "desc" else torch.from_numpy(z["w_" + case]).double().requires_grad_()
    out = _formula(tt, z, case, x, w)
    ins = [x] + ([] if w is None else [w])
    grads = torch.autograd.grad(out, ins, torch.from_numpy(z["go_" + case]).double())
    got = dict(zip(("gx", "gw"), grads), out=out.detach())
    assert len(got) == (2 if case == "desc" else 3)
    for name, g in got.items():
        want = torch.from_numpy(z["%s_%s" % (name, case)])
        assert g.dtype == torch.float64 and g.shape == want.shape
        e = float((g - want).abs().max() / want.abs().max())
        print("%s %s: %.3e" % (case, name, e))
        assert e <= 1e-12, (case, name, e)


def test_fixture_regenerates_from_the_reference_bit_for_bit():
    from oracle import ref_shim
    if not ref_shim.available():
        pytest.skip("no reference checkout")
    spec = importlib.util.spec_from_file_location("make_golden_head_tails", os.path.join(ROOT, "tools", "make_golden_head_tails.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    new = tool.generate()
    z = np.load(GOLDEN)
    assert sorted(new) == sorted(z.files)
    for k in z.files:
        a, b = np.asarray(new[k]), z[k]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k


def test_softmax_backward_identity():
    """gz_p = (y_p / T) (g_p - sum_q g_q y_q), exact including eps and the border mask, the mean detached: what the kernel evaluates."""
    from mickey_amd import train_tails as tt
    g = torch.Generator().manual_seed(7)
    B, C, H, W = 2, 64, 8, 9
    T, eps, border = 100.0, 1e-16, 3
    feat = torch.relu(torch.randn((B, C, H, W), generator=g, dtype=torch.float64)).requires_grad_()
    w = (torch.randn((1, C, 1, 1), generator=g, dtype=torch.float64) / C ** 0.5).requires_grad_()
    go = torch.randn((B, 1, H, W), generator=g, dtype=torch.float64)
    y = tt.score_tail_formula(feat, w, border, True, T, eps)
    gfeat, gw = torch.autograd.grad(y, (feat, w), go)
    yd = y.detach()
    gz = (yd / T) * (go - (go * yd).sum((1, 2, 3), keepdim=True))
    assert float(gz[:, :, :border].abs().max()) == 0.0 and float(gz[:, :, :, W - border:].abs().max()) == 0.0   # masked pixels: exact zeros
    w2 = w.detach().view(1, C)
    mine_feat = torch.einsum("bohw,oc->bchw", gz, w2)
    mine_w = torch.einsum("bohw,bchw->oc", gz, feat.detach()).view(1, C, 1, 1)
    for name, a, b in (("gfeat", mine_feat, gfeat), ("gw", mine_w, gw)):
        e = float((a - b).abs().max() / b.abs().max())
        print("softmax identity %s: %.3e" % (name, e))
        assert e <= 1e-12, (name, e)
    # an eps that matters (the scores of an image then sum to less than 1): the identity still holds
    y = tt.score_tail_formula(feat, w, border, True, 0.05, 0.5)
    gfeat, = torch.autograd.grad(y, (feat,), go)
    yd = y.detach()
    gz = (yd / 0.05) * (go - (go * yd).sum((1, 2, 3), keepdim=True))
    mine = torch.einsum("bohw,oc->bchw", gz, w2)
    assert float((mine - gfeat).abs().max() / gfeat.abs().max()) <= 1e-12 and float(yd.sum()) < 1.99


class _Boom:
    """stands in for the library: any touch fails the test"""
    def __getattr__(self, name):
        raise AssertionError("the library was touched (%s) before the arguments were checked" % name)


def test_bad_arguments_raise_before_anything_touches_the_library(monkeypatch):
    from mickey_amd import _native, ops, train_tails as tt
    x, w1, w2 = torch.zeros(2, 64, 5, 6), torch.zeros(1, 64, 1, 1), torch.zeros(2, 64, 1, 1)
    xd = torch.zeros(2, 128, 5, 6)
    # well-formed CPU tensors: no CPU fallback
    for call in (lambda: tt.score_tail_train(x, w1), lambda: tt.score_tail_train(x, w1, use_softmax=False), lambda: tt.offset_tail_train(x, w2),
                 lambda: tt.depth_tail_train(x, w1), lambda: tt.depth_tail_train(x, w1, True, 60.0), lambda: tt.desc_l2norm_train(xd)):
        with pytest.raises(_native.MickeyHipError):
            call()
    monkeypatch.setattr(_native, "load", lambda: _Boom())
    monkeypatch.setattr(_native, "_lib", None)
    monkeypatch.setattr(ops, "call", lambda *a: _Boom().call)
    monkeypatch.setattr(ops, "query", lambda *a: _Boom().query)
    bad_feats = [x.half(), x.double(), x.bfloat16(),                                   # dtype (autocast is not covered)
                 x[0], x[None], x.reshape(2, 64, 30),                                  # rank
                 torch.zeros(2, 66, 5, 6), torch.zeros(2, 2, 5, 6), torch.zeros(2, 260, 5, 6), torch.zeros(2, 0, 5, 6),   # width
                 torch.zeros(0, 64, 5, 6), torch.zeros(2, 64, 0, 6), torch.zeros(2, 64, 5, 0),   # B, H, W >= 1
                 x.numpy()]                                                            # not a tensor
    for f in bad_feats:
        for call in (lambda: tt.score_tail_train(f, w1), lambda: tt.offset_tail_train(f, w2), lambda: tt.depth_tail_train(f, w1),
                     lambda: tt.desc_l2norm_train(f)):
            with pytest.raises(ValueError):
                call()
    for wrong in (w1.double(), w1.half(), torch.zeros(1, 64), torch.zeros(1, 32, 1, 1), torch.zeros(1, 64, 3, 3), w2, w1.numpy()):
        with pytest.raises(ValueError):
            tt.score_tail_train(x, wrong)
        with pytest.raises(ValueError):
            tt.depth_tail_train(x, wrong)
    for wrong in (w2.double(), w1, torch.zeros(3, 64, 1, 1), torch.zeros(2, 64)):
        with pytest.raises(ValueError):
            tt.offset_tail_train(x, wrong)
    for border in (-1, 1.5, "3", None, True):
        with pytest.raises(ValueError):
            tt.score_tail_train(x, w1, border=border)
    for t in (0.0, -100.0, float("nan"), float("inf"), "100", None, True):
        with pytest.raises(ValueError):
            tt.score_tail_train(x, w1, temperature=t)
        with pytest.raises(ValueError):
            tt.depth_tail_train(x, w1, True, t)
    for eps in (-1e-16, float("nan"), float("inf"), "1e-16", None, True):
        with pytest.raises(ValueError):
            tt.score_tail_train(x, w1, eps=eps)
        with pytest.raises(ValueError):
            tt.desc_l2norm_train(xd, eps)


# ---- stand-ins for the reference's extractor heads: its attribute names, none of its code --------------------------------------
class _Block(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, cout, 3, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(cout)

    def forward(self, x, relu=True):
        x = self.bn1(self.conv1(x))
        return torch.relu(x) if relu else x


class _AttStack(nn.Module):
    def __init__(self):
        super().__init__()
        self.proj = nn.Linear(16, 16, bias=False)

    def forward(self, x):
        return x


class _Head(nn.Module):
    def __init__(self, kind, C=64, bias=False, **attrs):
        super().__init__()
        self.resblock1, self.resblock2, self.resblock3 = _Block(32, 32), _Block(32, 32), _Block(32, 32)
        self.resblock4 = _Block(32, 128 if kind == "desc" else C)
        self.sigmoid = nn.Sigmoid()
        if kind == "score":
            self.score = nn.Conv2d(C, 1, 1, bias=bias)
            self.use_softmax, self.tmp_softmax = True, 100
            self.logsigmoid, self.softmax = nn.LogSigmoid(), nn.Softmax(dim=-1)
            self.eps = nn.Parameter(torch.tensor(1e-16), requires_grad=False)
            self.offset_par1 = nn.Parameter(torch.tensor(0.5), requires_grad=False)
            self.offset_par2 = nn.Parameter(torch.tensor(2.), requires_grad=False)
            self.ones_kernel = nn.Parameter(torch.ones((1, 1, 3, 3)), requires_grad=False)
        elif kind == "offset":
            self.xy_offset = nn.Conv2d(C, 2, 1, bias=bias)
        elif kind == "depth":
            self.depth = nn.Conv2d(C, 1, 1, bias=bias)
            self.use_depth_sigmoid, self.max_depth = False, 60
        else:
            self.norm_desc = True
        for k, v in attrs.items():
            setattr(self, k, v)
        self.att_layer = _AttStack()


class _Extractor(nn.Module):
    def __init__(self):
        super().__init__()
        self.depth_head, self.det_offset, self.dsc_head, self.det_head = _Head("depth"), _Head("offset"), _Head("desc"), _Head("score")
        self.biased = _Head("score", bias=True)                 # a 1x1 conv with a bias
        self.odd_width = _Head("depth", C=66)                   # no multiple of 4
        self.wide = _Head("offset", C=260)                      # beyond 256
        self.plain_desc = _Head("desc", norm_desc=False)        # nothing to fuse
        self.no_flag = _Head("score", use_softmax=1)            # use_softmax must be a bool
        self.fp16 = _Head("offset").half()
        self.conv = nn.Conv2d(64, 1, 1, bias=False)             # a 1x1 conv that is no head
        self.conv3 = nn.Conv2d(64, 32, 3, padding=1, bias=False)


_LEFT_ALONE = ("biased", "odd_width", "wide", "plain_desc", "no_flag", "fp16")
_SWAPPED = {"det_head": "score", "det_offset": "offset", "depth_head": "depth", "dsc_head": "desc"}


def test_swap_contract():
    from mickey_amd import train_tails as tt
    m = _Extractor()
    m.det_offset.eval()
    m.depth_head.use_depth_sigmoid, m.depth_head.max_depth = True, 45.0
    keys = list(m.state_dict().keys())
    params = {n: id(p) for n, p in m.named_parameters()}
    assert sum(n.startswith("det_head.") and not p.requires_grad for n, p in m.named_parameters()) == 4   # eps, offset_par1/2, ones_kernel
    children = {n: dict(getattr(m, n)._modules) for n in _SWAPPED}
    assert tt.use_hip_tails(m) == 4
    for name, kind in _SWAPPED.items():
        head = getattr(m, name)
        assert type(head) is tt.HipHead and head.kind == kind, name
        assert list(head._modules) == list(children[name])
        for cname, child in children[name].items():
            assert head._modules[cname] is child, (name, cname)
    assert m.det_head.use_softmax is True and m.det_head.tmp_softmax == 100 and m.det_head.score_eps == float(np.float32(1e-16))
    assert m.depth_head.use_depth_sigmoid is True and m.depth_head.max_depth == 45.0 and m.dsc_head.norm_desc is True
    assert m.dsc_head.block4_takes_relu
    assert m.det_head.training and not m.det_offset.training
    for name in _LEFT_ALONE:
        assert type(getattr(m, name)) is _Head, name
    assert type(m.conv) is nn.Conv2d
    assert list(m.state_dict().keys()) == keys
    assert {n: id(p) for n, p in m.named_parameters()} == params
    assert tt.use_hip_tails(m) == 0   # idempotent
    m.load_state_dict(_Extractor().state_dict(), strict=True)
    # .train() / .eval() reach the very same children through the wrappers
    m.det_head.eval()
    assert not m.det_head.training and not children["det_head"]["resblock1"].bn1.training
    m.det_head.train()
    assert children["det_head"]["resblock1"].bn1.training
    assert tt.use_hip_tails(nn.Sequential(_Head("offset"), nn.ReLU(), _Head("score", bias=True))) == 1


def test_swap_composes_with_the_other_use_hip_calls():
    import mickey_amd
    from mickey_amd import train_attention as ta, train_encoder as te, train_heads as th, train_layer as tl, train_matcher as tm, train_tails as tt
    calls = (tt.use_hip_tails, tl.use_hip_encoder_layers, ta.use_hip_attention, th.use_hip_convs, tm.use_hip_matcher, te.use_hip_encoder)
    for order in ((0, 1, 2, 3, 4, 5), (5, 4, 3, 2, 1, 0)):
        m = _Extractor()
        keys = list(m.state_dict().keys())
        params = {n: id(p) for n, p in m.named_parameters()}
        counts = {i: calls[i](m) for i in order}
        assert counts[0] == 4 and counts[1] == 0 and counts[2] == 0 and counts[4] == 0 and counts[5] == 0, counts
        assert counts[3] == 36, counts   # the fp32 3x3 convs with Cout % 4 == 0: 4 in each of 8 heads, 3 in odd_width, conv3 (none in fp16)
        assert list(m.state_dict().keys()) == keys and {n: id(p) for n, p in m.named_parameters()} == params
        for name in _SWAPPED:
            assert type(getattr(m, name)) is tt.HipHead and isinstance(getattr(m, name).resblock1.conv1, th.Conv3x3)
        assert all(c(m) == 0 for c in calls[:1] + calls[3:4])
    m = _Extractor()
    got = mickey_amd.use_hip_training(m)
    assert got == {"use_hip_encoder": 0, "use_hip_convs": 36, "use_hip_encoder_layers": 0, "use_hip_attention": 0, "use_hip_tails": 4,
                   "use_hip_matcher": 0}
    assert mickey_amd.use_hip_training(m, split="auto", dtype="auto") == dict.fromkeys(got, 0)
    with pytest.raises(TypeError):
        mickey_amd.use_hip_training(m, tails=True)


def test_abi_of_the_new_entry_points(nv):
    lib = nv.load()
    raw = open(os.path.join(ROOT, "include", "mickey_hip.h")).read()
    declared = set(re.findall(r"\b(mk_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", raw, flags=re.S)))
    for name in NEW_SYMBOLS:
        assert name in declared and name in nv.SIGNATURES and hasattr(lib, name), name
    assert nv.missing_symbols() == []
    decl = raw.index("int mk_train_headtail_chunk_rows(")
    doc = raw[raw.rfind("/*", 0, decl):decl]
    for cite in ("mickey_extractor.py:98-124", "134-140", "172-176", "211-216", "248-249", "utils/extractor_utils.py:6-10"):
        assert cite in doc, cite
    from mickey_amd import ops
    for name in ("train_headtail_fwd", "train_headtail_bwd", "train_desc_l2norm_fwd", "train_desc_l2norm_bwd", "headtail_chunks"):
        assert callable(getattr(ops, name))
    # the chunking of a weight gradient: a function of the row count alone, the constant ops.py exports
    q = nv.query
    R = ops.HEADTAIL_CHUNK_ROWS
    assert q("mk_train_headtail_chunk_rows") == R
    for rows, chunks in ((1, 1), (R - 1, 1), (R, 1), (R + 1, 2), (3876, -(-3876 // R)), (24 * 1938, -(-24 * 1938 // R)), (0, 0), (-5, 0)):
        assert q("mk_train_headtail_chunks", rows) == chunks == ops.headtail_chunks(rows), rows
    assert (ops.TAIL_IDENTITY, ops.TAIL_SIGMOID, ops.TAIL_MASKED_SIGMOID, ops.TAIL_SOFTMAX) == (0, 1, 2, 3)
    for name, code in (("IDENTITY", 0), ("SIGMOID", 1), ("MASKED_SIGMOID", 2), ("SOFTMAX", 3)):
        assert re.search(r"MK_TAIL_%s = %d\b" % (name, code), raw)
    one = 16   # any non-null, aligned address: argument checks come before every launch and never touch it

    def fwd(**kw):
        a = dict(dict(feat=one, w=one, out=one, nimg=2, h=8, wd=9, C=64, Cout=1, act=3, scale=1.0, border=3, T=100.0, eps=1e-16), **kw)
        return lib.mk_train_headtail_fwd(a["feat"], a["w"], a["out"], a["nimg"], a["h"], a["wd"], a["C"], a["Cout"], a["act"], a["scale"],
                                         a["border"], a["T"], a["eps"], None)
    for bad in (dict(feat=None), dict(w=None), dict(out=None), dict(feat=8), dict(w=4), dict(nimg=0), dict(h=0), dict(wd=0), dict(C=0), dict(C=66),
                dict(C=260), dict(Cout=0), dict(Cout=3), dict(Cout=2), dict(act=2, Cout=2), dict(act=4), dict(act=-1), dict(border=-1),
                dict(T=0.0), dict(T=float("nan")), dict(T=float("inf")), dict(eps=-1.0), dict(eps=float("nan")), dict(act=1, scale=0.0)):
        assert fwd(**bad) == 1, bad
        assert b"mk_train_headtail_fwd" in lib.mk_last_error()

    def bwd(**kw):
        a = dict(dict(g=one, y=one, feat=one, w=one, dot=one, gfeat=one, part=one, gw=one, nimg=2, n=72, C=64, Cout=1, act=3, scale=1.0,
                      T=100.0), **kw)
        return lib.mk_train_headtail_bwd(a["g"], a["y"], a["feat"], a["w"], a["dot"], a["gfeat"], a["part"], a["gw"], a["nimg"], a["n"],
                                         a["C"], a["Cout"], a["act"], a["scale"], a["T"], None)
    for bad in (dict(g=None), dict(y=None), dict(dot=None), dict(w=None), dict(feat=None), dict(part=None), dict(gfeat=8), dict(part=4),
                dict(nimg=0), dict(n=0), dict(C=2), dict(C=258), dict(Cout=3), dict(Cout=2), dict(act=5), dict(T=0.0), dict(T=float("nan")),
                dict(act=1, scale=0.0), dict(act=1, scale=-2.0)):
        assert bwd(**bad) == 1, bad
        assert b"mk_train_headtail_bwd" in lib.mk_last_error()
    assert bwd(gfeat=None, gw=None) == 0                                  # nothing wanted: nothing launched
    assert bwd(act=0, y=None, dot=None, gfeat=None, gw=None) == 0         # the identity needs neither y nor dot
    assert lib.mk_train_desc_l2norm_fwd(None, one, one, 2, 72, 128, 1e-10, None) == 1
    assert lib.mk_train_desc_l2norm_fwd(one, None, one, 2, 72, 128, 1e-10, None) == 1
    for nimg, n, C, eps in ((0, 72, 128, 1e-10), (2, 0, 128, 1e-10), (2, 72, 130, 1e-10), (2, 72, 0, 1e-10), (2, 72, 260, 1e-10),
                            (2, 72, 128, -1.0), (2, 72, 128, float("nan")), (65536, 72, 128, 1e-10)):
        assert lib.mk_train_desc_l2norm_fwd(one, one, None, nimg, n, C, eps, None) == 1
        assert b"mk_train_desc_l2norm_fwd" in lib.mk_last_error()
    for args in ((None, one, one, one, 2, 72, 128), (one, None, one, one, 2, 72, 128), (one, one, None, one, 2, 72, 128),
                 (one, one, one, None, 2, 72, 128), (one, one, one, one, 0, 72, 128), (one, one, one, one, 2, 0, 128),
                 (one, one, one, one, 2, 72, 6)):
        assert lib.mk_train_desc_l2norm_bwd(*args, None) == 1
        assert b"mk_train_desc_l2norm_bwd" in lib.mk_last_error()
