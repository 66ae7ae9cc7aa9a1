"""mickey_amd.train_block without a GPU: basic_block_formula / batchnorm_act_formula against the reference's own BasicBlock under fp64
autograd (skipped where there is no reference checkout), the swap contract of use_hip_blocks / use_hip_training(blocks=True), the
argument checks of the ops and the C ABI of the new entry points."""
import copy
import os
import re

import pytest
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mk_train_bn_chunk_rows", "mk_train_bn_chunks", "mk_train_bn_work_floats", "mk_train_bn_fwd", "mk_train_bn_bwd")


@pytest.fixture(scope="module")
def nv():
    from mickey_amd import build, _native
    if not os.path.exists(build.lib_path()):
        build.build(verbose=False)
    _native.load()
    return _native


@pytest.fixture(scope="module")
def ref_block():
    from oracle import ref_shim
    if not ref_shim.available():
        pytest.skip("no reference checkout")
    ref_shim.install()
    try:
        from lib.models.MicKey.modules.utils.extractor_utils import BasicBlock
    finally:
        ref_shim.uninstall()
    return BasicBlock


def _bn_args(bn):
    return (bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked, bn.momentum, bn.eps)


def _randomise(block, g):
    """affine parameters and running statistics away from their initial 1 / 0, in place"""
    with torch.no_grad():
        for bn in (block.bn1, block.bn2):
            bn.weight.copy_(torch.rand(bn.weight.shape, generator=g, dtype=torch.float64) + 0.5)
            bn.bias.copy_(torch.randn(bn.bias.shape, generator=g, dtype=torch.float64))
            bn.running_mean.copy_(torch.randn(bn.bias.shape, generator=g, dtype=torch.float64))
            bn.running_var.copy_(torch.rand(bn.bias.shape, generator=g, dtype=torch.float64) + 0.5)


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


# ---- 1: the formulas against the reference's BasicBlock, fp64 ------------------------------------------------------------------
@pytest.mark.parametrize("cin,cout", [(8, 4), (8, 8)])        # with and without a shortcut
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("training", [True, False])
def test_block_formula_reproduces_the_reference_autograd(ref_block, cin, cout, relu, training):
    from mickey_amd import train_block as tb
    g = torch.Generator().manual_seed(100 * cin + 10 * cout + 2 * relu + training)
    ref = ref_block(cin, cout).double()
    assert hasattr(ref, "shortcut") == (cin != cout)
    _randomise(ref, g)
    ref.train(training)
    mine = copy.deepcopy(ref)
    steps = 2
    for step in range(steps):
        x = torch.randn((3, cin, 5, 6), generator=g, dtype=torch.float64)
        go = torch.randn((3, cout, 5, 6), generator=g, dtype=torch.float64)
        xr, xm = x.clone().requires_grad_(), x.clone().requires_grad_()
        want = ref(xr, relu=relu)
        params_r = [p for p in ref.parameters()]
        want_g = torch.autograd.grad(want, [xr] + params_r, go)
        sc = mine.shortcut[0].weight if hasattr(mine, "shortcut") else None
        got = tb.basic_block_formula(xm, mine.conv1.weight, _bn_args(mine.bn1), mine.conv2.weight, _bn_args(mine.bn2), sc,
                                     training=training, relu=relu)
        got_g = torch.autograd.grad(got, [xm] + [p for p in mine.parameters()], go)
        names = ["out", "gx"] + ["g:" + n for n, _ in ref.named_parameters()]
        assert len(names) == 2 + len(params_r) == 1 + len(got_g)
        for name, a, b in zip(names, (got.detach(),) + got_g, (want.detach(),) + want_g):
            e = _rel(a, b)
            print("block %d->%d relu %s training %s step %d %s: %.3e" % (cin, cout, relu, training, step, name, e))
            assert a.dtype == torch.float64 and e <= 1e-12, (name, e)
    for name in ("bn1", "bn2"):
        a, b = getattr(mine, name), getattr(ref, name)
        assert int(a.num_batches_tracked) == int(b.num_batches_tracked) == (steps if training else 0)
        for buf in ("running_mean", "running_var"):
            e = _rel(getattr(a, buf), getattr(b, buf))
            print("block %d->%d training %s %s.%s after %d steps: %.3e" % (cin, cout, training, name, buf, steps, e))
            assert e <= 1e-12, (name, buf, e)


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("with_resid", [True, False])
def test_op_formula_reproduces_batchnorm_under_fp64_autograd(relu, training, with_resid):
    """the op's formula against nn.BatchNorm2d + add + F.relu, the lines of the reference's forward, two steps"""
    from mickey_amd import train_block as tb
    g = torch.Generator().manual_seed(4 * relu + 2 * training + with_resid)
    C = 8
    bn = nn.BatchNorm2d(C, momentum=0.3).double().train(training)
    holder = nn.Module()
    holder.bn1 = holder.bn2 = bn
    _randomise(holder, g)
    mine = copy.deepcopy(bn)
    for step in range(2):
        x = torch.randn((2, C, 4, 5), generator=g, dtype=torch.float64) * 3 + 5
        r = torch.randn((2, C, 4, 5), generator=g, dtype=torch.float64)
        go = torch.randn((2, C, 4, 5), generator=g, dtype=torch.float64)
        xr, rr, xm, rm = (t.clone().requires_grad_() for t in (x, r, x, r))
        want = bn(xr) + rr if with_resid else bn(xr)
        want = torch.relu(want) if relu else want
        got = tb.batchnorm_act_formula(xm, *_bn_args(mine)[:5], training, mine.momentum, mine.eps, resid=rm if with_resid else None, relu=relu)
        ins_r = [xr, bn.weight, bn.bias] + ([rr] if with_resid else [])
        ins_m = [xm, mine.weight, mine.bias] + ([rm] if with_resid else [])
        got_g = torch.autograd.grad(got, ins_m, go)
        for name, a, b in zip(("out", "gx", "gw", "gb", "gresid"), (got.detach(),) + got_g, (want.detach(),) + torch.autograd.grad(want, ins_r, go)):
            assert _rel(a, b) <= 1e-12, (name, step)
        if relu:   # a constant mask in place of the sign test: the same values and gradients
            xk, keep = x.clone().requires_grad_(), copy.deepcopy(mine)
            again = tb.batchnorm_act_formula(xk, *_bn_args(keep)[:5], training, keep.momentum, keep.eps, resid=r if with_resid else None,
                                             mask=(want.detach() > 0).double())
            (gk,) = torch.autograd.grad(again, [xk], go)
            assert _rel(again.detach(), want.detach()) <= 1e-12 and _rel(gk, got_g[0]) <= 1e-12
    assert int(mine.num_batches_tracked) == int(bn.num_batches_tracked) == (2 if training else 0)
    assert _rel(mine.running_mean, bn.running_mean) <= 1e-12 and _rel(mine.running_var, bn.running_var) <= 1e-12
    with pytest.raises(ValueError):
        tb.batchnorm_act_formula(torch.zeros((1, C, 1, 1), dtype=torch.float64), *_bn_args(mine)[:5], True, 0.1, 1e-5)


# ---- 2: the swap contract ------------------------------------------------------------------------------------------------------
class _Block(nn.Module):
    """The attribute names of the reference's BasicBlock, none of its code."""
    def __init__(self, cin, cout, bn=True, shortcut="auto", **bn_kw):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, cout, 3, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(cout, **bn_kw) if bn else nn.Identity()
        self.conv2 = nn.Conv2d(cout, cout, 3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(cout, **bn_kw) if bn else nn.Identity()
        if shortcut == "auto":
            if cin != cout:
                self.shortcut = nn.Sequential(nn.Conv2d(cin, cout, 1, bias=False))
        elif shortcut is not None:
            self.shortcut = shortcut

    def forward(self, x, relu=True):
        s = self.shortcut(x) if hasattr(self, "shortcut") else x
        out = torch.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out)) + s
        return torch.relu(out) if relu else out


class _Att(nn.Module):
    def forward(self, x):
        return x


class _Head(nn.Module):
    def __init__(self):
        super().__init__()
        self.resblock1, self.resblock2, self.resblock3, self.resblock4 = _Block(64, 32), _Block(32, 32), _Block(32, 32), _Block(32, 64)
        self.xy_offset = nn.Conv2d(64, 2, 1, bias=False)
        self.att_layer = _Att()

    def forward(self, x):
        return torch.sigmoid(self.xy_offset(self.resblock4(self.att_layer(self.resblock3(self.resblock2(self.resblock1(x)))))))


class _Model(nn.Module):
    def __init__(self):
        super().__init__()
        self.head = _Head()
        self.empty_shortcut = _Block(32, 32, shortcut=nn.Sequential())
        self.eval_block = _Block(32, 16).eval()
        # left alone
        self.no_bn = _Block(32, 32, bn=False)                                                       # the config's BN: False
        self.cumulative = _Block(32, 32, momentum=None)
        self.no_affine = _Block(32, 32, affine=False)
        self.no_stats = _Block(32, 32, track_running_stats=False)
        self.odd_width = _Block(32, 6)
        self.wide = _Block(32, 1028)
        self.bn_shortcut = _Block(32, 16, shortcut=nn.Sequential(nn.Conv2d(32, 16, 1, bias=False), nn.BatchNorm2d(16)))
        self.biased_shortcut = _Block(32, 16, shortcut=nn.Sequential(nn.Conv2d(32, 16, 1, bias=True)))
        self.strided_shortcut = _Block(32, 16, shortcut=nn.Sequential(nn.Conv2d(32, 16, 1, stride=2, bias=False)))
        self.narrow_shortcut = _Block(32, 8)                                                        # Cout % 16 != 0
        self.bare_shortcut = _Block(32, 16, shortcut=nn.Conv2d(32, 16, 1, bias=False))              # no nn.Sequential
        self.fp64 = _Block(32, 32).double()
        self.half_block = nn.Sequential(nn.Conv2d(32, 32, 3, padding=1, bias=False), nn.BatchNorm2d(32))   # no conv2 / bn2


_TAKEN = ("head.resblock1", "head.resblock2", "head.resblock3", "head.resblock4", "empty_shortcut", "eval_block")
_LEFT_ALONE = ("no_bn", "cumulative", "no_affine", "no_stats", "odd_width", "wide", "bn_shortcut", "biased_shortcut", "strided_shortcut",
               "narrow_shortcut", "bare_shortcut", "fp64")


def test_swap_contract():
    from mickey_amd import train_block as tb
    m = _Model()
    keys = list(m.state_dict().keys())
    params = {n: id(p) for n, p in m.named_parameters()}
    buffers = {n: id(b) for n, b in m.named_buffers()}
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)                       # made before the swap
    children = {n: dict(m.get_submodule(n)._modules) for n in _TAKEN}
    assert tb.use_hip_blocks(m) == len(_TAKEN)
    for name in _TAKEN:
        blk = m.get_submodule(name)
        assert type(blk) is tb.HipBasicBlock, name
        assert list(blk._modules) == list(children[name])
        for cname, child in children[name].items():
            assert blk._modules[cname] is child, (name, cname)
    assert m.head.resblock1.training and not m.eval_block.training and not m.eval_block.bn1.training
    for name in _LEFT_ALONE:
        assert type(m.get_submodule(name)) is _Block, name
    assert type(m.half_block) is nn.Sequential
    assert list(m.state_dict().keys()) == keys
    assert {n: id(p) for n, p in m.named_parameters()} == params and {n: id(b) for n, b in m.named_buffers()} == buffers
    assert {id(p) for grp in opt.param_groups for p in grp["params"]} == set(params.values())
    assert tb.use_hip_blocks(m) == 0                                      # a second call finds none
    m.load_state_dict(_Model().state_dict(), strict=True)
    m.head.eval()
    assert not children["head.resblock1"]["bn1"].training
    m.head.train()
    assert children["head.resblock1"]["bn1"].training
    import inspect
    assert "relu" in inspect.signature(m.head.resblock4.forward).parameters   # HipHead may pass it


def test_swap_composes_with_the_other_use_hip_calls():
    import mickey_amd
    from mickey_amd import train_block as tb, train_heads as th, train_tails as tt
    calls = (tb.use_hip_blocks, th.use_hip_convs, tt.use_hip_tails)
    for order in ((0, 1, 2), (2, 1, 0), (1, 0, 2)):
        m = _Model()
        keys = list(m.state_dict().keys())
        params = {n: id(p) for n, p in m.named_parameters()}
        counts = {i: calls[i](m) for i in order}
        assert counts[0] == len(_TAKEN) and counts[2] == 1 and counts[1] > 0, counts
        assert list(m.state_dict().keys()) == keys and {n: id(p) for n, p in m.named_parameters()} == params
        assert type(m.head) is tt.HipHead and type(m.head.resblock2) is tb.HipBasicBlock and type(m.head.resblock2.conv1) is th.Conv3x3
        assert m.head.block4_takes_relu
        assert all(c(m) == 0 for c in calls)
    plain = mickey_amd.use_hip_training(_Model())
    assert list(plain) == ["use_hip_encoder", "use_hip_convs", "use_hip_encoder_layers", "use_hip_attention", "use_hip_tails", "use_hip_matcher"]
    m = _Model()
    assert mickey_amd.use_hip_training(m, blocks=False) == plain and not any(type(b) is tb.HipBasicBlock for b in m.modules())
    m = _Model()
    got = mickey_amd.use_hip_training(m, blocks=True)
    assert got == dict(plain, use_hip_blocks=len(_TAKEN)) and list(got)[-1] == "use_hip_blocks"
    assert mickey_amd.use_hip_training(m, blocks=True) == dict.fromkeys(got, 0)
    with pytest.raises(TypeError):
        mickey_amd.use_hip_training(m, blocks=True, block=True)


# ---- 3: argument checks --------------------------------------------------------------------------------------------------------
class _Boom:
    """stands in for the library: any touch fails the test"""
    def __getattr__(self, name):
        raise AssertionError("the library was touched (%s) before the arguments were checked" % name)


def test_bad_arguments_raise_before_anything_touches_the_library(monkeypatch):
    from mickey_amd import _native, ops, train_block as tb
    C = 8
    x, w, b, rm, rv, n = torch.zeros(2, C, 3, 4), torch.ones(C), torch.zeros(C), torch.zeros(C), torch.ones(C), torch.zeros((), dtype=torch.int64)

    def bn(x=x, w=w, b=b, rm=rm, rv=rv, n=n, training=True, momentum=0.1, eps=1e-5, **kw):
        return tb.batchnorm_act_train(x, w, b, rm, rv, n, training, momentum, eps, **kw)
    w1 = torch.zeros(16, 32, 1, 1)
    x1 = torch.zeros(2, 32, 3, 4)
    for call in (bn, lambda: bn(training=False), lambda: bn(resid=x, relu=False), lambda: tb.conv1x1_train(x1, w1)):
        with pytest.raises(_native.MickeyHipError):     # well-formed CPU tensors: no CPU fallback
            call()
    monkeypatch.setattr(_native, "load", lambda: _Boom())
    monkeypatch.setattr(_native, "_lib", None)
    monkeypatch.setattr(ops, "call", lambda *a: _Boom().call)
    monkeypatch.setattr(ops, "query", lambda *a: _Boom().query)
    bad = [dict(x=x.half()), dict(x=x.double()), dict(x=x.bfloat16()), dict(x=x[0]), dict(x=x[None]), dict(x=x.numpy()),
           dict(x=torch.zeros(2, 6, 3, 4), w=torch.ones(6), b=torch.ones(6), rm=torch.ones(6), rv=torch.ones(6)),    # C % 4
           dict(x=torch.zeros(2, 1028, 3, 4), w=torch.ones(1028), b=torch.ones(1028), rm=torch.ones(1028), rv=torch.ones(1028)),
           dict(x=torch.zeros(0, C, 3, 4)), dict(x=torch.zeros(2, C, 0, 4)),
           dict(x=torch.zeros(1, C, 1, 1)),                                                                           # one value per channel
           dict(w=torch.ones(C + 4)), dict(b=b.double()), dict(rm=torch.zeros(C, 1)), dict(rv=rv.half()), dict(w=None),
           dict(n=torch.zeros(())), dict(n=torch.zeros(2, dtype=torch.int64)), dict(n=0),
           dict(resid=torch.zeros(2, C, 4, 3)), dict(resid=x.double()), dict(resid=x[:1]),
           dict(training=1), dict(training=None),
           dict(momentum=None), dict(momentum=-0.1), dict(momentum=float("nan")), dict(momentum="0.1"), dict(momentum=True),
           dict(eps=-1e-5), dict(eps=float("inf")), dict(eps=None)]
    for kw in bad:
        with pytest.raises(ValueError):
            bn(**kw)
    bn_eval_one = dict(x=torch.zeros(1, C, 1, 1), training=False)     # eval takes a single value per channel: only the device is wrong
    with pytest.raises(_native.MickeyHipError):
        bn(**bn_eval_one)
    for xx, ww in ((x1.half(), w1), (x1, w1.double()), (x1[0], w1), (x1, w1[:, :, 0]), (x1, torch.zeros(16, 32, 3, 3)),
                   (torch.zeros(2, 16, 3, 4), w1), (torch.zeros(2, 24, 3, 4), torch.zeros(16, 24, 1, 1)), (x1, torch.zeros(8, 32, 1, 1)),
                   (x1.numpy(), w1), (torch.zeros(0, 32, 3, 4), w1)):
        with pytest.raises(ValueError):
            tb.conv1x1_train(xx, ww)


# ---- 4: the C ABI ----------------------------------------------------------------------------------------------------------------
def test_abi_of_the_new_entry_points(nv):
    lib = nv.load()
    raw = open(os.path.join(ROOT, "include", "mickey_hip.h")).read()
    declared = set(re.findall(r"\b(mk_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", raw, flags=re.S)))
    for name in NEW_SYMBOLS:
        assert name in declared and name in nv.SIGNATURES and hasattr(lib, name), name
    assert nv.missing_symbols() == []
    decl = raw.index("int mk_train_bn_chunk_rows(")
    doc = raw[raw.rfind("/*", 0, decl):decl]
    for cite in ("utils/extractor_utils.py:12-35", "extractor_utils.py:19,21", ":32", ":30,33-34", ":23-26,29",
                 "mickey_extractor.py:76-79,155-158,194-197,232-235"):
        assert cite in doc, cite
    from mickey_amd import ops
    for name in ("train_bn_fwd", "train_bn_bwd", "bn_chunks"):
        assert callable(getattr(ops, name))
    q = nv.query
    R = ops.BN_CHUNK_ROWS
    assert q("mk_train_bn_chunk_rows") == R and R % 16 == 0
    for rows, chunks in ((1, 1), (R - 1, 1), (R, 1), (R + 1, 2), (2 * R + 1, 3), (3876, -(-3876 // R)), (24 * 1938, -(-24 * 1938 // R)), (0, 0), (-5, 0)):
        assert q("mk_train_bn_chunks", rows) == chunks == ops.bn_chunks(rows), rows
        assert q("mk_train_bn_work_floats", rows, 64) == chunks * 8 * 64
    one = 16   # any non-null, aligned address: argument checks come before every launch and never touch it

    def fwd(**kw):
        a = dict(dict(x=one, ldx=64, gamma=one, beta=one, resid=one, ldr=64, rm=one, rv=one, nbt=one, mom=0.1, eps=1e-5, work=one, y=one, ldy=64,
                      mean=one, rstd=one, mask=one, M=100, C=64, relu=1, training=1), **kw)
        return lib.mk_train_bn_fwd(a["x"], a["ldx"], a["gamma"], a["beta"], a["resid"], a["ldr"], a["rm"], a["rv"], a["nbt"], a["mom"], a["eps"],
                                   a["work"], a["y"], a["ldy"], a["mean"], a["rstd"], a["mask"], a["M"], a["C"], a["relu"], a["training"], None)
    for bad in (dict(x=None), dict(gamma=None), dict(beta=None), dict(y=None), dict(rm=None), dict(rv=None), dict(nbt=None), dict(work=None),
                dict(x=8), dict(y=4), dict(resid=24), dict(mask=8), dict(work=4), dict(gamma=4),
                dict(M=0), dict(M=-1), dict(M=1), dict(C=0), dict(C=6), dict(C=2), dict(C=1028), dict(ldx=60), dict(ldx=66), dict(ldy=32),
                dict(ldr=63), dict(eps=-1.0), dict(eps=float("nan")), dict(mom=-0.5), dict(mom=float("inf")), dict(relu=0)):
        assert fwd(**bad) == 1, bad
        assert b"mk_train_bn_fwd" in lib.mk_last_error()
    assert fwd(M=0, training=0) == 1 and fwd(C=6, training=0) == 1 and fwd(rm=None, training=0) == 1

    def bwd(**kw):
        a = dict(dict(g=one, ldg=64, x=one, ldx=64, gamma=one, mean=one, rstd=one, mask=one, work=one, gx=one, ldgx=64, gresid=one, ldgr=64,
                      dgamma=one, dbeta=one, eps=1e-5, M=100, C=64, training=1), **kw)
        return lib.mk_train_bn_bwd(a["g"], a["ldg"], a["x"], a["ldx"], a["gamma"], a["mean"], a["rstd"], a["mask"], a["work"], a["gx"], a["ldgx"],
                                   a["gresid"], a["ldgr"], a["dgamma"], a["dbeta"], a["eps"], a["M"], a["C"], a["training"], None)
    for bad in (dict(g=None), dict(x=None), dict(gamma=None), dict(mean=None), dict(rstd=None), dict(work=None), dict(g=8), dict(gx=4),
                dict(gresid=8), dict(mask=4), dict(M=0), dict(M=1), dict(C=6), dict(C=0), dict(C=1028), dict(ldg=62), dict(ldx=32),
                dict(ldgx=66), dict(ldgr=60), dict(eps=-1.0), dict(eps=float("nan"))):
        assert bwd(**bad) == 1, bad
        assert b"mk_train_bn_bwd" in lib.mk_last_error()
    assert bwd(gx=None, gresid=None, dgamma=None, dbeta=None) == 0      # nothing wanted: nothing launched
