"""mickey_amd.train_optim / train_step without a GPU: the formulas against torch.optim.Adam + clip_grad_norm_ in fp64, the chunk planner
as a pure host function, the host checks of HipAdam (all of them run before anything touches the library) and the C ABI of the new
entry points."""
import os
import re

import pytest
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mk_optim_chunk_elems", "mk_optim_chunks", "mk_optim_grad_stats", "mk_optim_reduce", "mk_optim_adam")


@pytest.fixture(scope="module")
def nv():
    from mickey_amd import build, _native
    if not os.path.exists(build.lib_path()):
        build.build(verbose=False)
    _native.load()
    return _native


# ---- 1: the formulas against torch, fp64 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("weight_decay", [0.0, 0.05])
def test_formulas_reproduce_torch_adam_and_clip_in_fp64(weight_decay):
    """three steps: one clipped, one not, one with a NaN gradient, which must change nothing (the reference's `return False`)"""
    from mickey_amd import train_optim as to
    g = torch.Generator().manual_seed(7)
    shapes = [(), (3,), (4, 5), (2, 3, 2, 2)]
    init = [torch.randn(s, generator=g, dtype=torch.float64) for s in shapes]
    ref = [nn.Parameter(t.clone()) for t in init]
    hyper = [dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-6, weight_decay=weight_decay)] * 2 + \
            [dict(lr=3e-3, betas=(0.8, 0.99), eps=1e-8, weight_decay=weight_decay)] * 2
    opt = torch.optim.Adam([dict(params=ref[:2], **hyper[0]), dict(params=ref[2:], **hyper[2])])
    ours = [t.clone() for t in init]
    state = [dict(step=0, exp_avg=torch.zeros_like(t), exp_avg_sq=torch.zeros_like(t)) for t in init]
    for kind, scale in (("clipped", 10.0), ("unclipped", 0.1), ("nan", 1.0), ("clipped", 7.0)):
        grads = [torch.randn(s, generator=g, dtype=torch.float64) * scale for s in shapes]
        if kind == "nan":
            grads[2][1, 2] = float("nan")
        for p, gr in zip(ref, grads):
            p.grad = gr.clone()
        norm = torch.nn.utils.clip_grad_norm_(ref, max_norm=5)
        bad = sum(bool(torch.isnan(p.grad).any()) for p in ref) != 0       # model.py:140-143
        if not bad:
            opt.step()
        mine = [gr.clone() for gr in grads]
        before = [t.clone() for t in ours]
        ok, total, coef = to.guarded_step_formula(ours, mine, state, hyper, max_norm=5)
        assert ok == (not bad)
        if kind == "nan":
            assert all(torch.equal(a, b) for a, b in zip(ours, before))
            assert all(torch.equal(a, b) for a, b in zip(mine[:2] + mine[3:], grads[:2] + grads[3:]))
            continue
        assert abs(total - float(norm)) <= 1e-13 * total
        assert (coef < 1.0) == (kind == "clipped")
        for i, p in enumerate(ref):
            torch.testing.assert_close(ours[i], p.detach(), rtol=1e-12, atol=1e-14)
            torch.testing.assert_close(mine[i], p.grad, rtol=1e-12, atol=0)
            torch.testing.assert_close(state[i]["exp_avg"], opt.state[p]["exp_avg"], rtol=1e-12, atol=1e-16)
            torch.testing.assert_close(state[i]["exp_avg_sq"], opt.state[p]["exp_avg_sq"], rtol=1e-12, atol=1e-16)
            assert state[i]["step"] == int(opt.state[p]["step"])
    assert [s["step"] for s in state] == [3] * 4


def test_formula_skips_on_also_finite_and_on_missing_gradients():
    from mickey_amd import train_optim as to
    p = [torch.ones(3, dtype=torch.float64), torch.ones(2, dtype=torch.float64)]
    state = [dict(step=0, exp_avg=torch.zeros(3, dtype=torch.float64), exp_avg_sq=torch.zeros(3, dtype=torch.float64)),
             dict(step=0, exp_avg=torch.zeros(2, dtype=torch.float64), exp_avg_sq=torch.zeros(2, dtype=torch.float64))]
    hyper = dict(lr=0.1, betas=(0.9, 0.999), eps=1e-8, weight_decay=0)
    grads = [torch.ones(3, dtype=torch.float64), None]
    for bad in (float("nan"), float("inf"), -float("inf")):
        ok, total, coef = to.guarded_step_formula(p, grads, state, hyper, max_norm=None, also_finite=(torch.tensor([0.0, bad]),))
        assert not ok and coef == 1.0 and torch.equal(p[0], torch.ones(3, dtype=torch.float64)) and state[0]["step"] == 0
    ok, total, coef = to.guarded_step_formula(p, grads, state, hyper, also_finite=(torch.zeros(2),))
    assert ok and abs(total - 3 ** 0.5) < 1e-15 and coef == 1.0
    assert state[0]["step"] == 1 and state[1]["step"] == 0 and torch.equal(p[1], torch.ones(2, dtype=torch.float64))
    torch.testing.assert_close(p[0], torch.full((3,), 0.9, dtype=torch.float64), rtol=1e-7, atol=0)   # the first Adam step is lr sign(g)
    grads[0] = torch.tensor([float("inf"), 0.0, 0.0], dtype=torch.float64)
    assert to.guarded_step_formula(p, grads, state, hyper)[0] is False and state[0]["step"] == 1


# ---- 2: the chunk planner -----------------------------------------------------------------------------------------------------------
def test_chunk_planner_covers_every_element_once(nv):
    from mickey_amd import train_optim as to
    E = to.CHUNK_ELEMS
    assert nv.query("mk_optim_chunk_elems") == E and E % 1024 == 0
    for numel, chunks in ((1, 1), (E - 1, 1), (E, 1), (E + 1, 2), (2 * E, 2), (2 * E + 3, 3), (0, 0), (-4, 0), (2 ** 33 + 1, 2 ** 33 // E + 1)):
        assert nv.query("mk_optim_chunks", numel) == chunks, numel
    for e in (4, 16, E):
        numels = [1, 3, e - 1, e, e + 1, 2 * e - 1, 2 * e, 2 * e + 1, 5 * e + 3, 1]
        plan = to.plan_chunks(numels, e)
        assert plan.dtype == torch.int32 and plan.shape == (sum(-(-n // e) for n in numels), 2)
        seen = [torch.zeros(n, dtype=torch.int32) for n in numels]
        for t, i in plan.tolist():
            assert 0 <= t < len(numels) and i * e < numels[t]          # no chunk starts past its tensor's end
            seen[t][i * e:min((i + 1) * e, numels[t])] += 1
        assert all(bool((s == 1).all()) for s in seen)
        assert plan[:, 0].tolist() == sorted(plan[:, 0].tolist())       # tensors in order: the parameters' chunks come first
        assert torch.equal(plan, to.plan_chunks(list(numels), e))       # a function of the counts alone
    assert [to._nchunks(n) for n in (1, E, E + 1)] == [1, 1, 2]
    for bad in ([0], [4, -1], []):
        if bad:
            with pytest.raises(ValueError):
                to.plan_chunks(bad)
    assert to.plan_chunks([], 4).shape == (0, 2)


def test_row_layout_matches_the_header():
    from mickey_amd import train_optim as to
    raw = open(os.path.join(ROOT, "include", "mickey_hip.h")).read()
    body = raw[raw.index("typedef struct mk_optim_row {"):raw.index("} mk_optim_row;")]
    assert re.sub(r"\s+", " ", body.split("{", 1)[1]).strip() == \
        "float *p, *g, *m, *v, *step; long long numel; double lr, beta1, beta2, eps, weight_decay; long long flags;"
    assert to._ROW.size == 96 and to.ROW_WORDS == 12
    assert "#define MK_OPTIM_NORM %d" % to.FLAG_NORM in raw and "#define MK_OPTIM_PARAM %d" % to.FLAG_PARAM in raw
    row = to._ROW.unpack(to._ROW.pack(1, 2, 3, 4, 5, 6, 0.5, 0.25, 0.125, 1e-6, 0.0, 3))
    assert row == (1, 2, 3, 4, 5, 6, 0.5, 0.25, 0.125, 1e-6, 0.0, 3)


# ---- 3: the host checks --------------------------------------------------------------------------------------------------------------
class _Boom:
    def __getattr__(self, name):
        raise AssertionError("the library was touched (%s) before the arguments were checked" % name)


def _param(t, grad=None):
    p = nn.Parameter(t)
    p.grad = grad
    return p


def test_bad_tensors_raise_before_anything_touches_the_library(monkeypatch):
    from mickey_amd import _native, train_optim as to
    monkeypatch.setattr(_native, "load", lambda: _Boom())
    monkeypatch.setattr(_native, "_lib", None)
    monkeypatch.setattr(_native, "call", lambda *a: _Boom().call)
    good = torch.zeros(4, 6)

    def step(p, guarded=True, **kw):
        opt = to.HipAdam([_param(torch.zeros(2)), p])       # parameter 0 has no gradient and is left out: the offender is parameter 1
        return opt.step_guarded(**kw) if guarded else opt.step()

    for guarded in (True, False):
        with pytest.raises(_native.MickeyHipError, match="parameter 1"):     # well-formed CPU tensors: no CPU fallback
            step(_param(good.clone(), good.clone()), guarded)
    wide = torch.zeros(4, 12)
    cl = torch.zeros(2, 4, 3, 3).contiguous(memory_format=torch.channels_last)
    bad = [_param(good.double(), good.double()),                             # not fp32
           _param(good.half(), good.half()),
           _param(wide[:, ::2], torch.zeros(4, 6)),                          # the parameter is not dense
           _param(good.clone(), wide[:, :6]),                                # the gradient is not dense
           _param(good.clone(), torch.zeros(6, 4).t()),                      # dense, but not in the parameter's order
           _param(cl.clone(memory_format=torch.preserve_format), torch.zeros(2, 4, 3, 3)),   # channels_last against contiguous
           _param(good.clone(), torch.zeros(4, 1).expand(4, 6)),             # overlapping
           _param(good.clone(), torch.zeros(4, 6).to_sparse())]              # sparse
    for i, p in enumerate(bad):
        with pytest.raises(ValueError, match="parameter 1"):
            step(p)
        with pytest.raises(ValueError, match="parameter 1"):
            step(p, guarded=False)
    # a channels_last pair is fine: only the device is wrong
    with pytest.raises(_native.MickeyHipError):
        step(_param(cl.clone(memory_format=torch.preserve_format), cl.clone(memory_format=torch.preserve_format)))
    # a parameter without a gradient is left out: with none at all nothing happens, and no state appears
    opt = to.HipAdam([_param(good.clone())])
    assert opt.step_guarded(max_norm=5) is None and opt.step() is None and len(opt.state) == 0
    # state tensors that somebody replaced
    for key, value in (("exp_avg", torch.zeros(6, 4).t()), ("exp_avg_sq", torch.zeros(4, 6, dtype=torch.float64)), ("exp_avg", torch.zeros(4, 5))):
        p = _param(good.clone(), good.clone())
        opt = to.HipAdam([p])
        opt.state[p] = dict(step=torch.zeros(1), exp_avg=torch.zeros(4, 6), exp_avg_sq=torch.zeros(4, 6))
        opt.state[p][key] = value
        with pytest.raises(ValueError, match="%s of parameter 0" % key):
            opt.step_guarded()
    # also_finite
    # also_finite (checked after the parameters, in order)
    for extra in (good.double(), wide[:, ::2], None, 3.0, torch.zeros(0), good.to_sparse()):
        with pytest.raises(ValueError, match=r"also_finite\[0\]"):
            to.HipAdam([_param(torch.zeros(2))]).step_guarded(also_finite=(extra,))
    with pytest.raises(_native.MickeyHipError, match=r"also_finite\[0\]"):
        to.HipAdam([_param(torch.zeros(2))]).step_guarded(also_finite=(good,))
    p = _param(good.clone(), good.clone())
    for max_norm in (-1.0, float("nan"), float("inf"), "5", True):
        with pytest.raises(ValueError, match="max_norm"):
            to.HipAdam([p]).step_guarded(max_norm=max_norm)


def test_bad_hyper_parameters_and_modes_raise():
    from mickey_amd import train_optim as to
    w = lambda: [_param(torch.zeros(3))]
    for kw in (dict(lr=-1e-3), dict(lr=float("nan")), dict(lr="1e-3"), dict(lr=torch.tensor(1e-3)), dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1)),
               dict(betas=0.9), dict(betas=(0.9, 0.99, 0.999)), dict(eps=-1e-8), dict(eps=None), dict(weight_decay=-0.1), dict(weight_decay=float("inf"))):
        with pytest.raises(ValueError):
            to.HipAdam(w(), **kw)
    opt = to.HipAdam(w())
    opt.param_groups[0]["lr"] = -1.0                                        # changed on the host after construction: seen at the next step
    opt.param_groups[0]["params"][0].grad = torch.zeros(3)
    with pytest.raises(ValueError, match="lr"):
        opt.step()
    for kw in (dict(amsgrad=True), dict(maximize=True), dict(capturable=True), dict(differentiable=True)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            to.HipAdam.from_torch(torch.optim.Adam(w(), **kw))
    with pytest.raises(ValueError, match="decoupled_weight_decay"):
        to.HipAdam.from_torch(torch.optim.AdamW(w()))
    with pytest.raises(ValueError):
        to.HipAdam.from_torch(torch.optim.SGD(w(), lr=0.1))
    sd = torch.optim.Adam(w(), amsgrad=True).state_dict()
    with pytest.raises(ValueError, match="amsgrad"):
        to.HipAdam(w()).load_state_dict(sd)


def test_optimizer_plumbing_on_the_host():
    """param groups, a scheduler, from_torch's adoption and the state_dict layout -- everything that needs no launch"""
    from mickey_amd import train_optim as to
    a, b = _param(torch.zeros(3)), _param(torch.zeros(2, 2))
    opt = to.HipAdam([dict(params=[a], lr=1e-2), dict(params=[b])], lr=1e-3, eps=1e-6)
    assert isinstance(opt, torch.optim.Optimizer)
    assert [g["lr"] for g in opt.param_groups] == [1e-2, 1e-3] and all(g["eps"] == 1e-6 for g in opt.param_groups)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    sched.step()
    assert [g["lr"] for g in opt.param_groups] == [5e-3, 5e-4]
    ref = torch.optim.Adam([dict(params=[a], lr=1e-2), dict(params=[b])], lr=1e-3, eps=1e-6)
    sd, rd = opt.state_dict(), ref.state_dict()
    assert sd["state"] == {} and [set(g) - {"initial_lr"} for g in sd["param_groups"]] == [set(g) for g in rd["param_groups"]]
    a.grad, b.grad = torch.ones(3), torch.ones(2, 2)
    ref.step()
    new = to.HipAdam.from_torch(ref)
    assert new.state[a]["exp_avg"] is ref.state[a]["exp_avg"] and new.state[b]["exp_avg_sq"] is ref.state[b]["exp_avg_sq"]
    assert [g["lr"] for g in new.param_groups] == [1e-2, 1e-3] and new.param_groups[0]["params"][0] is a
    out = new.state_dict()
    for k in (0, 1):
        s, r = out["state"][k], ref.state_dict()["state"][k]
        assert set(s) == set(r) and s["step"].shape == () and s["step"].dtype == torch.float32 and s["step"].device.type == "cpu"
        assert float(s["step"]) == 1.0 and torch.equal(s["exp_avg"], r["exp_avg"])
    ref2 = torch.optim.Adam([dict(params=[a], lr=1e-2), dict(params=[b])], lr=1e-3, eps=1e-6)
    ref2.load_state_dict(out)                                              # torch continues from ours
    ref2.step()
    assert float(ref2.state[a]["step"]) == 2.0
    back = to.HipAdam([dict(params=[a]), dict(params=[b])])
    back.load_state_dict(ref2.state_dict())                                 # and ours from torch's
    assert back.state[a]["step"].tolist() == [2.0] and back.param_groups[0]["lr"] == 1e-2
    assert torch.equal(back.state[b]["exp_avg"], ref2.state[b]["exp_avg"])


def test_backward_step_refuses_other_optimisers_and_returns_none_without_hypotheses():
    from mickey_amd import train_optim as to, train_step as ts
    p = _param(torch.ones(3), torch.ones(3))
    with pytest.raises(ValueError, match="HipAdam"):
        ts.backward_step(None, {}, {}, [None], None, 1, torch.optim.Adam([p]))
    opt = to.HipAdam([p])
    assert ts.backward_step(None, {}, {}, [None], None, 0, opt) is None      # model.py:97-99: nothing but zero_grad()
    assert p.grad is None and len(opt.state) == 0
    src = open(ts.__file__).read().split('"""', 2)[2] + open(to.__file__).read().split("class HipAdam", 1)[1].split("def state_dict", 1)[0]
    assert not re.search(r"\.any\(|\.item\(|bool\(|\.cpu\(|synchronize", src)


def test_the_three_kernels_use_no_scratch(nv):
    from mickey_amd import build
    kernels = build.resource_usage().get("mk_train_optim.hip")
    assert kernels is not None, "no resource report for mk_train_optim.hip: rebuild with `python -m mickey_amd.build --force`"
    names = [k["name"] for k in kernels]
    for want in ("optim_grad_stats_kernel", "optim_reduce_kernel", "optim_adam_kernel"):
        assert sum(want in n for n in names) == 1, (want, names)
    for k in kernels:
        assert k["scratch"] == 0 and k["sgpr_spill"] == 0 and k["vgpr_spill"] == 0, k


# ---- 4: the C ABI ----------------------------------------------------------------------------------------------------------------
def test_abi_of_the_new_entry_points(nv):
    lib = nv.load()
    raw = open(os.path.join(ROOT, "include", "mickey_hip.h")).read()
    declared = set(re.findall(r"\b(mk_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", raw, flags=re.S)))
    for name in NEW_SYMBOLS:
        assert name in declared and name in nv.SIGNATURES and hasattr(lib, name), name
    assert nv.missing_symbols() == []
    decl = raw.index("typedef struct mk_optim_row")
    doc = raw[raw.rfind("/*", 0, decl):decl]
    for cite in ("lib/models/MicKey/model.py:104-145", ":104-108", ":140", ":137", ":145"):
        assert cite in doc, cite
    one = 16   # any non-null, aligned address: argument checks come before every launch and never touch it

    def stats(**kw):
        a = dict(dict(table=one, rows=3, map=one, chunks=5, partials=one), **kw)
        return lib.mk_optim_grad_stats(a["table"], a["rows"], a["map"], a["chunks"], a["partials"], None)

    def reduce(**kw):
        a = dict(dict(partials=one, chunks=5, max_norm=5.0, state=one), **kw)
        return lib.mk_optim_reduce(a["partials"], a["chunks"], a["max_norm"], a["state"], None)

    def adam(**kw):
        a = dict(dict(table=one, rows=3, map=one, chunks=5, state=one), **kw)
        return lib.mk_optim_adam(a["table"], a["rows"], a["map"], a["chunks"], a["state"], None)

    common = (dict(table=None), dict(table=12), dict(rows=0), dict(rows=-1), dict(map=None), dict(map=18), dict(chunks=0), dict(chunks=-3))
    for fn, name, bads in ((stats, b"mk_optim_grad_stats", common + (dict(partials=None), dict(partials=24))),
                           (reduce, b"mk_optim_reduce", (dict(partials=None), dict(partials=24), dict(chunks=0), dict(chunks=-3), dict(state=None),
                                                         dict(state=8), dict(max_norm=float("nan")), dict(max_norm=float("inf")))),
                           (adam, b"mk_optim_adam", common + (dict(state=None), dict(state=24)))):
        for bad in bads:
            assert fn(**bad) == 1, (name, bad)
            assert name in lib.mk_last_error()
