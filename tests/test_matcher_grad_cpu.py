"""The differentiable dual-softmax matcher without a GPU: the backward's formulas (mk_matcher_bwd.hip) against torch autograd of
the reference formula in fp64, the golden file, the ABI's argument checks and the Python layer's validation / module contract."""
import ctypes
import os

import numpy as np
import pytest
import torch

from mickey_amd import _native
from mickey_amd.train_matcher import DualSoftmax, dual_softmax_train, use_hip_matcher
from tests.helpers import matcher_refs as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "matcher_grad.npz")
MK_ERR_INVALID_ARGUMENT = 1


def ref_final(d0, d1, s0, s1, dustbin, temperature):
    """the reference formula: dualSoftmax (feature_matcher.py:64-83) x kp_matrix_scores (compute_correspondences.py:46-50)"""
    S = torch.matmul(d0.transpose(1, 2), d1) / temperature
    if dustbin is not None:
        B, m, n = S.shape
        Z = torch.cat([torch.cat([S, dustbin.expand(B, m, 1)], -1), torch.cat([dustbin.expand(B, 1, n), dustbin.expand(B, 1, 1)], -1)], 1)
        P = (torch.softmax(Z, 1) * torch.softmax(Z, 2))[:, :-1, :-1]
    else:
        P = torch.softmax(S, 1) * torch.softmax(S, 2)
    return P if s0 is None else P * torch.matmul(s0.transpose(1, 2), s1)


def formula_grads(d0, d1, s0, s1, dustbin, temperature, G):
    """tests/helpers/matcher_refs.py::formula_grads as the five gradients autograd returns: the dustbin's summed over the pairs"""
    g = R.formula_grads(d0, d1, s0, s1, dustbin, temperature, G)["g"]
    return g[:4] + [g[4].sum() if g[4] is not None else None]


def rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-300))


@pytest.mark.parametrize("dustbin", [None, 1.3])
@pytest.mark.parametrize("scores", [False, True])
def test_formulas_equal_autograd_fp64(dustbin, scores):
    g = torch.Generator().manual_seed(1 + scores + 2 * (dustbin is not None))
    B, C, n0, n1, T = 2, 16, 37, 29, 0.1
    d0, d1 = torch.randn((B, C, n0), generator=g, dtype=torch.float64), torch.randn((B, C, n1), generator=g, dtype=torch.float64)
    d0, d1 = d0 / d0.norm(dim=1, keepdim=True), d1 / d1.norm(dim=1, keepdim=True)
    s0 = torch.rand((B, 1, n0), generator=g, dtype=torch.float64) if scores else None
    s1 = torch.rand((B, 1, n1), generator=g, dtype=torch.float64) if scores else None
    if scores:
        s0[:, :, :3] = 0.0   # border keypoints: exactly zero scores
        s1[:, :, -2:] = 0.0
    a = torch.tensor(dustbin, dtype=torch.float64) if dustbin is not None else None
    G = torch.randn((B, n0, n1), generator=g, dtype=torch.float64)
    x = [t.clone().requires_grad_() if t is not None else None for t in (d0, d1, s0, s1, a)]
    ref_final(x[0], x[1], x[2], x[3], x[4], T).backward(G)
    got = formula_grads(d0, d1, s0, s1, a, T, G)
    for k, (mine, t) in enumerate(zip(got, x)):
        if t is None:
            assert mine is None
            continue
        assert rel(mine, t.grad) <= 1e-12, (k, rel(mine, t.grad))


def test_golden_file_is_self_consistent():
    z = np.load(GOLD)
    assert os.path.getsize(GOLD) < 1 << 20
    d0, d1, s0, s1, G = (torch.from_numpy(z[k]) for k in ("dsc0", "dsc1", "scr0", "scr1", "G"))
    B, C, n0 = d0.shape
    n1 = d1.shape[2]
    assert (C, tuple(d1.shape), tuple(s0.shape), tuple(s1.shape), tuple(G.shape)) == (128, (B, C, n1), (B, 1, n0), (B, 1, n1), (B, n0, n1))
    assert torch.allclose(d0.double().norm(dim=1), torch.ones(B, n0, dtype=torch.float64), atol=1e-6)
    assert bool((s0[:, :, :7] == 0).all()) and bool((s1[:, :, -5:] == 0).all())   # the zero border scores are in
    T = float(z["temperature"])
    for tag, db in (("nodb", None), ("db", torch.tensor(float(z["dustbin"]), dtype=torch.float64))):
        dd = [t.double() for t in (d0, d1, s0, s1)]
        final = ref_final(dd[0], dd[1], dd[2], dd[3], db, T)
        got = formula_grads(dd[0], dd[1], dd[2], dd[3], db, T, G.double() / (final + 1e-16))
        names = ["dsc0", "dsc1", "scr0", "scr1"] + (["dustbin"] if db is not None else [])
        for k, mine in zip(names, got):
            stored = torch.from_numpy(z["g_%s_%s" % (k, tag)])
            assert stored.shape == (mine.shape if k != "dustbin" else ())
            # the fixture is the reference's fp32 autograd; this is fp64
            assert rel(mine, stored) <= 1e-4, (tag, k, rel(mine, stored))


def test_native_symbols_complete():
    assert "mk_dual_softmax_train" in _native.SIGNATURES and "mk_dual_softmax_bwd" in _native.SIGNATURES
    assert _native.missing_symbols() == []


def _p(v):
    return ctypes.c_void_p(v) if v else None


FAKE = 0x100000   # never dereferenced: every call below fails its argument checks before any launch


@pytest.mark.parametrize("bad", ["dsc0", "lse", "work", "outputs", "C", "B", "n0", "split_T", "unaligned"])
def test_train_abi_rejects_without_launching(bad):
    a = dict(dsc0=FAKE, dsc1=FAKE, scr0=0, scr1=0, invT=10.0, db=0, scores=FAKE, kp=0, fin=0, lse=FAKE, work=FAKE, B=2, C=128,
             n0=10, n1=12, split=0)
    if bad == "outputs":
        a["scores"] = 0
    elif bad == "split_T":
        a.update(split=1, invT=100.0)
    elif bad == "unaligned":
        a["work"] = FAKE + 4
    elif bad in ("C", "B", "n0"):
        a[bad] = 64 if bad == "C" else 0
    else:
        a[bad] = 0
    lib = _native.load()
    rc = lib.mk_dual_softmax_train(_p(a["dsc0"]), _p(a["dsc1"]), _p(a["scr0"]), _p(a["scr1"]), a["invT"], _p(a["db"]),
                                   _p(a["scores"]), _p(a["kp"]), _p(a["fin"]), _p(a["lse"]), _p(a["work"]), a["B"], a["C"], a["n0"],
                                   a["n1"], a["split"], None)
    assert rc == MK_ERR_INVALID_ARGUMENT, lib.mk_last_error()


@pytest.mark.parametrize("bad", ["dsc1", "G", "lse", "work", "C", "n1", "scr_pair", "g_scr", "g_dustbin", "split_T", "unaligned"])
def test_bwd_abi_rejects_without_launching(bad):
    a = dict(dsc0=FAKE, dsc1=FAKE, scr0=0, scr1=0, invT=10.0, db=0, lse=FAKE, G=FAKE, g0=FAKE, g1=FAKE, gs0=0, gs1=0, gd=0,
             work=FAKE, B=2, C=128, n0=10, n1=12, split=0)
    if bad == "scr_pair":
        a["scr0"] = FAKE
    elif bad == "g_scr":
        a["gs0"] = FAKE
    elif bad == "g_dustbin":
        a["gd"] = FAKE
    elif bad == "split_T":
        a.update(split=1, invT=100.0)
    elif bad == "unaligned":
        a["work"] = FAKE + 8
    elif bad in ("C", "n1"):
        a[bad] = 96 if bad == "C" else -1
    else:
        a[bad] = 0
    lib = _native.load()
    rc = lib.mk_dual_softmax_bwd(_p(a["dsc0"]), _p(a["dsc1"]), _p(a["scr0"]), _p(a["scr1"]), a["invT"], _p(a["db"]), _p(a["lse"]),
                                 _p(a["G"]), _p(a["g0"]), _p(a["g1"]), _p(a["gs0"]), _p(a["gs1"]), _p(a["gd"]), _p(a["work"]), a["B"],
                                 a["C"], a["n0"], a["n1"], a["split"], None)
    assert rc == MK_ERR_INVALID_ARGUMENT, lib.mk_last_error()


def test_work_sizes():
    lib = _native.load()
    assert lib.mk_dual_softmax_train_work_floats(8, 1938, 1938, 1) == lib.mk_dual_softmax_split_work_floats(8, 1938, 1938)
    assert lib.mk_dual_softmax_train_work_floats(8, 1938, 1938, 0) == lib.mk_dual_softmax_work_floats(8, 1938, 1938, 0)
    split, exact = lib.mk_dual_softmax_bwd_work_floats(8, 1938, 1938, 1), lib.mk_dual_softmax_bwd_work_floats(8, 1938, 1938, 0)
    assert split > exact > 0 and split % 4 == 0 and exact % 4 == 0


def _d(*shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype)


@pytest.mark.parametrize("case", ["C", "dim", "B", "C_mismatch", "dtype", "scr_alone", "scr_shape", "scr_dtype", "temperature",
                                  "dustbin", "split", "not_tensor", "cpu"])
def test_dual_softmax_train_raises_value_error(case):
    d0, d1, s0, s1, kw = _d(2, 128, 10), _d(2, 128, 12), None, None, {}
    if case == "C":
        d0, d1 = _d(2, 64, 10), _d(2, 64, 12)
    elif case == "dim":
        d0 = _d(128, 10)
    elif case == "B":
        d1 = _d(3, 128, 12)
    elif case == "C_mismatch":
        d1 = _d(2, 127, 12)
    elif case == "dtype":
        d0 = _d(2, 128, 10, dtype=torch.float16)
    elif case == "scr_alone":
        s0 = _d(2, 10)
    elif case == "scr_shape":
        s0, s1 = _d(2, 11), _d(2, 12)
    elif case == "scr_dtype":
        s0, s1 = _d(2, 10, dtype=torch.float64), _d(2, 12, dtype=torch.float64)
    elif case == "temperature":
        kw["temperature"] = 0.0
    elif case == "dustbin":
        kw["dustbin"] = _d(2)
    elif case == "split":
        kw["split"] = "yes"
    elif case == "not_tensor":
        d0 = np.zeros((2, 128, 10), np.float32)
    with pytest.raises(ValueError):
        dual_softmax_train(d0, d1, s0, s1, **kw)


def test_dual_softmax_module_raises_value_error():
    m = DualSoftmax({"TEMPERATURE": 0.1, "USE_DUSTBIN": True})
    with pytest.raises(ValueError):
        m(_d(2, 128, 10), _d(2, 64, 12))
    with pytest.raises(ValueError):
        m(_d(2, 128), _d(2, 128, 12))


def test_dual_softmax_module_contract():
    """reference dualSoftmax(cfg) (feature_matcher.py:54-62): attributes, dustbin_score = 1.0, state_dict keys"""
    m = DualSoftmax({"TEMPERATURE": 0.1, "USE_DUSTBIN": True})
    assert m.temperature == 0.1 and m.use_dustbin is True
    assert isinstance(m.dustbin_score, torch.nn.Parameter) and m.dustbin_score.shape == () and float(m.dustbin_score.detach()) == 1.0
    assert list(m.state_dict()) == ["dustbin_score"]
    m2 = DualSoftmax({"TEMPERATURE": 0.05, "USE_DUSTBIN": False})
    assert m2.use_dustbin is False and list(m2.state_dict()) == [] and not hasattr(m2, "dustbin_score")


class _StandIn(torch.nn.Module):
    def __init__(self, use_dustbin):
        super().__init__()
        self.temperature = 0.1
        self.use_dustbin = False
        if use_dustbin:
            self.dustbin_score = torch.nn.Parameter(torch.tensor(1.))
            self.use_dustbin = True


class _SinkhornLike(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.dustbin_score = torch.nn.Parameter(torch.tensor(1.))
        self.sinkhorn_iterations = 20


def test_use_hip_matcher_swaps_by_contract():
    model = torch.nn.Module()
    model.a = torch.nn.Module()
    model.a.matching_mat = _StandIn(True)
    model.b = torch.nn.Module()
    model.b.matching_mat = _StandIn(False)
    model.c = torch.nn.Module()
    model.c.matching_mat = _SinkhornLike()
    p = model.a.matching_mat.dustbin_score
    keys = sorted(model.state_dict())
    assert use_hip_matcher(model) == 2
    assert isinstance(model.a.matching_mat, DualSoftmax) and model.a.matching_mat.dustbin_score is p
    assert isinstance(model.b.matching_mat, DualSoftmax) and not model.b.matching_mat.use_dustbin
    assert isinstance(model.c.matching_mat, _SinkhornLike)
    assert sorted(model.state_dict()) == keys
    assert use_hip_matcher(model) == 0
