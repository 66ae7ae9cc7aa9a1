"""The differentiable dual-softmax matcher on the GPU (mickey_amd.train_matcher: mk_dual_softmax_train / mk_dual_softmax_bwd):
gradients against fp64 torch autograd of the reference formula and against the reference's own autograd (golden file), the forward
against the inference matcher bit for bit, determinism, batch invariance, and the training step end to end."""
import os

import numpy as np
import pytest
import torch

from mickey_amd import ops
from mickey_amd.train_matcher import DualSoftmax, dual_softmax_train, use_hip_matcher

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = 0.1
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "matcher_grad.npz")


def rel_pairs(a, b):
    """largest per-pair relative Frobenius error"""
    a, b = a.detach().double().reshape(a.shape[0], -1), b.detach().double().reshape(b.shape[0], -1)
    return float(((a - b).norm(dim=1) / (b.norm(dim=1) + 1e-300)).max())


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / (b.norm() + 1e-300))


def ref_final(d0, d1, s0, s1, dustbin, temperature=T):
    """the reference formula (feature_matcher.py:64-83 x compute_correspondences.py:46-50) in whatever dtype it is given"""
    S = torch.matmul(d0.transpose(1, 2), d1) / temperature
    if dustbin is not None:
        B, m, n = S.shape
        Z = torch.cat([torch.cat([S, dustbin.expand(B, m, 1)], -1), torch.cat([dustbin.expand(B, 1, n), dustbin.expand(B, 1, 1)], -1)], 1)
        P = (torch.softmax(Z, 1) * torch.softmax(Z, 2))[:, :-1, :-1]
    else:
        P = torch.softmax(S, 1) * torch.softmax(S, 2)
    if s0 is None:
        return P
    return P * torch.matmul(s0.transpose(1, 2), s1)


def make_inputs(B, n0, n1, seed, dev=DEV):
    g = torch.Generator().manual_seed(seed)
    d0 = torch.randn((B, 128, n0), generator=g)
    d1 = torch.randn((B, 128, n1), generator=g)
    d0, d1 = d0 / d0.norm(dim=1, keepdim=True), d1 / d1.norm(dim=1, keepdim=True)
    s0 = torch.softmax(torch.randn((B, 1, n0), generator=g), -1)
    s1 = torch.softmax(torch.randn((B, 1, n1), generator=g), -1)
    s0[:, :, :3] = 0.0   # border keypoints: exact zeros (remove_brd_and_softmax)
    s1[:, :, -2:] = 0.0
    return [t.to(dev) for t in (d0, d1, s0, s1)], g


def hip_grads(d0, d1, s0, s1, dustbin, G, split):
    x = [t.clone().requires_grad_() for t in (d0, d1)]
    sc = [t.clone().requires_grad_() for t in (s0, s1)] if s0 is not None else [None, None]
    db = torch.tensor(dustbin, device=DEV, requires_grad=True) if dustbin is not None else None
    out = dual_softmax_train(x[0], x[1], sc[0], sc[1], T, db, split=split)
    out.backward(G)
    return [x[0].grad, x[1].grad, sc[0].grad if sc[0] is not None else None, sc[1].grad if sc[1] is not None else None,
            db.grad if db is not None else None]


def fp64_grads(d0, d1, s0, s1, dustbin, G):
    x = [t.double().requires_grad_() for t in (d0, d1)]
    sc = [t.double().requires_grad_() for t in (s0, s1)] if s0 is not None else [None, None]
    db = torch.tensor(dustbin, device=DEV, dtype=torch.float64, requires_grad=True) if dustbin is not None else None
    out = ref_final(x[0], x[1], sc[0], sc[1], db)
    out.backward(G.double())
    return out.detach(), [x[0].grad, x[1].grad, sc[0].grad if sc[0] is not None else None,
                          sc[1].grad if sc[1] is not None else None, db.grad if db is not None else None]


def check(got, want, tag):
    errs = {}
    for k, a, b, tol in zip(("dsc0", "dsc1", "scr0", "scr1", "dustbin"), got, want, (1e-4, 1e-4, 1e-5, 1e-5, 1e-4)):
        if b is None:
            assert a is None, k
            continue
        assert bool(torch.isfinite(a).all()), k
        errs[k] = rel_pairs(a, b) if k != "dustbin" else rel(a, b)
        assert errs[k] <= tol, (tag, k, errs[k])
    print("GRADERR", tag, " ".join("%s=%.2e" % kv for kv in errs.items()))


def reinforce_G(final, g):
    """nonzero at ~20 x 2048 sampled cells per pair (with repeats, as REINFORCE's counts), divided by final + 1e-16"""
    B, n0, n1 = final.shape
    G = torch.zeros(B * n0 * n1, dtype=torch.float64)
    cells = torch.randint(0, n0 * n1, (B, 20 * 2048), generator=g) + (torch.arange(B) * n0 * n1)[:, None]
    G.index_add_(0, cells.reshape(-1), torch.randn(cells.numel(), generator=g, dtype=torch.float64))
    return (G.reshape(B, n0, n1).to(DEV) / (final + 1e-16)).float()


@pytest.mark.parametrize("n0,n1", [(77, 130), (196, 196), (1938, 1938)])
@pytest.mark.parametrize("dustbin", [None, 1.0])
@pytest.mark.parametrize("scores", [False, True])
@pytest.mark.parametrize("gkind", ["dense", "reinforce"])
def test_grad_vs_fp64(n0, n1, dustbin, scores, gkind):
    (d0, d1, s0, s1), g = make_inputs(2, n0, n1, seed=n0 * 7 + n1 + (dustbin is not None) * 3 + scores)
    if not scores:
        s0 = s1 = None
    with torch.no_grad():
        final64 = ref_final(d0.double(), d1.double(), s0.double() if scores else None, s1.double() if scores else None,
                            torch.tensor(dustbin, device=DEV, dtype=torch.float64) if dustbin is not None else None)
    G = torch.randn((2, n0, n1), generator=g).to(DEV) if gkind == "dense" else reinforce_G(final64, g)
    _, want = fp64_grads(d0, d1, s0, s1, dustbin, G)
    for split in (True, False):
        got = hip_grads(d0, d1, s0, s1, dustbin, G, split)
        check(got, want, "%dx%d db=%s scores=%s G=%s split=%s" % (n0, n1, dustbin, scores, gkind, split))


def test_golden_reference_autograd():
    """tests/golden/matcher_grad.npz: the reference's own dualSoftmax x kp_matrix_scores, log(. + 1e-16), backward (fp32, CPU)"""
    z = np.load(GOLD)
    d0, d1, s0, s1, G = (torch.from_numpy(z[k]).to(DEV) for k in ("dsc0", "dsc1", "scr0", "scr1", "G"))
    for tag, db in (("nodb", None), ("db", float(z["dustbin"]))):
        for split in (True, False):
            x = [t.clone().requires_grad_() for t in (d0, d1, s0, s1)]
            dbt = torch.tensor(db, device=DEV, requires_grad=True) if db is not None else None
            final = dual_softmax_train(x[0], x[1], x[2], x[3], float(z["temperature"]), dbt, split=split)
            torch.autograd.backward(torch.log(final + 1e-16), G)
            errs = {k: rel(t.grad, torch.from_numpy(z["g_%s_%s" % (k, tag)]).to(DEV))
                    for k, t in zip(("dsc0", "dsc1", "scr0", "scr1"), x)}
            if dbt is not None:
                errs["dustbin"] = rel(dbt.grad, torch.from_numpy(z["g_dustbin_db"]).to(DEV))
            print("GOLDEN", tag, "split=%s" % split, " ".join("%s=%.2e" % kv for kv in errs.items()))
            assert all(e <= 1e-4 for e in errs.values()), errs


@pytest.mark.parametrize("n0,n1", [(77, 130), (196, 196), (1938, 1938)])
@pytest.mark.parametrize("split", [True, False])
def test_forward_equals_inference_matcher(n0, n1, split):
    (d0, d1, s0, s1), _ = make_inputs(2, n0, n1, seed=5)
    for dustbin in (None, 1.0):
        ref_scores, _, ref_fin = ops.dual_softmax(d0, d1, s0.reshape(2, n0).contiguous(), s1.reshape(2, n1).contiguous(), T, dustbin,
                                                  want_kp=False, split=split)
        db = torch.tensor(dustbin, device=DEV) if dustbin is not None else None
        fin = dual_softmax_train(d0, d1, s0, s1, T, db, split=split)
        scores = dual_softmax_train(d0, d1, None, None, T, db, split=split)
        assert torch.equal(fin, ref_fin) and torch.equal(scores, ref_scores)


@pytest.mark.parametrize("split", [True, False])
def test_deterministic_and_batch_invariant(split):
    n0, n1 = 301, 257
    (d0, d1, s0, s1), g = make_inputs(9, n0, n1, seed=11)
    G = torch.randn((9, n0, n1), generator=g).to(DEV)
    a = hip_grads(d0, d1, s0, s1, 0.7, G, split)
    b = hip_grads(d0, d1, s0, s1, 0.7, G, split)
    assert all(torch.equal(x, y) for x, y in zip(a, b))          # two backward runs: bit-identical
    four = hip_grads(d0[:4], d1[:4], s0[:4], s1[:4], 0.7, G[:4], split)
    for B, full in ((4, four), (9, a)):   # B = 4 (one unit per pair spread over the chip) and B = 9 (XCD-grouped grid)
        for p in range(B):
            one = hip_grads(d0[p:p + 1], d1[p:p + 1], s0[p:p + 1], s1[p:p + 1], 0.7, G[p:p + 1], split)
            for k in range(4):
                assert torch.equal(full[k][p], one[k][0]), (B, p, k)
    # the dustbin gradient: per pair values summed by the caller -- pair b's contribution is that of the pair alone
    gz = hip_grads(d0[:4], d1[:4], s0[:4], s1[:4], 0.7, torch.zeros_like(G[:4]), split)
    for t in gz:
        assert bool((t == 0).all())                                # G = 0: exact zeros


def test_dustbin_per_pair_values_batch_invariant():
    n0, n1 = 140, 96
    (d0, d1, s0, s1), g = make_inputs(4, n0, n1, seed=3)
    G = torch.randn((4, n0, n1), generator=g).to(DEV)
    db = torch.tensor([0.9], device=DEV)
    out, lse = ops.dual_softmax_train_fwd(d0, d1, s0.reshape(4, n0).contiguous(), s1.reshape(4, n1).contiguous(), T, db, True)
    full = ops.dual_softmax_bwd(d0, d1, s0.reshape(4, n0).contiguous(), s1.reshape(4, n1).contiguous(), T, db, lse, G, True,
                                (False, False, False, False, True))[4]
    for p in range(4):
        _, l1 = ops.dual_softmax_train_fwd(d0[p:p + 1], d1[p:p + 1], s0[p].contiguous(), s1[p].contiguous(), T, db, True)
        one = ops.dual_softmax_bwd(d0[p:p + 1], d1[p:p + 1], s0[p].contiguous(), s1[p].contiguous(), T, db, l1, G[p:p + 1], True,
                                   (False, False, False, False, True))[4]
        assert torch.equal(full[p], one[0])


def test_training_step_end_to_end():
    """native MetricPoseLoss on final_scores from dual_softmax_train, then the reference trainer's
    backward(log(final + 1e-16), probs_grad) (model.py:133-134): gradients against the fp64 torch path fed the same probs_grad"""
    from mickey_amd.config import _wrap
    from mickey_amd.train_ransac import MetricPoseLoss
    from tests.test_train_oracle import load_case
    cfg, batch, _ = load_case("default")
    b = {k: v.to(DEV) for k, v in batch.items()}
    B, n0, n1 = b["final_scores"].shape
    (d0, d1, s0, s1), _ = make_inputs(B, n0, n1, seed=17)
    x = [t.clone().requires_grad_() for t in (d0, d1, s0, s1)]
    db = torch.nn.Parameter(torch.tensor(1.0, device=DEV))
    final = dual_softmax_train(x[0], x[1], x[2], x[3], T, db)
    b["final_scores"] = final
    avg_loss, outputs, probs_grad, nvalid = MetricPoseLoss(_wrap(cfg), seed=3)(b)
    assert nvalid >= 1 and bool(torch.isfinite(probs_grad[0]).all())
    torch.autograd.backward(torch.log(final + 1e-16), probs_grad[0])
    y = [t.double().requires_grad_() for t in (d0, d1, s0, s1)]
    db64 = torch.tensor(1.0, device=DEV, dtype=torch.float64, requires_grad=True)
    torch.autograd.backward(torch.log(ref_final(y[0], y[1], y[2], y[3], db64) + 1e-16), probs_grad[0].double())
    check([t.grad for t in x] + [db.grad], [t.grad for t in y] + [db64.grad], "end-to-end")


class _StandInDualSoftmax(torch.nn.Module):
    """the reference dualSoftmax's attribute contract (feature_matcher.py:54-62), not the reference class"""

    def __init__(self, temperature, use_dustbin):
        super().__init__()
        self.temperature = temperature
        self.use_dustbin = False
        if use_dustbin:
            self.dustbin_score = torch.nn.Parameter(torch.tensor(1.))
            self.use_dustbin = True

    def forward(self, dsc0, dsc1):
        return ref_final(dsc0, dsc1, None, None, self.dustbin_score if self.use_dustbin else None, self.temperature)


class _StandInModel(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.matcher = torch.nn.Module()
        self.matcher.matching_mat = _StandInDualSoftmax(T, True)
        self.head = torch.nn.Linear(4, 4)


def test_use_hip_matcher_fills_the_original_parameter():
    model = _StandInModel().to(DEV)
    param = model.matcher.matching_mat.dustbin_score
    keys = sorted(model.state_dict())
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    (d0, d1, _, _), g = make_inputs(2, 90, 70, seed=23)
    G = torch.randn((2, 90, 70), generator=g).to(DEV)
    with torch.no_grad():
        want = model.matcher.matching_mat(d0, d1)
    assert use_hip_matcher(model) == 1
    mm = model.matcher.matching_mat
    assert isinstance(mm, DualSoftmax) and mm.dustbin_score is param and sorted(model.state_dict()) == keys
    assert use_hip_matcher(model) == 0   # already swapped
    scores = mm(d0, d1)
    assert rel(scores, want) <= 1e-5
    scores.backward(G)
    _, ref = fp64_grads(d0, d1, None, None, 1.0, G)
    assert param.grad is not None and rel(param.grad, ref[4]) <= 1e-4
    before = param.detach().clone()
    opt.step()
    assert not torch.equal(param.detach(), before)   # the optimiser's Parameter is the one that moved
