"""No GPU: the references of tests/test_matcher_grad_edges_gpu.py (tests/helpers/matcher_refs.py: formula_grads, its magnitude sums
M, grad_case, grad_cases) are what that file takes them for -- the formulas equal fp64 autograd of the reference formula at the
edge shapes, per-pair dustbin gradient included; M bounds |g| and vanishes only where the gradient does; the fp32 formula's own
error (floor32g, which sets the GPU tolerance) is an fp32 rounding error and nothing else; the case lists are the ones the GPU
file runs."""
import pytest
import torch

from tests.helpers import matcher_refs as R

T = R.TEMPERATURE


def _rel(a, b):
    return float((a - b).norm() / (b.norm() + 1e-300))


def _all_cases():
    """every distinct (family, B, n0, n1, dustbin, gkind) the GPU file puts through the element-wise metric"""
    cs = R.grad_cases()
    out = set()
    for n0, n1, _, db in cs["test_backward_elementwise"]:
        out.add(("unit", 2, n0, n1, db, "dense"))
    for family, gkind, n0, n1, _ in cs["test_backward_sparse_G_and_hot"]:
        for db in R.DUSTBINS:
            out.add((family, 2, n0, n1, db, gkind))
    for n0, n1, _ in cs["test_chain_forward_lse"]:
        out.add(("unit", 2, n0, n1, 0.7, "dense"))
    for B, n0, n1, _ in cs["test_batches"]:
        out.add(("unit", B, n0, n1, 0.7, "dense"))
    return sorted(out, key=repr)


@pytest.mark.parametrize("n0,n1", R.GRAD_SHAPES)
def test_formulas_equal_autograd_fp64_at_the_edge_shapes(n0, n1):
    """formula_grads against torch autograd of ref_final, fp64, relative norm <= 1e-12; the dustbin gradient pair by pair"""
    for db in R.DUSTBINS:
        for scores in (True, False):
            c = R.grad_case("unit", 2, n0, n1, db, "dense", scores)
            x = [t.double().clone().requires_grad_() if t is not None else None for t in (c["d0"], c["d1"], c["s0"], c["s1"], c["db"])]
            G = c["G"].double()
            R.ref_final(*x, T).backward(G)
            for k, (mine, t) in enumerate(zip(c["g64"], x)):
                if t is None:
                    assert mine is None
                    continue
                want = t.grad if k < 4 else None
                if k == 4:   # per pair: the backward of pair p's output alone
                    want = torch.zeros(2, dtype=torch.float64)
                    for p in range(2):
                        a = x[4].detach().clone().requires_grad_()
                        y = [t[p:p + 1].detach() if t is not None else None for t in x[:4]]
                        R.ref_final(*y, a, T).backward(G[p:p + 1])
                        want[p] = a.grad[0]
                    assert _rel(mine.sum(), t.grad[0]) <= 1e-12
                assert mine.shape == want.shape and _rel(mine, want) <= 1e-12, (n0, n1, db, scores, R.GRAD_KINDS[k], _rel(mine, want))
            # lse2: the log-sums the forward saves, in the layout of ops.dual_softmax_train_fwd
            assert c["lse64"].shape == (2, 2, max(n0, n1))
            S = torch.matmul(x[0].detach().transpose(1, 2), x[1].detach()) / T
            if db is not None:
                S = torch.cat([torch.cat([S, x[4].detach().expand(2, n0, 1)], -1), x[4].detach().expand(2, 1, n1 + 1)], 1)
            lr, lc = S.exp().sum(2).log2()[:, :n0], S.exp().sum(1).log2()[:, :n1]
            assert float((c["lse64"][:, 0, :n0] - lr).abs().max()) <= 1e-12 and float((c["lse64"][:, 1, :n1] - lc).abs().max()) <= 1e-12


def test_magnitude_sums_bound_the_gradients_and_floor32g_is_an_fp32_rounding_error():
    lo, hi = float("inf"), 0.0
    for family, B, n0, n1, db, gkind in _all_cases():
        c = R.grad_case(family, B, n0, n1, db, gkind)
        what = (family, B, n0, n1, db, gkind)
        for k, (g, M, fl) in enumerate(zip(c["g64"], c["M"], c["floor"])):
            if g is None:
                assert db is None and k == 4 and M is None and fl is None
                continue
            assert g.shape == M.shape and bool(torch.isfinite(g).all()) and bool(torch.isfinite(M).all())
            assert bool((M >= g.abs()).all()), what + (R.GRAD_KINDS[k],)
            if gkind == "dense":
                assert bool((M > 0).all()), what + (R.GRAD_KINDS[k],)
            else:
                assert bool(((M == 0) == (g == 0)).all()), what + (R.GRAD_KINDS[k],)
            # a sanity cap on the inputs, not a tolerance: the fp32 formula is an fp32 computation
            assert fl <= 2.0 ** -17, what + (R.GRAD_KINDS[k], fl)
            lo, hi = min(lo, fl), max(hi, fl)
        if family == "unit":   # (the only family whose lse is compared)
            assert c["floor_lse"] <= 2.0 ** -17, what + (c["floor_lse"],)
    print("floor32g over all cases: %.3g .. %.3g" % (lo, hi))


def test_sparse_G_has_empty_rows_and_planted_scores_are_zero():
    """what the sparse family and the score builder are for: rows / columns of G with no non-zero cell (M == 0 there: the kernel
    must return an exact zero), border keypoints with score 0 and a non-zero score gradient"""
    for n0, n1 in R.GRAD_SPARSE_SHAPES:
        c = R.grad_case("unit", 2, n0, n1, 0.7, "sparse")
        share = float((c["G"] != 0).double().mean())
        assert 0.03 < share < 0.07, share
        assert int((c["M"][2] == 0).sum()) + int((c["M"][3] == 0).sum()) >= 1 or min(n0, n1) > 64
    c = R.grad_case("unit", 2, 33, 31, 0.7, "sparse")
    assert int((c["M"][2] == 0).sum()) >= 1
    for n0, n1 in R.GRAD_SHAPES:
        c = R.grad_case("unit", 2, n0, n1, 0.7, "dense")
        for s, n, g in ((c["s0"], n0, c["g64"][2]), (c["s1"], n1, c["g64"][3])):
            zeros = sorted({k for k in R.ZERO_SCORE_KEYPOINTS + (n - 1,) if k < n}) if n >= 3 else []
            assert sorted(set(torch.nonzero(s == 0)[:, 1].tolist())) == zeros
            assert bool((g[:, zeros] != 0).all())


def test_case_lists_are_what_the_gpu_file_runs():
    import tests.test_matcher_grad_edges_gpu as Gm
    cs = R.grad_cases()
    names = sorted(n for n in dir(Gm) if n.startswith("test_"))
    assert names == sorted(cs)
    for name in names:
        marks = [m for m in getattr(Gm, name).pytestmark if m.name == "parametrize"]
        assert len(marks) == 1 and list(marks[0].args[1]) == cs[name], name
    shapes = [(1, 1), (1, 40), (40, 1), (31, 33), (32, 32), (33, 31), (64, 96), (128, 128), (127, 130), (129, 65), (65, 129),
              (130, 257), (257, 132), (96, 545), (545, 96)]
    full = [(n0, n1, sp, db) for n0, n1 in shapes for sp in (False, True) for db in (None, 0.7, 8.0)]
    assert cs["test_backward_elementwise"] == full and cs["test_lse_elementwise"] == full
    assert max(max(s) for s in shapes) <= 545
    assert cs["test_backward_sparse_G_and_hot"] == [("unit", "sparse", n0, n1, sp) for n0, n1 in ((33, 31), (129, 65), (130, 257))
                                                    for sp in (False, True)] + [("hot", "dense", n0, n1, False) for n0, n1 in R.DS_HOT_SHAPES]
    assert cs["test_chain_forward_lse"] == [(n0, n1, sp) for n0, n1 in ((33, 31), (129, 65), (257, 132)) for sp in (False, True)]
    assert cs["test_unused_lse_slots_and_dirty_work"] == [(n0, n1, sp) for n0, n1 in ((129, 65), (65, 129)) for sp in (False, True)]
    assert cs["test_batches"] == [(B, n0, n1, sp) for B in (1, 8, 9) for n0, n1 in ((33, 31), (129, 65)) for sp in (False, True)]
    assert cs["test_pair_isolation"] == [(3, 65, 129, False), (3, 65, 129, True)]
    assert cs["test_output_subsets"] == [(129, 65, False), (129, 65, True)]
    assert cs["test_misaligned_outputs"] == [(n0, n1, sp) for n0, n1 in ((32, 32), (129, 64)) for sp in (False, True)]
    assert R.GRAD_SUBSETS == [(True, False, False, False, False), (False, True, False, False, False),
                              (False, False, True, True, False), (False, False, False, False, True)]
