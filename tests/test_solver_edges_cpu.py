"""The case tables, references and bounds of the pose-solver edge tests (tests/helpers/solver_refs.py), checked on the CPU: for every
case that tests/test_solver_edges_gpu.py runs,
  * the case has the edge it is listed for;
  * its fitted sets are well conditioned (s2 / s1 >= 0.1, s3 / s2 >= 0.1 for full-rank fits) -- EVERY hypothesis, none filtered;
  * every refinement case keeps every residual of every round MARGIN = 16 x (the fp32 oracle's own residual error, measured here)
    away from the threshold -- the share of exempt elements is zero;
  * a correct fp32 evaluation (the oracle's arithmetic in fp32) meets every bound;
  * a subtly wrong reference -- one match dropped, centroid divided by the count, reflection fix left out, n0 for n1 in the cell
    split, tie rule reversed, a wrong sampling law -- misses it on at least one element."""
import pytest
import torch

from oracle import train_oracle as TO
from tests.helpers import solver_refs as R


# ================================================================ gather + back-projection ======================================
def test_gather_table_has_the_edges():
    ks = {c[3] for c in R.GATHER_CASES}
    assert {1, 255, 256, 257} <= ks
    assert {(c[4], c[5]) for c in R.GATHER_CASES} == {(7, 13), (13, 7), (1, 5)}
    assert {c[1] for c in R.GATHER_CASES} == {1, 3} and {c[2] for c in R.GATHER_CASES} == {1, 3}
    assert BACKPROJECT_ROUNDINGS() == 18


def BACKPROJECT_ROUNDINGS():
    """the count behind BACKPROJECT_FACTOR, restated: cofactor 3, determinant 3 + 5 on top, reciprocal 1, entry 1, evaluation 5"""
    n = 3 + (3 + 5) + 1 + 1 + 5
    assert R.BACKPROJECT_FACTOR == n / 2
    return n


@pytest.mark.parametrize("name,B,rpp,k,n0,n1,K", R.GATHER_CASES)
def test_gather_case(name, B, rpp, k, n0, n1, K):
    c = R.gather_case(name, B, rpp, k, n0, n1, K)
    assert n0 != n1 and int(c["idx"].max()) < n0 * n1 and int(c["idx"].min()) >= 0
    want = R.edge_cells(n0, n1)[:k]
    for r in range(B * rpp):
        assert set(want) <= set(c["idx"][r].tolist()), (name, r)
    for K_ in (c["K0"], c["K1"]):
        assert bool((K_[:, 0, 1] != 0).all()) and bool((K_[:, 0, 0] != K_[:, 1, 1]).all())
    if K is not None:
        assert K < B and c["kf"].tolist()[:1] == [1] and (len(set(c["kf"].tolist())) < B or "out of range" in name)
        assert ("out of range" in name) == (not bool(c["valid_pair"].all())) and int(c["valid_pair"].sum()) >= B - 1
    for nm in ("X", "Y"):                      # the fp32 oracle meets the bound by a factor of BACKPROJECT_FACTOR at least
        assert c[nm + "_floor"] <= 2 * R.EPS32, c[nm + "_floor"] / R.EPS32
    if k >= 5:                                 # n0 used for n1 in the cell split
        w = R.gather_ref(c, B, rpp, n0, n1, split_n=n0)
        worst = max(R.ratio(w[nm], c[nm], c[nm + "_scale"], c[nm + "_floor"], R.BACKPROJECT_FACTOR)[0] for nm in ("X", "Y"))
        assert worst > 100 and not torch.equal(w["corr"], c["corr"]), worst


@pytest.mark.parametrize("mode", R.GATHER_BWD_MODES)
def test_gather_backward_reference(mode):
    name, B, rpp, k, n0, n1 = ("k 257", 3, 1, 257, 7, 13) if mode != "no repeats" else ("no repeats", 3, 1, 7, 7, 13)
    c = R.gather_case(name, B, rpp, k, n0, n1, None, mode)
    ref, sc = R.gather_bwd_ref(c, B, rpp, n0, n1)
    r32 = R.gather_bwd_ref(c, B, rpp, n0, n1, dtype=torch.float32)
    counts = torch.stack([torch.bincount(c["i1"][r], minlength=n1) for r in range(B)])
    if mode == "one keypoint of image 1":
        assert bool((counts[:, 3] == k).all()) and int(counts.sum()) == B * k
    if mode == "no repeats":
        assert int(counts.max()) == 1
    # one cell's contribution dropped (the last sample of the last row): its keypoint misses the bound
    d = dict(c)
    d["gX"], d["gY"] = c["gX"].clone(), c["gY"].clone()
    d["gX"][-1, -1] = 0
    d["gY"][-1, -1] = 0
    wrong, _ = R.gather_bwd_ref(d, B, rpp, n0, n1)
    for a, b, w, s in zip(r32, ref, wrong, sc):
        s = s.clamp_min(1e-300)
        fl = R.floor32(a, b, s)
        assert fl < 1e-5 and bool((b[s <= 1e-300] == 0).all())
        assert R.ratio(a, b, s, fl)[0] <= 1.0 / R.FACTOR + 1e-12
        assert R.ratio(w, b, s, fl)[0] > 10.0


# ================================================================ hypotheses ====================================================
def _hyp_args():
    return [(2, 17, k) for k in R.HYP_K] + [(3, it, 65) for it in R.HYP_IT] + [(n, it, k) for _, n, it, k in R.regime_cases(256)]


@pytest.mark.parametrize("nsets,it,k", _hyp_args())
def test_hypotheses_case(nsets, it, k):
    c = R.hypotheses_case(nsets, it, k)
    r21, _ = R.sing_ratios(c["ref"]["H"])
    assert float(r21.min()) >= R.COND and r21.numel() == nsets * it          # every hypothesis, none dropped
    i3 = c["idx3"]
    assert bool((i3[:, 0] != i3[:, 1]).all() and (i3[:, 0] != i3[:, 2]).all() and (i3[:, 1] != i3[:, 2]).all())
    for j in (63, 64, 255, 256, k - 1):
        if j < k and it >= 6:
            assert bool((i3 == j).any()), j
    for nm in ("R", "t", "score"):
        assert c["floor"][nm] < 1e-5
    X, Y = c["X"], c["Y"]
    r32 = R.hypotheses_ref(X, Y, i3, it, dtype=torch.float32)
    drop = R.hypotheses_ref(X, Y, i3, it, dtype=torch.float32, drop_last=True)
    mirror = R.hypotheses_ref(X, Y, i3, it, dtype=torch.float32, reflection=False)
    for nm in ("R", "t", "score"):
        assert R.ratio(r32[nm], c["ref"][nm], c["scale"][nm], c["floor"][nm])[0] <= 1.0 / R.FACTOR + 1e-12
    assert R.ratio(drop["score"], c["ref"]["score"], c["scale"]["score"], c["floor"]["score"])[0] > 10.0      # the last match dropped
    assert R.ratio(mirror["R"], c["ref"]["R"], c["scale"]["R"], c["floor"]["R"])[0] > 100.0                    # no reflection fix


def test_hypotheses_tables_and_regimes():
    assert R.HYP_K == [3, 4, 5, 63, 64, 65, 255, 256, 257, 2016, 2017, 4768] and R.HYP_IT == [1, 15, 16, 17, 33, 100, 129, 132]
    assert (2016 * 8 + 256) * 4 == 64 * 1024 and (2017 * 8 + 256) * 4 > 64 * 1024 and 4768 * 32 + 1024 == 150 * 1024
    assert R.split_parts(256, 23, 100) == (23, 5, 3, 1)                       # 23 sets x 100 hypotheses on 256 CUs: three empty parts
    for cus in (64, 104, 228, 256, 304):
        cases = R.regime_cases(cus)
        ns = [R.split_parts(cus, n, it) for _, n, it, _ in cases]
        assert ns[0][0] == 1
        assert ns[1][0] == 4 and ns[1][1] == 33 and ns[1][3] == 2            # a second pass of ONE hypothesis
        assert ns[2][0] == 25
        assert ns[3][2] > 0 and ns[3][0] * ns[3][1] > 100 + ns[3][1]
        assert ns[4][0] == 4 and ns[4][1] == 33 and ns[4][3] == 2 and len(cases) == 5
    assert R.split_parts(256, 3, 129)[3] == 1 and R.split_parts(256, 128, 132)[1] == 33


@pytest.mark.parametrize("k,kind", R.race_cases())
def test_race_case(k, kind):
    c = R.race_case(k, kind)
    keys = c["keys"]
    if kind == "dense":
        assert torch.equal(torch.topk(keys, 3, dim=1).values, torch.gather(keys, 1, c["idx3"]))
        assert bool((c["w"] == 0).any()) or k < 8
    elif not (k == 3 and kind == "two"):       # (k = 3 with two positive weights: the one zero key is third, nothing ties)
        if kind != "two":                      # an exact tie among the wanted three ("two": between the third and the rest)
            top = torch.gather(keys, 1, c["idx3"])
            assert bool((top[:, :-1] == top[:, 1:]).any(1).all())
        assert not torch.equal(c["idx3"], R.topk_lowest_index(keys, 3, reverse_ties=True))    # the reversed rule differs
    if kind == "tie lanes":
        assert c["idx3"][:, :2].tolist() == [[5, 9]] * 10 and 5 // 4 != 9 // 4
    if kind == "tie stride":
        assert c["idx3"][:, :2].tolist() == [[6, 262]] * 10 and 6 // 4 == (262 - 256) // 4
    if kind in ("one", "two"):
        npos = 1 if kind == "one" else 2
        assert bool(((c["w"] > 0).sum(1) == npos).all())
        assert c["idx3"][0, npos:].tolist() == sorted(set(range(k)) - set(c["idx3"][0, :npos].tolist()))[:3 - npos]
    assert {k for k, _ in R.race_cases()} == {3, 4, 5, 255, 256, 257, 513}


def test_draw_law_check_has_teeth():
    """sequential sampling without replacement passes; picking the second match uniformly, or with the first one's weight left in,
    is caught"""
    g = R.gen("law")
    support = (0, 255, 512)
    w = torch.tensor(R.DRAW_WEIGHTS)
    n = 20000
    good = torch.tensor(support)[torch.multinomial(w.expand(n, 3), 3, generator=g)]
    assert R.draw_law_violations(good, support) == []
    uniform = good.clone()
    swap = torch.rand(n, generator=g) < 0.5
    uniform[swap] = uniform[swap][:, [0, 2, 1]]
    assert R.draw_law_violations(uniform, support)
    first = torch.multinomial(w.expand(n, 3), 1, generator=g)
    w2 = w.expand(n, 3).clone()
    w2.scatter_(1, first, 0.0)
    second = torch.multinomial(w2 * torch.tensor([1.0, 1.0, 1.6]), 1, generator=g)       # a cdf that is off after the first pick
    third = 3 - first - second
    assert R.draw_law_violations(torch.tensor(support)[torch.cat([first, second, third], 1)], support)
    assert [k for k, _ in R.draw_cases()] == [3, 257, 513, 513, 2017, 2017]


# ================================================================ refinement ====================================================
@pytest.mark.parametrize("case", R.REFINE_CASES, ids=[c[0] for c in R.REFINE_CASES])
def test_refine_case(case):
    name, k, B, it_m, it_r, num_ref, rule, want_rounds, tie = case
    c = R.refine_case(*case)
    HP = it_m * it_r
    print("%s: seed %d, rounds %s, margin %.3g = %.1f x err32 %.3g, floors %s" % (name, c["seed"], c["rounds"], c["margin"],
                                                                                c["margin"] / c["err32"], c["err32"], c["floor"]))
    assert c["margin"] >= R.MARGIN_FACTOR * c["err32"] > 0                  # every residual of every round: nothing exempt
    score = c["score"].view(B, HP)
    for b, p in enumerate(c["pairs"]):
        m64, m32 = p["m64"], p["m32"]
        assert len(m64["dists"]) == m64["rounds"] + (1 if m64["rounds"] == num_ref else 2) or num_ref == 0
        assert all(float((d - R.f32(R.TH_INLIER)).abs().min()) >= c["margin"] for d in m64["dists"])
        assert torch.equal(m32["mask"], m64["mask"]) and m32["rounds"] == m64["rounds"]
        assert R.well_conditioned(m64["Hs"], full_rank=k > 3)
        assert int(score[b].argmax()) == p["win"] and float(score[b, p["win"]]) == float(score[b].max())
        if p["later"] is not None:
            assert p["later"] > p["win"] and float(score[b, p["later"]]) == float(score[b, p["win"]])
            assert int(score[b].flip(0).argmax()) == HP - 1 - p["later"]   # the reversed tie rule picks the other one
            a, z = p["win"], p["later"]
            assert {"stride": z == a + 512, "lanes": a // 64 == z // 64 and a % 64 != z % 64, "waves": (a % 512) // 64 != (z % 512) // 64}[tie]
        if rule == "first":
            assert m64["counts"][0] == c["min_inl"] or b > 0
        if rule == "first-1":
            assert m64["counts"][0] == c["min_inl"] + 1 or b > 0
    if want_rounds is not None:
        assert c["rounds"][0] == want_rounds
    if rule == "first":
        assert c["rounds"][0] == 0
    if rule == "first-1":
        assert c["rounds"][0] >= 1
    for nm in ("R", "t", "conf"):
        assert c["floor"][nm] < 1e-5
    # one match dropped from the fits of pair 0: R misses the bound
    p = c["pairs"][0]
    if p["m64"]["rounds"] and k > 3:
        s = p["set"]
        inl = torch.nonzero((R.f32(R.TH_INLIER) - p["m64"]["dists"][0]) >= 0).view(-1)      # the matches of the first fit
        X, Y = c["X"][s].clone(), c["Y"][s].clone()
        Y[inl[-1]] += 5.0                                                   # the last of them never enters a fit
        wrong = R.refine_machine(X, Y, c["Rh"][p["win"]].view(3, 3), c["th"][p["win"]], R.TH_INLIER, num_ref, c["min_inl"])
        assert R.ratio(wrong["R"].reshape(1, 9), c["ref"]["R"][:1], c["scale"]["R"], c["floor"]["R"])[0] > 1.0


def test_refine_table_covers_every_edge():
    cases = [R.refine_case(*c) for c in R.REFINE_CASES]
    rounds = {r for c in cases for r in c["rounds"]}
    assert rounds >= {0, 1, 2, 3, 4}, rounds
    assert {c[3] * c[4] for c in R.REFINE_CASES} >= R.REFINE_HP
    assert {c[1] for c in R.REFINE_CASES} == {3, 5, 511, 512, 513, 1025}
    assert {c[5] for c in R.REFINE_CASES} == {0, 1, 4}
    assert {c[8] for c in R.REFINE_CASES} >= {"stride", "lanes", "waves"}
    for k in (3, 5, 511, 512, 513, 1025):            # the winning set is not set 0 in at least one case per k
        assert any(p["win"] // spec[4] > 0 for spec, c in zip(R.REFINE_CASES, cases) if spec[1] == k for p in c["pairs"]), k


# ================================================================ training RANSAC ===============================================
@pytest.mark.parametrize("S,nc,it_r,num_ref", R.TRAIN_CASES)
def test_train_case(S, nc, it_r, num_ref):
    c = R.train_case(S, nc, it_r, num_ref)
    idx = c["idx"]
    if nc < S:
        for j in (63, 64, S - 1):
            if j < S:
                assert bool((idx == j).any()), j
    # the state machine of the helper IS train_oracle.refine_masks, hypothesis by hypothesis.  (refine_masks mixes .float() counts
    # with default-dtype state, so it runs in fp32 only; the margin below is what makes its fp32 path the fp64 one.)
    Xv, Yv = c["X"].repeat_interleave(it_r, 0), c["Y"].repeat_interleave(it_r, 0)
    fin, rounds = TO.refine_masks(Xv, Yv, idx, num_ref, R.f32(R.TH_INLIER), nc)
    assert torch.equal(fin.float(), c["mask"]) and torch.equal(rounds.int(), c["rounds"])
    if num_ref == 0:
        assert int(c["rounds"].abs().sum()) == 0 and bool((c["mask"].sum(1) == nc).all())
        return
    print("S %d: seed %d, rounds %s, margin %.3g = %.1f x err32 %.3g" % (S, c["seed"], c["rounds"].tolist(), c["margin"],
                                                                       c["margin"] / c["err32"], c["err32"]))
    assert c["margin"] >= R.MARGIN_FACTOR * c["err32"] > 0
    for h in c["hyps"]:
        assert all(float((d - R.f32(R.TH_INLIER)).abs().min()) >= c["margin"] for d in h["dists"])
        assert R.well_conditioned(h["Hs"], full_rank=nc > 3)
    # the fp32 oracle takes the same path; the centroid divided by S instead of sum |w| does not
    differs = False
    for i in range(idx.shape[0]):
        s = i // it_r
        m32 = R.train_machine(c["X"][s], c["Y"][s], idx[i], R.TH_INLIER, num_ref, dtype=torch.float32)
        assert torch.equal(m32["mask"], c["mask"][i]) and m32["rounds"] == int(c["rounds"][i])
        if nc < S:
            bad = R.train_machine(c["X"][s], c["Y"][s], idx[i], R.TH_INLIER, num_ref, centroid_by_count=True)
            differs |= not torch.equal(bad["mask"], c["mask"][i]) or bad["rounds"] != int(c["rounds"][i])
    assert differs or nc == S


def test_train_tables_cover_every_edge():
    assert {c[0] for c in R.TRAIN_CASES} == set(R.TRAIN_S) == {8, 63, 64, 65, 255, 256, 257, 512, 513, 1023, 1024}
    assert {c[1] for c in R.TRAIN_CASES if c[1] < c[0]} == {3, 8} and any(c[1] == c[0] for c in R.TRAIN_CASES)
    assert {c[2] for c in R.TRAIN_CASES} == {1, 4, 5} and {c[3] for c in R.TRAIN_CASES} == {0, 4}
    rounds = set()
    for c in R.TRAIN_CASES:
        rounds |= set(R.train_case(*c)["rounds"].tolist())
    assert rounds == {0, 1, 2, 3, 4}


@pytest.mark.parametrize("S,nc,kind", R.TRAIN_RACE_CASES)
def test_train_race_case(S, nc, kind):
    c = R.train_race_case(S, nc, kind)
    keys = c["keys"]
    if kind == "dense" and nc < S:
        assert torch.equal(torch.topk(keys, nc, dim=1).values, torch.gather(keys, 1, c["idx"]))
    if kind == "few":
        assert bool(((c["w"] > 0).sum(1) == 5).all()) and nc == 8
        assert c["idx"][0, 5:].tolist() == [0, 1, 3]                       # the lowest free indices (2 is one of the five)
        assert not torch.equal(c["idx"], R.topk_lowest_index(keys, nc, reverse_ties=True))
    if kind == "tie":
        assert c["idx"][:, :2].tolist() == [[70, 326]] * 10 and 70 % 64 == 326 % 64
        assert not torch.equal(c["idx"], R.topk_lowest_index(keys, nc, reverse_ties=True))
    srt = c["idx"].sort(1).values
    assert bool((srt[:, 1:] != srt[:, :-1]).all())


# ================================================================ REINFORCE scatter =============================================
@pytest.mark.parametrize("S,it_m", R.SCATTER_CASES)
def test_scatter_case(S, it_m):
    c = R.scatter_case(S, it_m)
    assert R.SCATTER_NCELL == 600 and c["idx"].shape == (c["B"] * it_m, S)
    srt = c["idx"].long().sort(1).values
    assert S == 1 or bool((srt[:, 1:] != srt[:, :-1]).all())               # distinct within a row
    if it_m > 1 and S > 1:
        hits = torch.zeros(c["B"], 600)
        for r in range(c["B"] * it_m):
            hits[r // it_m, c["idx"][r].long()] += 1
        assert int(hits.max()) == it_m                                      # rows overlap
    if S < 600:
        assert bool((~c["drawn"]).any()) and torch.equal(c["want"][~c["drawn"]], c["pre"][~c["drawn"]])
    # the last sample of every row dropped: different bits
    wrong = c["pre"].clone()
    for r in range(c["B"] * it_m):
        wrong[r // it_m, c["idx"][r, :-1].long()] += c["lv"][r]
    assert not torch.equal(wrong, c["want"])
    assert torch.equal(c["want_b"] - c["pre_b"], torch.stack([torch.bincount(c["idx"][b * it_m:(b + 1) * it_m].reshape(-1).long(), minlength=600)
                                                               for b in range(c["B"])]).float())


# ================================================================ aggregation ===================================================
@pytest.mark.parametrize("B,it_m,it_r,add_null,temp", R.AGG_CASES)
def test_aggregate_case(B, it_m, it_r, add_null, temp):
    c = R.aggregate_case(B, it_m, it_r, add_null, temp)
    ref, sc = c["ref"], c["ref"]["scale"]
    r32 = R.aggregate_ref(c["out"], it_m, it_r, add_null, temp, dtype=torch.float32)
    for n in ("loss_value", "per_pair", "coef"):
        assert R.ratio(r32[n], ref[n], sc[n], c["floor"][n])[0] <= 1.0 / R.FACTOR + 1e-12 and c["floor"][n] < (1e-5 if temp > 1 else 2e-3)
    # closed form of coef (what the kernel evaluates) == autograd, in fp64
    o = c["out"].double().reshape(-1, it_r, 4)
    sm = ref["coef"][:, 0].reshape(-1, it_r)
    closed = (sm * (o[..., 0] - ref["loss_value"][:, None]) / temp).reshape(-1)
    assert bool(((ref["coef"][:, 1] - closed).abs() <= 1e-10 * sc["coef"][:, 1]).all())
    assert float(c["out"][:, 3].max()) > 500 and c["rank1"] >= 1
    if temp < 1:        # the max subtraction: without it fp32 overflows
        naive = torch.exp(c["out"][:, 3] / temp)
        assert not bool(torch.isfinite(naive).all()) and float((c["out"][:, 3] / temp).max()) > 1e4
    elif it_r > 1:      # the last hypothesis of every set dropped
        w = R.aggregate_ref(c["out"], it_m, it_r, add_null, temp, drop_last=True)
        assert R.ratio(w["loss_value"], ref["loss_value"], sc["loss_value"], c["floor"]["loss_value"])[0] > 1.0
        assert R.ratio(w["per_pair"], ref["per_pair"], sc["per_pair"], c["floor"]["per_pair"])[0] > 1.0
    elif add_null:      # the null column left out
        w = R.aggregate_ref(c["out"], it_m, it_r, 0, temp)
        assert R.ratio(w["loss_value"], ref["loss_value"], sc["loss_value"], c["floor"]["loss_value"])[0] > 1.0


def test_aggregate_tables_cover_every_edge():
    assert {c[2] for c in R.AGG_CASES} == {1, 63, 64, 65, 129} and {c[1] for c in R.AGG_CASES} == {1, 4, 5, 64}
    assert {c[0] for c in R.AGG_CASES} == {1, 3} and {c[3] for c in R.AGG_CASES} == {0, 1} and {c[4] for c in R.AGG_CASES} == {20.0, 0.05}
    assert {b * m * r for b, m, r in R.AGG_BWD_CASES} >= {255, 256, 257}


# ================================================================ the differentiable tail =======================================
@pytest.mark.parametrize("S,it_r,kind,soft", R.TAIL_CASES)
def test_tail_case(S, it_r, kind, soft):
    c = R.tail_case(S, it_r, kind, soft)
    ref, sc, fl = c["ref"], c["scale"], c["floor"]
    nsets = R.TAIL_B * R.TAIL_ITM
    print("S %d: seed %d, s2 / s1 >= %.3f, s3 / s2 >= %.3f (full-rank fits), floors %s" % (S, c["seed"], c["cond"][0], c["cond"][1], fl))
    assert c["cond"][0] >= R.COND and c["cond"][1] >= R.COND                 # every hypothesis
    assert set(c["kinds"]) == set(R.MASK_KINDS) if it_r * nsets >= 3 else True
    m = c["mask"]
    for h, k in enumerate(c["kinds"]):
        n = int(m[h].sum())
        assert n == {"all": S, "eight": 5 + len({j for j in (63, 64, S - 1) if j < S}), "three": 3}[k]
        if k == "eight":
            assert all(float(m[h, j]) == 1 for j in (63, 64, S - 1) if j < S)
    det = torch.linalg.det(ref["H"])
    mirrored = torch.arange(nsets).repeat_interleave(it_r) % 2 == 1
    assert bool((det[c["full"] & mirrored] < 0).all()) and bool((det[c["full"] & ~mirrored] > 0).all())
    assert bool((c["full"] & mirrored).any()) and bool((c["full"] & ~mirrored).any())
    # the fp32 oracle meets every bound; the reflection fix left out and the centroid divided by S do not
    r32 = R.tail_ref(c, dtype=torch.float32, grad_out=c["grad_out"])
    for n in ("out", "Rt", "gX", "gY"):
        assert R.ratio(r32[n], ref[n], sc[n], fl[n])[0] <= 1.0 / R.FACTOR + 1e-12
    assert fl["Rt"] < 1e-5 and fl["out"] < 1e-4 and fl["gX"] < 1e-3 and fl["gY"] < 1e-3
    norefl = R.tail_ref(c, reflection=False)
    assert R.ratio(norefl["Rt"], ref["Rt"], sc["Rt"], fl["Rt"])[0] > 1e3
    wrong = R.tail_ref(c, grad_out=c["grad_out"], centroid_by_count=True)
    if set(c["kinds"]) != {"all"}:
        assert R.ratio(wrong["Rt"], ref["Rt"], sc["Rt"], fl["Rt"])[0] > 1.0 and R.ratio(wrong["gX"], ref["gX"], sc["gX"], fl["gX"])[0] > 1.0
    # one mirrored hypothesis' gradient: fp64 autograd through the SVD == central differences of the whole tail
    h = int(torch.nonzero(c["full"] & mirrored)[0])
    r, j = h // it_r, int(torch.nonzero(m[h])[0])
    eps = 1e-6
    num = torch.zeros(3, dtype=torch.float64)
    for a in range(3):
        vals = []
        for s in (+1, -1):
            d = dict(c)
            d["X"] = c["X"].double().clone()
            d["X"][r, j, a] += s * eps
            o = R.tail_ref(d)["out"]
            vals.append(float((o[:, 0] * c["grad_out"][:, 0].double()).sum() + (o[:, 3] * c["grad_out"][:, 1].double()).sum()))
        num[a] = (vals[0] - vals[1]) / (2 * eps)
    assert float((num - ref["gX"][r, j]).abs().max()) <= 1e-5 * float(sc["gX"][r]), (num, ref["gX"][r, j])


def test_tail_table_covers_every_edge():
    assert {c[0] for c in R.TAIL_CASES} == {8, 63, 64, 65, 255, 256, 257, 1024} and {c[1] for c in R.TAIL_CASES} == {1, 4, 5}
    assert {(c[2], c[3]) for c in R.TAIL_CASES} == {("VCRE", 0), ("VCRE", 1), ("POSE_ERR", 0), ("POSE_ERR", 1)}
    assert R.TAIL_B == 2 and R.TAIL_ITM == 3


@pytest.mark.parametrize("case", [R.TAIL_CASES[0], R.TAIL_CASES[3]], ids=["POSE_ERR", "VCRE"])
def test_closed_form_kabsch_adjoint_is_autograd(case):
    """the adjoint of the tail's header, in fp64 with torch, against autograd through the SVD on separated singular values, proper
    and mirrored sets alike"""
    c = R.tail_case(*case)
    cf = R.tail_closed_form(c)
    for n in ("gX", "gY"):
        assert R.floor32(cf[n], c["ref"][n], c["scale"][n]) < 1e-12
    assert int((torch.linalg.det(c["ref"]["H"])[c["full"]] < 0).sum()) > 0


def test_isotropic_case():
    c = R.isotropic_case()
    assert bool((c["sing"][0::2] == 2.0).all()) and float((c["sing"] - 2.0).abs().max()) < 1e-6      # exactly / to rounding equal
    for n in ("gX", "gY"):
        assert R.floor32(c["closed64"][n], c["ref"][n], c["scale"][n]) < 1e-7     # closed form (fp64) == central differences
        assert R.ratio(c["closed32"][n], c["ref"][n], c["scale"][n], c["floor"][n])[0] <= 1.0 / R.FACTOR + 1e-12
        assert 0 < c["floor"][n] < 1e-4
    auto = R.tail_ref(c, grad_out=c["grad_out"])
    assert not bool(torch.isfinite(auto["gX"]).all())            # why autograd is not the reference here
    assert bool((c["ref"]["gX"][:, 6:].abs().sum(-1) > 0).all()) and float(c["mask"][:, 6:].sum()) == 0
    # the antisymmetric part dropped from the adjoint (C = 0: the fit treated as a constant) misses the bound
    d = dict(c)
    d["grad_out"] = c["grad_out"] * torch.tensor([0.0, 1.0])
    score_only = R.tail_closed_form(d)
    assert R.ratio(score_only["gX"], c["ref"]["gX"], c["scale"]["gX"], c["floor"]["gX"])[0] > 1.0


# ================================================================ guarded windows of integer outputs ============================
@pytest.mark.parametrize("dtype", [torch.int32, torch.uint8])
def test_guarded_integer_windows(dtype):
    view, check = R.guarded_int(3, 5, dtype, "cpu")
    s = R.INT_SENTINEL[dtype]
    assert bool((view == s).all()) and s not in (0, 1) and view.data_ptr() % 256 == 0 and view.is_contiguous()
    view.fill_(1)
    check()
    esz = view.element_size()
    flat = torch.empty(0, dtype=dtype).set_(view.untyped_storage(), 0, (view.untyped_storage().nbytes() // esz,), (1,))
    off = (view.data_ptr() - view.untyped_storage().data_ptr()) // esz
    assert off * esz >= 256 and off >= 4 * 5 and flat.numel() - off - 15 >= max(4 * 5, 256 // esz)
    for where, at in ((off - 1, r"\(row -1, column 4\)"), (off + 15, r"\(row 3, column 0\)"), (0, "guard overwritten"), (flat.numel() - 1, "guard overwritten")):
        keep = int(flat[where])
        flat[where] = keep ^ 1
        with pytest.raises(AssertionError, match=at):
            check()
        flat[where] = keep
    check()
    filled, check2 = R.guarded_int(1, 2, dtype, "cpu", fill=0)
    assert bool((filled == 0).all())
    check2()
