"""-m gpu: the kernels of mk_solver.hip -- the last stage of every forward and the sampling half of the training loss -- ELEMENT by
element against fp64 at the smallest shapes that reach every loop edge (tests/helpers/solver_refs.py names the cases, derives the
bounds and states the three levels of comparison; tests/test_solver_edges_cpu.py asserts on the CPU that every case has its edge, its
conditioning and its threshold margin with no element exempt, and that subtly wrong references miss the bounds):
  mk_gather_backproject, _kf, _bwd    n0 != n1, k around 256, keyframe maps, shared / unshared keypoints in the backward
  mk_ransac_hypotheses                injected triples: k from 3 to the limit 4768, it_ransac up to a second HYP_PASS trip, the launch
                                      regimes of its nsplit rule read from the device's CU count (empty parts included), split invariance
                                      bit for bit; injected noise: the race with exact ties; on-device draws: their law on three matches
  mk_refine_pose + mk_pose_finalize   arg-max over HP around 512 with equal maxima, k around the 512 stride, min_inliers at and below the
                                      first count, 0 / 1 / 4 refinements, NaN scores, non-finite hypotheses
  mk_train_ransac_masks               S at every lane-slot edge up to 1024, masks and rounds of EVERY hypothesis, races, draws
  mk_reinforce_scatter                bit-exact against the sequential loop, presets kept
The entry points are called directly, as ops.py calls them, with every output in a guarded window (tests/helpers/guarded.py; solver_refs.guarded_int for int32 and uint8): the
guards are checked after every call and every wanted element is found overwritten.  Measured worst ratios:
profiles/solver_edges_parity.txt."""
import time

import pytest
import torch

from tests.helpers import solver_refs as R
from tests.helpers.guarded import bits, guarded, sentinel_bits

pytestmark = pytest.mark.gpu

WORST = {}       # (kernel, output) -> largest |error| / bound seen in this process
EXACT = {}       # (kernel, output) -> number of exact comparisons made
REGIMES = []     # the nsplit regimes reached on this device
RAN = [0]
F32, I32, U8 = torch.float32, torch.int32, torch.uint8


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _nv():
    from mickey_amd import _native
    return _native


@pytest.fixture(scope="module", autouse=True)
def _report():
    t0 = time.perf_counter()
    yield
    for (kernel, what), r in sorted(WORST.items()):
        print("solver edges worst |err| / bound: %-28s %-12s %.3f" % (kernel, what, r))
    for (kernel, what), n in sorted(EXACT.items()):
        print("solver edges exact comparisons:   %-28s %-12s %d" % (kernel, what, n))
    for line in REGIMES:
        print("solver edges nsplit regime: " + line)
    print("solver edges: %d tests in %.1f s" % (RAN[0], time.perf_counter() - t0))


@pytest.fixture(autouse=True)
def _count():
    yield
    RAN[0] += 1


def _sentinel(t):
    """-> (t as integers of its width, the sentinel of its window)"""
    if t.dtype in R.INT_SENTINEL:
        return t, R.INT_SENTINEL[t.dtype]
    return bits(t), sentinel_bits(t.dtype)


def _written(t):
    b, s = _sentinel(t)
    return not bool((b == s).any())


def _untouched(t):
    b, s = _sentinel(t)
    return bool((b == s).all())


class Outs:
    """guarded output windows of one call: .new(name, rows, cols, dtype) -> view; .check(msg, skip_rows) checks every guard and
    that every window is overwritten"""

    def __init__(self, dev):
        self.dev, self.items = dev, {}

    def new(self, name, rows, cols, dtype=F32, fill=None):
        view, chk = (R.guarded_int if dtype in R.INT_SENTINEL else guarded)(rows, cols, dtype, self.dev, fill=fill)
        self.items[name] = (view, chk, fill is None)
        return view

    def check(self, msg, unwritten_ok=()):
        torch.cuda.synchronize()
        for name, (view, chk, must_write) in self.items.items():
            try:
                chk()
            except AssertionError as e:
                raise AssertionError("%s, output %s: %s" % (msg, name, e))
            if must_write and name not in unwritten_ok:
                assert _written(view), "%s: an element of %s kept the sentinel" % (msg, name)


def _exact(kernel, what, got, want, msg, where=None):
    g = got.detach().cpu().reshape(-1)
    w = want.to(g.dtype).reshape(-1)
    assert g.shape == w.shape, (g.shape, w.shape)
    if g.dtype.is_floating_point:
        g, w = bits(g), bits(w)
    EXACT[(kernel, what)] = EXACT.get((kernel, what), 0) + 1
    ne = g != w
    if bool(ne.any()):
        i = int(torch.nonzero(ne)[0])
        raise AssertionError("%s %s, %s: %d of %d elements differ, first at %s: got %r, want %r"
                             % (kernel, what, msg, int(ne.sum()), ne.numel(), where(i) if where else "flat index %d" % i,
                                got.detach().cpu().reshape(-1)[i].item(), want.reshape(-1)[i].item()))


def _within(kernel, what, got, ref, scale, floor, msg, where=None, factor=R.FACTOR):
    got = got.detach().double().cpu().reshape(ref.shape)
    worst, i = R.ratio(got, ref, scale, floor, factor)
    WORST[(kernel, what)] = max(WORST.get((kernel, what), 0.0), worst)
    if not worst <= 1.0:
        raise AssertionError("%s %s, %s: |err| / bound = %.3g at %s: got %r, fp64 %r (floor32 %.3g, factor %g)"
                             % (kernel, what, msg, worst, where(i) if where else "flat index %d" % i, float(got.reshape(-1)[i]),
                                float(ref.reshape(-1)[i]), floor, factor))


# ================================================================ mk_gather_backproject (+ _kf) =================================
@pytest.mark.parametrize("name,B,rpp,k,n0,n1,K", R.GATHER_CASES)
def test_gather_backproject_elementwise(name, B, rpp, k, n0, n1, K):
    dev, nv = _dev(), _nv()
    c = R.gather_case(name, B, rpp, k, n0, n1, K)
    rows = B * rpp
    msg = "%s: B %d, %d rows per pair, k %d, %d x %d" % (name, B, rpp, k, n0, n1)
    d = {n: c[n].to(dev).contiguous() for n in ("idx", "fs", "kps0", "dep0", "kps1", "dep1", "K0", "K1")}
    o = Outs(dev)
    X, Y, wts, corr = o.new("X", rows * k, 3), o.new("Y", rows * k, 3), o.new("wts", rows, k), o.new("corr", rows * k, 6)
    args = [nv.ptr(d[n]) for n in ("idx", "fs", "kps0", "dep0", "kps1", "dep1", "K0", "K1")] + [nv.ptr(X), nv.ptr(Y), nv.ptr(wts), nv.ptr(corr),
                                                                                                 B, rpp, k, n0, n1]
    if K is None:
        nv.call("mk_gather_backproject", *args, nv.stream())
    else:
        kf = c["kf"].int().to(dev)
        nv.call("mk_gather_backproject_kf", *args, nv.ptr(kf), K, nv.stream())
    valid = c["valid_pair"][c["pair"]]                                   # per row
    o.check(msg, unwritten_ok=() if bool(valid.all()) else ("X", "Y", "wts", "corr"))
    vr = torch.nonzero(valid).view(-1)
    for nm, t, w in (("X", X, 3), ("Y", Y, 3), ("corr", corr, 6), ("wts", wts, 1)):
        t = t.view(rows, k, w)
        assert _written(t[vr.to(dev)]), msg + ": an element of %s kept the sentinel" % nm
        if not bool(valid.all()):
            assert _untouched(t[torch.nonzero(~valid).view(-1).to(dev)]), msg + ": %s of the pair without a keyframe was written" % nm

    def where(i):
        r, s, a = i // (k * 3), (i // 3) % k, i % 3
        cell = int(c["idx"][vr[r], s])
        return "row %d (pair %d), sample %d (thread %d of block %d), axis %d, cell %d = (%d, %d)" % (
            int(vr[r]), int(c["pair"][vr[r]]), s, s % 256, s // 256, a, cell, cell // n1, cell % n1)

    kern = "gather_backproject" + ("_kf" if K is not None else "")
    for nm, t in (("X", X), ("Y", Y)):
        _within(kern, nm, t.view(rows, k, 3)[vr.to(dev)], c[nm][vr], c[nm + "_scale"][vr], c[nm + "_floor"], msg, where, R.BACKPROJECT_FACTOR)
    _exact(kern, "wts", wts.view(rows, k)[vr.to(dev)], c["wts"][vr], msg)
    _exact(kern, "corr", corr.view(rows, k, 6)[vr.to(dev)], c["corr"][vr], msg)


GATHER_BWD = [c + ("random",) for c in R.GATHER_CASES if c[6] is None] + [
    ("k 257", 3, 1, 257, 7, 13, None, "one keypoint of image 1"), ("no repeats", 3, 1, 7, 7, 13, None, "no repeats")]


@pytest.mark.parametrize("name,B,rpp,k,n0,n1,K,mode", GATHER_BWD)
def test_gather_backproject_bwd_elementwise(name, B, rpp, k, n0, n1, K, mode):
    dev, nv = _dev(), _nv()
    c = R.gather_case(name, B, rpp, k, n0, n1, K, mode)
    msg = "%s (%s): B %d, %d rows per pair, k %d, %d x %d" % (name, mode, B, rpp, k, n0, n1)
    ref, scales = R.gather_bwd_ref(c, B, rpp, n0, n1)
    r32 = R.gather_bwd_ref(c, B, rpp, n0, n1, dtype=torch.float32)
    d = {n: c[n].to(dev).contiguous() for n in ("idx", "corr", "gX", "gY", "K0", "K1")}
    o = Outs(dev)
    outs = [o.new("gkps0", B * 2, n0, fill=0.0), o.new("gdep0", B, n0, fill=0.0), o.new("gkps1", B * 2, n1, fill=0.0),
            o.new("gdep1", B, n1, fill=0.0)]
    nv.call("mk_gather_backproject_bwd", *[nv.ptr(d[n]) for n in ("idx", "corr", "gX", "gY", "K0", "K1")], *[nv.ptr(t) for t in outs],
            B, rpp, k, n0, n1, nv.stream())
    o.check(msg)
    for nm, got, rf, r3, sc in zip(("gkps0", "gdep0", "gkps1", "gdep1"), outs, ref, r32, scales):
        n = rf.shape[-1]
        drawn = sc > 0
        sc1 = sc.clamp_min(1e-300)

        def where(i, n=n, nm=nm):
            return "%s[pair %d, channel %d, keypoint %d]" % (nm, i // (rf.shape[1] * n), (i // n) % rf.shape[1], i % n)

        _within("gather_backproject_bwd", nm, got, rf, sc1, R.floor32(r3, rf, sc1), msg, where)
        g = got.cpu().reshape(rf.shape)
        assert bool((bits(g)[~drawn] == 0).all()), msg + ": %s of a keypoint nobody drew is not +0" % nm
    if mode == "one keypoint of image 1":
        assert int((scales[3] > 0).sum()) == B and int((scales[2] > 0).sum()) == 2 * B
    if mode == "no repeats":
        assert int(torch.stack([torch.bincount(c["i0"][r], minlength=n0).max() for r in range(B)]).max()) == 1


# ================================================================ mk_ransac_hypotheses ==========================================
def _hypotheses(dev, X, Y, w, it, th=R.TH_SOFT, noise3=None, idx3_in=None, seed=0, offset=0, set_base=0, msg=""):
    """mk_ransac_hypotheses as ops.ransac_hypotheses calls it, outputs guarded -> Rh [nh, 9], th [nh, 3], score [nh, 1], idx3 [nh, 3]"""
    nv = _nv()
    nsets, k, _ = X.shape
    nh = nsets * it
    o = Outs(dev)
    Rh, tt, sc, i3 = o.new("Rh", nh, 9), o.new("th", nh, 3), o.new("score", nh, 1), o.new("idx3", nh, 3, I32)
    nv.call("mk_ransac_hypotheses", nv.ptr(X), nv.ptr(Y), nv.ptr(w), nv.ptr(noise3), nv.ptr(idx3_in), int(seed), int(offset), None,
            float(th), nv.ptr(Rh), nv.ptr(tt), nv.ptr(sc), nv.ptr(i3), nsets, it, k, int(set_base), nv.stream())
    o.check(msg)
    return Rh, tt, sc, i3


def _run_injected(dev, c, msg):
    X, Y = c["X"].to(dev), c["Y"].to(dev)
    w = torch.ones(X.shape[:2], device=dev)
    idx = c["idx3"].int().to(dev)
    Rh, tt, sc, i3 = _hypotheses(dev, X, Y, w, c["it_ransac"], idx3_in=idx, msg=msg)
    _exact("ransac_hypotheses", "idx3 echo", i3, c["idx3"], msg)
    for nm, got, wd in (("R", Rh, 9), ("t", tt, 3), ("score", sc, 1)):
        _within("ransac_hypotheses", nm, got, c["ref"][nm], c["scale"][nm], c["floor"][nm], msg, lambda i, wd=wd: R.hyp_where(c, i, wd))


@pytest.mark.parametrize("k", R.HYP_K)
def test_hypotheses_injected_triples_k(k):
    """it_ransac 17 (four blocks per set, five hypotheses in the first, two in the last): the staging loops, the 64-stride of the
    score and, from k = 2017, the opt-in dynamic LDS up to the documented limit"""
    dev = _dev()
    _run_injected(dev, R.hypotheses_case(2, 17, k), "2 sets x 17 hypotheses, k %d" % k)


@pytest.mark.parametrize("it", R.HYP_IT)
def test_hypotheses_injected_triples_it_ransac(it):
    dev = _dev()
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    ns, per, empty, passes = R.split_parts(cus, 3, it)
    _run_injected(dev, R.hypotheses_case(3, it, 65), "3 sets x %d hypotheses, k 65 (nsplit %d, %d per part, %d passes)" % (it, ns, per, passes))


@pytest.mark.parametrize("which", range(5))
def test_hypotheses_launch_regimes(which):
    """the nsplit rule restated from multi_processor_count: one block per set; four with a second pass of ONE hypothesis; one block
    per four hypotheses; a launch with empty parts; four with a second pass in every part -- each reached on this device, or the
    test fails"""
    dev = _dev()
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    regime, nsets, it, k = R.regime_cases(cus)[which]
    assert nsets is not None, "%s: no set count reaches it with %d CUs" % (regime, cus)
    ns, per, empty, passes = R.split_parts(cus, nsets, it)
    line = "%s: %d CUs, %d sets x %d hypotheses -> nsplit %d, %d per part, %d empty parts, %d passes" % (regime, cus, nsets, it, ns, per, empty, passes)
    REGIMES.append(line)
    print(line)
    if regime == "nsplit 1":
        assert ns == 1
    elif regime.startswith("nsplit 4, second pass of one"):
        assert ns == 4 and passes == 2 and per == 4 * R.HYP_PASS + 1, line
    elif regime.startswith("nsplit 4"):
        assert ns == 4 and passes == 2 and per * 4 == it, line
    elif regime.startswith("nsplit ceil"):
        assert ns == (it + 3) // 4 and ns > 4, line
    else:
        assert empty > 0 and ns * per > it + per, line
    _run_injected(dev, R.hypotheses_case(nsets, it, k), line)


@pytest.mark.parametrize("k", [2, 4769])
def test_hypotheses_reject_k_outside_3_to_4768(k):
    dev, nv = _dev(), _nv()
    X = torch.zeros((1, k, 3), device=dev)
    with pytest.raises(nv.MickeyHipError, match="mk_ransac_hypotheses: bad sizes"):
        _hypotheses(dev, X, X, torch.ones((1, k), device=dev), 4)


def test_hypotheses_bit_identical_for_any_split():
    """on-device draws, 100 hypotheses per set: set 0 alone (25 blocks) equals set 0 among 2 x CUs sets (4 blocks), bit for bit, and
    so does the last set alone with set_base"""
    dev = _dev()
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    nsets, it, k = 2 * cus, 100, 65
    assert R.nsplit_rule(cus, 1, it) == 25 and R.nsplit_rule(cus, nsets, it) == 4
    g = R.gen("split")
    X, Y = R.hyp_sets(g, nsets, k)
    w = (torch.rand(nsets, k, generator=g) + 0.05).to(dev)
    X, Y = X.to(dev), Y.to(dev)
    full = _hypotheses(dev, X, Y, w, it, seed=11, offset=5, msg="all sets")
    for s in (0, nsets - 1):
        alone = _hypotheses(dev, X[s:s + 1].contiguous(), Y[s:s + 1].contiguous(), w[s:s + 1].contiguous(), it, seed=11, offset=5, set_base=s,
                            msg="set %d alone" % s)
        for nm, a, f in zip(("Rh", "th", "score", "idx3"), alone, full):
            _exact("ransac_hypotheses", "split " + nm, a, f[s * it:(s + 1) * it].cpu(), "set %d alone against the same set among %d" % (s, nsets))
    i3 = full[3].cpu().long()
    assert bool((i3[:, 0] != i3[:, 1]).all() and (i3[:, 0] != i3[:, 2]).all() and (i3[:, 1] != i3[:, 2]).all())
    assert int(i3.min()) >= 0 and int(i3.max()) < k


@pytest.mark.parametrize("k,kind", R.race_cases())
def test_hypotheses_injected_noise_is_the_race(k, kind):
    """idx3 == the top-3 of w / noise with the lowest index winning exact ties: zero weights (their keys tie at 0), an exact maximal
    key in two lanes / in one lane's two strides"""
    dev = _dev()
    c = R.race_case(k, kind)
    g = R.gen("race points", k)
    X = R.points(g, c["nsets"], k).to(dev)
    _, _, _, i3 = _hypotheses(dev, X, X, c["w"].to(dev), c["it"], noise3=c["noise"].to(dev), msg="k %d, %s" % (k, kind))
    _exact("ransac_hypotheses", "race idx3", i3, c["idx3"], "k %d, %s" % (k, kind),
           lambda i: "hypothesis %d, pick %d: want %s" % (i // 3, i % 3, R.lane_slot(int(c["idx3"].reshape(-1)[i]))))


@pytest.mark.parametrize("k,support", R.draw_cases())
def test_hypotheses_on_device_draw_law(k, support):
    """weights positive on exactly three matches: every triple is a permutation of them, and over 20000 hypotheses the first pick
    and the second pick given the first follow w / (what is left), each frequency within 5 sigma; one fixed seed, nothing retried"""
    dev = _dev()
    nsets, it = 200, 100
    g = R.gen("draw", k)
    X = R.points(g, nsets, k).to(dev)
    w = torch.zeros(nsets, k)
    w[:, list(support)] = torch.tensor(R.DRAW_WEIGHTS)
    _, _, _, i3 = _hypotheses(dev, X, X, w.to(dev), it, seed=2024, offset=3, msg="k %d, support %s" % (k, support))
    i3 = i3.cpu().long()
    assert torch.equal(i3.sort(1).values, torch.tensor(sorted(support)).expand(nsets * it, 3)), "a triple is not a permutation of %s" % (support,)
    bad = R.draw_law_violations(i3, support)
    EXACT[("ransac_hypotheses", "draw law")] = EXACT.get(("ransac_hypotheses", "draw law"), 0) + 1
    assert not bad, "k %d, support %s: %s" % (k, support, "; ".join(bad))


# ================================================================ mk_refine_pose + mk_pose_finalize ==============================
def _refine(dev, X, Y, Rh, th, score, B, it_m, it_r, num_ref, min_inl, msg, th_in=R.TH_INLIER):
    nv = _nv()
    k = X.shape[1]
    o = Outs(dev)
    Ro, to, conf = o.new("R", B, 9), o.new("t", B, 3), o.new("conf", B, 1)
    best, rounds, mask = o.new("best", 1, B, I32), o.new("rounds", 1, B, I32), o.new("mask", B, k, U8)
    inv = o.new("invalid", 1, 1, I32, fill=0)
    nv.call("mk_refine_pose", nv.ptr(X), nv.ptr(Y), nv.ptr(Rh), nv.ptr(th), nv.ptr(score), float(th_in), int(num_ref), int(min_inl),
            nv.ptr(Ro), nv.ptr(to), nv.ptr(conf), nv.ptr(best), nv.ptr(mask), nv.ptr(rounds), nv.ptr(inv), B, it_m, it_r, k, nv.stream())
    o.check(msg + " (after mk_refine_pose)")
    nv.call("mk_pose_finalize", nv.ptr(Ro), nv.ptr(to), nv.ptr(conf), nv.ptr(inv), B, nv.stream())
    o.check(msg + " (after mk_pose_finalize)")
    return Ro, to, conf, best, mask, rounds, inv


@pytest.mark.parametrize("name,k,B,it_m,it_r,num_ref,min_rule,want_rounds,tie", R.REFINE_CASES)
def test_refine_pose(name, k, B, it_m, it_r, num_ref, min_rule, want_rounds, tie):
    dev = _dev()
    c = R.refine_case(name, k, B, it_m, it_r, num_ref, min_rule, want_rounds, tie)
    msg = "%s: B %d, HP %d x %d = %d, k %d, %d refinements, min_inliers %d (seed %d)" % (name, B, it_m, it_r, it_m * it_r, k, num_ref, c["min_inl"], c["seed"])
    Ro, to, conf, best, mask, rounds, inv = _refine(dev, *[c[n].to(dev).contiguous() for n in ("X", "Y", "Rh", "th", "score")], B, it_m, it_r,
                                                    num_ref, c["min_inl"], msg)
    _exact("refine_pose", "best", best, torch.tensor(c["best"]), msg,
           lambda i: "pair %d: winner %d = thread %d (wave %d, lane %d), trip %d; planted equal maximum at %r" % (
               i, c["best"][i], c["best"][i] % 512, (c["best"][i] % 512) // 64, c["best"][i] % 64, c["best"][i] // 512, c["pairs"][i]["later"]))
    _exact("refine_pose", "rounds", rounds, torch.tensor(c["rounds"]), msg, lambda i: "pair %d" % i)
    _exact("refine_pose", "mask", mask, c["mask"], msg, lambda i: "pair %d, %s" % (i // k, R.lane_slot(i % k)))
    assert int(inv) == 0
    for nm, got in (("R", Ro), ("t", to), ("conf", conf)):
        _within("refine_pose", nm, got, c["ref"][nm], c["scale"][nm], c["floor"][nm], msg,
                lambda i, nm=nm: "pair %d, element %d of %s (winner %d, set %d, %d rounds)" % (
                    i // c["ref"][nm].shape[1], i % c["ref"][nm].shape[1], nm, c["best"][i // c["ref"][nm].shape[1]],
                    c["pairs"][i // c["ref"][nm].shape[1]]["set"], c["rounds"][i // c["ref"][nm].shape[1]]))


def test_refine_pose_nan_scores():
    """all-NaN scores give best 0; a NaN among finite scores is skipped (also when it comes first, and in every wave)"""
    dev = _dev()
    name, k, B, it_m, it_r, num_ref, rule, want, tie = R.REFINE_CASES[3]
    c = R.refine_case(name, k, B, it_m, it_r, num_ref, rule, want, tie)
    HP = it_m * it_r
    d = [c[n].to(dev).contiguous() for n in ("X", "Y", "Rh", "th")]
    score = c["score"].clone().view(B, HP)
    score[0] = float("nan")
    score[1, ::64] = float("nan")
    score[1, 0:3] = float("nan")
    want_best = [0, int(torch.where(torch.isnan(score[1]), torch.tensor(-1.0), score[1]).argmax())]
    assert want_best[1] == c["best"][1]
    _, _, _, best, _, _, inv = _refine(dev, *d, score.reshape(-1).to(dev), B, it_m, it_r, 0, 3, "NaN scores")
    _exact("refine_pose", "best (NaN)", best, torch.tensor(want_best), "NaN scores")
    assert int(inv) == 0


@pytest.mark.parametrize("where", ["first element of pair 0's Rh", "last element of the last pair's th"])
@pytest.mark.parametrize("B", [1, 28, 29])
def test_pose_finalize_zeroes_every_pair(B, where):
    """one non-finite hypothesis value zeroes R, t, conf of ALL pairs; 9 B crosses finalize_kernel's 256-thread block at B = 29"""
    dev = _dev()
    it_m, it_r, k = 1, 2, 5
    g = R.gen("finalize", B)
    X = R.points(g, B * it_m, k)
    Rh = torch.eye(3).reshape(1, 9).repeat(B * it_m * it_r, 1)
    th = torch.zeros(B * it_m * it_r, 3)
    score = torch.rand(B * it_m * it_r, generator=g)
    clean = _refine(dev, X.to(dev), X.to(dev), Rh.to(dev), th.to(dev), score.to(dev), B, it_m, it_r, 0, 3, "clean, B %d" % B)
    assert int(clean[6]) == 0 and bool((clean[0].cpu() == Rh[:B]).all()) and float(clean[2].min()) > 0
    if where.startswith("first"):
        Rh[0, 0] = float("inf")
    else:
        th[-1, -1] = float("nan")
    Ro, to, conf, _, _, _, inv = _refine(dev, X.to(dev), X.to(dev), Rh.to(dev), th.to(dev), score.to(dev), B, it_m, it_r, 0, 3, "%s, B %d" % (where, B))
    assert int(inv) == 1
    for nm, t in (("R", Ro), ("t", to), ("conf", conf)):
        _exact("pose_finalize", nm, t, torch.zeros(t.shape), "%s, B %d" % (where, B))


# ================================================================ mk_train_ransac_masks =========================================
def _train_masks(dev, X, Y, w, it_r, num_ref, nc, noise=None, idx_in=None, seed=0, offset=0, set_base=0, msg="", th=R.TH_INLIER):
    nv = _nv()
    nsets, S, _ = X.shape
    nh = nsets * it_r
    o = Outs(dev)
    mask, idx, rounds = o.new("mask", nh, S), o.new("idx", nh, nc, I32), o.new("rounds", 1, nh, I32)
    nv.call("mk_train_ransac_masks", nv.ptr(X), nv.ptr(Y), nv.ptr(w), nv.ptr(noise), nv.ptr(idx_in), int(seed), int(offset), None, float(th),
            int(num_ref), int(nc), nv.ptr(mask), nv.ptr(idx), nv.ptr(rounds), nsets, it_r, S, int(set_base), nv.stream())
    o.check(msg)
    return mask, idx, rounds


@pytest.mark.parametrize("S,nc,it_r,num_ref", R.TRAIN_CASES)
def test_train_masks_injected_indices(S, nc, it_r, num_ref):
    """masks and rounds of EVERY hypothesis equal the fp64 state machine (the case keeps every residual of every round 16 fp32-oracle
    errors away from the threshold)"""
    dev = _dev()
    c = R.train_case(S, nc, it_r, num_ref)
    msg = "S %d, %d of them sampled, %d hypotheses per set, %d refinements (seed %d)" % (S, nc, it_r, num_ref, c["seed"])
    w = torch.ones(R.TRAIN_NSETS, S, device=dev)
    mask, idx, rounds = _train_masks(dev, c["X"].to(dev), c["Y"].to(dev), w, it_r, num_ref, nc, idx_in=c["idx"].int().to(dev), msg=msg)
    _exact("train_ransac_masks", "idx echo", idx, c["idx"], msg)
    _exact("train_ransac_masks", "rounds", rounds, c["rounds"], msg, lambda i: "set %d, hypothesis %d (wave %d)" % (i // it_r, i % it_r, (i % it_r) % 4))
    _exact("train_ransac_masks", "mask", mask, c["mask"], msg,
           lambda i: "set %d, hypothesis %d (wave %d), %s" % (i // S // it_r, (i // S) % it_r, ((i // S) % it_r) % 4, R.lane_slot(i % S)))


@pytest.mark.parametrize("S,nc,kind", R.TRAIN_RACE_CASES)
def test_train_masks_injected_noise_is_the_race(S, nc, kind):
    dev = _dev()
    c = R.train_race_case(S, nc, kind)
    msg = "S %d, %d sampled, %s" % (S, nc, kind)
    X = R.points(R.gen("train race points", S), 2, S).to(dev)
    mask, idx, rounds = _train_masks(dev, X, X, c["w"].to(dev), c["it"], 0, nc, noise=c["noise"].to(dev), msg=msg)
    _exact("train_ransac_masks", "race idx", idx, c["idx"], msg,
           lambda i: "hypothesis %d, pick %d: want %s" % (i // nc, i % nc, R.lane_slot(int(c["idx"].reshape(-1)[i]))))
    want = torch.zeros(2 * c["it"], S).scatter_(1, c["idx"], 1.0)
    _exact("train_ransac_masks", "race mask", mask, want, msg)
    _exact("train_ransac_masks", "race rounds", rounds, torch.zeros(2 * c["it"]), msg)


@pytest.mark.parametrize("S", [65, 1024])
def test_train_masks_on_device_draws(S):
    """distinct, in range, reproducible, and keyed by the global set index: the last set alone with set_base repeats its draws"""
    dev = _dev()
    g = R.gen("train draws", S)
    nsets, it_r, nc = 3, 5, 8
    X = R.points(g, nsets, S).to(dev)
    w = (torch.rand(nsets, S, generator=g) + 0.05).to(dev)
    a = _train_masks(dev, X, X, w, it_r, 4, nc, seed=11, offset=3, msg="S %d" % S)
    b = _train_masks(dev, X, X, w, it_r, 4, nc, seed=11, offset=3, msg="S %d again" % S)
    idx = a[1].cpu().long()
    srt = idx.sort(1).values
    assert bool((srt[:, 1:] != srt[:, :-1]).all()) and int(idx.min()) >= 0 and int(idx.max()) < S
    for nm, u, v in zip(("mask", "idx", "rounds"), a, b):
        _exact("train_ransac_masks", "draws again " + nm, u, v.cpu(), "S %d" % S)
    last = _train_masks(dev, X[2:].contiguous(), X[2:].contiguous(), w[2:].contiguous(), it_r, 4, nc, seed=11, offset=3, set_base=2,
                        msg="S %d, last set alone" % S)
    _exact("train_ransac_masks", "draws set_base", last[1], a[1][2 * it_r:].cpu(), "S %d" % S)
    other = _train_masks(dev, X, X, w, it_r, 4, nc, seed=12, offset=3, msg="S %d, other seed" % S)
    assert not torch.equal(other[1], a[1])


@pytest.mark.parametrize("S,nc", [(1025, 8), (64, 65)])
def test_train_masks_reject(S, nc):
    dev, nv = _dev(), _nv()
    X = torch.zeros((1, S, 3), device=dev)
    with pytest.raises(nv.MickeyHipError, match="mk_train_ransac_masks: bad sizes"):
        _train_masks(dev, X, X, torch.ones((1, S), device=dev), 4, 4, nc)


# ================================================================ mk_reinforce_scatter ==========================================
@pytest.mark.parametrize("S,it_m", R.SCATTER_CASES)
def test_reinforce_scatter_bit_exact(S, it_m):
    """the same fp32 additions in the same order as the sequential loop, on top of preset values; 600 cells, so rows overlap; cells
    nobody drew keep their preset bits"""
    dev, nv = _dev(), _nv()
    c = R.scatter_case(S, it_m)
    B, ncell = c["B"], R.SCATTER_NCELL
    msg = "S %d, %d rows per pair" % (S, it_m)
    o = Outs(dev)
    g, gb = o.new("gradients", B, ncell, fill=c["pre"]), o.new("gradients_b", B, ncell, fill=c["pre_b"])
    idx, lv = c["idx"].to(dev), c["lv"].to(dev)
    nv.call("mk_reinforce_scatter", nv.ptr(idx), nv.ptr(lv), nv.ptr(g), nv.ptr(gb), B, it_m, S, ncell, nv.stream())
    o.check(msg)
    where = lambda i: "pair %d, cell %d (drawn: %s)" % (i // ncell, i % ncell, bool(c["drawn"].reshape(-1)[i]))  # noqa: E731
    _exact("reinforce_scatter", "gradients", g, c["want"], msg, where)
    _exact("reinforce_scatter", "gradients_b", gb, c["want_b"], msg, where)
    assert torch.equal(g.cpu()[~c["drawn"]], c["pre"][~c["drawn"]])


# ================================================================ mk_train_aggregate_fwd / _bwd =================================
def _aggregate(dev, out, Rt, saved, B, it_m, it_r, temp, add_null, msg):
    nv = _nv()
    nh = B * it_m * it_r
    o = Outs(dev)
    lv, pp, coef = o.new("loss_value", 1, B * it_m), o.new("per_pair", B, 3), o.new("coef", nh, 2)
    flags = o.new("flags", 1, 2, I32, fill=0)
    nv.call("mk_train_aggregate_fwd", nv.ptr(out), nv.ptr(Rt), nv.ptr(saved), B, it_m, it_r, float(temp), int(add_null), float(R.NULL_LOSS),
            float(R.NULL_SCORE), nv.ptr(lv), nv.ptr(pp), nv.ptr(coef), nv.ptr(flags), nv.stream())
    o.check(msg)
    return lv, pp, coef, flags


@pytest.mark.parametrize("B,it_m,it_r,add_null,temp", R.AGG_CASES)
def test_train_aggregate_fwd_elementwise(B, it_m, it_r, add_null, temp):
    """every loss_value, per_pair and coef element against the fp64 softmax (autograd for coef); the rank-one count exact; then one
    non-finite value at the last element of the last hypothesis raises flag 0 and changes nothing else"""
    dev = _dev()
    c = R.aggregate_case(B, it_m, it_r, add_null, temp)
    msg = "B %d, %d sets x %d hypotheses, null %d, temperature %g" % (B, it_m, it_r, add_null, temp)
    d = [c[n].to(dev) for n in ("out", "Rt", "saved")]
    lv, pp, coef, flags = _aggregate(dev, *d, B, it_m, it_r, temp, add_null, msg)
    ref, sc = c["ref"], c["ref"]["scale"]
    _within("train_aggregate_fwd", "loss_value", lv, ref["loss_value"], sc["loss_value"], c["floor"]["loss_value"], msg,
            lambda i: "set %d (pair %d, wave %d)" % (i, i // it_m, (i % it_m) % 4))
    _within("train_aggregate_fwd", "per_pair", pp, ref["per_pair"], sc["per_pair"], c["floor"]["per_pair"], msg, lambda i: "pair %d, column %d" % (i // 3, i % 3))
    _within("train_aggregate_fwd", "coef", coef, ref["coef"], sc["coef"], c["floor"]["coef"], msg,
            lambda i: "hypothesis %d of set %d (lane %d, trip %d), column %d" % ((i // 2) % it_r, i // 2 // it_r, ((i // 2) % it_r) % 64, ((i // 2) % it_r) // 64, i % 2))
    _exact("train_aggregate_fwd", "flags", flags, torch.tensor([0, c["rank1"]]), msg)
    Rt = c["Rt"].clone()
    Rt[-1, -1] = float("inf")
    lv2, pp2, coef2, flags2 = _aggregate(dev, d[0], Rt.to(dev), d[2], B, it_m, it_r, temp, add_null, msg + ", non-finite t")
    _exact("train_aggregate_fwd", "flags (inf)", flags2, torch.tensor([1, c["rank1"]]), msg)
    _exact("train_aggregate_fwd", "coef (inf)", coef2, coef.cpu(), msg)


def test_train_aggregate_fwd_rejects_65_sets():
    dev, nv = _dev(), _nv()
    z = torch.zeros((65 * 32,), device=dev)
    with pytest.raises(nv.MickeyHipError, match="mk_train_aggregate_fwd: bad sizes"):
        _aggregate(dev, z, z, z, 1, 65, 1, 20.0, 0, "65 sets")


@pytest.mark.parametrize("B,it_m,it_r", R.AGG_BWD_CASES)
def test_train_aggregate_bwd_exact(B, it_m, it_r):
    """grad_out = g(pair) x coef: one fp32 product per element, so bit-exact; 255 / 256 / 257 hypotheses"""
    dev, nv = _dev(), _nv()
    g = R.gen("aggregate bwd", B, it_m, it_r)
    nh = B * it_m * it_r
    coef, gp = torch.randn(nh, 2, generator=g), torch.randn(B, generator=g)
    o = Outs(dev)
    out = o.new("grad_out", nh, 2)
    cd, gd = coef.to(dev), gp.to(dev)
    nv.call("mk_train_aggregate_bwd", nv.ptr(cd), nv.ptr(gd), B, it_m, it_r, nv.ptr(out), nv.stream())
    o.check("%d hypotheses" % nh)
    _exact("train_aggregate_bwd", "grad_out", out, gp.repeat_interleave(it_m * it_r)[:, None] * coef, "%d pairs x %d hypotheses" % (B, it_m * it_r),
           lambda i: "hypothesis %d (thread %d of block %d), column %d" % (i // 2, (i // 2) % 256, i // 2 // 256, i % 2))


# ================================================================ mk_train_tail_fwd / _bwd ======================================
def _tail_args(c, dev):
    nv = _nv()
    kind = 1 if c["kind"] == "POSE_ERR" else 0
    d = {n: c[n].to(dev).contiguous() for n in ("X", "Y", "mask", "Rgt", "tgt", "K")}
    nsets, S, _ = c["X"].shape
    head = [nv.ptr(d[n]) for n in ("X", "Y", "mask", "Rgt", "tgt", "K", "K")] + [nsets, c["it_r"], S, R.TAIL_ITM, float(R.TH_SOFT), kind, int(c["soft"]), 720.0]
    return d, head


@pytest.mark.parametrize("S,it_r,kind,soft", R.TAIL_CASES)
def test_train_tail_forward_and_backward(S, it_r, kind, soft):
    """proper and MIRRORED sets, full / eight-match / three-match masks, S at every lane-slot edge: out, R | t, the saved centroids,
    sum_w and d element by element, U diag(S) V^T against H; then the backward on the kernel's own saved state against fp64 autograd
    through the SVD, gX / gY element by element with the per-set scale"""
    dev, nv = _dev(), _nv()
    c = R.tail_case(S, it_r, kind, soft)
    msg = "S %d, %d hypotheses per set, %s, soft clipping %d (seed %d)" % (S, it_r, kind, soft, c["seed"])
    nsets, nh = R.TAIL_B * R.TAIL_ITM, R.TAIL_B * R.TAIL_ITM * it_r
    d, head = _tail_args(c, dev)
    o = Outs(dev)
    out, Rt, saved = o.new("out", nh, 4), o.new("Rt", nh, 12), o.new("saved", nh, 32, fill=0.0)
    nv.call("mk_train_tail_fwd", *head, nv.ptr(out), nv.ptr(Rt), nv.ptr(saved), nv.stream())
    o.check(msg)
    ref, sc, fl = c["ref"], c["scale"], c["floor"]

    def hyp(i, w):
        h = i // w
        return "hypothesis %d = %d of set %d (wave %d, %s set, mask '%s'), column %d" % (h, h % it_r, h // it_r, (h % it_r) % 4,
                                                                                       "mirrored" if (h // it_r) % 2 else "proper", c["kinds"][h], i % w)

    _within("train_tail_fwd", "out", out, ref["out"], sc["out"], fl["out"], msg, lambda i: hyp(i, 4))
    _within("train_tail_fwd", "R | t", Rt, ref["Rt"], sc["Rt"], fl["Rt"], msg, lambda i: hyp(i, 12))
    sv = saved.cpu().double()
    U, V, Sg = sv[:, 0:9].reshape(-1, 3, 3), sv[:, 9:18].reshape(-1, 3, 3), sv[:, 18:21]
    s1 = torch.linalg.svdvals(ref["H"])[:, :1, None]
    r32 = R.tail_ref(c, dtype=torch.float32)
    _within("train_tail_fwd", "U S V^T", U @ torch.diag_embed(Sg) @ V.transpose(1, 2), ref["H"], s1, R.floor32(r32["H"], ref["H"], s1), msg, lambda i: hyp(i, 9))
    assert bool((Sg[:, 0] >= Sg[:, 1]).all() and (Sg[:, 1] >= Sg[:, 2]).all() and (Sg[:, 2] >= 0).all())
    cs = torch.maximum(c["am"].norm(dim=1), c["bm"].norm(dim=1)).clamp_min(1.0)[:, None]
    _within("train_tail_fwd", "centroids", sv[:, 22:28], torch.cat([c["am"], c["bm"]], 1), cs, 0.0, msg, lambda i: hyp(i, 6))
    _exact("train_tail_fwd", "sum_w", saved[:, 28], c["sw"], msg)
    dref = torch.sign(torch.linalg.det(ref["H"]))
    _exact("train_tail_fwd", "d", saved[:, 21][c["full"].to(dev)], dref[c["full"]], msg)      # (rank two: the sign of the third pair is free)
    assert bool((saved[:, 21].abs() == 1).all()) and int((dref[c["full"]] < 0).sum()) > 0
    # backward, on the kernel's own Rt / saved as ops.train_tail_bwd does
    go = c["grad_out"].to(dev)
    ob = Outs(dev)
    work, gX, gY = ob.new("work", nh, 16), ob.new("gX", nsets * S, 3), ob.new("gY", nsets * S, 3)
    nv.call("mk_train_tail_bwd", *head, nv.ptr(Rt), nv.ptr(saved), nv.ptr(go), nv.ptr(work), nv.ptr(gX), nv.ptr(gY), nv.stream())
    ob.check(msg + ", backward")
    o.check(msg + ", forward outputs after the backward")

    def pt(i):
        j = (i // 3) % S
        r = i // (3 * S)
        inmask = [h for h in range(it_r) if float(c["mask"][r * it_r + h, j]) != 0]
        return "set %d (%s), %s, axis %d; in the masks of hypotheses %s" % (r, "mirrored" if r % 2 else "proper", R.lane_slot(j), i % 3, inmask)

    _within("train_tail_bwd", "gX", gX, ref["gX"], sc["gX"], fl["gX"], msg, pt)
    _within("train_tail_bwd", "gY", gY, ref["gY"], sc["gY"], fl["gY"], msg, pt)
    outside = c["mask"].reshape(nsets, it_r, S).sum(1) == 0            # a match outside every mask still gets its score-term gradient
    if bool(outside.any()):
        assert bool((gX.view(nsets, S, 3).cpu()[outside].abs().sum(-1) > 0).all())


def test_train_tail_rejects_1025_matches():
    dev, nv = _dev(), _nv()
    z = torch.zeros((1025 * 3,), device=dev)
    with pytest.raises(nv.MickeyHipError, match="mk_train_tail: bad sizes"):
        nv.call("mk_train_tail_fwd", nv.ptr(z), nv.ptr(z), nv.ptr(z), nv.ptr(z), nv.ptr(z), None, None, 1, 1, 1025, 1, 0.3, 1, 0, 720.0, nv.ptr(z), nv.ptr(z),
                nv.ptr(z), nv.stream())


def test_train_tail_isotropic_set_is_finite_and_right():
    """H with three equal singular values (exactly equal in the even sets): R, t and every gradient finite; gX / gY against fp64
    central differences of the whole tail -- torch's SVD backward is not finite here, the header's closed form is"""
    dev, nv = _dev(), _nv()
    c = R.isotropic_case()
    msg = "isotropic sets"
    nsets, S = c["X"].shape[:2]
    d, head = _tail_args(c, dev)
    o = Outs(dev)
    out, Rt, saved = o.new("out", nsets, 4), o.new("Rt", nsets, 12), o.new("saved", nsets, 32, fill=0.0)
    nv.call("mk_train_tail_fwd", *head, nv.ptr(out), nv.ptr(Rt), nv.ptr(saved), nv.stream())
    o.check(msg)
    ref = R.tail_ref(c)
    r32 = R.tail_ref(c, dtype=torch.float32)
    one = torch.ones((), dtype=torch.float64)
    _within("train_tail_fwd", "R | t (iso)", Rt, ref["Rt"], one, R.floor32(r32["Rt"], ref["Rt"], one), msg, lambda i: "set %d, element %d" % (i // 12, i % 12))
    Sg = saved[:, 18:21].cpu()
    assert bool((Sg[0::2] == 2.0).all()), Sg                        # the quarter-turn sets: exactly equal singular values
    assert float((Sg - 2.0).abs().max()) < 1e-5 and bool((saved[:, 21] == 1).all())
    go = c["grad_out"].to(dev)
    ob = Outs(dev)
    work, gX, gY = ob.new("work", nsets, 16), ob.new("gX", nsets * S, 3), ob.new("gY", nsets * S, 3)
    nv.call("mk_train_tail_bwd", *head, nv.ptr(Rt), nv.ptr(saved), nv.ptr(go), nv.ptr(work), nv.ptr(gX), nv.ptr(gY), nv.stream())
    ob.check(msg + ", backward")
    assert bool(torch.isfinite(gX).all() and torch.isfinite(gY).all())
    where = lambda i: "set %d (%s), match %d (%s), axis %d" % (i // (3 * S), "exact" if (i // (3 * S)) % 2 == 0 else "to rounding", (i // 3) % S,  # noqa: E731
                                                                "octahedron" if (i // 3) % S < 6 else "outside the mask", i % 3)
    _within("train_tail_bwd", "gX (iso)", gX, c["ref"]["gX"], c["scale"]["gX"], c["floor"]["gX"], msg, where)
    _within("train_tail_bwd", "gY (iso)", gY, c["ref"]["gY"], c["scale"]["gY"], c["floor"]["gY"], msg, where)
    assert bool((gX.view(nsets, S, 3)[:, 6:].abs().sum(-1) > 0).all())     # outside every mask: the score term alone
