"""-m gpu: the probabilistic-Procrustes solver kernels, stage-isolated against the CPU oracle with the
random draws INJECTED (SURVEY.md 8(c) parity protocol): sampled indices bit-exact, poses within 1e-4
Frobenius, plus seed-free statistical checks of the on-device Philox path (planted-pose recovery)."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _small_cfg(cfg, it_m=4, it_r=25):
    c = copy.deepcopy(cfg)
    c["PROCRUSTES"]["IT_MATCHES"] = it_m
    c["PROCRUSTES"]["IT_RANSAC"] = it_r
    return c


def _problem(B=3, h=14, w=12, seed=4321):
    from mickey_amd import synthetic as syn
    return syn.planted_pose_problem(B=B, h=h, w=w, seed=seed, angle_deg=(1.0, 1.5), t_norm=(0.03, 0.04))


def _assert_same_sample(idx, ref, keys):
    """Bit-exact index parity up to the order of EXACTLY tied keys (torch.topk's tie order is unspecified;
    with 2048 fp32 keys per row a tie happens about once in ten rows)."""
    idx = idx.cpu().long()
    diff = idx != ref
    if diff.any():
        assert torch.equal(torch.gather(keys, 1, idx), torch.gather(keys, 1, ref)), "sampled keys differ"
        assert torch.equal(idx.sort(1).values, ref.sort(1).values), "sampled sets differ"
        assert int(diff.sum()) <= 2 * max(2, idx.shape[0] // 2), "too many tie swaps: %d" % int(diff.sum())


def _to(d, dev):
    return {k: (v.to(dev).contiguous() if torch.is_tensor(v) else v) for k, v in d.items()}


def test_sampler_injected_noise_bit_exact():
    """mk_exprace_topk == torch.topk(p / noise) index for index, order included."""
    from mickey_amd import ops
    dev = _dev()
    data, _, _ = _problem()
    fs = data["final_scores"]
    B, n, _ = fs.shape
    rows = 5
    noise = torch.empty((B * rows, n * n)).exponential_(1.0, generator=torch.Generator().manual_seed(3))
    keys = fs.reshape(B, 1, n * n).expand(B, rows, n * n).reshape(B * rows, n * n) / noise
    ref = torch.topk(keys, 2048).indices
    idx, cnt = ops.exprace_topk(fs.reshape(B, n * n).to(dev), rows, 2048, noise=noise.to(dev))
    assert (cnt.cpu() == 2048).all()
    _assert_same_sample(idx, ref, keys)


def test_sampler_full_size_bit_exact():
    """Full Map-free size: 2048 of 1938^2 cells x 20 rows, ~45 % zero cells (border-masked scores)."""
    from mickey_amd import ops
    dev = _dev()
    n, rows = 1938, 20
    g = torch.Generator().manual_seed(9)
    s0 = torch.rand(n, generator=g) * (torch.rand(n, generator=g) > 0.25)
    s1 = torch.rand(n, generator=g) * (torch.rand(n, generator=g) > 0.25)
    fs = (s0[:, None] * s1[None, :] * torch.rand((n, n), generator=g).pow(8) * 1e-7).reshape(1, n * n)
    noise = torch.empty((rows, n * n)).exponential_(1.0, generator=g)
    keys = fs.expand(rows, -1) / noise
    ref = torch.topk(keys, 2048).indices
    idx, cnt = ops.exprace_topk(fs.to(dev), rows, 2048, noise=noise.to(dev))
    assert (cnt.cpu() == 2048).all()
    _assert_same_sample(idx, ref, keys)


@pytest.mark.parametrize("scale", [30.0, 1.0 / 200.0])
def test_sampler_exact_fallback(scale):
    """Noise that is NOT Exp(1)-distributed defeats the analytic threshold (too few / too many candidates above it): the
    on-device exact histogram path must take over and still return torch.topk(p / noise)."""
    from mickey_amd import ops
    dev = _dev()
    data, _, _ = _problem(B=2)
    fs = data["final_scores"]
    B, n, _ = fs.shape
    rows = 4
    g = torch.Generator().manual_seed(11)
    noise = torch.empty((B * rows, n * n)).exponential_(1.0, generator=g) * scale
    keys = fs.reshape(B, 1, n * n).expand(B, rows, n * n).reshape(B * rows, n * n) / noise
    ref = torch.topk(keys, 2048).indices
    idx, cnt = ops.exprace_topk(fs.reshape(B, n * n).to(dev), rows, 2048, noise=noise.to(dev))
    assert (cnt.cpu() == 2048).all()
    _assert_same_sample(idx, ref, keys)


def test_sampler_philox_properties():
    from mickey_amd import ops
    dev = _dev()
    data, _, _ = _problem(B=2)
    fs = data["final_scores"]
    B, n, _ = fs.shape
    p = fs.reshape(B, n * n).to(dev)
    a, ca = ops.exprace_topk(p, 20, 2048, seed=7, offset=1)
    b, _ = ops.exprace_topk(p, 20, 2048, seed=7, offset=1)
    c, _ = ops.exprace_topk(p, 20, 2048, seed=7, offset=2)
    assert torch.equal(a, b), "same (seed, offset) must reproduce the same draw"
    assert not torch.equal(a, c)
    a = a.cpu().long()
    assert (ca.cpu() == 2048).all()
    for r in range(a.shape[0]):
        assert a[r].unique().numel() == 2048  # without replacement
    # planted cells carry ~1000x the background weight: (almost) all of them must be drawn in every row
    planted = (fs.reshape(B, -1) > 1e-7)
    for r in range(a.shape[0]):
        hit = planted[r // 20][a[r]].sum().item()
        assert hit >= 0.98 * planted[r // 20].sum().item()
    # keys are sorted in descending order of p/e: a weak consequence is that the first half holds more
    # planted cells than the second half
    first = sum(planted[r // 20][a[r, :1024]].sum().item() for r in range(a.shape[0]))
    second = sum(planted[r // 20][a[r, 1024:]].sum().item() for r in range(a.shape[0]))
    assert first > second


def test_sampler_many_rows_and_frequencies():
    """On-device draws, 40 rows per pair (several row groups of the skip sampler): inclusion frequencies of a skewed 4096-cell
    problem over 40 rows x 30 calls must match torch.multinomial's (two-sample chi-square), and every row is a valid draw.
    (k / ncell = 6 %: the skip sampler takes its dense branch for most blocks here; the 10 000-cell test in
    test_bench_config_gpu.py and the one below run its skipping branch.)"""
    from mickey_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(11)
    ncell, k, rows = 4096, 256, 40
    p = (torch.rand(1, ncell, generator=g) ** 6 + 1e-4)
    p[0, :50] += 3.0                       # a few dominant cells (their blocks are tested densely)
    f_hip = torch.zeros(ncell, dtype=torch.float64)
    for call in range(30):
        idx, cnt = ops.exprace_topk(p.to(dev), rows, k, seed=3, offset=call)
        idx = idx.cpu().long()
        assert (cnt.cpu() == k).all()
        srt = torch.sort(idx, -1).values
        assert bool((srt[:, 1:] != srt[:, :-1]).all())
        assert not torch.equal(idx[3], idx[23])    # rows of different groups are different draws
        f_hip += torch.bincount(idx.reshape(-1), minlength=ncell).double()
    f_ref = torch.bincount(torch.multinomial(p.expand(rows * 30, ncell), k, generator=g).reshape(-1), minlength=ncell).double()
    keep = (f_hip + f_ref) >= 10
    chi2 = float((((f_hip - f_ref) ** 2) / (f_hip + f_ref))[keep].sum())
    dof = int(keep.sum())
    assert chi2 < dof + 6 * (2 * dof) ** 0.5, (chi2, dof)


def test_sampler_first_draw_is_categorical_and_sparse_frequencies():
    """(a) The first index of a row is the arg-max of the race keys = ONE categorical draw ~ p (what torch.multinomial draws
    first): one-sample chi-square of 61 440 first draws against p / sum(p).  This pins the law of the race KEYS the on-device
    generator produces (the skip sampler draws them from Exp(1) conditioned on the key clearing the threshold), not only which
    cells are included.  (b) 65 536 cells, k = 256 (inclusion ~4e-3: the skipping branch, several workgroup ranges, a few
    dominant cells that turn their blocks dense): two-sample chi-square of the inclusion counts against torch.multinomial."""
    from mickey_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(5)
    ncell, k, rows, B = 3000, 128, 40, 64
    p = torch.rand(ncell, generator=g) ** 4 + 1e-3
    p[::11] = 0.0
    p[5] = 40.0                                   # one dominant cell
    pd = p.to(dev)[None].repeat(B, 1).contiguous()
    first = torch.zeros(ncell, dtype=torch.float64)
    for call in range(24):
        idx, cnt = ops.exprace_topk(pd, rows, k, seed=21, offset=call)
        first += torch.bincount(idx[:, 0].cpu().long(), minlength=ncell).double()
    n = first.sum()
    assert n == 24 * B * rows
    exp = (p.double() / p.double().sum()) * n
    sel = exp >= 8
    rest_o, rest_e = first[~sel].sum(), exp[~sel].sum()
    chi2 = float((((first - exp) ** 2) / exp)[sel].sum() + (rest_o - rest_e) ** 2 / max(float(rest_e), 1e-9))
    df = int(sel.sum())
    assert abs(chi2 - df) < 5.0 * (2.0 * df) ** 0.5, (chi2, df)
    assert float(first[::11].sum()) == 0.0

    ncell, k, rows, B = 65536, 256, 20, 8
    p = torch.rand(ncell, generator=g) ** 8 + 1e-5
    p[torch.randperm(ncell, generator=g)[:40]] += 2.0
    pd = p.to(dev)[None].repeat(B, 1).contiguous()
    f_hip = torch.zeros(ncell, dtype=torch.float64)
    for call in range(12):
        idx, cnt = ops.exprace_topk(pd, rows, k, seed=9, offset=call, pair_base=8 * call)
        assert int(cnt.min()) == k
        srt = idx.long().sort(dim=1).values
        assert bool((srt[:, 1:] != srt[:, :-1]).all())
        f_hip += torch.bincount(idx.reshape(-1).cpu().long(), minlength=ncell).double()
    torch.manual_seed(2)
    f_ref = torch.zeros(ncell, dtype=torch.float64)
    for _ in range(12):
        f_ref += torch.bincount(torch.multinomial(pd[0][None].expand(B * rows, -1), k).reshape(-1).cpu(), minlength=ncell).double()
    # pool the many low-count cells by magnitude of p so that every bin is populated
    order = torch.argsort(p)
    a, b = f_hip[order], f_ref[order]
    nb = 512
    a, b = a.reshape(nb, -1).sum(1), b.reshape(nb, -1).sum(1)
    sel = (a + b) >= 20
    df = int(sel.sum()) - 1
    chi2 = float((((a - b) ** 2) / (a + b))[sel].sum())
    assert abs(chi2 - df) < 5.0 * (2.0 * df) ** 0.5, (chi2, df)


def test_sampler_queue_overflow_takes_the_exact_fallback():
    """One spike per 16-cell block: every block of the skip sampler's walk is a hit for most rows (rate bound 0.08 per cell, just
    under the dense cut), ~3000 hits per row where the workgroup's queue holds 1024 -> `redo` is raised on the device and the
    exact histogram passes redo the call.  The result must still be a valid weighted draw: k distinct cells, (almost) all of
    them spikes, inclusion counts of the spikes flat (chi-square against the uniform expectation)."""
    from mickey_amd import ops
    dev = _dev()
    ncell, k, rows, B = 65536, 256, 20, 4
    p = torch.full((ncell,), 1e-7)
    spikes = torch.arange(0, ncell, 16) + 5
    p[spikes] = 1.0
    pd = p.to(dev)[None].repeat(B, 1).contiguous()
    counts = torch.zeros(ncell, dtype=torch.float64)
    for call in range(6):
        idx, cnt = ops.exprace_topk(pd, rows, k, seed=4, offset=call)
        assert int(cnt.min()) == k
        srt = idx.long().sort(dim=1).values
        assert bool((srt[:, 1:] != srt[:, :-1]).all())
        counts += torch.bincount(idx.reshape(-1).cpu().long(), minlength=ncell).double()
    on = counts[spikes]
    assert on.sum() >= 0.995 * counts.sum()
    exp = on.sum() / len(spikes)
    chi2 = float(((on - exp) ** 2 / exp).sum())
    df = len(spikes) - 1
    assert abs(chi2 - df) < 5.0 * (2.0 * df) ** 0.5, (chi2, df)


def test_sampler_workspace_cleans_itself():
    """The chain has no zero-fill launch (mickey_hip.h): the state words at the head of the workspace are zero after every call --
    an ordinary one, one whose pair takes the exact fallback, one with injected noise -- so ONE buffer, zeroed at allocation,
    serves call after call with the results of a fresh buffer."""
    from mickey_amd import ops
    from mickey_amd._native import query
    dev = _dev()
    ncell, k, rows, B = 65536, 256, 20, 4
    gen = torch.Generator().manual_seed(9)
    benign = (torch.rand((B, ncell), generator=gen) + 0.5) * 1e-5
    spike = torch.full((ncell,), 1e-7)
    spike[torch.arange(0, ncell, 16) + 5] = 1.0
    mixed = benign.clone()
    mixed[2] = spike
    noise = -torch.log(torch.rand((B * rows, ncell), generator=gen).clamp_min(1e-12))
    benign, mixed, noise = benign.to(dev).contiguous(), mixed.to(dev).contiguous(), noise.to(dev)
    work = ops.exprace_work(B, rows, k, ncell, dev)
    nstate = query("mk_exprace_topk_state_bytes", B, rows)
    assert 0 < nstate < work.numel()
    for it, (pmat, nz) in enumerate(((benign, None), (mixed, None), (benign, noise), (benign, None), (mixed, None))):
        got = ops.exprace_topk(pmat, rows, k, noise=nz, seed=4, offset=it, work=work)
        assert int(work[:nstate].count_nonzero()) == 0, it
        ref = ops.exprace_topk(pmat, rows, k, noise=nz, seed=4, offset=it)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), it
    keys = (benign.repeat_interleave(rows, 0) / noise).cpu()
    _assert_same_sample(ops.exprace_topk(benign, rows, k, noise=noise, work=work)[0], torch.topk(keys, k, dim=1).indices, keys)


def test_sampler_overflow_of_one_pair_leaves_the_others_alone():
    """`redo` is per pair: a batch in which ONE pair overflows the skip sampler's queue (the spike matrix of the test above) sends
    that pair through the exact fallback -- and the other pairs' draws are bit-identical to the same pairs in a batch where
    nothing overflows (same seed / offset / pair positions): a pair's result does not depend on the batch it is in."""
    from mickey_amd import ops
    dev = _dev()
    ncell, k, rows, B = 65536, 256, 20, 4
    gen = torch.Generator().manual_seed(9)
    benign = (torch.rand((B, ncell), generator=gen) + 0.5) * 1e-5
    spike = torch.full((ncell,), 1e-7)
    spikes = torch.arange(0, ncell, 16) + 5
    spike[spikes] = 1.0
    mixed = benign.clone()
    mixed[2] = spike
    idx_b, cnt_b = ops.exprace_topk(benign.to(dev).contiguous(), rows, k, seed=4, offset=7)
    idx_m, cnt_m = ops.exprace_topk(mixed.to(dev).contiguous(), rows, k, seed=4, offset=7)
    ib, im = idx_b.reshape(B, rows, k), idx_m.reshape(B, rows, k)
    for pair in (0, 1, 3):
        assert torch.equal(ib[pair], im[pair]), pair
    assert int(cnt_m.min()) == k
    on_spikes = torch.isin(im[2].reshape(-1).cpu().long(), spikes).float().mean()
    assert float(on_spikes) > 0.99                      # the overflowing pair still gets a valid weighted draw
    srt = im[2].long().sort(dim=1).values
    assert bool((srt[:, 1:] != srt[:, :-1]).all())


def test_sampler_fallback_decision_does_not_depend_on_the_schedule():
    """Short rows are the rule here: near-flat p, k = 16 while the analytic threshold aims at 20 candidates per row, so almost
    every pair has a row below k and takes the exact fallback -- 512 pairs x 5 row groups of its 1024-thread workgroups, far
    more than the chip holds at once.  Whether a pair is redone must be decided the same way by all its workgroups in any
    order: two identical calls agree, and pairs of the batch (the last ones included) equal the same pair run alone with
    pair_base = its index."""
    from mickey_amd import ops
    dev = _dev()
    ncell, k, rows, B = 3000, 16, 20, 512
    p = torch.rand(ncell, generator=torch.Generator().manual_seed(17)) * 0.5 + 0.5
    pd = p.to(dev)[None].repeat(B, 1).contiguous()
    a, ca = ops.exprace_topk(pd, rows, k, seed=5, offset=3)
    b, cb = ops.exprace_topk(pd, rows, k, seed=5, offset=3)
    assert torch.equal(a, b) and torch.equal(ca, cb)
    assert int(ca.min()) == k
    srt = a.long().sort(dim=1).values
    assert bool((srt[:, 1:] != srt[:, :-1]).all())
    a = a.reshape(B, rows, k)
    for pair in (0, 1, 97, 300, B - 3, B - 2, B - 1):
        alone, _ = ops.exprace_topk(pd[pair:pair + 1], rows, k, seed=5, offset=3, pair_base=pair)
        assert torch.equal(alone, a[pair]), pair


def test_sampler_failed_call_leaves_a_clean_workspace(monkeypatch):
    """A call that raises may have stopped between the chain's launches and left state words behind: the wrapper zeroes the
    state of the caller's buffer before the error propagates, so the next call on the same buffer equals one on a fresh buffer."""
    from mickey_amd import ops
    from mickey_amd._native import MickeyHipError, query
    dev = _dev()
    ncell, k, rows, B = 65536, 256, 20, 4
    p = ((torch.rand((B, ncell), generator=torch.Generator().manual_seed(3)) + 0.5) * 1e-5).to(dev)
    work = ops.exprace_work(B, rows, k, ncell, dev)
    nstate = query("mk_exprace_topk_state_bytes", B, rows)
    real_call = ops.call

    def failing_call(name, *args):
        if name == "mk_exprace_topk":
            work[:nstate].fill_(0x5A)   # counts, flags and histograms of a chain that stopped half-way
            raise MickeyHipError("mk_exprace_topk failed (injected)")
        return real_call(name, *args)

    monkeypatch.setattr(ops, "call", failing_call)
    with pytest.raises(MickeyHipError, match="injected"):
        ops.exprace_topk(p, rows, k, seed=4, offset=1, work=work)
    monkeypatch.undo()
    assert int(work[:nstate].count_nonzero()) == 0
    got = ops.exprace_topk(p, rows, k, seed=4, offset=1, work=work)
    ref = ops.exprace_topk(p, rows, k, seed=4, offset=1)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])


def test_sampler_degenerate_inputs():
    from mickey_amd import ops
    dev = _dev()
    p = torch.zeros((2, 5000))
    p[0, :100] = 1.0       # fewer positive cells than k
    p[1, :] = 0.5
    inv = torch.zeros(1, dtype=torch.int32, device=dev)
    idx, cnt = ops.exprace_topk(p.to(dev), 3, 2048, seed=1, invalid=inv)
    assert cnt.cpu().tolist() == [100, 100, 100, 2048, 2048, 2048] and int(inv) == 0
    assert set(idx[0, :100].cpu().tolist()) == set(range(100))
    assert idx[0, 100:].cpu().tolist() == list(range(100, 2048))  # zero-probability tail in index order
    for bad in (float("nan"), float("inf"), -1.0):
        q = p.clone()
        q[1, 17] = bad
        inv.zero_()
        ops.exprace_topk(q.to(dev), 3, 2048, seed=1, invalid=inv)
        assert int(inv) == 1
    inv.zero_()
    ops.exprace_topk(torch.zeros((1, 5000), device=dev), 3, 2048, seed=1, invalid=inv)
    assert int(inv) == 1   # sum of probabilities <= 0


def test_solver_stages_vs_oracle(cfg):
    from mickey_amd import ops
    from oracle import mickey_oracle as O
    dev = _dev()
    scfg = _small_cfg(cfg)
    it_m, it_r = 4, 25
    data, _, _ = _problem()
    B, n, _ = data["final_scores"].shape
    torch.manual_seed(5)
    Ro, to, co, dbg = O.estimate_pose({k: v.clone() for k, v in data.items()}, scfg, return_debug=True)
    d = _to(data, dev)
    # (1) gathers + back-projection on the oracle's indices
    X, Y, w, corr = ops.gather_backproject(dbg["idx"].int().to(dev), d["final_scores"], d["kps0"], d["depth_kp0"], d["kps1"],
                                           d["depth_kp1"], d["K_color0"], d["K_color1"], it_m)
    assert torch.allclose(X.cpu(), dbg["X"], rtol=1e-5, atol=1e-6) and torch.allclose(Y.cpu(), dbg["Y"], rtol=1e-5, atol=1e-6)
    assert torch.equal(w.cpu(), dbg["weights"])
    # (2) inner sampler with the oracle's noise: indices bit-exact
    Rh, th, sc, idx3 = ops.ransac_hypotheses(dbg["X"].to(dev), dbg["Y"].to(dev), dbg["weights"].to(dev), it_r, 0.3,
                                             noise3=dbg["noise_inner"].to(dev))
    assert torch.equal(idx3.cpu().long(), dbg["idx3"])
    # (3) hypotheses: R, t within 1e-4 Frobenius on non-degenerate samples, scores within 1e-3
    S = torch.linalg.svdvals(dbg["H_hyp"].double())
    ok = (S[:, 1] / S[:, 0]) > 1e-3
    assert ok.float().mean() > 0.9
    dR = (Rh.cpu().reshape(-1, 3, 3) - dbg["R_hyp"]).norm(dim=(1, 2))
    dt = (th.cpu().reshape(-1, 1, 3) - dbg["t_hyp"]).norm(dim=(1, 2))
    assert float(dR[ok].max()) < 1e-4 and float(dt[ok].max()) < 1e-4, (float(dR[ok].max()), float(dt[ok].max()))
    det = torch.linalg.det(Rh.cpu().reshape(-1, 3, 3).double())
    assert torch.isfinite(Rh).all() and float((det - 1).abs().max()) < 1e-5     # also for degenerate samples
    assert float((sc.cpu()[ok] - dbg["score"].reshape(-1)[ok]).abs().max()) < 1e-3
    # explicit-index injection gives the same result
    Rh2, th2, sc2, _ = ops.ransac_hypotheses(dbg["X"].to(dev), dbg["Y"].to(dev), dbg["weights"].to(dev), it_r, 0.3,
                                             idx3_in=dbg["idx3"].int().to(dev))
    assert torch.equal(Rh2, Rh) and torch.equal(sc2, sc)
    # (4) arg-max + refinement on the oracle's hypotheses
    R, t, conf, best, mask, rounds, inv = ops.refine_pose(
        dbg["X"].to(dev), dbg["Y"].to(dev), dbg["R_hyp"].reshape(-1, 9).to(dev), dbg["t_hyp"].reshape(-1, 3).to(dev),
        dbg["score"].reshape(-1).to(dev), B, it_m, it_r, 0.15, 4, 3)
    assert torch.equal(best.cpu().long(), dbg["best"]) and int(inv) == 0
    assert float((R.cpu() - Ro).norm(dim=(1, 2)).max()) < 1e-4 and float((t.cpu() - to).norm(dim=(1, 2)).max()) < 1e-4
    assert torch.allclose(conf.cpu(), co, rtol=1e-3, atol=1e-3)
    ref_mask = O.hard_inliers(dbg["X_best"], dbg["Y_best"], Ro, to, 0.15)
    assert (mask.cpu().float() != ref_mask).sum() <= 2    # exact except points on the threshold


def test_solver_end_to_end_injected_noise(cfg):
    from mickey_amd import pipeline
    from oracle import mickey_oracle as O
    dev = _dev()
    scfg = _small_cfg(cfg)
    data, _, _ = _problem()
    d = _to(data, dev)
    B, n, _ = data["final_scores"].shape
    compared = 0
    for seed in range(12, 18):
        torch.manual_seed(seed)
        Ro, to, co, inl, dbg = O.estimate_pose({k: v.clone() for k, v in data.items()}, scfg, return_inliers=True,
                                               return_debug=True)
        sol = pipeline.solve(scfg, d["final_scores"], d["kps0"], d["depth_kp0"], d["kps1"], d["depth_kp1"], d["K_color0"],
                             d["K_color1"], noise_outer=dbg["noise_outer"].to(dev), noise_inner=dbg["noise_inner"].to(dev),
                             debug=True)
        keys = data["final_scores"].reshape(B, 1, n * n).expand(B, 4, n * n).reshape(B * 4, n * n) / dbg["noise_outer"]
        _assert_same_sample(sol["idx"], dbg["idx"], keys)
        if not torch.equal(sol["idx"].cpu().long(), dbg["idx"]):
            continue   # an exact key tie re-ordered two correspondences: downstream draws are not comparable
        compared += 1
        assert torch.equal(sol["idx3"].cpu().long(), dbg["idx3"])
        # hypothesis scores agree; our winner is (one of) the oracle's best within round-off.  Many hypotheses
        # drawn from planted inliers score identically to ~1e-5, so the arg-max itself is only pinned when equal
        sc = sol["score"].cpu().reshape(B, -1)
        S = torch.linalg.svdvals(dbg["H_hyp"].double())
        ok = ((S[:, 1] / S[:, 0]) > 1e-2).reshape(B, -1)    # fp32 SVD error of the reference ~ 1e-7 / (s2/s1)
        assert float((sc - dbg["score"])[ok].abs().max()) < 5e-3
        mine = sol["best"].cpu().long()
        ar = torch.arange(B)
        assert float((dbg["score"].max(1).values - dbg["score"][ar, mine]).max()) < 4e-3
        same = mine == dbg["best"]
        dR = (sol["R"].cpu() - Ro).norm(dim=(1, 2))
        dt = (sol["t"].cpu() - to).norm(dim=(1, 2))
        assert float(dR[same].max() if same.any() else 0) < 1e-4 and float(dt[same].max() if same.any() else 0) < 1e-4
        assert float(dR.max()) < 2e-2 and float(dt.max()) < 2e-2        # equally-scored winners: same planted pose
        assert torch.allclose(sol["inliers"].cpu()[same], co[same], rtol=1e-3, atol=1e-3)
        lst = pipeline.inliers_list(sol)
        for b, (a, r) in enumerate(zip(lst, inl)):
            assert a.shape[1] == 7
            if bool(same[b]):
                assert abs(a.shape[0] - r.shape[0]) <= 2
                if a.shape == r.shape:
                    assert torch.allclose(a.cpu(), r, rtol=1e-4, atol=1e-5)
        compared += 100
    assert compared >= 100, "no seed gave a tie-free comparison"


def test_solver_golden(golden, cfg):
    """Against the REFERENCE's own solver output (tests/golden/solver.npz): its sampled index sets are
    re-injected, so the pose must match the reference to 1e-4."""
    from mickey_amd import ops
    dev = _dev()
    g = golden("solver")
    data, _, _ = _problem()
    d = _to(data, dev)
    it_m, it_r, B = 4, 25, 3
    X, Y, w, _ = ops.gather_backproject(torch.from_numpy(g["idx"]).to(dev), d["final_scores"], d["kps0"], d["depth_kp0"],
                                        d["kps1"], d["depth_kp1"], d["K_color0"], d["K_color1"], it_m)
    Rh, th, sc, _ = ops.ransac_hypotheses(X, Y, w, it_r, 0.3, idx3_in=torch.from_numpy(g["idx3"]).to(dev))
    # hypothesis scores match the reference's; its arg-max is (one of) ours -- many hypotheses drawn from the
    # planted inliers score within round-off of each other, so an exact arg-max match is only required when the
    # reference's own top-2 gap is above the score tolerance
    ref_sc = torch.from_numpy(g["score"])
    from oracle import mickey_oracle as O
    i3 = torch.from_numpy(g["idx3"]).long()
    gsel = torch.arange(B * it_m).repeat_interleave(it_r)[:, None].expand(-1, 3)
    _, _, H = O.kabsch(X.cpu()[gsel, i3], Y.cpu()[gsel, i3])
    S = torch.linalg.svdvals(H.double())
    ok = ((S[:, 1] / S[:, 0]) > 1e-2).reshape(B, -1)      # near-collinear triples: R is ill-conditioned in fp32
    assert float((sc.cpu().reshape(B, -1) - ref_sc)[ok].abs().max()) < 5e-3
    ref_best = torch.from_numpy(g["best"]).long()
    mine = sc.cpu().reshape(B, -1)
    assert float((mine.max(1).values - mine[torch.arange(B), ref_best]).max()) < 2e-3
    top2 = ref_sc.topk(2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > 4e-3
    forced = sc.clone().reshape(B, -1)
    forced[torch.arange(B), ref_best.to(dev)] += 1.0     # continue from the reference's winner
    R, t, conf, best, _, _, _ = ops.refine_pose(X, Y, Rh, th, forced.reshape(-1), B, it_m, it_r, 0.15, 4, 3)
    assert torch.equal(best.cpu().long(), ref_best)
    assert torch.equal(mine.argmax(1)[clear], ref_best[clear])
    assert float((R.cpu() - torch.from_numpy(g["R"])).norm(dim=(1, 2)).max()) < 1e-4
    assert float((t.cpu() - torch.from_numpy(g["t"])).norm(dim=(1, 2)).max()) < 1e-4
    assert torch.allclose(conf.cpu(), torch.from_numpy(g["conf"]), rtol=1e-3, atol=1e-3)


def test_planted_pose_recovery_full_size(cfg):
    """Seed-free check of the Philox path at the Map-free size (51x38 grid, 20x100 hypotheses): the
    planted pose must be recovered (the reference lands at <= 3e-4 / 1.4e-3 on this family)."""
    from mickey_amd import pipeline
    from mickey_amd import synthetic as syn
    dev = _dev()
    data, Rgt, tgt = syn.planted_pose_problem(B=3, h=51, w=38, seed=4321)
    d = _to(data, dev)
    for off in (0, 10):
        sol = pipeline.solve(cfg, d["final_scores"], d["kps0"], d["depth_kp0"], d["kps1"], d["depth_kp1"], d["K_color0"],
                             d["K_color1"], seed=123, offset=off)
        eR = (sol["R"].cpu() - Rgt).norm(dim=(1, 2))
        et = (sol["t"].cpu() - tgt).norm(dim=(1, 2))
        assert float(eR.max()) < 5e-3 and float(et.max()) < 2e-2, (eR, et)
        assert float(sol["inliers"].min()) > 50


def test_zero_pose_on_invalid_matrix(cfg):
    from mickey_amd import pipeline
    dev = _dev()
    scfg = _small_cfg(cfg, 2, 5)
    data, _, _ = _problem(B=2)
    d = _to(data, dev)
    for kind in ("zeros", "nan"):
        fs = torch.zeros_like(d["final_scores"]) if kind == "zeros" else d["final_scores"].clone()
        if kind == "nan":
            fs[1, 3, 3] = float("nan")
        sol = pipeline.solve(scfg, fs, d["kps0"], d["depth_kp0"], d["kps1"], d["depth_kp1"], d["K_color0"], d["K_color1"])
        assert float(sol["R"].abs().sum()) == 0 and float(sol["t"].abs().sum()) == 0 and float(sol["inliers"].abs().sum()) == 0


def test_inner_three_sample_is_sequential_sampling_without_replacement():
    """The on-device draw of a hypothesis' 3 correspondences (probabilisticProcrustes.py:251: torch.multinomial(weights, 3)):
    sequential sampling through the prefix sums of the set's weights.  Against torch.multinomial on the same weights --
    frequencies of the FIRST pick, of the SECOND pick and of inclusion, two-sample chi-square each (the top-3 of an exponential
    race and sequential sampling without replacement are the same Plackett-Luce law, order included); never a repeated or a
    zero-weight index; draws keyed by the global hypothesis index (set_base) and reproducible."""
    import math
    from mickey_amd import ops
    dev = _dev()
    k, nsets, it_r = 96, 600, 100
    g = torch.Generator().manual_seed(5)
    w = torch.rand((k,), generator=g) ** 5 + 1e-3          # heavy tail: pick probabilities from 4e-4 to 0.1
    w[::9] = 0.0
    X = torch.randn((nsets, k, 3), generator=g).to(dev)
    Y = torch.randn((nsets, k, 3), generator=g).to(dev)
    wd = w.to(dev)[None].repeat(nsets, 1).contiguous()
    _, _, _, idx3 = ops.ransac_hypotheses(X, Y, wd, it_r, 0.3, seed=7, offset=4)
    idx3 = idx3.long().cpu()
    n = nsets * it_r
    assert idx3.shape == (n, 3)
    assert bool((idx3[:, 0] != idx3[:, 1]).all() and (idx3[:, 0] != idx3[:, 2]).all() and (idx3[:, 1] != idx3[:, 2]).all())
    assert bool((w[idx3] > 0).all())
    torch.manual_seed(2)
    ref = torch.multinomial(w[None].expand(n, -1), 3, replacement=False)
    for name, a, b in (("first", idx3[:, 0], ref[:, 0]), ("second", idx3[:, 1], ref[:, 1]), ("inclusion", idx3.reshape(-1), ref.reshape(-1))):
        ca, cb = torch.bincount(a, minlength=k).double(), torch.bincount(b, minlength=k).double()
        sel = (ca + cb) >= 20
        df = int(sel.sum()) - 1
        chi2 = float((((ca - cb) ** 2) / (ca + cb))[sel].sum())
        assert abs(chi2 - df) < 5.0 * math.sqrt(2.0 * df), (name, chi2, df)
    # reproducible; keyed by the global set index: sets [300, 600) drawn alone with set_base = 300 repeat their draws
    _, _, _, again = ops.ransac_hypotheses(X, Y, wd, it_r, 0.3, seed=7, offset=4)
    assert torch.equal(again.long().cpu(), idx3)
    _, _, _, part = ops.ransac_hypotheses(X[300:].contiguous(), Y[300:].contiguous(), wd[300:].contiguous(), it_r, 0.3, seed=7, offset=4,
                                          set_base=300)
    assert torch.equal(part.long().cpu(), idx3[300 * it_r:])
    _, _, _, other = ops.ransac_hypotheses(X, Y, wd, it_r, 0.3, seed=8, offset=4)
    assert not torch.equal(other.long().cpu(), idx3)
    # fewer than three positive weights: the remaining picks are the lowest free indices (the race's tie rule), never a repeat
    w2 = torch.zeros((1, k), device=dev)
    w2[0, 17] = 1.0
    _, _, _, d3 = ops.ransac_hypotheses(X[:1].contiguous(), Y[:1].contiguous(), w2, 8, 0.3, seed=1, offset=0)
    d3 = d3.long().cpu()
    assert bool((d3[:, 0] == 17).all()) and bool((d3[:, 1] == 0).all()) and bool((d3[:, 2] == 1).all())


def _kabsch64(x, y, w=None):
    """fp64 weighted Procrustes of the reference (solvers.py): R = V diag(1, 1, d) U^T for H = U S V^T, t = bbar - R abar"""
    x, y = x.double(), y.double()
    w = torch.ones(x.shape[0], dtype=torch.float64) if w is None else w.double()
    inv = 1.0 / (w.abs().sum() + 1e-16)
    am, bm = (w[:, None] * x).sum(0) * inv, (w[:, None] * y).sum(0) * inv
    H = (w[:, None] * (x - am)).T @ (y - bm)
    U, S, Vh = torch.linalg.svd(H)
    d = 1.0 if float(torch.linalg.det(Vh.T @ U.T)) >= 0.0 else -1.0
    R = Vh.T @ torch.diag(torch.tensor([1.0, 1.0, d], dtype=torch.float64)) @ U.T
    return R, bm - R @ am, S, d


def test_kabsch_degenerate_and_mirrored_sets():
    """The rigid fit of both solver halves on the inputs that take its rare branches.  (a) mk_ransac_hypotheses on a generic, a
    collinear, a two-coincident and a three-coincident triple: every R finite and a rotation, the generic one within 1e-4 of an
    fp64 Kabsch.  (b) mk_train_tail_fwd on a proper and a mirrored set, all matches and every third: R | t within 1e-4 of the
    fp64 formula, the saved d = +1 / -1; H's singular values are well separated, so the comparison is well conditioned."""
    from mickey_amd import ops
    dev = _dev()
    gen = torch.Generator().manual_seed(7)
    scale = torch.tensor([3.0, 2.0, 1.0], dtype=torch.float64)
    Xs = torch.randn((65, 3), generator=gen, dtype=torch.float64) * scale
    Q, r = torch.linalg.qr(torch.randn((3, 3), generator=gen, dtype=torch.float64))
    Q = Q * torch.linalg.det(Q)                                  # a proper rotation
    t0 = torch.randn((3,), generator=gen, dtype=torch.float64)
    # (a) k = 8: rows 0, 1, 2 collinear, rows 3 = 4, rows 5 = 6 = 7
    X = Xs[:8].clone()
    X[2] = 2.0 * X[1] - X[0]
    X[4] = X[3]
    X[6] = X[7] = X[5]
    X = X.float()
    Y = (X.double() @ Q.T + t0).float()
    triples = torch.tensor([[0, 3, 5], [0, 1, 2], [3, 4, 0], [5, 6, 7]])
    Rh, th, _, idx3 = ops.ransac_hypotheses(X[None].to(dev), Y[None].to(dev), torch.ones((1, 8), device=dev), 4, 0.3,
                                            idx3_in=triples.int().to(dev))
    assert torch.equal(idx3.cpu().long(), triples)
    assert bool(torch.isfinite(Rh).all()) and bool(torch.isfinite(th).all())
    det = torch.linalg.det(Rh.cpu().reshape(-1, 3, 3).double())
    print("det R - 1:", (det - 1).tolist())
    assert float((det - 1).abs().max()) < 1e-5
    Rref, tref, S, _ = _kabsch64(X[triples[0]], Y[triples[0]])
    assert float(S[0] / S[1]) < 1e3                              # the generic triple is far from collinear
    dR, dt = float((Rh[0].cpu().reshape(3, 3).double() - Rref).norm()), float((th[0].cpu().double() - tref).norm())
    print("generic triple: |dR| %.3g |dt| %.3g, s1 / s2 = %.3g" % (dR, dt, float(S[0] / S[1])))
    assert dR < 1e-4 and dt < 1e-4
    # (b) S = 65, 5 hypotheses per set, POSE_ERR (no intrinsics); set 0 proper, set 1 mirrored; masks alternate full / every third
    X = Xs.float()
    M = torch.diag(torch.tensor([1.0, 1.0, -1.0], dtype=torch.float64))
    Y = torch.stack([(X.double() @ Q.T + t0).float(), (X.double() @ (Q @ M).T + t0).float()])
    full, third = torch.ones(65), (torch.arange(65) % 3 == 0).float()
    mask = torch.stack([full, third, full, third, full] * 2)
    out, Rt, saved = ops.train_tail_fwd(X[None].repeat(2, 1, 1).to(dev), Y.to(dev), mask.to(dev), Q.float()[None].repeat(2, 1, 1).to(dev),
                                        t0.float()[None].repeat(2, 1).to(dev), None, None, 5, 1, 0.15, 1, 0)
    Rt, saved = Rt.cpu().double(), saved.cpu()
    for s in range(2):
        for h in range(5):
            Rref, tref, S, d = _kabsch64(X, Y[s], mask[s * 5 + h])
            assert float(S[0] / S[1]) >= 1.5 and float(S[1] / S[2]) >= 1.5, S
            err = float((Rt[s * 5 + h] - torch.cat([Rref.reshape(9), tref])).norm())
            print("set %d hypothesis %d: |d(R|t)| %.3g, singular value ratios %.3g %.3g, d %+d" % (
                s, h, err, float(S[0] / S[1]), float(S[1] / S[2]), int(saved[s * 5 + h, 21])))
            assert err < 1e-4
            assert d == (1.0 if s == 0 else -1.0) and float(saved[s * 5 + h, 21]) == d
