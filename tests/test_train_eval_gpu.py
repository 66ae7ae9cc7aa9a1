"""mickey_amd.train_eval on the GPU: mk_pose_metrics and mk_pose_summary against the fp64 restatements of tests/helpers/metric_refs.py
(themselves pinned to the reference's outputs by tests/test_train_eval_cpu.py), HipProcrustesSolver against pipeline.solve, and
validation_step with a ValidationAccumulator on a stub model.

Bounds.  mk_pose_metrics computes in fp64 and rounds once: |err| <= 4 * 2^-24 |value| + 1e-5 (deg / m / px) -- one fp32 rounding
(2^-24) plus the libm's slack in fp64, and an absolute floor for angles next to 0, where acos amplifies the last fp64 bit of its
argument.  mk_pose_summary adds fp64 terms in another fixed order than numpy: 1e-10 relative on the fp64 work values (N 2^-53 would
do), counts and precisions exact, the fp32 `out` the one rounding of the work values.
"""
import copy

import numpy as np
import pytest
import torch

from tests.helpers import metric_refs as mr
from tests.helpers.guarded import bits, guarded, sentinel_bits

pytestmark = pytest.mark.gpu

REL, ABS = 4 * 2.0 ** -24, 1e-5
THRESHOLDS = (0.25, 5, 0.5, 10, 90)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def te(dev):
    from mickey_amd import train_eval
    return train_eval


@pytest.fixture(scope="module")
def poses(golden):
    g = golden("pose_metrics")
    return {k: torch.from_numpy(g[k]) for k in ("R", "t", "T_0to1", "Kori_color0")}


def _close(got, ref, what):
    """got fp32 against ref fp64, elementwise: a NaN for a NaN, an Inf for the same Inf, else the bound of the module's head"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, what
    special = ~np.isfinite(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (what, got, ref)
    assert np.array_equal(got[special & ~np.isnan(ref)], ref[special & ~np.isnan(ref)]), (what, got, ref)
    err = np.abs(got[~special] - ref[~special])
    bound = REL * np.abs(ref[~special]) + ABS
    print("%s: worst error / bound = %.3g" % (what, (err / bound).max() if err.size else 0.0))
    assert np.all(err <= bound), (what, got, ref)


def _run_metrics(te, dev, R, t, T, K, conf, row0, W=540, H=720):
    """pose_metrics into a guarded window of row0 + B + 2 records -> (records [B, 8] on the host, the returned views)"""
    B = R.shape[0]
    cap = row0 + B + 2
    win, check = guarded(cap, 8, torch.float32, dev)
    views = te.pose_metrics(R.to(dev), t.to(dev), T.to(dev), K.to(dev), conf=None if conf is None else conf.to(dev), W=W, H=H,
                            out=win, row0=row0)
    torch.cuda.synchronize()
    check()
    untouched = torch.ones(cap, dtype=torch.bool)
    untouched[row0:row0 + B] = False
    assert bool((bits(win).cpu()[untouched] == sentinel_bits(torch.float32)).all()), "a row outside [row0, row0 + B) was written"
    return win[row0:row0 + B].cpu().numpy(), views


@pytest.mark.parametrize("row0", [0, 7])
@pytest.mark.parametrize("B", [1, 3, 5])
def test_pose_metrics_against_fp64(te, dev, poses, B, row0):
    sel = slice(B, 2 * B)
    R, t, T, K = (poses[k][sel] for k in ("R", "t", "T_0to1", "Kori_color0"))
    conf = torch.arange(B, dtype=torch.float32) * 1.5 + 0.25
    rec, views = _run_metrics(te, dev, R, t, T, K, conf, row0)
    _close(rec[:, :6], mr.pose_metrics_ref(R.numpy(), t.numpy(), T.numpy(), K.numpy()), "B %d row0 %d" % (B, row0))
    assert np.array_equal(rec[:, 6], conf.numpy()) and np.all(rec[:, 7] == 0)
    assert set(views) == set(mr.COLUMNS)
    for c, name in enumerate(mr.COLUMNS):   # the reference's shapes (metrics.py:48-52, 112), views of the records
        assert views[name].shape == ((B,) if name == "R_err" else (B, 1)), name
        assert np.array_equal(views[name].cpu().numpy().reshape(-1), rec[:, c]), name


def test_pose_metrics_other_image_size_and_no_conf(te, dev, poses):
    """W and H reach the clip (the fixture's points leave a 300 x 400 image), conf=None writes 0"""
    R, t, T, K = (poses[k][:4] for k in ("R", "t", "T_0to1", "Kori_color0"))
    rec, _ = _run_metrics(te, dev, R, t, T, K, None, 1, W=300, H=400)
    ref = mr.pose_metrics_ref(R.numpy(), t.numpy(), T.numpy(), K.numpy(), W=300.0, H=400.0)
    assert np.abs(ref[:, 5] - mr.pose_metrics_ref(R.numpy(), t.numpy(), T.numpy(), K.numpy())[:, 5]).min() > 1.0
    _close(rec[:, :6], ref, "W 300 H 400")
    assert np.all(rec[:, 6:] == 0)


def test_pose_metrics_special_poses(te, dev, poses):
    """Row 0: the exact pose (Rgt a quarter turn, so orthonormal to the last bit): t_err_euc and R_err exactly 0, t_err_ang the
    formula's sqrt(2e-9) / |t| rad (its 1e-9 in the denominator), VCRE sqrt(1e-6) px.  Row 1: R = 0, t = 0, what the solver returns
    for an invalid batch: every field the summary reads is finite (t_err_scale_sym is the formula's |tgt| / 0 = inf, as in the
    reference).  Row 2: a NaN in t: NaN in the fields that read t, in that row only (R_err does not read t).  Row 3: a fixture pose."""
    T = poses["T_0to1"][:4].clone()
    T[0, :3, :3] = torch.tensor([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    R, t = poses["R"][:4].clone(), poses["t"][:4].clone()
    R[0], t[0, 0] = T[0, :3, :3], T[0, :3, 3]
    R[1], t[1] = 0.0, 0.0
    t[2, 0, 1] = float("nan")
    K = poses["Kori_color0"][:4]
    rec, _ = _run_metrics(te, dev, R, t, T, K, torch.ones(4), 0)
    ref = mr.pose_metrics_ref(R.numpy(), t.numpy(), T.numpy(), K.numpy())
    _close(rec[:, :6], ref, "special poses")
    assert rec[0, 3] == 0.0 and rec[0, 4] == 0.0 and rec[0, 1] == 1.0 and rec[0, 2] == 1.0
    assert 0.0 <= rec[0, 0] < 0.01 and abs(rec[0, 5] - 1e-3) < 1e-6
    assert np.all(np.isfinite(rec[1, [0, 1, 3, 4, 5, 6]])) and np.isposinf(rec[1, 2])
    assert rec[1, 0] == 90.0 and rec[1, 4] == 120.0
    assert np.all(np.isnan(rec[2, [0, 1, 2, 3, 5]])) and np.isfinite(rec[2, 4])
    assert not np.isnan(rec[[0, 1, 3]]).any()


# ---- the summary -------------------------------------------------------------------------------------------------------------
def _records(n, seed, conf="ties"):
    """fp32 [n, 8] with metrics on both sides of every threshold; conf: heavy ties / all distinct / all tied"""
    rng = np.random.default_rng(seed)
    r = np.zeros((n, 8), np.float32)
    r[:, 0] = rng.uniform(0, 90, n)
    r[:, 1] = rng.uniform(0.5, 2, n)
    r[:, 2] = np.maximum(r[:, 1], 1 / r[:, 1])
    r[:, 3] = rng.uniform(0, 0.8, n)
    r[:, 4] = rng.uniform(0, 16, n)
    r[:, 5] = rng.uniform(0, 200, n)
    r[:, 6] = {"ties": rng.integers(0, 9, n) * 12.5, "distinct": rng.permutation(n) * 0.75 + 1.0, "tied": np.full(n, 33.0)}[conf]
    return r


def _run_summary(dev, rec, failures, losses):
    from mickey_amd import ops
    r = torch.from_numpy(rec).to(dev)
    ls = None if losses is None else torch.from_numpy(losses).to(dev)
    out, work = ops.pose_summary(r, rec.shape[0], failures, THRESHOLDS, ls, 0 if losses is None else losses.shape[0])
    out2, work2 = ops.pose_summary(r, rec.shape[0], failures, THRESHOLDS, ls, 0 if losses is None else losses.shape[0])
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), out2.view(torch.int32)) and torch.equal(work.view(torch.int64), work2.view(torch.int64)), \
        "two runs differ"
    return out.cpu().numpy(), work.cpu().numpy()


def _check_summary(dev, rec, failures, losses, what):
    out, work = _run_summary(dev, rec, failures, losses)
    ref = mr.summary_ref(rec, failures, THRESHOLDS, losses)
    fin = work[-1]
    assert fin.shape == (16,) and work.shape[0] == -(-rec.shape[0] // _tile()) + 1
    exact = [0, 1, 6, 8, 10, 15]          # counts, and precisions = count / (N + failures): one fp64 division on either side
    assert np.array_equal(fin[exact], ref[exact]), (what, fin, ref)
    rest = [k for k in range(16) if k not in exact]
    assert np.array_equal(np.isnan(fin[rest]), np.isnan(ref[rest])), (what, fin, ref)
    ok = ~np.isnan(ref[rest])
    err = np.abs(fin[rest][ok] - ref[rest][ok])
    print("%s: worst relative error of the fp64 results %.3g" % (what, (err / np.maximum(np.abs(ref[rest][ok]), 1e-300)).max()))
    assert np.all(err <= 1e-10 * np.abs(ref[rest][ok])), (what, fin, ref)
    assert np.array_equal(out.view(np.int32), fin.astype(np.float32).view(np.int32)), "out is not the fp32 rounding of the work row"
    return out, fin, ref


def _tile():
    from mickey_amd import ops
    return ops.pose_summary_tile()


def _losses(s, seed):
    return np.random.default_rng(seed).uniform(0.1, 3.0, (s, 3)).astype(np.float32)


@pytest.mark.parametrize("failures, with_losses", [(0, False), (2, True)])
@pytest.mark.parametrize("shape", ["1", "T-1", "T", "T+1", "2T+3"])
def test_summary_sizes(dev, shape, failures, with_losses):
    T = _tile()
    n = {"1": 1, "T-1": T - 1, "T": T, "T+1": T + 1, "2T+3": 2 * T + 3}[shape]
    rec = _records(n, 100 + n)
    losses = _losses(max(1, n // 2), n) if with_losses else None
    out, fin, ref = _check_summary(dev, rec, failures, losses, "N %d failures %d" % (n, failures))
    assert fin[0] == n and fin[1] == 0
    if not with_losses:
        assert np.all(fin[12:15] == 0)
    if n > 1:
        assert 0 < fin[7] < 1 and 0 < fin[11] < 1      # (a summary of zeros or ones would compare nothing)


def test_summary_more_loss_rows_than_threads(dev):
    """S beyond one pass of the loss loop (S > blocks * tile): every row is read once"""
    T = _tile()
    rec = _records(3, 7)
    _check_summary(dev, rec, 0, _losses(2 * T + 5, 8), "N 3, S 2T + 5")


@pytest.mark.parametrize("failures", [0, 2])
def test_summary_tie_group_across_a_tile_edge(dev, failures):
    T = _tile()
    rec = _records(2 * T + 3, 11, conf="distinct")
    rec[T - 3:T + 4, 6] = rec[T, 6]
    rec[2 * T - 1:2 * T + 2, 6] = rec[5, 6]            # a group with members in all three tiles
    _check_summary(dev, rec, failures, None, "tie groups across tile edges")


@pytest.mark.parametrize("failures", [0, 2])
def test_summary_all_tied(dev, failures):
    T = _tile()
    rec = _records(2 * T + 3, 12, conf="tied")
    out, fin, ref = _check_summary(dev, rec, failures, _losses(4, 1), "all tied")
    assert np.allclose(fin[[7, 9, 11]], fin[[6, 8, 10]], rtol=1e-12, atol=0)   # one group: AP = N (k / N) / (N + F) = its precision


def test_summary_bad_confidences_rank_last(dev):
    T = _tile()
    rec = _records(T + 1, 13, conf="distinct")
    rec[3, 6], rec[T, 6] = np.nan, np.inf
    out, fin, ref = _check_summary(dev, rec, 0, None, "two non-finite confidences")
    assert fin[1] == 2
    moved = rec.copy()
    moved[[3, T], 6] = -1e30                            # the same ranking with a finite confidence below all others
    assert np.allclose(mr.summary_ref(moved)[[7, 9, 11]], ref[[7, 9, 11]], rtol=1e-14, atol=0)


def test_summary_nan_metric(dev):
    T = _tile()
    rec = _records(T + 1, 14)
    clean = mr.summary_ref(rec)
    rec[T, 4] = np.nan                                  # R_err of a record of the second workgroup
    out, fin, ref = _check_summary(dev, rec, 0, None, "one NaN metric")
    assert np.isnan(fin[4]) and not np.isnan(np.delete(fin, 4)).any()
    same = [2, 3, 5, 10, 11]                            # what does not read R_err is what it was without the NaN
    assert np.allclose(fin[same], clean[same], rtol=1e-10, atol=0)
    assert fin[6] <= clean[6] and fin[8] <= clean[8]    # a NaN is never accepted


def test_summary_refuses_bad_arguments(dev):
    from mickey_amd import ops
    from mickey_amd._native import MickeyHipError
    r = torch.zeros((4, 8), device=dev)
    for kw in (dict(N=0), dict(N=(1 << 18) + 1), dict(failures=-1), dict(S=1)):
        a = dict(N=4, failures=0, S=0)
        a.update(kw)
        with pytest.raises(MickeyHipError, match="mk_pose_summary"):
            ops.pose_summary(r, a["N"], a["failures"], THRESHOLDS, None, a["S"], work=torch.zeros((2, 16), device=dev, dtype=torch.float64))
    for kw in (dict(row0=-1), dict(row0=3)):
        with pytest.raises(MickeyHipError, match="mk_pose_metrics"):
            ops.pose_metrics(torch.zeros((2, 3, 3), device=dev), torch.zeros((2, 1, 3), device=dev), torch.zeros((2, 4, 4), device=dev),
                             torch.zeros((2, 3, 3), device=dev), None, 540, 720, r, **kw)
    torch.cuda.synchronize()
    assert not r.any()


# ---- the solver --------------------------------------------------------------------------------------------------------------
def _to(d, dev):
    return {k: v.to(dev) for k, v in d.items()}


def _small(cfg):
    c = copy.deepcopy(cfg)
    c["PROCRUSTES"]["IT_MATCHES"], c["PROCRUSTES"]["IT_RANSAC"] = 4, 25
    return c


def _same(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def test_solver_is_pipeline_solve(te, dev, cfg):
    from mickey_amd import pipeline
    from mickey_amd import synthetic as syn
    scfg = _small(cfg)
    data, _, _ = syn.planted_pose_problem(B=3, h=14, w=12, seed=4321, angle_deg=(1.0, 1.5), t_norm=(0.03, 0.04))
    d = _to(data, dev)
    args = [d[k] for k in ("final_scores", "kps0", "depth_kp0", "kps1", "depth_kp1", "K_color0", "K_color1")]

    def direct(offset, pair_base=0):
        s = pipeline.solve(scfg, *args, seed=77, offset=offset, pair_base=pair_base)
        return s["R"], s["t"], s["inliers"].reshape(-1)

    solver = te.HipProcrustesSolver(scfg, seed=77)
    first = solver.estimate_pose_vectorized(d)
    assert [tuple(v.shape) for v in first] == [(3, 3, 3), (3, 1, 3), (3,)]
    second = solver.estimate_pose_vectorized(d)
    assert _same(first, direct(0)) and _same(second, direct(2))
    assert not _same(first, second), "the second call drew what the first one drew"
    solver.reseed(77, 0)
    assert _same(solver.estimate_pose_vectorized(d), first)
    solver.reseed(77, 1)
    assert _same(solver.estimate_pose_vectorized(dict(d, pair_base=5)), direct(2, pair_base=5))
    solver.reseed(77, 0)
    R, t, inl, lst = solver.estimate_pose_vectorized(d, return_inliers=True)
    assert _same((R, t, inl), first) and len(lst) == 3 and all(v.shape[1] == 7 for v in lst)


def test_solver_recovers_the_planted_pose(te, dev, cfg):
    """the bounds of tests/test_solver_gpu.py::test_planted_pose_recovery_full_size for this generator"""
    from mickey_amd import synthetic as syn
    data, Rgt, tgt = syn.planted_pose_problem(B=2, h=51, w=38, seed=4321)
    R, t, inl = te.HipProcrustesSolver(cfg, seed=123).estimate_pose_vectorized(_to(data, dev))
    eR = (R.cpu() - Rgt).norm(dim=(1, 2))
    et = (t.cpu() - tgt).norm(dim=(1, 2))
    assert float(eR.max()) < 5e-3 and float(et.max()) < 2e-2, (eR, et)
    assert float(inl.min()) > 50


# ---- validation_step ---------------------------------------------------------------------------------------------------------
class _StubModel(torch.nn.Module):
    """forward() leaves in the batch what the matcher of a real model leaves there"""

    def __init__(self, data):
        super().__init__()
        self.data, self.eval_calls = data, 0

    def is_eval_model(self, flag):
        self.eval_calls += 1

    def forward(self, batch):
        i = batch["which"]
        for k in ("kps0", "kps1", "depth_kp0", "depth_kp1"):
            batch[k] = self.data[k][i:i + 2]
        batch["scores"] = self.data["final_scores"][i:i + 2]
        batch["kp_scores"] = torch.ones_like(batch["scores"])


def _stub_loss(batch):   # the tuple of MetricPoseLoss.forward, from device arithmetic only
    s = batch["final_scores"].sum()
    outputs = {"avg_loss_rot": s * 2.0, "avg_loss_trans": s * 3.0}
    return s * 5.0, outputs, [batch["final_scores"]], 1


def test_validation_step_accumulates_without_synchronising(te, dev, cfg):
    from mickey_amd import synthetic as syn
    data, Rgt, tgt = syn.planted_pose_problem(B=4, h=14, w=12, seed=99, angle_deg=(1.0, 1.5), t_norm=(0.03, 0.04))
    T = torch.eye(4).repeat(4, 1, 1)
    T[:, :3, :3], T[:, :3, 3] = Rgt, tgt[:, 0]
    T[1, :3, 3] += 1.0                      # one pair whose ground truth the solver cannot meet: records on both sides of the tests
    d = _to(data, dev)
    model = _StubModel(d)
    solver = te.HipProcrustesSolver(_small(cfg), seed=3)
    acc = te.ValidationAccumulator(4, dev, steps=2)
    kori = torch.tensor([[590.0, 0, 270], [0, 590, 360], [0, 0, 1]]).repeat(2, 1, 1).to(dev)

    def batch(i):
        return {"which": i, "T_0to1": T[i:i + 2].to(dev), "Kori_color0": kori, "K_color0": d["K_color0"][i:i + 2],
                "K_color1": d["K_color1"][i:i + 2]}

    batches = [batch(0), batch(2)]          # (uploaded before the mode below is switched on: a copy from pageable memory waits)
    outs = [te.validation_step(model, batches[0], _stub_loss, solver, acc, batch_idx=0)]
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):   # the mode is live: a read-back is refused
            acc.records[0, 0].item()
        outs.append(te.validation_step(model, batches[1], _stub_loss, solver, acc, batch_idx=1))
        out_t, work_t = acc.summary_tensors()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    summary = acc.summary()
    assert model.eval_calls == 2 and acc.n == 4 and acc.n_steps == 2
    for o in outs:                          # model.py:73-85
        assert {"loss", "avg_loss_rot", "avg_loss_trans", "metric_ours_t_err_ang", "metric_ours_t_err_euc", "metric_ours_R_err",
                "metric_inliers", "metric_ours_vcre"} <= set(o)
        assert o["loss"].shape == () and o["metric_ours_R_err"].shape == (2,) and o["metric_inliers"].shape == (2,)
        for k in ("metric_ours_t_err_ang", "metric_ours_t_err_euc", "metric_ours_vcre"):
            assert o[k].shape == (2, 1), k
    rec, losses = acc.records.cpu().numpy(), acc.losses.cpu().numpy()
    assert np.array_equal(rec[2:, 3], outs[1]["metric_ours_t_err_euc"].cpu().numpy().reshape(-1))
    assert np.array_equal(rec[:, 6], torch.cat([o["metric_inliers"] for o in outs]).cpu().numpy())
    assert np.array_equal(losses[1], np.array([float(outs[1][k]) for k in ("loss", "avg_loss_rot", "avg_loss_trans")], np.float32))
    assert rec[0, 3] < 0.25 and rec[1, 3] > 0.5    # the planted pose is met; the shifted ground truth is not
    ref = mr.summary_ref(rec, 0, THRESHOLDS, losses)
    names = {2: "val_metric_pose/ours_t_err_ang", 3: "val_metric_pose/ours_t_err_euc", 4: "val_metric_pose/ours_R_err",
             5: "val_vcre/metric_ours_vcre", 6: "val_AUC_pose/prec_pose_ours", 7: "val_AUC_pose/auc_pose",
             8: "val_AUC_pose/prec_pose_ours_10", 9: "val_AUC_pose/auc_pose_10", 10: "val_vcre/prec_vcre_ours", 11: "val_vcre/auc_vcre",
             12: "val_loss/loss", 13: "val_loss/loss_R", 14: "val_loss/loss_t"}
    assert set(summary) == set(names.values()) | {"n", "n_bad_conf"} and summary["n"] == 4 and summary["n_bad_conf"] == 0
    for k, name in names.items():
        assert abs(summary[name] - ref[k]) <= 2.0 ** -23 * abs(ref[k]), (name, summary[name], ref[k])
    assert np.array_equal(np.asarray(out_t.cpu()), np.asarray([summary["n"], 0] + [summary[names[k]] for k in range(2, 15)] + [0],
                                                              dtype=np.float32))
    with pytest.raises(ValueError, match="do not fit"):
        acc.add(torch.zeros((1, 3, 3), device=dev), torch.zeros((1, 1, 3), device=dev), torch.zeros(1, device=dev), batches[0])
    acc.reset()
    with pytest.raises(ValueError, match="no records"):
        acc.summary()
