"""mickey_amd.train_eval without a GPU: the formulas the kernels and the GPU tests restate (tests/helpers/metric_refs.py) against the
reference's own fp32 outputs (tests/golden/pose_metrics.npz, tools/make_golden_pose_metrics.py), the binding of the two entry points,
and every argument check made on the host."""
import importlib.util
import os
import types

import numpy as np
import pytest
import torch

from tests.helpers import metric_refs as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g(golden):
    return golden("pose_metrics")


# ---- the formulas ---------------------------------------------------------------------------------------------------------------
def test_eye_grid_is_the_references(g):
    """the kernels' grid (fp32 products of the fp32 step 0.3f) against the reference's (fp64 products, rounded to fp32): the same
    points in the same order, at most one fp32 unit apart"""
    assert g["eye_grid"].shape == (196, 3)
    ref = g["eye_grid"].astype(np.float64)
    assert np.all(np.abs(mr.eye_grid() - ref) <= 2.0 ** -23 * np.abs(ref))


def test_fixture_poses_are_well_conditioned(g):
    """what the 1e-3 bound below rests on: residual rotations in [2, 178] degrees, every moved grid point in front of the camera"""
    assert g["R"].shape[0] >= 16
    assert 2.0 <= g["ref_R_err"].min() and g["ref_R_err"].max() <= 178.0
    R, t, T = (g[k].astype(np.float64) for k in ("R", "t", "T_0to1"))
    moved = np.einsum("bij,pj->bpi", R, mr.eye_grid()) + (t.reshape(-1, 3) - T[:, :3, 3])[:, None]
    z = np.einsum("bji,bpj->bpi", T[:, :3, :3], moved)[..., 2]
    assert z.min() >= 0.3


@pytest.mark.parametrize("name", mr.COLUMNS)
def test_metric_formulas_match_the_reference(g, name):
    """A guard against a wrong formula, not a measurement: the fp64 restatement against the reference's fp32 result, relative gap
    <= 1e-3 (the reference's own fp32 error on such poses is <= 1e-4)."""
    ours = mr.pose_metrics_ref(g["R"], g["t"], g["T_0to1"], g["Kori_color0"])[:, mr.COLUMNS.index(name)]
    ref = g["ref_" + name].reshape(-1).astype(np.float64)
    assert ref.shape == ours.shape and np.all(np.isfinite(ref)) and np.all(ref > 0)
    gap = np.abs(ours - ref) / np.abs(ref)
    print(name, "worst relative gap %.3g" % gap.max())
    assert gap.max() <= 1e-3


def test_reference_output_shapes(g):
    B = g["R"].shape[0]
    for name in mr.COLUMNS:
        assert g["ref_" + name].shape == ((B,) if name == "R_err" else (B, 1)), name


def test_all_pairs_average_precision_matches_precision_recall(g):
    """AP = 1 / (N + F) sum_i cumTP_i / cumN_i against the reference's precision_recall; the reference rounds each of its G recall
    points to fp32 (np.arange(N, dtype=np.float32)): bound 2 G 2^-24."""
    kinds = set()
    for s in range(int(g["num_sets"])):
        conf, tp, failures = g["set%d_conf" % s], g["set%d_tp" % s], int(g["set%d_failures" % s])
        groups = len(np.unique(conf))
        ap = mr.average_precision_ref(conf, tp, failures)
        err = abs(ap - float(g["set%d_ap" % s]))
        print("set %d: N %d, %d groups, failures %d: |AP - reference| = %.3g" % (s, len(conf), groups, failures, err))
        assert err <= 2 * groups * 2.0 ** -24
        n = len(conf)
        kinds.add("tied" if groups == 1 and n > 1 else "distinct" if groups == n and n > 1 else
                  "n-1" if n > 2 and np.bincount(np.unique(conf, return_inverse=True)[1]).max() == n - 1 else "mixed")
        kinds.add("failures%d" % failures)
        kinds.update(["tp_none"] if not tp.any() else ["tp_all"] if tp.all() else [])
    assert kinds >= {"tied", "distinct", "n-1", "failures0", "failures2", "tp_none", "tp_all"}, kinds


def test_fixture_regenerates_from_the_reference_bit_for_bit(g):
    from oracle import ref_shim
    if not ref_shim.available():
        pytest.skip("no reference checkout")
    spec = importlib.util.spec_from_file_location("make_golden_pose_metrics", os.path.join(ROOT, "tools", "make_golden_pose_metrics.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    new = tool.generate()
    assert sorted(new) == sorted(g)
    for k in g:
        a, b = np.asarray(new[k]), g[k]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k


def test_summary_ref_ranks_bad_confidences_last():
    rec = np.zeros((4, 8), np.float32)
    rec[:, 6] = [5.0, np.nan, 7.0, np.inf]
    rec[:, 5] = [10, 10, 200, 10]         # vcre: records 0, 1, 3 accepted by the third test
    out = mr.summary_ref(rec)
    assert out[1] == 2
    # order: 7 (tp 0), 5 (tp 1), then the tie group of the two bad ones (both tp): 0/1 + 1/2 + 2 * 3/4
    assert out[11] == pytest.approx((0.0 + 0.5 + 1.5) / 4, abs=1e-15)


# ---- the binding ----------------------------------------------------------------------------------------------------------------
def test_entry_points_in_the_header_derived_binding():
    from mickey_amd import _native
    assert _native.SIGNATURES["mk_pose_metrics"] == ("i", "pppppffplilp")
    assert _native.PARAM_NAMES["mk_pose_metrics"] == ("R", "t", "T_gt", "K", "conf", "W", "H", "records", "row0", "B", "capacity",
                                                      "stream")
    assert _native.SIGNATURES["mk_pose_summary"] == ("i", "piifffffpippp")
    assert _native.PARAM_NAMES["mk_pose_summary"] == ("records", "N", "failures", "th_t", "th_R", "th_t2", "th_R2", "th_px", "losses",
                                                      "S", "out", "work", "stream")
    assert _native.SIGNATURES["mk_pose_summary_tile"] == ("i", "")
    assert _native.SIGNATURES["mk_pose_summary_work_doubles"] == ("l", "i")


def test_library_exports_the_entry_points():
    from mickey_amd import _native
    missing = set(_native.missing_symbols())
    assert not missing & {"mk_pose_metrics", "mk_pose_summary", "mk_pose_summary_tile", "mk_pose_summary_work_doubles"}
    tile = _native.query("mk_pose_summary_tile")
    assert tile >= 64 and tile % 64 == 0
    assert _native.query("mk_pose_summary_work_doubles", 1) == 32
    assert _native.query("mk_pose_summary_work_doubles", tile + 1) == 48
    assert _native.query("mk_pose_summary_work_doubles", 0) == 0


# ---- host checks ----------------------------------------------------------------------------------------------------------------
def _pose_args(B=2):
    return dict(R=torch.eye(3).repeat(B, 1, 1), t=torch.ones(B, 1, 3), T_0to1=torch.eye(4).repeat(B, 1, 1),
                Kori_color0=torch.eye(3).repeat(B, 1, 1))


@pytest.mark.parametrize("change, match", [
    (dict(R=torch.eye(3)), "R must have 3 dimensions"),
    (dict(R=torch.zeros(2, 3, 4)), "R must be"),
    (dict(R=torch.eye(3).repeat(2, 1, 1).double()), "R must be float32"),
    (dict(R=np.eye(3)), "R must be a tensor"),
    (dict(t=torch.ones(2, 3)), "t must be"),
    (dict(t=torch.ones(3, 1, 3)), "t must be"),
    (dict(t=torch.ones(2, 1, 3).half()), "t must be float32"),
    (dict(T_0to1=torch.eye(3).repeat(2, 1, 1)), "T_0to1 must be"),
    (dict(T_0to1=torch.eye(4).repeat(2, 1, 1).long()), "T_0to1 must be a floating-point"),
    (dict(Kori_color0=torch.eye(3).repeat(3, 1, 1)), "Kori_color0 must be"),
    (dict(Kori_color0=None), "Kori_color0 must be a tensor"),
    (dict(conf=torch.ones(3)), "conf must be"),
    (dict(conf=torch.ones(2).double()), "conf must be float32"),
    (dict(W=0), "W must be"),
    (dict(H=float("nan")), "H must be"),
    (dict(H="720"), "H must be"),
    (dict(row0=1), "needs an out"),
    (dict(out=torch.zeros(4, 7)), "out must be 8"),
    (dict(out=torch.zeros(4, 8).double()), "out must be float32"),
    (dict(out=torch.zeros(4, 16)[:, :8]), "contiguous"),
    (dict(out=torch.zeros(5, 8), row0=-1), "row0 must be"),
    (dict(out=torch.zeros(5, 8), row0=1.0), "row0 must be"),
    (dict(out=torch.zeros(5, 8), row0=True), "row0 must be"),
    (dict(out=torch.zeros(5, 8), row0=4), "do not fit"),
    (dict(out=torch.zeros(1, 8)), "do not fit"),
])
def test_pose_metrics_refuses(change, match):
    from mickey_amd import train_eval
    args = _pose_args()
    args.update(change)
    with pytest.raises(ValueError, match=match):
        train_eval.pose_metrics(**args)


def test_pose_metrics_has_no_cpu_fallback():
    from mickey_amd import train_eval
    from mickey_amd._native import MickeyHipError
    with pytest.raises(MickeyHipError, match="no CPU fallback"):
        train_eval.pose_metrics(out=torch.zeros(5, 8), row0=3, conf=torch.ones(2, 1), **_pose_args())


def test_accumulator_host_checks():
    from mickey_amd import train_eval
    from mickey_amd._native import MickeyHipError
    for bad in (dict(capacity=0), dict(capacity=2.0), dict(capacity=True), dict(capacity=(1 << 18) + 1), dict(capacity=4, steps=0),
                dict(capacity=4, W=-1), dict(capacity=4, H=0)):
        kw = dict(device="cpu")
        kw.update(bad)
        with pytest.raises(ValueError, match="ValidationAccumulator"):
            train_eval.ValidationAccumulator(**kw)
    acc = train_eval.ValidationAccumulator(3, "cpu", steps=1)
    assert acc.records.shape == (3, 8) and acc.losses.shape == (1, 3) and acc.capacity == 3 and acc.n == 0
    a = _pose_args(2)
    batch = {"T_0to1": a["T_0to1"], "Kori_color0": a["Kori_color0"]}
    with pytest.raises(ValueError, match="batch lacks 'Kori_color0'"):
        acc.add(a["R"], a["t"], torch.ones(2), {"T_0to1": a["T_0to1"]})
    with pytest.raises(ValueError, match="loss_outputs\\['avg_loss_rot'\\]"):
        acc.add(a["R"], a["t"], torch.ones(2), batch, loss_outputs={"loss": torch.zeros(())})
    with pytest.raises(MickeyHipError):      # everything fits; the tensors are not on a GPU
        acc.add(a["R"], a["t"], torch.ones(2), batch)
    assert acc.n == 0 and acc.n_steps == 0   # a refused add leaves the counts alone
    acc.n = 2                                # (as after one batch of two)
    with pytest.raises(ValueError, match="2 more records do not fit: 2 of 3"):
        acc.add(a["R"], a["t"], torch.ones(2), batch)
    acc.n, acc.n_steps = 0, 1
    losses = {"loss": torch.zeros(()), "avg_loss_rot": torch.zeros(()), "avg_loss_trans": torch.zeros(())}
    with pytest.raises(ValueError, match="loss rows are taken"):
        acc.add(a["R"], a["t"], torch.ones(2), batch, loss_outputs=losses)
    acc.reset()
    assert acc.n == 0 and acc.n_steps == 0


def test_summary_host_checks():
    from mickey_amd import train_eval
    acc = train_eval.ValidationAccumulator(3, "cpu")
    with pytest.raises(ValueError, match="no records"):       # N = 0
        acc.summary()
    acc.n = 1
    for kw in (dict(failures=-1), dict(failures=1.5), dict(failures=True), dict(thresholds=(1, 2, 3)),
               dict(thresholds=(0.25, 5, 0.5, float("inf"), 90)), dict(thresholds=(0.25, 5, 0.5, -1, 90))):
        with pytest.raises(ValueError, match="ValidationAccumulator.summary"):
            acc.summary(**kw)


class _RefSolver:   # the attributes of e2eProbabilisticProcrustesSolver (probabilisticProcrustes.py:12-20)
    def __init__(self, k3=3):
        self.it_RANSAC, self.it_matches, self.num_samples_matches, self.num_corr_3d_3d = 7, 3, 64, k3
        self.num_refinements, self.th_inlier, self.th_soft_inlier = 2, 0.125, 0.25


class _Trainer(torch.nn.Module):
    def __init__(self, solver):
        super().__init__()
        self.e2e_Procrustes = solver
        self.lin = torch.nn.Linear(2, 2)


def test_use_hip_solver_swaps_and_keeps_the_attributes():
    from mickey_amd import train_eval
    shared = _RefSolver()
    outer = torch.nn.Module()
    outer.a, outer.b, outer.c = _Trainer(shared), _Trainer(shared), _Trainer(_RefSolver())
    outer.c.e2e_Procrustes.th_inlier = 0.5
    outer.d = torch.nn.Linear(2, 2)
    outer.d.e2e_Procrustes = types.SimpleNamespace(it_RANSAC=1)      # not the reference solver's attributes: left alone
    assert train_eval.use_hip_solver(outer, seed=5) == 3
    new = outer.a.e2e_Procrustes
    assert isinstance(new, train_eval.HipProcrustesSolver) and outer.b.e2e_Procrustes is new and outer.c.e2e_Procrustes is not new
    for attr, value in vars(shared).items():
        assert getattr(new, attr) == value, attr
    assert outer.c.e2e_Procrustes.th_inlier == 0.5 and new.seed == 5
    assert isinstance(outer.d.e2e_Procrustes, types.SimpleNamespace)
    assert train_eval.use_hip_solver(outer) == 0                      # nothing left to swap
    plain = types.SimpleNamespace(e2e_Procrustes=_RefSolver())        # a trainer that is no nn.Module
    assert train_eval.use_hip_solver(plain) == 1 and isinstance(plain.e2e_Procrustes, train_eval.HipProcrustesSolver)


def test_use_hip_solver_refuses_four_point_samples_before_any_swap():
    from mickey_amd import train_eval
    outer = torch.nn.Module()
    outer.a, outer.b = _Trainer(_RefSolver()), _Trainer(_RefSolver(k3=4))
    with pytest.raises(ValueError, match="num_corr_3d_3d must be 3"):
        train_eval.use_hip_solver(outer)
    assert isinstance(outer.a.e2e_Procrustes, _RefSolver) and isinstance(outer.b.e2e_Procrustes, _RefSolver)
    with pytest.raises(ValueError, match="num_corr_3d_3d must be 3"):
        train_eval.HipProcrustesSolver({"PROCRUSTES": {"IT_RANSAC": 1, "IT_MATCHES": 1, "NUM_SAMPLED_MATCHES": 8, "NUM_CORR_3D_3D": 4,
                                                       "NUM_REFINEMENTS": 1, "TH_INLIER": 0.1, "TH_SOFT_INLIER": 0.1}})


def test_solver_view_and_host_checks(cfg):
    from mickey_amd import train_eval
    from mickey_amd._native import MickeyHipError
    from mickey_amd.model import _SolverView
    s = train_eval.HipProcrustesSolver(cfg, seed=3)
    assert vars(_SolverView(cfg)).items() <= vars(s).items()
    s.reseed(9, calls=4)
    assert (s.seed, s._calls) == (9, 4)
    n = 6
    batch = {"final_scores": torch.rand(1, n, n), "kps0": torch.rand(1, 2, n), "depth_kp0": torch.rand(1, 1, n), "kps1": torch.rand(1, 2, n),
             "depth_kp1": torch.rand(1, 1, n), "K_color0": torch.eye(3)[None], "K_color1": torch.eye(3)[None]}
    with pytest.raises(MickeyHipError, match="no CPU fallback"):
        s.estimate_pose_vectorized(batch)
    assert s._calls == 4                     # a refused call draws nothing
    del batch["kps1"]
    with pytest.raises(ValueError, match="batch lacks 'kps1'"):
        s.estimate_pose_vectorized(batch)
