"""The validation tail of the reference trainer on the HIP kernels (lib/models/MicKey/model.py:66-89 validation_step, :163-171 the
pose log of tensorboard_log_step, :205-280 on_validation_epoch_end).

    HipProcrustesSolver(cfg, seed)     the contract of e2eProbabilisticProcrustesSolver (utils/probabilisticProcrustes.py:183-348), backed
                                       by pipeline.solve -- the solver of the inference path
    use_hip_solver(model)              puts one in the place of every `e2e_Procrustes` the trainer built for itself
    pose_metrics(R, t, T_0to1, K)      pose_error_torch + vcre_torch (lib/utils/metrics.py:12-53, 83-125) in one launch
    ValidationAccumulator              the epoch's records on the device; summary() is the epoch's one device -> host copy
    validation_step(...)               model.py:66-89 with the three above

Nothing in here reads a device tensor on the host except ValidationAccumulator.summary().  (The loss is the caller's: MetricPoseLoss
reads its own two words per call.)  Every argument check raises ValueError before anything is launched, except a tensor that is not
on a GPU: MickeyHipError (there is no CPU fallback).
"""
import numbers

import torch

from . import ops, pipeline
from ._train_common import check_devices, check_f32, check_number, check_tensor

_SOLVER_ATTRS = (("it_RANSAC", "IT_RANSAC"), ("it_matches", "IT_MATCHES"), ("num_samples_matches", "NUM_SAMPLED_MATCHES"),
                 ("num_corr_3d_3d", "NUM_CORR_3D_3D"), ("num_refinements", "NUM_REFINEMENTS"), ("th_inlier", "TH_INLIER"),
                 ("th_soft_inlier", "TH_SOFT_INLIER"))
_SOLVER_INPUTS = ("final_scores", "kps0", "depth_kp0", "kps1", "depth_kp1", "K_color0", "K_color1")
RECORD_WIDTH = 8
MAX_RECORDS = 1 << 18      # mk_pose_summary ranks every record against every record
THRESHOLDS = (0.25, 5, 0.5, 10, 90)   # model.py:225-226, 237-238, 250: t [m], R [deg], t, R of the second test, VCRE [px]
# out[k] of mk_pose_summary under the name the trainer logs it with (model.py:258-274)
_LOG_NAMES = {2: "val_metric_pose/ours_t_err_ang", 3: "val_metric_pose/ours_t_err_euc", 4: "val_metric_pose/ours_R_err",
              5: "val_vcre/metric_ours_vcre", 6: "val_AUC_pose/prec_pose_ours", 7: "val_AUC_pose/auc_pose",
              8: "val_AUC_pose/prec_pose_ours_10", 9: "val_AUC_pose/auc_pose_10", 10: "val_vcre/prec_vcre_ours",
              11: "val_vcre/auc_vcre"}
_LOSS_NAMES = {12: "val_loss/loss", 13: "val_loss/loss_R", 14: "val_loss/loss_t"}


def _get(cfg, key):
    return cfg[key] if isinstance(cfg, dict) or not hasattr(cfg, key) else getattr(cfg, key)


def _check_num_corr(fn, k3):
    if int(k3) != 3:
        raise ValueError("%s: num_corr_3d_3d must be 3 (the HIP solver fits minimal 3-point samples), got %r" % (fn, k3))


class HipProcrustesSolver:
    """e2eProbabilisticProcrustesSolver's contract on pipeline.solve.  cfg: a configuration with a PROCRUSTES section (keys or
    attributes).  Call c (counted from 0) draws from the Philox streams (seed, 2 c) and (seed, 2 c + 1), keyed further by the pair's
    global index batch.get("pair_base", 0) + b: the same seed, call number and inputs give the same bits."""

    def __init__(self, cfg, seed=0):
        P = _get(cfg, "PROCRUSTES")
        for attr, key in _SOLVER_ATTRS:
            setattr(self, attr, _get(P, key))
        _check_num_corr("HipProcrustesSolver", self.num_corr_3d_3d)
        self.seed = int(seed)
        self._calls = 0
        self._ws = pipeline.Workspace()

    @classmethod
    def from_solver(cls, old, seed=0):
        """A solver with the attributes of `old` (the reference's solver, or anything that carries its seven attributes)."""
        return cls({"PROCRUSTES": {key: getattr(old, attr) for attr, key in _SOLVER_ATTRS}}, seed)

    def reseed(self, seed, calls=0):
        """The next call draws as call number `calls` of a solver constructed with `seed`."""
        self.seed, self._calls = int(seed), int(calls)

    def _cfg(self):
        return {"PROCRUSTES": {key: getattr(self, attr) for attr, key in _SOLVER_ATTRS}}

    @torch.no_grad()
    def estimate_pose_vectorized(self, batch, return_inliers=False):
        """-> (R [B, 3, 3], t [B, 1, 3], inliers [B]) and, with return_inliers, the per-pair inlier lists [m_i, 7] (this one reads
        the solver's invalid word on the host)."""
        fn = "HipProcrustesSolver.estimate_pose_vectorized"
        for k in _SOLVER_INPUTS:
            if k not in batch:
                raise ValueError("%s: batch lacks %r" % (fn, k))
            check_tensor(fn, "batch[%r]" % k, batch[k])
        check_devices(fn, [("batch[%r]" % k, batch[k]) for k in _SOLVER_INPUTS])
        _check_num_corr(fn, self.num_corr_3d_3d)
        a = [batch[k].detach().float().contiguous() for k in _SOLVER_INPUTS]
        offset = 2 * self._calls
        self._calls += 1
        sol = pipeline.solve(self._cfg(), *a, seed=self.seed, offset=offset, pair_base=int(batch.get("pair_base", 0)), ws=self._ws)
        out = (sol["R"], sol["t"], sol["inliers"].reshape(-1))
        return out + (pipeline.inliers_list(sol),) if return_inliers else out


def _is_reference_solver(obj):
    return obj is not None and not isinstance(obj, HipProcrustesSolver) and all(hasattr(obj, a) for a, _ in _SOLVER_ATTRS)


def use_hip_solver(model, seed=0):
    """Replace, in place, every attribute `e2e_Procrustes` of model and of the modules inside it that carries the reference solver's
    attributes by a HipProcrustesSolver built from them (one per distinct solver object).  Returns the number of attributes replaced.
    A solver with num_corr_3d_3d != 3 raises ValueError before anything is swapped."""
    owners = list(model.modules()) if isinstance(model, torch.nn.Module) else [model]
    found = [(o, o.__dict__["e2e_Procrustes"]) for o in owners if _is_reference_solver(getattr(o, "__dict__", {}).get("e2e_Procrustes"))]
    for _, old in found:
        _check_num_corr("use_hip_solver", old.num_corr_3d_3d)
    made = {}
    for owner, old in found:
        if id(old) not in made:
            made[id(old)] = (old, HipProcrustesSolver.from_solver(old, seed))
        owner.__dict__["e2e_Procrustes"] = made[id(old)][1]
    return len(found)


def _metric_views(rec):
    return {"t_err_ang": rec[:, 0:1], "t_err_scale": rec[:, 1:2], "t_err_scale_sym": rec[:, 2:3], "t_err_euc": rec[:, 3:4],
            "R_err": rec[:, 4], "repr_err": rec[:, 5:6]}


def pose_metrics(R, t, T_0to1, Kori_color0, conf=None, W=540, H=720, out=None, row0=0):
    """pose_error_torch(R, t, T_0to1) and vcre_torch(R, t, T_0to1, Kori_color0, H=H, W=W) of the reference (reduce=None) in one
    launch: R [B, 3, 3], t [B, 1, 3] fp32, T_0to1 [B, 4, 4], Kori_color0 [B, 3, 3] (any floating type; read as fp32), conf [B] or
    [B, 1] fp32 or None.  -> {"t_err_ang", "t_err_scale", "t_err_scale_sym", "t_err_euc", "repr_err": [B, 1], "R_err": [B]}, views of
    the rows row0 .. row0 + B of `out` (fp32 [capacity, 8]; None: a new [B, 8]), whose columns 6 and 7 hold conf (0 without) and 0."""
    fn = "pose_metrics"
    check_f32(fn, "R", R, rank=3)
    B = R.shape[0]
    check_f32(fn, "R", R, shape=(B, 3, 3))
    check_f32(fn, "t", t, shape=(B, 1, 3))
    named = [("R", R), ("t", t), ("T_0to1", T_0to1), ("Kori_color0", Kori_color0)]
    for name, v, shape in (("T_0to1", T_0to1, (B, 4, 4)), ("Kori_color0", Kori_color0, (B, 3, 3))):
        check_tensor(fn, name, v)
        if not v.is_floating_point() or tuple(v.shape) != shape:
            raise ValueError("%s: %s must be a floating-point tensor of shape %s, got %s %s" % (fn, name, shape, v.dtype, tuple(v.shape)))
    if conf is not None:
        check_f32(fn, "conf", conf)
        if tuple(conf.shape) not in ((B,), (B, 1)):
            raise ValueError("%s: conf must be [%d] or [%d, 1], got %s" % (fn, B, B, tuple(conf.shape)))
        named.append(("conf", conf))
    check_number(fn, "W", W, positive=True)
    check_number(fn, "H", H, positive=True)
    if out is None and row0 != 0:
        raise ValueError("%s: row0 = %r needs an out to index" % (fn, row0))
    if out is not None:
        check_f32(fn, "out", out, rank=2, width=RECORD_WIDTH)
        if not out.is_contiguous() or out.data_ptr() % 16:
            raise ValueError("%s: out must be contiguous and start at a 16-byte boundary" % fn)
        named.append(("out", out))
    if isinstance(row0, bool) or not isinstance(row0, numbers.Integral) or row0 < 0:
        raise ValueError("%s: row0 must be a non-negative integer, got %r" % (fn, row0))
    if out is not None and row0 + B > out.shape[0]:
        raise ValueError("%s: rows [%d, %d) do not fit into the %d records of out" % (fn, row0, row0 + B, out.shape[0]))
    check_devices(fn, named)
    if out is None:
        out = torch.empty((B, RECORD_WIDTH), device=R.device, dtype=torch.float32)
    ops.pose_metrics(R.detach(), t.detach(), T_0to1.detach().float(), Kori_color0.detach().float(),
                     None if conf is None else conf.detach().reshape(B), W, H, out, row0)
    return _metric_views(out[row0:row0 + B])


class ValidationAccumulator:
    """The records of a validation epoch on the device: [capacity, 8] for the pairs (pose_metrics' layout) and [steps, 3] for the
    (loss, loss_R, loss_t) of the validation steps, allocated once.  The row counts live on the host: add() reads nothing from the
    device, summary() is the one device -> host copy.  capacity <= 2^18 (the summary's ranking is quadratic in the record count).
    (The buffers are allocated on whatever `device` names; add() on tensors that are not on a GPU raises MickeyHipError.)"""

    def __init__(self, capacity, device, steps=None, W=540, H=720):
        fn = "ValidationAccumulator"
        steps = capacity if steps is None else steps
        for name, v in (("capacity", capacity), ("steps", steps)):
            if isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < 1:
                raise ValueError("%s: %s must be a positive integer, got %r" % (fn, name, v))
        if capacity > MAX_RECORDS:
            raise ValueError("%s: capacity %d is beyond the %d records the summary ranks (every record against every record)"
                             % (fn, capacity, MAX_RECORDS))
        check_number(fn, "W", W, positive=True)
        check_number(fn, "H", H, positive=True)
        self.W, self.H = W, H
        self.records = torch.zeros((int(capacity), RECORD_WIDTH), device=device, dtype=torch.float32)
        self.losses = torch.zeros((int(steps), 3), device=device, dtype=torch.float32)
        self.n = 0        # records held
        self.n_steps = 0  # loss rows held

    @property
    def capacity(self):
        return self.records.shape[0]

    def reset(self):
        self.n = self.n_steps = 0

    def add(self, R, t, inliers, batch, loss_outputs=None):
        """The metrics of one batch's poses against batch["T_0to1"] / batch["Kori_color0"], written into the next B rows (returned
        as pose_metrics returns them).  loss_outputs: the step's outputs dict, whose "loss", "avg_loss_rot" and "avg_loss_trans"
        (device scalars) become the next loss row."""
        fn = "ValidationAccumulator.add"
        for k in ("T_0to1", "Kori_color0"):
            if k not in batch:
                raise ValueError("%s: batch lacks %r" % (fn, k))
        check_tensor(fn, "R", R)
        B = R.shape[0] if R.dim() else 0
        if self.n + B > self.capacity:
            raise ValueError("%s: %d more records do not fit: %d of %d rows are taken" % (fn, B, self.n, self.capacity))
        row = None
        if loss_outputs is not None:
            if self.n_steps + 1 > self.losses.shape[0]:
                raise ValueError("%s: the %d loss rows are taken" % (fn, self.losses.shape[0]))
            for k in ("loss", "avg_loss_rot", "avg_loss_trans"):
                if k not in loss_outputs or not torch.is_tensor(loss_outputs[k]) or loss_outputs[k].numel() != 1:
                    raise ValueError("%s: loss_outputs[%r] must be a tensor of one element" % (fn, k))
            row = [loss_outputs[k].detach().reshape(()).to(device=self.records.device, dtype=torch.float32, non_blocking=True)
                   for k in ("loss", "avg_loss_rot", "avg_loss_trans")]
        views = pose_metrics(R, t, batch["T_0to1"], batch["Kori_color0"], conf=inliers, W=self.W, H=self.H, out=self.records,
                             row0=self.n)
        self.n += B
        if row is not None:
            torch.stack(row, out=self.losses[self.n_steps])
            self.n_steps += 1
        return views

    def summary_tensors(self, failures=0, thresholds=THRESHOLDS):
        """The summary's two launches, nothing read back: (out fp32 [16], work fp64 [blocks + 1, 16]) of ops.pose_summary."""
        fn = "ValidationAccumulator.summary"
        if self.n == 0:
            raise ValueError("%s: no records (add() has not been called since the last reset())" % fn)
        if isinstance(failures, bool) or not isinstance(failures, numbers.Integral) or failures < 0:
            raise ValueError("%s: failures must be a non-negative integer, got %r" % (fn, failures))
        thresholds = tuple(thresholds)
        if len(thresholds) != 5:
            raise ValueError("%s: thresholds must be (t, R, t2, R2, px), got %r" % (fn, thresholds))
        for v in thresholds:
            check_number(fn, "a threshold", v)
        return ops.pose_summary(self.records, self.n, failures, thresholds, self.losses if self.n_steps else None, self.n_steps)

    def summary(self, failures=0, thresholds=THRESHOLDS):
        """on_validation_epoch_end's numbers (model.py:205-280; the precisions over N + failures, benchmark/mapfree.py:105-108) under
        the trainer's log names, plus "n" and "n_bad_conf" (records whose confidence was not finite: ranked last).  The val_loss/*
        means are present when loss rows were added."""
        out = self.summary_tensors(failures, thresholds)[0].tolist()
        res = {"n": int(out[0]), "n_bad_conf": int(out[1])}
        res.update((name, out[k]) for k, name in _LOG_NAMES.items())
        if self.n_steps:
            res.update((name, out[k]) for k, name in _LOSS_NAMES.items())
        return res


def validation_step(model, batch, loss_fn, solver, acc, batch_idx=0):
    """model.py:66-89 for a model on the HIP kernels: the forward, prepare_batch_for_loss, the loss, the pose of `solver` (a
    HipProcrustesSolver) and its metrics, written into acc (a ValidationAccumulator) -- which takes the place of the reference's
    validation_step_outputs list.  Returns the outputs dict the reference builds."""
    if hasattr(model, "is_eval_model"):
        model.is_eval_model(True)
    model(batch)
    if hasattr(model, "prepare_batch_for_loss"):
        model.prepare_batch_for_loss(batch, batch_idx)
    else:
        batch["batch_idx"] = batch_idx
        batch["final_scores"] = batch["scores"] * batch["kp_scores"]
    avg_loss, outputs, probs_grad, num_its = loss_fn(batch)
    outputs["loss"] = avg_loss
    R, t, inliers = solver.estimate_pose_vectorized(batch)
    m = acc.add(R, t, inliers, batch, loss_outputs=outputs)
    outputs["metric_ours_t_err_ang"] = m["t_err_ang"]
    outputs["metric_ours_t_err_euc"] = m["t_err_euc"]
    outputs["metric_ours_R_err"] = m["R_err"]
    outputs["metric_inliers"] = inliers
    outputs["metric_ours_vcre"] = m["repr_err"]
    return outputs
