"""Differentiable dual-softmax matcher for training, on the HIP kernels (mk_dual_softmax_train / mk_dual_softmax_bwd).

The reference trainer back-propagates the REINFORCE gradient of its pose loss through the matcher
(lib/models/MicKey/model.py:124-134):

    torch.autograd.backward(torch.log(batch['final_scores'] + 1e-16), probs_grad[0])

with final_scores = dualSoftmax(dsc0, dsc1) * (scr0^T scr1) (feature_matcher.py:64-83, compute_correspondences.py:46-50,
model.py:201).  Its autograd graph keeps several [B, n0, n1] fp32 tensors per step (couplings, both softmaxes, their product,
kp_scores, final_scores).  Here the forward keeps only its inputs and the row / column log-sums ([B, 2, max(n0, n1)]); the
backward recomputes the correlation on the matrix cores (mk_matcher_bwd.hip).

    dual_softmax_train(dsc0, dsc1, scr0, scr1, temperature, dustbin)   the fused op: final_scores (scores without scr0 / scr1)
    DualSoftmax(cfg)                                                   drop-in for the reference's dualSoftmax(cfg) module
    use_hip_matcher(model)                                             swaps it into a reference-style model in place
"""
import math
import numbers

import torch

from . import ops
from ._train_common import check_f32, swap_modules


def _is_split(C, temperature, split):
    if split == "auto":
        return ops.dual_softmax_split_ok(C, temperature)
    if split is True or split is False:
        if split and not ops.dual_softmax_split_ok(C, temperature):
            raise ValueError("dual_softmax_train: split=True needs C == 128 and temperature >= log2(e) / 100 (mk_dual_softmax_split), "
                             "got C=%d, temperature=%g" % (C, temperature))
        return split
    raise ValueError("dual_softmax_train: split must be 'auto', True or False, got %r" % (split,))


_FN = "dual_softmax_train"


def _check_f32_device(name, t, dev):
    check_f32(_FN, name, t)
    if not t.is_cuda or (dev is not None and t.device != dev):   # (kept here: for this op a CPU tensor is a ValueError, not check_devices' MickeyHipError)
        raise ValueError("%s: %s must be a device tensor on %s, got %s" % (_FN, name, dev if dev is not None else "the GPU", t.device))


def _validate(dsc0, dsc1, scr0, scr1, temperature, dustbin):
    """Every check of dual_softmax_train, on the host, before anything is launched: raises ValueError."""
    for name, d in (("dsc0", dsc0), ("dsc1", dsc1)):
        if not torch.is_tensor(d) or d.dim() != 3:
            raise ValueError("%s: %s must be a [B, C, n] tensor, got %s" % (_FN, name, tuple(d.shape) if torch.is_tensor(d) else type(d).__name__))
    B, C, n0 = dsc0.shape
    if dsc1.shape[0] != B or dsc1.shape[1] != C:
        raise ValueError("%s: dsc0 %s and dsc1 %s must share B and C" % (_FN, tuple(dsc0.shape), tuple(dsc1.shape)))
    n1 = dsc1.shape[2]
    if B < 1 or n0 < 1 or n1 < 1:
        raise ValueError("%s: empty descriptors: dsc0 %s, dsc1 %s" % (_FN, tuple(dsc0.shape), tuple(dsc1.shape)))
    if C != 128:
        raise ValueError("%s: the HIP matcher backward needs C == 128 descriptor channels, got %d" % (_FN, C))
    _check_f32_device("dsc0", dsc0, None)
    _check_f32_device("dsc1", dsc1, dsc0.device)
    if (scr0 is None) != (scr1 is None):
        raise ValueError("%s: scr0 and scr1 go together (keypoint scores of both images, or neither)" % _FN)
    if scr0 is not None:
        for name, s, n in (("scr0", scr0, n0), ("scr1", scr1, n1)):
            if not torch.is_tensor(s) or s.numel() != B * n or tuple(s.shape) not in ((B, n), (B, 1, n)):
                raise ValueError("%s: %s must be [%d, %d] or [%d, 1, %d], got %s" %
                                 (_FN, name, B, n, B, n, tuple(s.shape) if torch.is_tensor(s) else type(s).__name__))
            _check_f32_device(name, s, dsc0.device)
    # (kept here: a bool passes as a temperature, as it always has; check_number refuses one)
    if not isinstance(temperature, numbers.Real) or not math.isfinite(float(temperature)) or float(temperature) <= 0:
        raise ValueError("%s: temperature must be a finite positive number, got %r" % (_FN, temperature))
    if dustbin is not None and not isinstance(dustbin, numbers.Real):
        if not torch.is_tensor(dustbin) or dustbin.numel() != 1:
            raise ValueError("%s: dustbin must be None, a number or a one-element tensor, got %r" % (_FN, dustbin))
        _check_f32_device("dustbin", dustbin, dsc0.device)
    return B, C, n0, n1


class DualSoftmaxTrainFn(torch.autograd.Function):
    """final_scores (scores without keypoint scores) of the dual softmax; saves its inputs and the [B, 2, max(n0, n1)] log-sums
    only.  Inputs: contiguous fp32 device tensors dsc0 [B, C, n0], dsc1 [B, C, n1], scr0 [B, n0] / scr1 [B, n1] or None,
    dustbin [1] or None (validated by dual_softmax_train)."""

    @staticmethod
    def forward(ctx, dsc0, dsc1, scr0, scr1, dustbin, temperature, split):
        out, lse = ops.dual_softmax_train_fwd(dsc0, dsc1, scr0, scr1, temperature, dustbin, split)
        ctx.save_for_backward(dsc0, dsc1, scr0, scr1, dustbin, lse)
        ctx.temperature, ctx.split = temperature, split
        return out

    @staticmethod
    def backward(ctx, grad):
        dsc0, dsc1, scr0, scr1, dustbin, lse = ctx.saved_tensors
        need = tuple(bool(x) for x in ctx.needs_input_grad[:5])
        if not any(need):
            return (None,) * 7
        need = (need[0], need[1], need[2] and scr0 is not None, need[3] and scr1 is not None, need[4] and dustbin is not None)
        g0, g1, gs0, gs1, gd = ops.dual_softmax_bwd(dsc0, dsc1, scr0, scr1, ctx.temperature, dustbin, lse,
                                                    grad.to(torch.float32).contiguous(), ctx.split, need)
        if gd is not None:
            gd = gd.sum().reshape(dustbin.shape)   # one value per pair, summed here in a fixed order
        return g0, g1, gs0, gs1, gd, None, None


def dual_softmax_train(dsc0, dsc1, scr0=None, scr1=None, temperature=0.1, dustbin=None, split="auto"):
    """Differentiable dualSoftmax (feature_matcher.py:64-83) times kp_matrix_scores (compute_correspondences.py:46-50).

    dsc0 [B, 128, n0], dsc1 [B, 128, n1] fp32 device tensors; scr0 / scr1 [B, n] or [B, 1, n] keypoint scores, or None.
    dustbin: None, a number (constant) or a one-element fp32 device tensor (e.g. the trainable dustbin_score Parameter; read on
    the device, no host synchronisation).  split: "auto" (ops.dual_softmax_split_ok: split-fp16 correlation for C == 128), True
    (split-fp16; descriptors must be unit-norm) or False (exact fp32 correlation).
    Returns final_scores [B, n0, n1] = scores * scr0^T scr1, or scores when no keypoint scores are given; differentiable in every
    tensor input that requires grad.  Bad shapes, dtypes, devices or C != 128 raise ValueError before anything is launched."""
    B, C, n0, n1 = _validate(dsc0, dsc1, scr0, scr1, temperature, dustbin)
    split = _is_split(C, float(temperature), split)
    if dustbin is not None and not torch.is_tensor(dustbin):
        dustbin = torch.tensor([float(dustbin)], device=dsc0.device, dtype=torch.float32)
    db = dustbin.reshape(1) if dustbin is not None else None
    s0 = scr0.reshape(B, n0).contiguous() if scr0 is not None else None
    s1 = scr1.reshape(B, n1).contiguous() if scr1 is not None else None
    return DualSoftmaxTrainFn.apply(dsc0.contiguous(), dsc1.contiguous(), s0, s1, db, float(temperature), bool(split))


class DualSoftmax(torch.nn.Module):
    """The reference's dualSoftmax(cfg) (feature_matcher.py:54-83) on the HIP kernels: cfg['TEMPERATURE'], cfg['USE_DUSTBIN'];
    attributes temperature / use_dustbin, a dustbin_score Parameter initialised to 1.0 with the dustbin (the same state_dict
    keys); forward(dsc0, dsc1) -> scores, differentiable in the descriptors and the dustbin.  split: as in dual_softmax_train."""

    def __init__(self, cfg, split="auto"):
        super().__init__()
        self.temperature = cfg["TEMPERATURE"]
        self.use_dustbin = False
        if cfg["USE_DUSTBIN"]:
            self.dustbin_score = torch.nn.Parameter(torch.tensor(1.))
            self.use_dustbin = True
        self.split = split

    def forward(self, dsc0, dsc1):
        return dual_softmax_train(dsc0, dsc1, temperature=self.temperature,
                                  dustbin=self.dustbin_score if self.use_dustbin else None, split=self.split)


def _is_dual_softmax(m):
    """The reference dualSoftmax's attribute contract: a numeric `temperature`, a boolean `use_dustbin`, and with the dustbin a
    scalar Parameter `dustbin_score` (the Sinkhorn matcher has no temperature / use_dustbin)."""
    if not isinstance(m, torch.nn.Module) or isinstance(m, DualSoftmax):
        return False
    if not isinstance(getattr(m, "temperature", None), numbers.Real) or not isinstance(getattr(m, "use_dustbin", None), bool):
        return False
    if m.use_dustbin:
        p = getattr(m, "dustbin_score", None)
        return isinstance(p, torch.nn.Parameter) and p.numel() == 1
    return True


def use_hip_matcher(model, split="auto"):
    """Replace every dual-softmax `matching_mat` inside `model` (a reference-style training model: featureMatcher.matching_mat,
    feature_matcher.py:13) by DualSoftmax, in place.  The dustbin_score Parameter OBJECT is kept, so optimiser state and
    checkpoints stay valid.  Returns the number of modules swapped."""
    def make(old):
        if not _is_dual_softmax(old):
            return None
        new = DualSoftmax({"TEMPERATURE": old.temperature, "USE_DUSTBIN": False}, split=split)
        if old.use_dustbin:
            new.dustbin_score = old.dustbin_score
            new.use_dustbin = True
        return new.train(old.training)

    return swap_modules(model, make, name="matching_mat")
