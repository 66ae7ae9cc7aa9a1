"""The reference trainer's backward_step (lib/models/MicKey/model.py:91-147) for a HipAdam, without a host synchronisation.

The reference runs avg_loss.backward(), asks the host five times whether probs_grad[0] or a keypoint / depth gradient holds a NaN
or an Inf, runs the second backward, clips, asks once more about every parameter's gradient and steps.  Here the two backward
passes are enqueued back to back and HipAdam.step_guarded makes every one of those decisions on the device.

One deviation: where a check fires, the reference returns BEFORE the second backward; this version runs it and skips the update on
the device.  Parameters, exp_avg, exp_avg_sq and the step counts end up the same; the .grad tensors, which the next zero_grad()
discards, differ.
"""
import torch

from .train_optim import HipAdam

_WATCHED = ("kps0", "kps1", "depth0", "depth1")


def backward_step(model, batch, outputs, probs_grad, avg_loss, num_its, opt):
    """model.py:91-147 for opt, a HipAdam over model's trainable parameters.  batch, outputs, probs_grad, avg_loss and num_its are
    what the reference's training_step hands to its backward_step: outputs["kps0" | "kps1" | "depth0" | "depth1"] retain their
    gradients, batch["final_scores" | "kps0" | "kps1" | "depth_kp0" | "depth_kp1"] are the graph's ends of the second backward.
    Returns None, with nothing launched, when num_its == 0 (no valid hypotheses); else the fp32 device tensor [ok, total_norm] of
    step_guarded(max_norm=5, also_finite=(probs_grad[0] and the keypoint / depth gradients that exist)): ok == 0 means the step
    was skipped where the reference returns False.  Nothing in here reads a device tensor."""
    if not isinstance(opt, HipAdam):
        raise ValueError("backward_step: opt must be a mickey_amd.train_optim.HipAdam, got %s" % type(opt).__name__)
    opt.zero_grad()
    if num_its == 0:
        return None
    avg_loss.backward()
    grads = {k: outputs[k].grad for k in _WATCHED}
    log_scores = torch.log(batch["final_scores"] + 1e-16)
    if batch["kps0"].requires_grad:
        torch.autograd.backward((log_scores, batch["kps0"], batch["kps1"], batch["depth_kp0"], batch["depth_kp1"]),
                                (probs_grad[0], grads["kps0"], grads["kps1"], grads["depth0"], grads["depth1"]))
    elif batch["depth_kp0"].requires_grad:
        torch.autograd.backward((log_scores, batch["depth_kp0"], batch["depth_kp1"]), (probs_grad[0], grads["depth0"], grads["depth1"]))
    else:
        torch.autograd.backward((log_scores,), (probs_grad[0],))
    watched = (probs_grad[0],) + tuple(grads[k] for k in _WATCHED if grads[k] is not None)
    return opt.step_guarded(max_norm=5, also_finite=watched)
