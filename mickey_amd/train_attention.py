"""Trainable linear attention of the four heads on the HIP kernels: forward and backward (mk_linattn_train_fwd / _bwd).

Every head runs Transformer_self_att(d_model=128, num_layers=3); each EncoderLayer calls Attention.forward_linear
(att_layers/attention.py:46-64): two elu + 1 maps, three einsums on [N, L, 8, 16] tensors, a sum, a reciprocal and several
broadcasts -- about 25 small device ops forward and 28 backward in torch, with 11 saved tensors.  Here, per image n and head h
(D = 16), phi(x) = x + 1 for x > 0, else exp(x):

    forward   M[d, v] = sum_s phi(k)[s, d] (v[s, v] / S)        ks[d] = sum_s phi(k)[s, d]
              den[l]  = phi(q)[l] . ks + eps                     out[l, v] = (phi(q)[l] . M[:, v]) / den[l] * S
    backward  gnum[l, v] = gO[l, v] S / den[l]                   gden[l] = -(gO[l] . out[l]) / den[l]
              gQ[l, d] = (sum_v gnum[l, v] M[d, v] + gden[l] ks[d]) phi'(q[l, d])        phi'(x) = 1 for x > 0, else phi(x)
              gM[d, v] = sum_l phi(q)[l, d] gnum[l, v]           gks[d] = sum_l phi(q)[l, d] gden[l]
              gK[s, d] = (sum_v (v[s, v] / S) gM[d, v] + gks[d]) phi'(k[s, d])
              gV[s, v] = (sum_d phi(k)[s, d] gM[d, v]) / S

in three launches forward and three backward, all fp32.  The forward keeps q, k, v and the [N H, 272] block M | ks; the backward
recomputes den and out.  Both token sums are chunked and added in a fixed order (no atomics): results are bit-identical from run
to run, and image i of a batch gets the bits it gets alone.  A NaN or an Inf in q, k, v or the incoming gradient reaches every
value computed from it.

    linear_attention_train(q, k, v, eps)    the differentiable op
    LinearAttention(eps)                    parameterless nn.Module with the reference Attention's call contract
    use_hip_attention(model)                swaps it into a reference-style model in place (next to use_hip_matcher /
                                            use_hip_encoder / use_hip_convs)

Not covered here: the q / k / v / merge / MLP nn.Linears and the LayerNorms of EncoderLayer (train_layer.py runs the whole layer
around this core as one node); BatchNorm, ReLU and the 1x1 shortcut of BasicBlock (train_block.py), the 1x1 tail convolutions (train_tails.py); autocast and half-precision inputs (ValueError); double backward; head sizes other than 16; hipGraph capture
of a step.
"""
import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import ops
from ._train_common import aligned_copy, check_devices, check_f32, check_grad, check_number, is_number, rows_in_place, swap_modules

HEAD_DIM = 16
MAX_CHANNELS = 128


# ---- the formulas the kernels implement, as plain torch (any device, any float dtype: tests, documentation) --------------------
def feature_map(x):
    """phi(x) = elu(x) + 1 = x + 1 for x > 0, else exp(x)."""
    return torch.where(x > 0, x + 1, torch.exp(torch.clamp(x, max=0)))


def _dphi(x, p):
    return torch.where(x > 0, torch.ones_like(p), p)


def _forward_terms(q, k, v, eps):
    S = v.shape[1]
    Qp, Kp = feature_map(q), feature_map(k)
    M = torch.einsum("nshd,nshv->nhdv", Kp, v / S)
    ks = Kp.sum(dim=1)
    den = torch.einsum("nlhd,nhd->nlh", Qp, ks) + eps
    out = torch.einsum("nlhd,nhdv->nlhv", Qp, M) / den[..., None] * S
    return S, Qp, Kp, M, ks, den, out


def linear_attention_formula(q, k, v, eps=1e-6):
    """out [N, L, H, D] of the forward formulas above; q [N, L, H, D], k, v [N, S, H, D]."""
    return _forward_terms(q, k, v, eps)[-1]


def linear_attention_grads(q, k, v, go, eps=1e-6):
    """(gQ, gK, gV) of the backward formulas above for the incoming gradient go [N, L, H, D], without autograd."""
    S, Qp, Kp, M, ks, den, out = _forward_terms(q, k, v, eps)
    gnum = go * S / den[..., None]
    gden = -(go * out).sum(dim=-1) / den
    gq = (torch.einsum("nlhv,nhdv->nlhd", gnum, M) + gden[..., None] * ks[:, None]) * _dphi(q, Qp)
    gM = torch.einsum("nlhd,nlhv->nhdv", Qp, gnum)
    gks = torch.einsum("nlhd,nlh->nhd", Qp, gden)
    gk = (torch.einsum("nshv,nhdv->nshd", v / S, gM) + gks[:, None]) * _dphi(k, Kp)
    gv = torch.einsum("nshd,nhdv->nshv", Kp, gM) / S
    return gq, gk, gv


# ---- the op ----------------------------------------------------------------------------------------------------------------
def _validate(q, k, v, eps):
    """Every check of linear_attention_train, on the host, before anything is launched."""
    fn = "linear_attention_train"
    for name, t in (("q", q), ("k", k), ("v", v)):
        check_f32(fn, name, t, rank=4, width=HEAD_DIM, why=" ([N, tokens, H, 16]: heads of 16 channels only)")
    if q.shape[2] * HEAD_DIM > MAX_CHANNELS:
        raise ValueError("%s: at most %d channels (%d heads), got %d heads" % (fn, MAX_CHANNELS, MAX_CHANNELS // HEAD_DIM, q.shape[2]))
    if k.shape[0] != q.shape[0] or k.shape[2] != q.shape[2]:
        raise ValueError("%s: q %s and k %s must share N and H" % (fn, tuple(q.shape), tuple(k.shape)))
    if tuple(v.shape) != tuple(k.shape):
        raise ValueError("%s: k %s and v %s must have the same shape" % (fn, tuple(k.shape), tuple(v.shape)))
    check_number(fn, "eps", eps)
    check_devices(fn, [("q", q), ("k", k), ("v", v)])


def _rows(t):
    """The [N, T, H, 16] tensor itself when the kernels can read it in place (the last two dimensions dense, token rows by
    _train_common.rows_in_place, images any non-negative multiple of 4 elements apart), else a contiguous, aligned copy."""
    N, T, H, _ = t.shape
    C = H * HEAD_DIM
    if ((H == 1 or t.stride(2) == HEAD_DIM) and (N == 1 or (t.stride(0) >= 0 and t.stride(0) % 4 == 0))
            and rows_in_place(t, C, t.stride(1) if T > 1 else C)):
        return t
    return aligned_copy(t)


class LinearAttentionTrainFn(torch.autograd.Function):
    """out = linear attention of (q, k, v).  Saves q, k, v and the [N H, 272] block M | ks; under torch.no_grad() nothing.  Inputs
    validated and laid out by linear_attention_train."""

    @staticmethod
    def forward(ctx, q, k, v, eps):
        with torch.cuda.device(q.device):
            out, kv = ops.linattn_train_fwd(q.detach(), k.detach(), v.detach(), eps)
        ctx.eps = eps
        if any(ctx.needs_input_grad[:3]):
            ctx.save_for_backward(q, k, v, kv)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, go):
        q, k, v, kv = ctx.saved_tensors
        check_grad("linear_attention_train", go)
        with torch.cuda.device(go.device):
            gq, gk, gv = ops.linattn_train_bwd(q, k, v, kv, go.contiguous(), ctx.eps, tuple(ctx.needs_input_grad[:3]))
        return gq, gk, gv, None


def linear_attention_train(q, k, v, eps=1e-6):
    """Differentiable Attention.forward_linear (att_layers/attention.py:46-64) on the HIP kernels.

    q: fp32 [N, L, H, 16] device tensor; k, v: fp32 [N, S, H, 16]; H <= 8; L and S may differ.  Tensors whose last two dimensions
    are dense (e.g. the three thirds of one packed [N, L, 3 C] buffer) are read in place, other layouts are made contiguous first.
    Returns a contiguous fp32 [N, L, H, 16]; differentiable in q, k and v (only the gradients that are needed are computed).
    Wrong dtypes / ranks / head sizes, more than 128 channels, mismatched N, H or S and empty tensors raise ValueError, CPU tensors
    MickeyHipError, all before any launch.  Not covered: autocast (half-precision inputs), double backward."""
    _validate(q, k, v, eps)
    return LinearAttentionTrainFn.apply(_rows(q), _rows(k), _rows(v), float(eps))


class LinearAttention(nn.Module):
    """The reference's Attention(attention='linear') (att_layers/attention.py:14-21,46-64) on the HIP kernels: no parameters, the
    attributes `eps` and `attention`, forward(queries [N, L, H, 16], keys [N, S, H, 16], values [N, S, H, 16]) -> [N, L, H, 16]."""

    def __init__(self, eps=1e-6):
        super().__init__()
        check_number("LinearAttention", "eps", eps)
        self.eps = eps
        self.attention = "linear"

    def extra_repr(self):
        return "eps=%g, attention='linear'" % self.eps

    def forward(self, queries, keys, values):
        return linear_attention_train(queries, keys, values, self.eps)


_PROBE = (-3.0, -1.0, -0.25, 0.0, 0.5, 2.0)


def _is_linear_attention(m):
    """The reference Attention's attribute contract, not its class: attention == 'linear', a numeric eps, no parameters, and a
    callable feature_map that IS elu(x) + 1 (probed on a small vector)."""
    if not isinstance(m, nn.Module) or isinstance(m, LinearAttention):
        return False
    if getattr(m, "attention", None) != "linear":
        return False
    if not is_number(getattr(m, "eps", None)):
        return False
    if next(m.parameters(), None) is not None:
        return False
    fm = getattr(m, "feature_map", None)
    if not callable(fm):
        return False
    x = torch.tensor(_PROBE, dtype=torch.float64)
    try:
        with torch.no_grad():
            y = fm(x.clone())
    except Exception:
        return False
    return torch.is_tensor(y) and y.shape == x.shape and bool(torch.allclose(y.double(), feature_map(x), rtol=1e-12, atol=0.0))


def use_hip_attention(model):
    """Replace, in place, every submodule of `model` that has the reference linear Attention's attributes (attention == 'linear', a
    numeric eps, no parameters, feature_map == elu + 1) by a LinearAttention with the same eps.  'full' and 'flash' attention
    modules and everything else are left alone; the modules swapped hold no parameters or buffers, so state-dict keys and
    Parameter objects do not change.  Returns the number of modules swapped; a second call finds none."""
    def make(m):
        if _is_linear_attention(m):
            return LinearAttention(m.eps).train(m.training)

    return swap_modules(model, make)
