"""Trainable BasicBlock of the four heads on the HIP kernels: what a block runs around its two 3x3 convolutions, as small ops.

A BasicBlock (utils/extractor_utils.py:12-35; 16 per model, mickey_extractor.py:76-79,155-158,194-197,232-235) is two 3x3
convolutions and, around them, two nn.BatchNorm2d in batch-statistics mode, two ReLUs, the residual add and -- where the channel count
changes -- a bias-free 1x1 shortcut convolution: in torch about a dozen launches forward and as many backward, each a full pass over
an [M, C] fp32 tensor (M = B H W).  Here BatchNorm, the residual add and the ReLU are ONE autograd node of at most 2 launches forward
(1 in eval mode) and 2 backward on mk_train_bn_* (mk_train_bn.hip), and the shortcut is one node over the Linear kernels of the
EncoderLayer (mk_train_linear_*, mk_train_tail): fp32 data on the vector ALU (the BatchNorm backward takes its per-channel sums and
its x - mean terms in fp64), every sum in an order fixed by the shape.  Results are bit-identical from
run to run, gradients are bit-linear in the incoming gradient under a power-of-two scale, nothing synchronises with the host, and
the running statistics are updated on the device.  Activations are read where the preceding op left them when they are
channels_last (what conv3x3_train returns); results are channels_last.

    batchnorm_act_train(x, bn_weight, bn_bias, running_mean, running_var, num_batches_tracked, training, momentum, eps,
                        resid=None, relu=True)       act(BatchNorm2d(x) (+ resid))
    conv1x1_train(x, weight)                         the bias-free 1x1 shortcut
    batchnorm_act_formula(...), basic_block_formula(...)      the same in plain torch, any device / float dtype
    HipBasicBlock                                    a block made of the very children of the one it replaces
    use_hip_blocks(model)                            swaps it into a reference-style model, returns the count

The block's input at resblock1 is the encoder's contiguous NCHW tensor: the shortcut copies it to rows once per block (a
channels_last output of FrozenDinoV2 is not covered).  Not covered either: momentum=None (the cumulative average), BatchNorm without
affine parameters or running statistics, widths that are no multiple of 4 or beyond 1024, shortcuts with a bias, a stride or widths
that are no multiple of 16 (all left alone by use_hip_blocks, ValueError from the ops), autocast and half precision (ValueError),
double backward, hipGraph capture of a step, SyncBatchNorm, folding the statistics into the convolution's epilogue, one launch across
the four heads.
"""
import torch
import torch.nn.functional as F
from torch import nn
from torch.autograd.function import once_differentiable

from . import ops
from ._train_common import (adopt, aligned_copy, check_devices, check_f32, check_grad, check_number, check_tensor, is_number,
                            rows_in_place, swap_modules)
from .train_layer import LinearTrainFn


# ---- the block as plain torch (any device, any float dtype) ------------------------------------------------------------------
def batchnorm_act_formula(x, bn_weight, bn_bias, running_mean, running_var, num_batches_tracked, training, momentum, eps,
                          resid=None, relu=True, mask=None):
    """utils/extractor_utils.py:30-34 restated for one BatchNorm: act(BatchNorm2d(x) (+ resid)), x [B, C, H, W].  In training the
    batch's mean and biased variance normalise, and running_mean / running_var (with the unbiased variance) / num_batches_tracked
    are updated in place as nn.BatchNorm2d does; in eval the running statistics normalise.  mask (a constant [B, C, H, W] tensor of
    zeros and ones) replaces the ReLU's own sign test: y = z mask."""
    C = x.shape[1]
    shape = (1, C, 1, 1)
    if training:
        M = x.numel() // C
        if M <= 1:
            raise ValueError("Expected more than 1 value per channel when training, got input size %s" % (tuple(x.shape),))
        mean = x.mean((0, 2, 3))
        var = (x - mean.view(shape)).pow(2).mean((0, 2, 3))
        with torch.no_grad():
            running_mean.mul_(1 - momentum).add_(momentum * mean)
            running_var.mul_(1 - momentum).add_(momentum * (var * (M / (M - 1))))
            num_batches_tracked.add_(1)
    else:
        mean, var = running_mean, running_var
    xhat = (x - mean.view(shape)) * (var.view(shape) + eps).rsqrt()
    z = xhat * bn_weight.view(shape) + bn_bias.view(shape)
    if resid is not None:
        z = z + resid
    if not relu:
        return z
    return z * mask if mask is not None else torch.relu(z)


def basic_block_formula(x, conv1_weight, bn1, conv2_weight, bn2, shortcut_weight=None, training=True, relu=True):
    """utils/extractor_utils.py:28-35 restated: bn1 and bn2 are (weight, bias, running_mean, running_var, num_batches_tracked,
    momentum, eps) of the two BatchNorms (the buffers are updated in place in training); shortcut_weight [Cout, Cin, 1, 1] or None."""
    shortcut = x if shortcut_weight is None else F.conv2d(x, shortcut_weight)
    w1, b1, rm1, rv1, n1, mom1, eps1 = bn1
    w2, b2, rm2, rv2, n2, mom2, eps2 = bn2
    out = batchnorm_act_formula(F.conv2d(x, conv1_weight, padding=1), w1, b1, rm1, rv1, n1, training, mom1, eps1)
    return batchnorm_act_formula(F.conv2d(out, conv2_weight, padding=1), w2, b2, rm2, rv2, n2, training, mom2, eps2, resid=shortcut, relu=relu)


# ---- layouts ---------------------------------------------------------------------------------------------------------------
def _row_stride(x):
    """the distance between the [C] rows of x [B, C, H, W] when its memory holds them evenly spaced in (b, h, w) order and the kernels
    can read them in place (_train_common.rows_in_place; a channel slice of a wider channels_last map included), else 0"""
    B, C, H, W = x.shape
    dims = [(n, s) for n, s in ((W, x.stride(3)), (H, x.stride(2)), (B, x.stride(0))) if n > 1]   # innermost first
    ld = dims[0][1] if dims else C
    span = 1
    for n, s in dims:
        if s != span * ld:
            return 0
        span *= n
    return ld if rows_in_place(x.permute(0, 2, 3, 1), C, ld) else 0


def _rows2d(x):
    """[B, C, H, W] -> the [B H W, C] rows the kernels read: a view of x's own memory when it holds channels_last rows, else of one
    channels_last copy.  Differentiable (dense rows: plain view ops)."""
    B, C, H, W = x.shape
    ld = _row_stride(x)
    if ld == C:
        return x.permute(0, 2, 3, 1).reshape(B * H * W, C)   # a view: the rows are dense
    if ld:
        return x.as_strided((B * H * W, C), (ld, 1), x.storage_offset())
    return aligned_copy(x.permute(0, 2, 3, 1)).view(B * H * W, C)


def _nchw(rows, B, H, W):
    """dense rows [B H W, C] as a [B, C, H, W] tensor in channels_last memory: no copy"""
    return rows.view(B, H, W, rows.shape[1]).permute(0, 3, 1, 2)


# ---- BatchNorm + residual + ReLU -----------------------------------------------------------------------------------------------
class BatchNormActFn(torch.autograd.Function):
    """y = act(BatchNorm(x) (+ resid)), [B, C, H, W] in and out (the layouts are settled in here: one autograd node, no view nodes
    around it).  Saves x's rows, the weight, mean | rstd (2 C floats) and, for the ReLU, one byte per element; neither y nor resid.
    Under torch.no_grad() nothing is saved (the running statistics still move in training)."""

    @staticmethod
    def forward(ctx, x, weight, bias, resid, buffers, training, momentum, eps, relu, grad_on):
        need = grad_on and any(ctx.needs_input_grad)   # (under torch.no_grad() needs_input_grad still names the leaves)
        B, C, H, W = x.shape
        running_mean, running_var, nbt = buffers
        x2 = _rows2d(x.detach())
        with torch.cuda.device(x.device):
            y, stats, mask = ops.train_bn_fwd(x2, aligned_copy(weight.detach()), aligned_copy(bias.detach()), running_mean, running_var, nbt,
                                              training, momentum, eps, resid=None if resid is None else _rows2d(resid.detach()), relu=relu,
                                              want_saved=need)
        if training:
            torch.autograd.graph.increment_version(buffers)   # written by the kernel: autograd's in-place checks see it, as with torch's batch_norm
        if need:
            ctx.cfg = (training, relu, eps, (B, H, W))
            ctx.save_for_backward(x2, weight, stats, mask)
        return _nchw(y, B, H, W)

    @staticmethod
    @once_differentiable
    def backward(ctx, go):
        training, relu, eps, (B, H, W) = ctx.cfg
        x2, weight, stats, mask = ctx.saved_tensors
        check_grad("batchnorm_act_train", go)
        nx, nw, nb, nr = ctx.needs_input_grad[:4]
        with torch.cuda.device(go.device):
            gx, gresid, affine = ops.train_bn_bwd(_rows2d(go), x2, aligned_copy(weight.detach()), stats, mask, training, eps, want_gx=nx,
                                                  want_gresid=nr and relu, want_affine=nw or nb)
        if nr:
            gresid = _nchw(gresid, B, H, W) if relu else go   # no ReLU: the residual's gradient is the incoming one itself
        return (_nchw(gx, B, H, W) if nx else None, affine[0] if nw else None, affine[1] if nb else None, gresid if nr else None,
                None, None, None, None, None, None)


def _check_bn_args(fn, x, bn_weight, bn_bias, running_mean, running_var, num_batches_tracked, training, momentum, eps, resid):
    check_f32(fn, "x", x, rank=4, why=" ([B, C, H, W])")
    C = x.shape[1]
    if C < ops.BN_MIN_C or C > ops.BN_MAX_C or C % 4:
        raise ValueError("%s: the channel count of x must be a multiple of 4 in [%d, %d], got %d" % (fn, ops.BN_MIN_C, ops.BN_MAX_C, C))
    named = [("x", x)]
    for name, t in (("bn_weight", bn_weight), ("bn_bias", bn_bias), ("running_mean", running_mean), ("running_var", running_var)):
        check_f32(fn, name, t, shape=(C,), why=" (affine BatchNorm2d with running statistics)")
        named.append((name, t))
    for name, t in (("running_mean", running_mean), ("running_var", running_var)):   # updated where they lie: no copy can stand in
        if not t.is_contiguous() or t.data_ptr() % 16:
            raise ValueError("%s: %s must be contiguous and start at a 16-byte boundary" % (fn, name))
    check_tensor(fn, "num_batches_tracked", num_batches_tracked)
    if num_batches_tracked.dtype != torch.int64 or num_batches_tracked.numel() != 1:
        raise ValueError("%s: num_batches_tracked must be one int64 element, got %s %s"
                         % (fn, num_batches_tracked.dtype, tuple(num_batches_tracked.shape)))
    named.append(("num_batches_tracked", num_batches_tracked))
    if resid is not None:
        check_f32(fn, "resid", resid, shape=tuple(x.shape), why=" (the shape of x)")
        named.append(("resid", resid))
    if not isinstance(training, bool):
        raise ValueError("%s: training must be a bool, got %r" % (fn, training))
    check_number(fn, "momentum", momentum)
    check_number(fn, "eps", eps)
    if training and x.numel() // C <= 1:
        raise ValueError("%s: Expected more than 1 value per channel when training, got input size %s" % (fn, tuple(x.shape)))
    check_devices(fn, named)


def batchnorm_act_train(x, bn_weight, bn_bias, running_mean, running_var, num_batches_tracked, training, momentum, eps, resid=None,
                        relu=True):
    """Differentiable act(nn.BatchNorm2d(x) (+ resid)) (utils/extractor_utils.py:30-34) on the HIP kernels: x and resid fp32
    [B, C, H, W] device tensors (channels_last rows are read in place, any other layout is copied once), bn_weight / bn_bias /
    running_mean / running_var the module's own [C] tensors, num_batches_tracked its int64 buffer; C a multiple of 4 in [4, 1024].
    training: the batch's statistics normalise and the three buffers are updated on the device (also under torch.no_grad()); else
    the running statistics normalise and nothing is updated.  relu=False: the identity.  Returns [B, C, H, W] in channels_last
    memory.  Differentiable in x, bn_weight, bn_bias and resid; only the gradients that are needed are computed.  Bad dtypes /
    shapes / channel counts / momentum / eps and a single value per channel in training raise ValueError, CPU tensors MickeyHipError,
    all before any launch."""
    fn = "batchnorm_act_train"
    _check_bn_args(fn, x, bn_weight, bn_bias, running_mean, running_var, num_batches_tracked, training, momentum, eps, resid)
    return BatchNormActFn.apply(x, bn_weight, bn_bias, resid, (running_mean, running_var, num_batches_tracked), training, float(momentum),
                                float(eps), bool(relu), torch.is_grad_enabled())


# ---- the 1x1 shortcut ----------------------------------------------------------------------------------------------------------
def supported_shortcut(cin, cout):
    return cin > 0 and cout > 0 and cin % 16 == 0 and cout % 16 == 0


def conv1x1_train(x, weight):
    """Differentiable bias-free nn.Conv2d(kernel_size=1, stride=1) (utils/extractor_utils.py:23-26) on mk_train_linear_fwd / _dgrad /
    _wgrad and mk_train_tail: the 1x1 weight [Cout, Cin, 1, 1] is dense in nn.Linear's [N, K] layout.  x: fp32 [B, Cin, H, W] device
    tensor (channels_last rows are read in place; a contiguous NCHW tensor, which is what the encoder hands to resblock1, is copied
    to rows once); Cin and Cout multiples of 16.  Returns [B, Cout, H, W] in channels_last memory.  Differentiable in both."""
    fn = "conv1x1_train"
    check_f32(fn, "x", x, rank=4, why=" ([B, Cin, H, W])")
    check_f32(fn, "weight", weight, rank=4, why=" ([Cout, Cin, 1, 1])")
    if tuple(weight.shape[2:]) != (1, 1):
        raise ValueError("%s: weight must be [Cout, Cin, 1, 1], got %s" % (fn, tuple(weight.shape)))
    if x.shape[1] != weight.shape[1]:
        raise ValueError("%s: x has %d channels, weight expects %d" % (fn, x.shape[1], weight.shape[1]))
    if not supported_shortcut(weight.shape[1], weight.shape[0]):
        raise ValueError("%s: Cin and Cout must be multiples of 16, got Cin=%d, Cout=%d" % (fn, weight.shape[1], weight.shape[0]))
    check_devices(fn, [("x", x), ("weight", weight)])
    B, _, H, W = x.shape
    out = LinearTrainFn.apply(_rows2d(x), aligned_copy(weight.reshape(weight.shape[0], weight.shape[1])))
    return _nchw(out, B, H, W)


# ---- the block and the swap ----------------------------------------------------------------------------------------------------
class HipBasicBlock(nn.Module):
    """A BasicBlock made of the very children of the one it replaces (conv1, bn1, conv2, bn2 and, where there is one, shortcut) under
    the same names.  forward calls the child convolutions whatever they are (nn.Conv2d, or Conv3x3 after use_hip_convs) and runs
    BatchNorm, residual and ReLU as batchnorm_act_train, the shortcut as conv1x1_train."""

    @classmethod
    def adopt(cls, block):
        return adopt(cls, block)

    @staticmethod
    def _bn(x, bn, resid=None, relu=True):
        return batchnorm_act_train(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked, bn.training,
                                   bn.momentum, bn.eps, resid=resid, relu=relu)

    def forward(self, x, relu=True):
        shortcut = self._modules.get("shortcut")
        resid = conv1x1_train(x, shortcut[0].weight) if shortcut is not None and len(shortcut) else x
        out = self._bn(self.conv1(x), self.bn1)
        return self._bn(self.conv2(out), self.bn2, resid=resid, relu=relu)


def _is_bn(m):
    return (type(m) is nn.BatchNorm2d and m.affine and m.track_running_stats and is_number(m.momentum) and m.weight.dtype == torch.float32
            and m.running_mean is not None and m.running_mean.dtype == torch.float32 and is_number(m.eps)
            and ops.BN_MIN_C <= m.num_features <= ops.BN_MAX_C and m.num_features % 4 == 0)


def _is_shortcut(m, cout):
    """no shortcut, an empty nn.Sequential, or an nn.Sequential of exactly one 1x1 convolution that conv1x1_train covers"""
    if m is None:
        return True
    if type(m) is not nn.Sequential or len(m) > 1:
        return False
    if len(m) == 0:
        return True
    c = m[0]
    return (type(c) is nn.Conv2d and c.bias is None and c.kernel_size == (1, 1) and c.stride == (1, 1) and c.padding == (0, 0)
            and c.dilation == (1, 1) and c.groups == 1 and c.weight.dtype == torch.float32 and c.out_channels == cout
            and supported_shortcut(c.in_channels, c.out_channels))


def _takes(m):
    if not isinstance(m, nn.Module) or isinstance(m, HipBasicBlock):
        return False
    mods = m._modules
    if any(not isinstance(mods.get(n), nn.Module) for n in ("conv1", "conv2", "bn1", "bn2")):
        return False
    if set(mods) - {"conv1", "conv2", "bn1", "bn2", "shortcut"}:
        return False
    return _is_bn(mods["bn1"]) and _is_bn(mods["bn2"]) and _is_shortcut(mods.get("shortcut"), mods["bn2"].num_features)


def use_hip_blocks(model):
    """Replace, in place, every submodule of `model` that has the structure of the reference's BasicBlock -- children conv1, bn1,
    conv2, bn2 and nothing else but an optional `shortcut`; both BatchNorms nn.BatchNorm2d with affine parameters, running statistics,
    a numeric momentum, fp32 and a channel count that is a multiple of 4 in [4, 1024]; the shortcut absent, an empty nn.Sequential, or
    an nn.Sequential of exactly one bias-free 1x1 stride-1 nn.Conv2d with Cin and Cout multiples of 16 -- by a HipBasicBlock that
    holds the very same children, Parameters and buffers under the same names: state-dict keys, Parameter objects, optimiser state
    and checkpoints do not change; only forward differs.  Anything else is left alone: blocks built with bn=False (nn.Identity),
    momentum=None, a shortcut that holds a BatchNorm, a bias or a stride.  Composes with the other use_hip_* calls in any order.
    Returns the number of blocks swapped; a second call finds none."""
    def make(m):
        if _takes(m):
            return HipBasicBlock.adopt(m)

    return swap_modules(model, make)
