"""Trainable tails of the four heads on the HIP kernels: what each head runs after resblock4, one autograd node per head.

The detector's 1x1 `score` conv with remove_brd_and_softmax (or remove_borders(sigmoid(.))), the offset head's 1x1 `xy_offset` conv
with its sigmoid, the depth head's 1x1 `depth` conv (optionally max_depth * sigmoid(.)) and the descriptors' desc_l2norm
(mickey_extractor.py:98-124, 134-140, 172-176, 211-216, 248-249; utils/extractor_utils.py:6-10) are in torch about 30 launches of a
few hundred KB forward and about 40 backward per extractor call.  Here a tail is one launch forward (two for the detector softmax)
and at most three backward (one for the descriptors) on mk_train_headtail_* / mk_train_desc_l2norm_* (mk_train_headtails.hip): fp32
on the vector ALU, every sum in an order fixed by the shape.  Results are bit-identical from run to run, image i of a batch gets the
forward and input-gradient bits it gets alone, gradients are bit-linear in the incoming gradient under a power-of-two scale, and
nothing synchronises with the host.  The features are read where the preceding op left them when they are channels_last; the
descriptors come out contiguous [B, C, H, W], the layout the matcher reads.

    score_tail_train(feat, weight, border, use_softmax, temperature, eps)    the detector tail
    offset_tail_train(feat, weight)                                          sigmoid(xy_offset(feat))
    depth_tail_train(feat, weight, use_sigmoid, max_depth)                   depth(feat) or max_depth sigmoid(depth(feat))
    desc_l2norm_train(x, eps)                                                x / sqrt(sum_c x^2 + eps)
    *_formula(...)                                                           the same in plain torch, any device / dtype
    use_hip_tails(model)                                                     swaps them into a reference-style model, returns the count

Not covered: 1x1 convs with a bias or more than 2 outputs, widths that are no multiple of 4 or beyond 256 (ValueError), autocast and
half precision (ValueError), double backward, hipGraph capture of a step, BatchNorm / ReLU / the shortcut of BasicBlock (they are
train_block.py), the positional encoding, get_abs_kpts_coordinates, one launch across the four heads.
"""
import inspect
import numbers

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import ops
from ._train_common import adopt, aligned_copy, check_devices, check_f32, check_grad, check_number, is_number, is_real, swap_modules


# ---- the tails as plain torch (any device, any float dtype) ---------------------------------------------------------------------
def _interior(h, w, border, like):
    m = torch.zeros((h, w), dtype=like.dtype, device=like.device)
    if h > 2 * border and w > 2 * border:
        m[border:h - border, border:w - border] = 1
    return m


def _conv1x1(feat, weight):
    return torch.einsum("bchw,oc->bohw", feat, weight.reshape(weight.shape[0], -1))


def score_tail_formula(feat, weight, border=3, use_softmax=True, temperature=100.0, eps=1e-16):
    """mickey_extractor.py:134-140 with :98-124 restated: feat [B, C, H, W], weight [1, C, 1, 1] -> scores [B, 1, H, W]."""
    z = _conv1x1(feat, weight)
    B, _, H, W = z.shape
    mask = _interior(H, W, border, z)
    if not use_softmax:
        return mask * torch.sigmoid(z)
    z = z - (z.reshape(B, -1).mean(-1).view(B, 1, 1, 1) + eps).detach()
    e = mask * torch.exp(z / temperature)
    return e / (e.sum(-1).sum(-1).view(B, 1, 1, 1) + eps)


def offset_tail_formula(feat, weight):
    """mickey_extractor.py:172-176 restated: -> [B, 2, H, W] in (0, 1)."""
    return torch.sigmoid(_conv1x1(feat, weight))


def depth_tail_formula(feat, weight, use_sigmoid=False, max_depth=60.0):
    """mickey_extractor.py:211-216 restated: -> [B, 1, H, W]."""
    z = _conv1x1(feat, weight)
    return max_depth * torch.sigmoid(z) if use_sigmoid else z


def desc_l2norm_formula(x, eps=1e-10):
    """utils/extractor_utils.py:6-10 restated: x [B, C, H, W] (or [N, C]) -> the same shape, unit length over dim 1."""
    return x / x.pow(2).sum(dim=1, keepdim=True).add(eps).pow(0.5)


# ---- argument checks and layouts ---------------------------------------------------------------------------------------------
def _check_feat(fn, name, t):
    check_f32(fn, name, t, rank=4, why=" ([B, C, H, W])")
    C = t.shape[1]
    if C < ops.TAIL_MIN_C or C > ops.TAIL_MAX_C or C % 4:
        raise ValueError("%s: the width of %s must be a multiple of 4 in [%d, %d], got %d" % (fn, name, ops.TAIL_MIN_C, ops.TAIL_MAX_C, C))


def _channels_last(x):
    """[B, C, H, W] -> the same values as a tensor whose [B H W, C] rows are dense and 16-byte aligned: x itself when it already is
    (channels_last memory, read in place), else one copy.  Differentiable."""
    rows = x.permute(0, 2, 3, 1)
    copy = aligned_copy(rows)
    return x if copy is rows else copy.permute(0, 3, 1, 2)


def _rows(x4):
    B, C, H, W = x4.shape
    return x4.permute(0, 2, 3, 1).reshape(B * H * W, C)   # a view: the rows are dense


def _weight2d(w):
    return aligned_copy(w.reshape(w.shape[0], w.shape[1]))


class HeadTailFn(torch.autograd.Function):
    """out [B, Cout, H, W] = act(conv1x1(feat, weight)); feat: channels_last-dense [B, C, H, W].  Saves feat, the weight and the small
    output (not even that for the identity); under torch.no_grad() nothing."""

    @staticmethod
    def forward(ctx, feat, weight, act, scale, border, temperature, eps):
        B, C, H, W = feat.shape
        cout = weight.shape[0]
        with torch.cuda.device(feat.device):
            y = ops.train_headtail_fwd(_rows(feat.detach()), _weight2d(weight.detach()), B, H, W, act, scale, border, temperature, eps)
        if any(ctx.needs_input_grad):
            ctx.cfg = (act, scale, temperature)
            if act == ops.TAIL_IDENTITY:
                ctx.save_for_backward(feat, weight)
            else:
                ctx.save_for_backward(feat, weight, y)
        return y.view(B, cout, H, W)

    @staticmethod
    @once_differentiable
    def backward(ctx, go):
        act, scale, temperature = ctx.cfg
        feat, weight = ctx.saved_tensors[:2]
        y = ctx.saved_tensors[2] if act != ops.TAIL_IDENTITY else None
        check_grad("head tail", go)
        B, C, H, W = feat.shape
        nf, nw = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        with torch.cuda.device(go.device):
            gfeat, gw = ops.train_headtail_bwd(go.contiguous(), y, _rows(feat), _weight2d(weight), B, H * W, act, scale, temperature,
                                               want_gfeat=nf, want_gw=nw)
        return (gfeat.view(B, H, W, C).permute(0, 3, 1, 2) if nf else None, gw.view(weight.shape) if nw else None,
                None, None, None, None, None)


class DescL2NormFn(torch.autograd.Function):
    """y [B, C, H, W] contiguous = x / sqrt(sum_c x^2 + eps); x: channels_last-dense.  Saves y and the [B H W] reciprocal norms."""

    @staticmethod
    def forward(ctx, x, eps):
        B, C, H, W = x.shape
        need = ctx.needs_input_grad[0]
        with torch.cuda.device(x.device):
            y, rnorm = ops.train_desc_l2norm_fwd(_rows(x.detach()), B, H * W, eps, want_saved=need)
        if need:
            ctx.save_for_backward(y, rnorm)
        return y.view(B, C, H, W)

    @staticmethod
    @once_differentiable
    def backward(ctx, go):
        y, rnorm = ctx.saved_tensors
        check_grad("desc_l2norm_train", go)
        B, C, n = y.shape
        _, _, H, W = go.shape
        with torch.cuda.device(go.device):
            gx = ops.train_desc_l2norm_bwd(go.contiguous(), y, rnorm, B, n, C)
        return gx.view(B, H, W, C).permute(0, 3, 1, 2), None


def _tail(fn, feat, weight, cout, act, scale=1.0, border=0, temperature=1.0, eps=0.0):
    _check_feat(fn, "feat", feat)
    check_f32(fn, "weight", weight, shape=(cout, feat.shape[1], 1, 1), why=" (a bias-free 1x1 conv)")
    check_devices(fn, [("feat", feat), ("weight", weight)])
    return HeadTailFn.apply(_channels_last(feat), weight, act, float(scale), int(border), float(temperature), float(eps))


def score_tail_train(feat, weight, border=3, use_softmax=True, temperature=100.0, eps=1e-16):
    """Differentiable detector tail (mickey_extractor.py:134-140, 98-124) on the HIP kernels: feat fp32 [B, C, H, W] device tensor
    (channels_last memory is read in place, any other layout is copied once), weight the `score` conv's own [1, C, 1, 1] Parameter.
    use_softmax: mean = sum z / n + eps over all pixels (detached), e = in exp((z - mean) / temperature), y = e / (sum e + eps), per
    image, `in` = 1 on pixels at least `border` from every edge; else in sigmoid(z).  Returns [B, 1, H, W].  Differentiable in feat
    and weight; only the gradients that are needed are computed.  Bad dtypes / ranks / widths / weight shapes, a negative border, a
    temperature that is not finite and positive or an eps that is not finite and non-negative raise ValueError, CPU tensors
    MickeyHipError, all before any launch."""
    fn = "score_tail_train"
    if isinstance(border, bool) or not isinstance(border, numbers.Integral) or border < 0:
        raise ValueError("%s: border must be a non-negative integer, got %r" % (fn, border))
    check_number(fn, "temperature", temperature, positive=True)
    check_number(fn, "eps", eps)
    act = ops.TAIL_SOFTMAX if use_softmax else ops.TAIL_MASKED_SIGMOID
    return _tail(fn, feat, weight, 1, act, 1.0, int(border), temperature, eps)


def offset_tail_train(feat, weight):
    """Differentiable sigmoid(xy_offset(feat)) (mickey_extractor.py:172-176): weight [2, C, 1, 1] -> [B, 2, H, W]."""
    return _tail("offset_tail_train", feat, weight, 2, ops.TAIL_SIGMOID)


def depth_tail_train(feat, weight, use_sigmoid=False, max_depth=60.0):
    """Differentiable depth tail (mickey_extractor.py:211-216): weight [1, C, 1, 1] -> depth(feat), or max_depth sigmoid(depth(feat))
    with use_sigmoid; [B, 1, H, W]."""
    fn = "depth_tail_train"
    if use_sigmoid:
        check_number(fn, "max_depth", max_depth, positive=True)
        return _tail(fn, feat, weight, 1, ops.TAIL_SIGMOID, max_depth)
    return _tail(fn, feat, weight, 1, ops.TAIL_IDENTITY)


def desc_l2norm_train(x, eps=1e-10):
    """Differentiable desc_l2norm (utils/extractor_utils.py:6-10) of a feature map: x fp32 [B, C, H, W] device tensor -> [B, C, H, W]
    CONTIGUOUS, so that .view(B, C, H W) is the [B, C, n] tensor the matcher reads."""
    fn = "desc_l2norm_train"
    _check_feat(fn, "x", x)
    check_number(fn, "eps", eps)
    check_devices(fn, [("x", x)])
    return DescL2NormFn.apply(_channels_last(x), float(eps))


# ---- the head wrappers and the swap ------------------------------------------------------------------------------------------
_BLOCKS = ("resblock1", "resblock2", "resblock3", "resblock4")
_ATTRS = ("use_softmax", "tmp_softmax", "use_depth_sigmoid", "max_depth", "norm_desc")
_BORDER = 3   # mickey_extractor.py:138,140


class HipHead(nn.Module):
    """A head of the reference's extractor (DeepResBlock_det / _offset / _depth / _desc) made of the very same children, Parameters
    and buffers under the same names; forward(feature_volume) runs the children in the reference's order and then the fused tail."""

    @classmethod
    def adopt(cls, head, kind):
        new = adopt(cls, head)
        for name in _ATTRS:
            if name in head.__dict__:
                setattr(new, name, head.__dict__[name])
        new.kind = kind
        new.block4_takes_relu = _takes_relu(head.resblock4)
        # the detector's eps Parameter, read once here: no .item() per step
        new.score_eps = float(head.eps.detach().cpu()) if kind == "score" and isinstance(getattr(head, "eps", None), torch.Tensor) else 1e-16
        return new

    def forward(self, feature_volume):
        x = self.resblock1(feature_volume)
        x = self.resblock2(x)
        x = self.resblock3(x)
        x = self.att_layer(x)
        if self.kind == "desc":
            x = self.resblock4(x, relu=False) if self.block4_takes_relu else self.resblock4(x)
            return desc_l2norm_train(x)
        x = self.resblock4(x)
        if self.kind == "score":
            return score_tail_train(x, self.score.weight, _BORDER, self.use_softmax, self.tmp_softmax, self.score_eps)
        if self.kind == "offset":
            return offset_tail_train(x, self.xy_offset.weight)
        return depth_tail_train(x, self.depth.weight, self.use_depth_sigmoid, self.max_depth)


def _takes_relu(block):
    try:
        return "relu" in inspect.signature(block.forward).parameters
    except (TypeError, ValueError):
        return False


def _is_tail_conv(m, cout):
    return (type(m) is nn.Conv2d and m.bias is None and m.out_channels == cout and m.kernel_size == (1, 1) and m.stride == (1, 1)
            and m.padding == (0, 0) and m.dilation == (1, 1) and m.groups == 1 and m.weight.dtype == torch.float32
            and ops.TAIL_MIN_C <= m.in_channels <= ops.TAIL_MAX_C and m.in_channels % 4 == 0)


def _head_kind(m):
    """'score' / 'offset' / 'depth' / 'desc' for a module with the structure of one of the reference's heads, by attributes and not by
    class; None for anything else."""
    if not isinstance(m, nn.Module) or isinstance(m, HipHead):
        return None
    mods = m._modules
    if any(not isinstance(mods.get(n), nn.Module) for n in _BLOCKS + ("att_layer",)):
        return None
    kinds = []
    d = m.__dict__
    if "score" in mods and _is_tail_conv(mods["score"], 1) and isinstance(d.get("use_softmax"), bool) and is_number(d.get("tmp_softmax"), True):
        kinds.append("score")
    if "xy_offset" in mods and _is_tail_conv(mods["xy_offset"], 2):
        kinds.append("offset")
    if ("depth" in mods and _is_tail_conv(mods["depth"], 1) and isinstance(d.get("use_depth_sigmoid"), bool)
            and is_real(d.get("max_depth")) and (d["max_depth"] > 0 or not d["use_depth_sigmoid"])):   # (unused without the sigmoid: any sign)
        kinds.append("depth")
    if isinstance(d.get("norm_desc"), bool):
        kinds.append("desc")
    if len(kinds) != 1 or sum(n in mods for n in ("score", "xy_offset", "depth")) != (0 if kinds == ["desc"] else 1):
        return None
    if kinds == ["desc"] and not d["norm_desc"]:
        return None   # (no tail to fuse)
    return kinds[0]


def use_hip_tails(model):
    """Replace, in place, every submodule of `model` that has the structure of one of the reference's four heads -- children resblock1
    ... resblock4 and att_layer, and exactly one of: a bias-free 1x1 nn.Conv2d `score` with 1 output (plus a boolean use_softmax and a
    numeric tmp_softmax), `xy_offset` with 2 outputs, `depth` with 1 output (plus use_depth_sigmoid, max_depth), or norm_desc == True
    -- by a HipHead that holds the very same children, Parameters (the detector's non-trainable eps, offset_par1, offset_par2 and
    ones_kernel included) and buffers under the same names: state-dict keys, Parameter objects, optimiser state and checkpoints do
    not change; only forward differs.  The detector's eps is read once, here.  Convs with a bias, other widths and norm_desc == False
    are left alone.  Composes with the other use_hip_* calls in any order.  Returns the number of heads swapped; a second call finds
    none."""
    def make(m):
        kind = _head_kind(m)
        if kind is not None:
            return HipHead.adopt(m, kind)

    return swap_modules(model, make)
