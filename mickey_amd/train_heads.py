"""Trainable 3x3 convolutions of the four heads on the HIP kernels: forward, input gradient and weight gradient.

The heads are the only trainable part of the reference model; their 3x3 convolutions (utils/extractor_utils.py:18-31:
nn.Conv2d(k=3, stride=1, padding=1, bias=False), run in fp32, mickey_extractor.py:53-56) are 99 % of their flops.  Here all
three passes are split-fp16 implicit GEMMs on bordered feature maps (mickey_hip.h):

    forward   y  = conv3x3(x, W)                      mk_conv3x3_split_dscale on x's planes
    dgrad     gX = conv3x3(gY, W'), W'[ci, co, ky, kx] = W[co, ci, 2 - ky, 2 - kx]     the same kernel on gY's planes
    wgrad     dW[co, tap, ci] = sum_r gY_b[r, co] * X_b[r + dy (W + 1) + dx, ci]       mk_conv_wgrad (A^T . B over bordered rows)

Every operand is held as two fp16 planes, v * s = hi + lo, with s a power of two that follows the tensor's abs-max (input,
weight and gradient alike: a REINFORCE gradient has no known magnitude) and stays in device memory -- forward and backward never
synchronise with the host.  Results are bit-identical from run to run (no atomics; the K split of the weight gradient is a
function of the shape and its partials are added in a fixed order).  A gradient (or input) that holds an Inf or a NaN makes
every value computed from it NaN, so the trainer's finite check (model.py:139-143) still fires.

    conv3x3_train(x, weight)     the differentiable op
    Conv3x3(cin, cout)           nn.Module with nn.Conv2d's `weight` Parameter and state-dict key
    use_hip_convs(model)         swaps it into a reference-style model in place (next to use_hip_matcher / use_hip_encoder)

BatchNorm (batch statistics in training), ReLU and the 1x1 shortcut are train_block.py, the 1x1 score / offset / depth convolutions
train_tails.py, the attention layers train_layer.py.  Autocast is not covered: inputs and weights must be float32 (a half-precision input raises ValueError).
"""
import torch
import torch.nn.functional as F
from torch import nn

from . import ops
from ._train_common import check_devices, check_f32, check_grad, check_tensor, swap_modules


# ---- the formulas the kernels implement, as plain torch (any device, any float dtype: tests, documentation) --------------------
def dgrad_weight(weight):
    """W'[ci, co, ky, kx] = W[co, ci, 2 - ky, 2 - kx]: conv3x3(gY, W') is the input gradient of conv3x3(x, W)."""
    return weight.flip(2, 3).transpose(0, 1).contiguous()


def bordered_map(x):
    """[B, C, H, W] -> the bordered feature map [(B (H + 1) + 1)(W + 1) + 1, C] of mickey_hip.h (zero border rows)."""
    B, C, H, W = x.shape
    out = x.new_zeros(((B * (H + 1) + 1) * (W + 1) + 1, C))
    b, y, xx = torch.meshgrid(torch.arange(B), torch.arange(H), torch.arange(W), indexing="ij")
    rows = ((b * (H + 1) + y + 1) * (W + 1) + xx + 1).reshape(-1).to(x.device)
    out[rows] = x.permute(0, 2, 3, 1).reshape(B * H * W, C)
    return out


def wgrad_bordered(x, gy):
    """The weight gradient as the kernel computes it: a plain sum over ALL bordered rows with one row shift per tap,
    dW[co, ci, ky, kx] = sum_r gY_b[r, co] * X_b[r + (ky - 1)(W + 1) + kx - 1, ci] (gY's zero border rows make it exact)."""
    W = x.shape[3]
    xb, gb = bordered_map(x), bordered_map(gy)
    R = xb.shape[0]
    pad = W + 2
    xp = F.pad(xb, (0, 0, pad, pad))   # the rows a shift reaches beyond the map meet zero rows of gY
    taps = []
    for ky in range(3):
        for kx in range(3):
            s = (ky - 1) * (W + 1) + kx - 1
            taps.append(gb.t() @ xp[pad + s: pad + s + R])   # [Cout, Cin]
    return torch.stack(taps, -1).reshape(gy.shape[1], x.shape[1], 3, 3)


def weight_planes(weight, scale, transposed=False):
    """The interleaved (32 hi | 32 lo) fp16 planes mk_conv_train_weight_planes writes, on the host: weights.split_conv_weight of
    the tap-major weight [Cout, 9 Cin] -- or, transposed, of the input gradient's [Cin, 9 Cp] (Cp = Cout rounded up to 32)."""
    from . import weights as wts
    Cout, Cin = weight.shape[:2]
    if transposed:
        Cp = (Cout + 31) // 32 * 32
        w = F.pad(dgrad_weight(weight), (0, 0, 0, 0, 0, Cp - Cout))   # [Cin, Cp, 3, 3]
    else:
        w = weight
    return wts.split_conv_weight(w.permute(0, 2, 3, 1).reshape(w.shape[0], -1), float(scale))


# ---- the op ----------------------------------------------------------------------------------------------------------------
def supported_channels(cin, cout):
    return cin % 32 == 0 and cout % 4 == 0 and cin > 0 and cout > 0


def _validate(x, weight):
    """Every check of conv3x3_train, on the host, before anything is launched."""
    fn = "conv3x3_train"
    check_tensor(fn, "x", x)
    check_tensor(fn, "weight", weight)
    check_devices(fn, [("x", x), ("weight", weight)])   # (this op looks at the devices before the dtypes: a CPU half tensor is a MickeyHipError)
    check_f32(fn, "x", x, rank=4, why=" ([B, Cin, H, W])")
    check_f32(fn, "weight", weight, rank=4, why=" ([Cout, Cin, 3, 3])")
    if tuple(weight.shape[2:]) != (3, 3):
        raise ValueError("%s: weight must be [Cout, Cin, 3, 3], got %s" % (fn, tuple(weight.shape)))
    if x.shape[1] != weight.shape[1]:
        raise ValueError("%s: x has %d channels, weight expects %d" % (fn, x.shape[1], weight.shape[1]))
    if not supported_channels(weight.shape[1], weight.shape[0]):
        raise ValueError("%s: Cin must be a multiple of 32 and Cout of 4, got Cin=%d, Cout=%d" % (fn, weight.shape[1], weight.shape[0]))


def _nchw_view(rows, B, H, W, C):
    """The kernel's dense rows [B * H * W, C] as a [B, C, H, W] tensor in channels_last memory: no copy."""
    return rows.view(B, H, W, C).permute(0, 3, 1, 2)


class Conv3x3TrainFn(torch.autograd.Function):
    """y = conv3x3(x, weight), padding 1, no bias.  Saves x's operand planes (the bytes of the fp32 input), the weight and three
    8-byte scale tensors; under torch.no_grad() nothing.  Inputs validated by conv3x3_train."""

    @staticmethod
    def forward(ctx, x, weight):
        B, Cin, H, W = x.shape
        Cout = weight.shape[0]
        xd, wd = x.detach(), weight.detach().contiguous()
        with torch.cuda.device(x.device):
            sx, sw = ops.absmax_scale(xd), ops.absmax_scale(wd)
            buf, xh, xl = ops.conv_train_plane_buffer(B, H, W, Cin, x.device)
            ops.conv_train_planes(xd, sx, xh, xl)
            wpl, acc = ops.conv_train_weight_planes(wd, sw, sx)
            out = torch.empty((B * H * W, Cout), device=x.device, dtype=torch.float32)
            ops.conv3x3_split_dscale((xh, xl), Cin, wpl, out, Cout, B, H, W, acc)
        ctx.geom = (B, Cin, Cout, H, W)
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            # the planes are needed by the weight gradient only; the weight (not its planes) serves the input gradient
            ctx.save_for_backward(buf if ctx.needs_input_grad[1] else None, sx, weight, sw)
        return _nchw_view(out, B, H, W, Cout)

    @staticmethod
    def backward(ctx, gy):
        B, Cin, Cout, H, W = ctx.geom
        buf, sx, weight, sw = ctx.saved_tensors
        check_grad("conv3x3_train", gy)
        Cp = (Cout + 31) // 32 * 32
        gx = dw = None
        with torch.cuda.device(gy.device):
            gyd = gy.detach()
            sg = ops.absmax_scale(gyd)
            _, gh, gl = ops.conv_train_plane_buffer(B, H, W, Cp, gy.device)
            ops.conv_train_planes(gyd, sg, gh, gl)
            if ctx.needs_input_grad[1]:
                lead = buf.shape[1] - gh.shape[0]
                dw = ops.conv_wgrad((gh, gl), Cp, (buf[0, lead:], buf[1, lead:]), Cout, Cin, B, H, W, sg, sx)
            if ctx.needs_input_grad[0]:
                wt, acc = ops.conv_train_weight_planes(weight.detach().contiguous(), sw, sg, transposed=True)
                rows = torch.empty((B * H * W, Cin), device=gy.device, dtype=torch.float32)
                ops.conv3x3_split_dscale((gh, gl), Cp, wt, rows, Cin, B, H, W, acc)
                gx = _nchw_view(rows, B, H, W, Cin)
        return gx, dw


def conv3x3_train(x, weight):
    """Differentiable nn.Conv2d(k=3, stride=1, padding=1, bias=False) on the HIP kernels.

    x: fp32 [B, Cin, H, W] device tensor, contiguous, channels_last or any strided view; weight: fp32 [Cout, Cin, 3, 3];
    Cin % 32 == 0, Cout % 4 == 0.  Returns fp32 [B, Cout, H, W] in channels_last memory (the kernel's dense rows, no copy);
    the input gradient comes back likewise.  CPU tensors raise MickeyHipError, wrong dtypes / shapes ValueError, both before any
    launch.  Not covered: autocast (half-precision inputs), double backward."""
    _validate(x, weight)
    return Conv3x3TrainFn.apply(x, weight)


class Conv3x3(nn.Module):
    """nn.Conv2d(in_channels, out_channels, kernel_size=3, stride=1, padding=1, bias=False) on the HIP kernels: the same `weight`
    Parameter [Cout, Cin, 3, 3], the same state-dict key, the same default initialisation."""

    kernel_size, stride, padding, dilation, groups, padding_mode = (3, 3), (1, 1), (1, 1), (1, 1), 1, "zeros"

    def __init__(self, in_channels, out_channels, weight=None):
        super().__init__()
        if not supported_channels(in_channels, out_channels):
            raise ValueError("Conv3x3: in_channels must be a multiple of 32 and out_channels of 4, got %d -> %d" % (in_channels, out_channels))
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        if weight is None:
            weight = nn.Parameter(torch.empty(out_channels, in_channels, 3, 3))
            nn.init.kaiming_uniform_(weight, a=5 ** 0.5)   # nn.Conv2d.reset_parameters
        elif not isinstance(weight, nn.Parameter) or tuple(weight.shape) != (out_channels, in_channels, 3, 3):
            raise ValueError("Conv3x3: weight must be a Parameter of shape %s" % ((out_channels, in_channels, 3, 3),))
        self.weight = weight
        self.register_parameter("bias", None)

    def extra_repr(self):
        return "%d, %d, kernel_size=(3, 3), stride=(1, 1), padding=(1, 1), bias=False" % (self.in_channels, self.out_channels)

    def forward(self, x):
        return conv3x3_train(x, self.weight)


def _takes(m):
    return (type(m) is nn.Conv2d and m.kernel_size == (3, 3) and m.stride == (1, 1) and m.padding == (1, 1) and m.dilation == (1, 1)
            and m.groups == 1 and m.bias is None and m.padding_mode == "zeros" and supported_channels(m.in_channels, m.out_channels)
            and m.weight.dtype == torch.float32)


def use_hip_convs(model):
    """Replace, in place, every nn.Conv2d inside `model` with kernel 3, stride 1, padding 1, dilation 1, groups 1, no bias, zeros
    padding, fp32 weights, Cin % 32 == 0 and Cout % 4 == 0 by a Conv3x3 that holds the SAME Parameter object (optimiser state and
    checkpoints stay valid; state-dict keys do not change).  Every other module is left alone.  Returns the number of
    convolutions swapped; a second call finds none."""
    def make(m):
        if _takes(m):
            return Conv3x3(m.in_channels, m.out_channels, weight=m.weight).train(m.training)

    return swap_modules(model, make)
