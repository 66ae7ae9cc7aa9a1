"""Trainable EncoderLayer of the four heads' transformer on the HIP kernels: one autograd node for the whole layer.

Every head runs three EncoderLayers (att_layers/transformer_utils.py:40-66) on each image set of a pair.  With use_hip_attention
only the attention core of a layer is HIP; the q / k / v / merge / MLP nn.Linears, the two LayerNorms, the concat, the ReLU and
the residual stay about 12 torch launches forward and twice that backward, with about 17 [rows, 128] tensors kept for backward.
Here the whole layer

    q = x Wq^T,  k, v = source Wk^T, source Wv^T           att = forward_linear(q, k, v)   (8 heads of 16)
    m = LN1(att Wm^T)          h = relu([x | m] W1^T)      out = x + LN2(h W2^T)

is one torch.autograd.Function on mk_train_linear_* / mk_train_ln128_* (mk_train_layer.hip) around mk_linattn_train_fwd / _bwd:
fp32 throughout, every contraction an exact fp32 fma chain on the fp32-input MFMA in an order fixed by the shape, every sum over
rows chunked and added in chunk order.  Results are bit-identical from run to run, image i of a batch gets the forward bits it
gets alone, gradients are bit-linear in the incoming gradient under a power-of-two scale, and nothing synchronises with the host.
For self attention the node keeps x, the packed [rows, 384] q | k | v, att, x-hat of both LayerNorms, m and h: 10 units of
rows x 128 x 4 bytes, plus two [rows] rstd vectors and the attention's [N 8, 272] block.

    encoder_layer_train(x, source, wq, wk, wv, wm, w1, w2, ln1_w, ln1_b, ln2_w, ln2_b, ...)   the differentiable op
    linear_train(x, weight)                     y = x W^T on the same kernels (forward, input gradient, weight gradient)
    layernorm_train(x, weight, bias, eps)       LayerNorm(128) on the same kernels
    HipEncoderLayer                             nn.Module with the reference EncoderLayer's children and call contract
    use_hip_encoder_layers(model)               swaps it into a reference-style model in place, returns the count
    encoder_layer_formula(...)                  the same layer in plain torch, any device / dtype (tests, documentation)

Not covered: d_model other than 128 or nhead other than 8 (ValueError), biases, autocast and half precision (ValueError), double
backward, hipGraph capture of a step, BatchNorm / ReLU / the 1x1 shortcut of BasicBlock (train_block.py), the head tails (train_tails.py), the positional
encoding and the NCHW <-> token rearrangement around the stack.
"""
import torch
import torch.nn.functional as F
from torch import nn
from torch.autograd.function import once_differentiable

from . import ops
from ._train_common import adopt, aligned_copy, check_devices, check_f32, check_grad, check_number, rows_in_place, swap_modules
from .train_attention import LinearAttention, _is_linear_attention, linear_attention_formula

D_MODEL = 128
NHEAD = 8
_W_SHAPES = (("wq", (128, 128)), ("wk", (128, 128)), ("wv", (128, 128)), ("wm", (128, 128)), ("w1", (256, 256)), ("w2", (128, 256)),
             ("ln1_w", (128,)), ("ln1_b", (128,)), ("ln2_w", (128,)), ("ln2_b", (128,)))
# the flat gradient buffer of one backward pass: wq | wk | wv | wm | w1 | w2, then gamma2 | beta2 | gamma1 | beta1
_OFF = {"wq": 0, "wk": 16384, "wv": 32768, "wm": 49152, "w1": 65536, "w2": 131072}
_NW = 163840
_NL = 512


# ---- the layer as plain torch (any device, any float dtype) ----------------------------------------------------------------------
def encoder_layer_formula(x, source, wq, wk, wv, wm, w1, w2, ln1_w, ln1_b, ln2_w, ln2_b, attn_eps=1e-6, ln1_eps=1e-5, ln2_eps=1e-5,
                          nhead=NHEAD):
    """EncoderLayer.forward (transformer_utils.py:51-66) restated: x [N, L, C], source [N, S, C] -> [N, L, C]."""
    N, L, C = x.shape
    q = F.linear(x, wq).view(N, L, nhead, C // nhead)
    k = F.linear(source, wk).view(N, -1, nhead, C // nhead)
    v = F.linear(source, wv).view(N, -1, nhead, C // nhead)
    att = linear_attention_formula(q, k, v, attn_eps).reshape(N, L, C)
    m = F.layer_norm(F.linear(att, wm), (C,), ln1_w, ln1_b, ln1_eps)
    h = torch.relu(F.linear(torch.cat([x, m], dim=2), w1))
    return x + F.layer_norm(F.linear(h, w2), (C,), ln2_w, ln2_b, ln2_eps)


# ---- argument checks and layouts ---------------------------------------------------------------------------------------------
_ONLY = " (d_model == 128 and nhead == 8 only)"


def _validate(x, source, weights, attn_eps, ln1_eps, ln2_eps):
    """Every check of encoder_layer_train, on the host, before anything is launched."""
    fn = "encoder_layer_train"
    check_f32(fn, "x", x, rank=3, width=D_MODEL, why=_ONLY)
    check_f32(fn, "source", source, rank=3, width=D_MODEL, why=_ONLY)
    if source.shape[0] != x.shape[0]:
        raise ValueError("%s: x %s and source %s must share N" % (fn, tuple(x.shape), tuple(source.shape)))
    for (name, shape), w in zip(_W_SHAPES, weights):
        check_f32(fn, name, w, shape=shape, why=_ONLY)
    for name, eps in (("attn_eps", attn_eps), ("ln1_eps", ln1_eps), ("ln2_eps", ln2_eps)):
        check_number(fn, name, eps)
    check_devices(fn, [("x", x), ("source", source)] + [(n, w) for (n, _), w in zip(_W_SHAPES, weights)])


def _rows2d(t):
    """[..., C] fp32 tensor -> a 2-D [rows, C] tensor the kernels read: a view when t is contiguous, or 3-D with evenly spaced rows
    (stride(0) == T * stride(1), since two dimensions become one) that _train_common.rows_in_place accepts; else a view of a
    contiguous, aligned copy."""
    C = t.shape[-1]
    rows = t.numel() // C
    if (not t.is_contiguous() and t.dim() == 3 and (t.shape[0] == 1 or t.stride(0) == t.shape[1] * t.stride(1))
            and rows_in_place(t, C, t.stride(1))):
        return t.as_strided((rows, C), (t.stride(1), 1))
    return aligned_copy(t).view(rows, C)


def _heads(t2d, N, T, col):
    """columns [col, col + 128) of a 2-D row buffer as the [N, T, 8, 16] operand of the attention kernels (read in place)"""
    ld = t2d.stride(0) if t2d.shape[0] > 1 else t2d.shape[1]
    return t2d.as_strided((N, T, NHEAD, D_MODEL // NHEAD), (T * ld, ld, D_MODEL // NHEAD, 1), t2d.storage_offset() + col)


class _Partials:
    """Work memory of one backward pass: chunk partials of the weight gradients, step partials of the LayerNorm gradients, and the
    flat buffer the tail launch adds them into."""

    def __init__(self, rows, device, nw=_NW, nl=_NL, ln_rows=None):
        self.rpc, self.chunks = ops.train_chunks(rows)              # sized by the longest operand; a shorter one leaves zeros
        self.steps = ops.train_ln_steps(rows if ln_rows is None else ln_rows)
        self.nw, self.nl = nw, nl
        self.wpart = torch.empty(self.chunks * nw, device=device, dtype=torch.float32) if nw else None
        self.lpart = torch.empty(self.steps * nl, device=device, dtype=torch.float32) if nl else None
        self.flat = torch.empty(nw + nl, device=device, dtype=torch.float32)

    def wgrad(self, off, g, a1, a2=None):
        ops.train_linear_wgrad(g, a1, self.wpart[off:], self.nw, self.rpc, self.chunks, a2=a2)

    def finish(self, want_w, want_l):
        if want_w or want_l:
            ops.train_tail(self.wpart, self.nw, self.chunks, self.nw if want_w else 0, self.lpart, self.nl, self.steps,
                           self.nl if want_l else 0, self.flat if want_w else self.flat[self.nw:])

    def weight(self, off, shape):
        return self.flat[off:off + shape[0] * shape[1]].view(shape)

    def ln(self, off):
        return self.flat[self.nw + off:self.nw + off + D_MODEL]


class EncoderLayerTrainFn(torch.autograd.Function):
    """out = the whole layer.  x2 / s2: the 2-D row views of x and source (s2 is None for self attention).  Saves x, the packed
    projections, att, x-hat and rstd of both LayerNorms, m, h and the attention's M | ks block; under torch.no_grad() nothing."""

    @staticmethod
    def forward(ctx, x2, s2, N, L, S, eps, wq, wk, wv, wm, w1, w2, g1, b1, g2, b2):
        need = any(ctx.needs_input_grad)
        self_att = s2 is None
        with torch.cuda.device(x2.device):
            xd = x2.detach()
            if self_att:
                proj = ops.train_linear_fwd(xd, (wq.detach(), wk.detach(), wv.detach()))                     # [rows, 384]
                q, k, v = _heads(proj, N, L, 0), _heads(proj, N, L, 128), _heads(proj, N, L, 256)
                kvp = None
            else:
                sd = s2.detach()
                proj = ops.train_linear_fwd(xd, wq.detach())                                                 # [rows, 128]
                kvp = torch.empty((sd.shape[0], 256), device=xd.device, dtype=torch.float32)
                ops.train_linear_fwd(sd, wk.detach(), out=kvp[:, :128])
                ops.train_linear_fwd(sd, wv.detach(), out=kvp[:, 128:])
                q, k, v = _heads(proj, N, L, 0), _heads(kvp, N, S, 0), _heads(kvp, N, S, 128)
            att, kvblk = ops.linattn_train_fwd(q, k, v, eps[0])
            att = att.view(N * L, D_MODEL)
            m, xh1, rs1 = ops.train_linear_ln128_fwd(att, wm.detach(), g1.detach(), b1.detach(), eps[1], want_saved=need)
            h = ops.train_linear_fwd(xd, w1.detach(), a2=m, relu=True)
            out, xh2, rs2 = ops.train_linear_ln128_fwd(h, w2.detach(), g2.detach(), b2.detach(), eps[2], resid=xd, want_saved=need)
        if need:
            ctx.dims = (N, L, S, eps[0], self_att)
            saved = [x2, proj, att, kvblk, xh1, rs1, m, h, xh2, rs2, wq, wk, wv, wm, w1, w2, g1, g2]
            if not self_att:
                saved += [s2, kvp]
            ctx.save_for_backward(*saved)
        return out.view(N, L, D_MODEL)

    @staticmethod
    @once_differentiable
    def backward(ctx, go):
        N, L, S, attn_eps, self_att = ctx.dims
        x2, proj, att, kvblk, xh1, rs1, m, h, xh2, rs2, wq, wk, wv, wm, w1, w2, g1, g2 = ctx.saved_tensors[:18]
        s2, kvp = (None, None) if self_att else ctx.saved_tensors[18:]
        check_grad("encoder_layer_train", go)
        nx, ns = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        nwq, nwk, nwv, nwm, nw1, nw2, ng1, nb1, ng2, nb2 = ctx.needs_input_grad[6:]
        want_w = nwq or nwk or nwv or nwm or nw1 or nw2
        want_l = ng1 or nb1 or ng2 or nb2
        need_att = nx or ns or nwq or nwk or nwv          # anything behind the attention core
        need_m = need_att or nwm or ng1 or nb1            # anything behind mlp[0]'s input gradient
        M, Ms = N * L, N * S
        dev = go.device
        new = lambda *s: torch.empty(s, device=dev, dtype=torch.float32)   # noqa: E731
        with torch.cuda.device(dev):
            go2 = _rows2d(go)
            if not go2.is_contiguous():
                go2 = go2.contiguous()
            P = _Partials(max(M, Ms), dev, _NW if want_w else 0, _NL if want_l else 0, ln_rows=M)
            lp = P.lpart
            gx = gs = None
            # norm2 (its residual passes go straight to x), mlp[2], the ReLU, mlp[0]
            gu2 = new(M, D_MODEL)
            ops.train_ln128_bwd(go2, xh2, rs2, g2, gu=gu2, part=lp if (ng2 or nb2) else None, part_stride=_NL)
            if nw2:
                P.wgrad(_OFF["w2"], gu2, h)
            gh = None
            if nx or need_m or nw1:
                gh = new(M, 2 * D_MODEL)
                ops.train_linear_dgrad(gu2, w2, gh, mask=h)
                if nw1:
                    P.wgrad(_OFF["w1"], gh, x2, a2=m)
            del gu2   # (work tensors go back to the allocator as soon as their last reader is queued: the peak of a step)
            if nx or need_m:
                gx = go2.clone() if nx else new(M, D_MODEL)
                gm = new(M, D_MODEL)
                ops.train_linear_dgrad(gh, w1, gx, o2=gm, accumulate=1 if nx else 0)
            gh = None
            if need_m:
                # norm1, merge
                gu1 = new(M, D_MODEL) if (need_att or nwm) else None
                ops.train_ln128_bwd(gm, xh1, rs1, g1, gu=gu1, part=lp[2 * D_MODEL:] if (ng1 or nb1) else None, part_stride=_NL)
                if nwm:
                    P.wgrad(_OFF["wm"], gu1, att)
                gm = None
            if need_att:
                gatt = new(M, D_MODEL)
                ops.train_linear_dgrad(gu1, wm, gatt)
                gu1 = None
                # the attention core: q, k, v read in place from the projection buffers, gq | gk | gv written as planes of one buffer
                if self_att:
                    q, k, v = _heads(proj, N, L, 0), _heads(proj, N, L, 128), _heads(proj, N, L, 256)
                    gqkv = new(3, M, D_MODEL)
                    planes = (gqkv[0], gqkv[1], gqkv[2])
                    want = (nx or nwq, nx or nwk, nx or nwv)
                else:
                    q, k, v = _heads(proj, N, L, 0), _heads(kvp, N, S, 0), _heads(kvp, N, S, 128)
                    planes = (new(M, D_MODEL), new(Ms, D_MODEL), new(Ms, D_MODEL))
                    want = (nx or nwq, ns or nwk, ns or nwv)
                ops.linattn_train_bwd(q, k, v, kvblk, gatt.view(N, L, NHEAD, D_MODEL // NHEAD), attn_eps, want, out=planes)
                gq, gk, gv = planes
                gatt = None
                # the three projections
                if self_att:
                    if nx:
                        ops.train_linear_dgrad(gqkv, (wq, wk, wv), gx, accumulate=1)
                    if nwq and nwk and nwv:
                        P.wgrad(_OFF["wq"], gqkv, x2)
                    else:
                        for flag, name, g in ((nwq, "wq", gq), (nwk, "wk", gk), (nwv, "wv", gv)):
                            if flag:
                                P.wgrad(_OFF[name], g, x2)
                else:
                    if nx:
                        ops.train_linear_dgrad(gq, wq, gx, accumulate=1)
                    if ns:
                        gs = new(Ms, D_MODEL)
                        ops.train_linear_dgrad(gk, wk, gs)
                        ops.train_linear_dgrad(gv, wv, gs, accumulate=1)
                    for flag, name, g, a in ((nwq, "wq", gq, x2), (nwk, "wk", gk, s2), (nwv, "wv", gv, s2)):
                        if flag:
                            P.wgrad(_OFF[name], g, a)
            P.finish(want_w, want_l)
        W = lambda flag, name, shape: P.weight(_OFF[name], shape) if flag else None   # noqa: E731
        return (gx if nx else None, gs if ns else None, None, None, None, None,
                W(nwq, "wq", (128, 128)), W(nwk, "wk", (128, 128)), W(nwv, "wv", (128, 128)), W(nwm, "wm", (128, 128)),
                W(nw1, "w1", (256, 256)), W(nw2, "w2", (128, 256)),
                P.ln(256) if ng1 else None, P.ln(384) if nb1 else None, P.ln(0) if ng2 else None, P.ln(128) if nb2 else None)


def encoder_layer_train(x, source, wq, wk, wv, wm, w1, w2, ln1_w, ln1_b, ln2_w, ln2_b, attn_eps=1e-6, ln1_eps=1e-5, ln2_eps=1e-5):
    """Differentiable EncoderLayer.forward (att_layers/transformer_utils.py:51-66) on the HIP kernels.

    x: fp32 [N, L, 128] device tensor, source: fp32 [N, S, 128] (pass x itself for self attention: one packed projection, the case
    this is built for); wq, wk, wv, wm [128, 128], w1 [256, 256], w2 [128, 256] in nn.Linear's layout, the LayerNorm affine
    parameters [128].  Returns fp32 [N, L, 128], differentiable in x, source and every parameter; only the gradients that are
    needed are computed, under torch.no_grad() nothing is kept.  Inputs whose rows are dense and 16-byte aligned are read in
    place, other layouts are copied first.  Wrong dtypes / ranks / widths, mismatched N, empty tensors and a bad eps raise
    ValueError, CPU tensors MickeyHipError, all before any launch."""
    weights = (wq, wk, wv, wm, w1, w2, ln1_w, ln1_b, ln2_w, ln2_b)
    _validate(x, source, weights, attn_eps, ln1_eps, ln2_eps)
    N, L, _ = x.shape
    S = source.shape[1]
    x2 = _rows2d(x)
    s2 = None if source is x else _rows2d(source)
    weights = tuple(aligned_copy(w) for w in weights)
    out = EncoderLayerTrainFn.apply(x2, s2, N, L, S, (float(attn_eps), float(ln1_eps), float(ln2_eps)), *weights)
    return out


# ---- the single ops ----------------------------------------------------------------------------------------------------------
class LinearTrainFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x2, w):
        with torch.cuda.device(x2.device):
            out = ops.train_linear_fwd(x2.detach(), w.detach())
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(x2, w)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, go):
        x2, w = ctx.saved_tensors
        check_grad("linear_train", go)
        M, K = x2.shape
        N = w.shape[0]
        gx = gw = None
        with torch.cuda.device(go.device):
            g = _rows2d(go)
            if ctx.needs_input_grad[0]:
                gx = torch.empty((M, K), device=go.device, dtype=torch.float32)
                ops.train_linear_dgrad(g, w, gx)
            if ctx.needs_input_grad[1]:
                P = _Partials(M, go.device, N * K, 0)
                P.wgrad(0, g, x2)
                P.finish(True, False)
                gw = P.flat.view(N, K)
        return gx, gw


def linear_train(x, weight):
    """y = x W^T (nn.Linear without bias) on mk_train_linear_fwd / _dgrad / _wgrad: x fp32 [..., K] device tensor, weight [N, K],
    K and N multiples of 16.  Differentiable in both."""
    fn = "linear_train"
    check_f32(fn, "x", x)
    check_f32(fn, "weight", weight, rank=2)
    if x.dim() < 1 or x.shape[-1] != weight.shape[1] or weight.shape[0] % 16 or weight.shape[1] % 16:
        raise ValueError("%s: x %s and weight %s must share K; K and N must be multiples of 16" % (fn, tuple(x.shape), tuple(weight.shape)))
    check_devices(fn, [("x", x), ("weight", weight)])
    x2 = _rows2d(x if x.dim() != 1 else x[None])
    return LinearTrainFn.apply(x2, aligned_copy(weight)).view(*x.shape[:-1], weight.shape[0])


class LayerNormTrainFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x2, w, b, eps):
        need = any(ctx.needs_input_grad)
        with torch.cuda.device(x2.device):
            out, xh, rs = ops.train_ln128_fwd(x2.detach(), w.detach(), b.detach(), eps, want_saved=need)
        if need:
            ctx.save_for_backward(xh, rs, w)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, go):
        xh, rs, w = ctx.saved_tensors
        check_grad("layernorm_train", go)
        M = xh.shape[0]
        nx, nw, nb = ctx.needs_input_grad[:3]
        with torch.cuda.device(go.device):
            g = _rows2d(go)
            if not g.is_contiguous():
                g = g.contiguous()
            gu = torch.empty_like(xh) if nx else None
            P = _Partials(M, go.device, 0, 2 * D_MODEL if (nw or nb) else 0)
            ops.train_ln128_bwd(g, xh, rs, w, gu=gu, part=P.lpart, part_stride=2 * D_MODEL)
            P.finish(False, nw or nb)
        return gu, (P.flat[:D_MODEL] if nw else None), (P.flat[D_MODEL:] if nb else None), None


def layernorm_train(x, weight, bias, eps=1e-5):
    """nn.LayerNorm(128) with affine parameters on mk_train_ln128_fwd / _bwd: x fp32 [..., 128] device tensor."""
    fn = "layernorm_train"
    check_f32(fn, "x", x, width=D_MODEL)
    check_f32(fn, "weight", weight, shape=(D_MODEL,))
    check_f32(fn, "bias", bias, shape=(D_MODEL,))
    check_number(fn, "eps", eps)
    check_devices(fn, [("x", x), ("weight", weight), ("bias", bias)])
    x2 = _rows2d(x if x.dim() != 1 else x[None])
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    return LayerNormTrainFn.apply(x2, weight.contiguous(), bias.contiguous(), float(eps)).view(x.shape)


# ---- the module and the swap -------------------------------------------------------------------------------------------------
_CHILDREN = ("q_proj", "k_proj", "v_proj", "attention", "merge", "mlp", "norm1", "norm2")


class HipEncoderLayer(nn.Module):
    """The reference's EncoderLayer(d_model=128, nhead=8, attention='linear') (att_layers/transformer_utils.py:14-66) with the same
    children under the same names (q_proj, k_proj, v_proj, attention, merge, mlp, norm1, norm2) and forward(x, source) as ONE
    autograd node on the HIP kernels."""

    def __init__(self, d_model=D_MODEL, nhead=NHEAD, attention="linear"):
        super().__init__()
        if d_model != D_MODEL or nhead != NHEAD or attention != "linear":
            raise ValueError("HipEncoderLayer: d_model == 128, nhead == 8 and attention == 'linear' only, got %r, %r, %r"
                             % (d_model, nhead, attention))
        self.dim = d_model // nhead
        self.nhead = nhead
        self.q_proj = nn.Linear(d_model, d_model, bias=False)
        self.k_proj = nn.Linear(d_model, d_model, bias=False)
        self.v_proj = nn.Linear(d_model, d_model, bias=False)
        self.attention = LinearAttention()
        self.merge = nn.Linear(d_model, d_model, bias=False)
        self.mlp = nn.Sequential(nn.Linear(d_model * 2, d_model * 2, bias=False), nn.ReLU(True), nn.Linear(d_model * 2, d_model, bias=False))
        self.norm1 = nn.LayerNorm(d_model)
        self.norm2 = nn.LayerNorm(d_model)

    @classmethod
    def adopt(cls, layer):
        """A HipEncoderLayer made of the very child modules of `layer` (same names, same order, same Parameter objects)."""
        new = adopt(cls, layer)   # (layer holds no Parameters or buffers of its own: _is_encoder_layer)
        new.dim, new.nhead = D_MODEL // NHEAD, NHEAD
        return new

    def forward(self, x, source):
        return encoder_layer_train(x, source, self.q_proj.weight, self.k_proj.weight, self.v_proj.weight, self.merge.weight,
                                   self.mlp[0].weight, self.mlp[2].weight, self.norm1.weight, self.norm1.bias, self.norm2.weight,
                                   self.norm2.bias, self.attention.eps, self.norm1.eps, self.norm2.eps)


def _is_linear(m, fin, fout):
    return (type(m) is nn.Linear and m.bias is None and m.in_features == fin and m.out_features == fout
            and m.weight.dtype == torch.float32)


def _is_norm(m):
    return (type(m) is nn.LayerNorm and tuple(m.normalized_shape) == (D_MODEL,) and m.elementwise_affine and m.weight is not None
            and m.bias is not None and m.weight.dtype == torch.float32 and m.bias.dtype == torch.float32)


def _is_encoder_layer(m):
    """The reference EncoderLayer's structure, by attributes and not by class."""
    if not isinstance(m, nn.Module) or isinstance(m, HipEncoderLayer):
        return False
    if set(m._modules) != set(_CHILDREN) or next(iter(m._parameters.values()), None) is not None or len(m._buffers):
        return False
    if getattr(m, "nhead", None) != NHEAD or isinstance(m.nhead, bool):
        return False
    if not all(_is_linear(getattr(m, n), D_MODEL, D_MODEL) for n in ("q_proj", "k_proj", "v_proj", "merge")):
        return False
    mlp = m.mlp
    if not (isinstance(mlp, nn.Sequential) and len(mlp) == 3 and _is_linear(mlp[0], 2 * D_MODEL, 2 * D_MODEL) and type(mlp[1]) is nn.ReLU
            and _is_linear(mlp[2], 2 * D_MODEL, D_MODEL)):
        return False
    if not (_is_norm(m.norm1) and _is_norm(m.norm2)):
        return False
    return isinstance(m.attention, LinearAttention) or _is_linear_attention(m.attention)


def use_hip_encoder_layers(model):
    """Replace, in place, every submodule of `model` that has the reference EncoderLayer's structure (q_proj, k_proj, v_proj, merge:
    Linear(128, 128) without bias; mlp: Linear(256, 256), ReLU, Linear(256, 128) without biases; norm1, norm2: LayerNorm(128) with
    affine parameters; nhead == 8; a linear attention; fp32 parameters) by a HipEncoderLayer holding the very same child modules
    under the same names: state-dict keys, Parameter objects, optimiser state and checkpoints do not change.  Layers with biases,
    other widths or 'full' attention are left alone.  Composes with the other use_hip_* calls in any order.  Returns the number of
    registrations swapped; a second call finds none."""
    def make(m):
        if _is_encoder_layer(m):
            return HipEncoderLayer.adopt(m)

    return swap_modules(model, make)
