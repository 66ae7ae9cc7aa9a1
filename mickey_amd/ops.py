"""Tensor-level wrappers over the C ABI (include/mickey_hip.h).  Each function allocates its outputs
with torch (device memory only), passes raw pointers + the current HIP stream to libmickey_hip.so and
returns tensors.  No arithmetic happens here."""

import numpy as np
import torch


from . import _native
from ._native import ACT_GELU, ACT_NONE, ACT_RELU, call, dtype_code, ptr, query, stream  # noqa: F401

LOG2E = 1.4426950408889634


def _chk(t, dtype=None):
    assert t.is_cuda and t.is_contiguous(), "expected a contiguous device tensor"
    if dtype is not None:
        assert t.dtype == dtype, "expected %s, got %s" % (dtype, t.dtype)
    return t


def preprocess_u8(frames, H, W, out=None):
    """uint8 [n, Hs, Ws, 3] device frames -> fp32 [n, 3, H, W] in [0, 1] (resize + /255 + CHW, mk_preprocess_u8)."""
    assert frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[3] == 3 and frames.is_contiguous()
    n, Hs, Ws, _ = frames.shape
    if out is None:
        out = torch.empty((n, 3, H, W), device=frames.device, dtype=torch.float32)
    call("mk_preprocess_u8", ptr(frames), Hs * Ws * 3, n, Hs, Ws, ptr(out), H, W, stream())
    return out


def gemm_set_tile(mode):
    """Dev knob (mickey_hip_dev.h): 0 auto, 1 force 128x128, 2 force 64x128, 7 force the 8-wave ping-pong, 10 force one wave
    per SIMD; 500 / 501: automatic use of the 64x128 tiling off / on."""
    call("mk_gemm_set_tile", int(mode))


def gemm(a, w, bias=None, act=ACT_NONE, out_f32=False, out=None, lda=None, K=None):
    """out = act(a[:, :K] @ w[:, :K].T + bias).  a [M, lda] lp, w [N, ldw] lp."""
    M = a.shape[0]
    lda = a.shape[1] if lda is None else lda
    N, ldw = w.shape
    K = min(lda, ldw) if K is None else K
    if out is None:
        out = torch.empty((M, N), device=a.device, dtype=torch.float32 if out_f32 else a.dtype)
    call("mk_gemm", ptr(a), lda, ptr(w), ldw, ptr(bias), ptr(out), out.stride(0), M, N, K, act,
         int(out.dtype == torch.float32), dtype_code(a.dtype), stream())
    return out


def gemm_grouped(a, w, bias, out, groups, M, N, K, lda, ldw, ldc, stride_a, stride_w, stride_bias, stride_out, act=ACT_NONE):
    call("mk_gemm_grouped", ptr(a), lda, stride_a, ptr(w), ldw, stride_w, ptr(bias), stride_bias, ptr(out), ldc, stride_out,
         groups, M, N, K, act, int(out.dtype == torch.float32), dtype_code(a.dtype), stream())
    return out


def gemm_ls_residual(a, w, bias, gamma, x):
    """x += gamma * (a @ w.T + bias), x fp32 [M, N] in place."""
    M, K = a.shape
    N = w.shape[0]
    call("mk_gemm_ls_residual", ptr(a), a.stride(0), ptr(w), w.stride(0), ptr(bias), ptr(gamma), ptr(x), x.stride(0), M, N, K,
         dtype_code(a.dtype), stream())
    return x


def gemm_qkv(a, w, bias, q, k, vt, nimg, ntok, ntok_pad, heads):
    qscale = (64.0 ** -0.5) * LOG2E
    call("mk_gemm_qkv", ptr(a), a.stride(0), ptr(w), w.stride(0), ptr(bias), ptr(q), ptr(k), ptr(vt), nimg, ntok, ntok_pad,
         heads, qscale, dtype_code(a.dtype), stream())


# ---- LayerNorm folded into the GEMMs around it (mickey_hip.h: mk_gemm_*_ln) -------------------------------------------------
def gemm_ls_residual_ln(a, w, bias, gamma, xh, xl, stats, x_out=None, shift=None):
    """(xh + xl) += gamma * (a @ w.T + bias) on the split residual stream (two 16-bit planes, x = hi + lo); stats[m, N // 64, 2]
    receives the per-slot (sum, sum of squares) of the new fp32 rows.  With x_out (fp32 [M, N]) the new rows are written there
    instead and xh / xl / stats are left alone (last block).  shift (fp32 [M], as published by the consumer before): row
    centring, the rows become x + branch - shift (mickey_hip.h)."""
    M, K = a.shape
    N = w.shape[0]
    call("mk_gemm_ls_residual_ln", ptr(a), a.stride(0), ptr(w), w.stride(0), ptr(bias), ptr(gamma), ptr(xh), ptr(xl),
         xh.stride(0), ptr(stats), ptr(shift), ptr(x_out), x_out.stride(0) if x_out is not None else N, M, N, K,
         dtype_code(a.dtype), stream())


def gemm_patch_embed_ln(a, w, bias, pos, xh, xl, stats, nimg, npatch):
    D = w.shape[0]
    call("mk_gemm_patch_embed_ln", ptr(a), a.stride(0), ptr(w), w.stride(0), ptr(bias), ptr(pos), ptr(xh), ptr(xl), ptr(stats),
         nimg, npatch, D, w.shape[1], dtype_code(a.dtype), stream())


def cls_token_ln(cls, pos, xh, xl, stats, nimg, ntok, D):
    call("mk_cls_token_ln", ptr(cls), ptr(pos), ptr(xh), ptr(xl), ptr(stats), nimg, ntok, D, dtype_code(xh.dtype), stream())


def recentre_split(xh, xl, stats):
    """Every row of the split stream (xh + xl) minus its own mean, in place; stats rewritten (mk_recentre_split)."""
    rows, D = xh.shape
    call("mk_recentre_split", ptr(xh), ptr(xl), ptr(stats), rows, D, dtype_code(xh.dtype), stream())


def gemm_ln(a, w, bias, colsum, stats, eps, act=ACT_NONE, out=None, shift_out=None):
    """out = act(LN(x) @ W.T + b) with a = the hi plane of x, w = W * ln_weight, bias = b + W @ ln_bias (folded on the host).
    shift_out (fp32 [M]): receives every row's mean, for the next producer's row centring."""
    M, K = a.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty((M, N), device=a.device, dtype=a.dtype)
    call("mk_gemm_ln", ptr(a), a.stride(0), ptr(w), w.stride(0), ptr(bias), ptr(colsum), ptr(stats), float(eps), ptr(shift_out),
         ptr(out), out.stride(0), M, N, K, act, dtype_code(a.dtype), stream())
    return out


def gemm_qkv_ln(a, w, bias, colsum, stats, eps, q, k, vt, nimg, ntok, ntok_pad, heads, shift_out=None):
    qscale = (64.0 ** -0.5) * LOG2E
    call("mk_gemm_qkv_ln", ptr(a), a.stride(0), ptr(w), w.stride(0), ptr(bias), ptr(colsum), ptr(stats), float(eps),
         ptr(shift_out), ptr(q), ptr(k), ptr(vt), nimg, ntok, ntok_pad, heads, qscale, dtype_code(a.dtype), stream())


def im2col_patch14(img, gh, gw, ldo, dtype, out=None):
    """img fp32 [nimg, 3, H, W] (any strides with unit innermost) -> [nimg*gh*gw, ldo] lp (out: rows to write into)."""
    assert img.dtype == torch.float32 and img.stride(3) == 1
    nimg = img.shape[0]
    if out is None:
        out = torch.empty((nimg * gh * gw, ldo), device=img.device, dtype=dtype)
    assert out.shape == (nimg * gh * gw, ldo) and out.dtype == dtype and out.is_contiguous()
    call("mk_im2col_patch14", ptr(img), img.stride(0), img.stride(1), img.stride(2), nimg, gh, gw, ptr(out), ldo,
         dtype_code(dtype), stream())
    return out


def gemm_patch_embed(a, w, bias, pos, x, nimg, npatch):
    D = w.shape[0]
    call("mk_gemm_patch_embed", ptr(a), a.stride(0), ptr(w), w.stride(0), ptr(bias), ptr(pos), ptr(x), nimg, npatch, D,
         w.shape[1], dtype_code(a.dtype), stream())


def cls_token(cls, pos, x, nimg, ntok, D):
    call("mk_cls_token", ptr(cls), ptr(pos), ptr(x), nimg, ntok, D, stream())


def layernorm(x, w, b, eps, out=None, out_dtype=torch.bfloat16, resid=None, rows_out=None, rows_per_img=None, skip=0,
              ldo=None, wgroup_rows=0, ldx=None, ldr=None, bordered=None, sat=None):
    """LayerNorm rows of fp32 x [rows, D]; see mk_layernorm for the row remap and the residual form.
    bordered = (nimg, H, W): `out` is a stack of bordered feature maps (rows_out = k * nimg * H * W pixels).
    sat (plane outputs only): the saturation word (sat_word)."""
    D = w.shape[-1]
    rows_in = x.numel() // x.shape[-1]
    if rows_per_img is None:
        rows_per_img = rows_in
    if rows_out is None:
        rows_out = rows_in - skip * (rows_in // rows_per_img)
    if isinstance(out, (tuple, list)):   # (hi, lo) fp16 planes: the operand form of the split-operand head kernels
        oh, ol = out   # ol None: the hi plane alone = the rows rounded to fp16 (mk_layernorm_planes)
        assert oh.dtype == torch.float16 and (ol is None or (ol.dtype == torch.float16 and oh.stride() == ol.stride()))
        ldo = oh.stride(-2) if ldo is None else ldo
        bh, bw, bm = (bordered[1], bordered[2], bordered[0] * bordered[1] * bordered[2]) if bordered else (0, 0, 0)
        call("mk_layernorm_planes", ptr(x), x.stride(-2) if ldx is None else ldx, ptr(w), ptr(b), float(eps), ptr(oh), ptr(ol), ldo,
             SPLIT_ACT_SCALE, ptr(resid), (resid.stride(-2) if resid is not None else D) if ldr is None else ldr, rows_out, D,
             rows_per_img, skip, wgroup_rows, bh, bw, bm, sat_word(sat), stream())
        return out
    if out is None and out_dtype is not None:
        out = torch.empty((rows_out, D), device=x.device, dtype=out_dtype)
    is_f32 = out is not None and out.dtype == torch.float32
    ldo = (out.stride(-2) if out is not None else D) if ldo is None else ldo
    lp = out.dtype if (out is not None and not is_f32) else torch.bfloat16
    bh, bw, bm = (bordered[1], bordered[2], bordered[0] * bordered[1] * bordered[2]) if bordered else (0, 0, 0)
    call("mk_layernorm", ptr(x), x.stride(-2) if ldx is None else ldx, ptr(w), ptr(b), float(eps), ptr(out), ldo, int(is_f32),
         ptr(resid), (resid.stride(-2) if resid is not None else D) if ldr is None else ldr, rows_out, D, rows_per_img, skip,
         wgroup_rows, bh, bw, bm, dtype_code(lp), stream())
    return out


def layernorm_nchw(x, w, b, eps, nimg, npix, rows_per_img, skip=1, round_fp16=False, out=None):
    """mk_layernorm_nchw: LayerNorm of rows skip .. skip + npix of each image's rows_per_img rows of fp32 x [*, D], written
    channel-major: fp32 [nimg, D, npix], bit-identical to layernorm(..., out_dtype=float32) of the same rows.  round_fp16: every
    value rounded to fp16 and widened back (tensor.half().float()).  out: a contiguous fp32 tensor of nimg * D * npix elements."""
    D = w.shape[-1]
    _chk(x, torch.float32)
    assert x.shape[-1] == D and x.numel() // D >= nimg * rows_per_img, "x holds fewer than nimg * rows_per_img rows"
    if out is None:
        out = torch.empty((nimg, D, npix), device=x.device, dtype=torch.float32)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == nimg * D * npix
    call("mk_layernorm_nchw", ptr(x), x.stride(-2), ptr(w), ptr(b), float(eps), ptr(out), nimg, npix, D, rows_per_img, skip,
         int(bool(round_fp16)), stream())
    return out


def gemm_ln128(a, w, ln_w, ln_b, eps, out, groups, M, K, lda=None, ldo=None, resid=None, bordered=None):
    """mk_gemm_ln128: out = LayerNorm(a[g] @ w[g]^T) * ln_w[g] + ln_b[g] (+ resid, updated in place) for 128 output features;
    a lp [groups, M, >= K], w lp [groups, 128, K], out lp (dense rows or, bordered = (nimg, H, W), bordered feature maps)."""
    assert a.dtype == w.dtype == out.dtype and w.shape[-2] == 128 and w.shape[-1] == K
    lda = a.stride(-2) if lda is None else lda
    ldo = out.stride(-2) if ldo is None else ldo
    bh, bw = (bordered[1], bordered[2]) if bordered else (0, 0)
    call("mk_gemm_ln128", ptr(a), lda, a.stride(0) if a.dim() == 3 else 0, ptr(w), w.stride(-2), w.stride(0) if w.dim() == 3 else 0, ptr(ln_w), ptr(ln_b),
         float(eps), ptr(resid), resid.stride(-2) if resid is not None else 128, ptr(out), ldo, groups, M, K, bh, bw, dtype_code(a.dtype),
         stream())
    return out


def attn_set_mode(mode):
    """Dev knob (mickey_hip_dev.h): attention kernel variant, 0 = automatic (tests / benchmarks)."""
    call("mk_attn_set_mode", int(mode))


def flash_attn(q, k, vt, out, nimg, heads, ntok, ntok_pad):
    call("mk_flash_attn_fwd", ptr(q), ptr(k), ptr(vt), ptr(out), out.stride(0), nimg, heads, ntok, ntok_pad,
         dtype_code(q.dtype), stream())
    return out


CONV_OUT_DENSE, CONV_OUT_BORDERED, CONV_OUT_F32 = _native.MK_CONV_OUT_DENSE, _native.MK_CONV_OUT_BORDERED, _native.MK_CONV_OUT_F32


def bordered_rows(nimg, H, W):
    """Rows of a bordered feature map of nimg H x W grids (mickey_hip.h: mk_bordered_rows)."""
    return int(query("mk_bordered_rows", nimg, H, W))


def bordered_empty(lead, nimg, H, W, C, dtype, device):
    """Zeroed stack of bordered feature maps, [*lead, mk_bordered_rows, C]: the border rows stay zero for ever."""
    return torch.zeros(tuple(lead) + (bordered_rows(nimg, H, W), C), dtype=dtype, device=device)


def bordered_index(nimg, H, W, device):
    """Row of pixel (b, y, x) in a bordered feature map, int64 [nimg * H * W] (tests, tools)."""
    b, y, x = torch.meshgrid(torch.arange(nimg, device=device), torch.arange(H, device=device),
                             torch.arange(W, device=device), indexing="ij")
    return (((b * (H + 1) + y + 1) * (W + 1)) + x + 1).reshape(-1)


def conv3x3(in1, C1, w, bias, out, Cout, groups, nimg, H, W, act=ACT_NONE, in2=None, C2=0, resid=None,
            stride_in1=0, stride_in2=0, stride_w=0, stride_bias=0, stride_out=0, stride_resid=0, out_bordered=False):
    """in1 / in2 / resid: bordered feature maps; out: fp32 dense rows, or lp dense / bordered rows (mk_conv3x3)."""
    kind = CONV_OUT_F32 if out.dtype == torch.float32 and in1.dtype != torch.float32 else \
        (CONV_OUT_BORDERED if out_bordered else CONV_OUT_DENSE)
    call("mk_conv3x3", ptr(in1), stride_in1, C1, ptr(in2), stride_in2, C2, ptr(w), w.shape[-1], stride_w, ptr(bias), stride_bias,
         ptr(resid), stride_resid, ptr(out), Cout, stride_out, groups, nimg, H, W, act, kind, dtype_code(in1.dtype), stream())
    return out


SPLIT_ACT_SCALE, SPLIT_W_SCALE = 64.0, 1024.0   # powers of two: activations up to 1023, weights up to 63 stay finite in fp16


def sat_word(flag):
    """The per-call saturation word of the plane-writing entry points (mickey_hip.h: sat_flag): None, or a zero-initialised
    int32 [1] device tensor that a kernel ORs 1 into when it had to clamp |x * scale| at fp16's largest finite value or met a
    NaN.  Returns the device pointer (None = nobody watches: no per-element work)."""
    if flag is None:
        return None
    assert flag.dtype == torch.int32 and flag.numel() >= 1 and flag.is_cuda
    return ptr(flag)


def plane_pair(shape, device, zero=False):
    """(hi, lo) fp16 planes as the two halves of ONE allocation: the split-operand kernels address both planes of a source from
    one base pointer (mickey_hip.h: within 2 GiB of each other)."""
    t = (torch.zeros if zero else torch.empty)((2,) + tuple(shape), device=device, dtype=torch.float16)
    return t[0], t[1]


def split_planes(x, hi, lo, scale=SPLIT_ACT_SCALE, sat=None):
    """fp32 tensor -> fp16 planes with x * scale = hi + lo (mk_split_planes); hi / lo: preallocated, same shape.  x, hi, lo
    may be column blocks of wider row-major matrices (views whose last dimension is contiguous and whose rows are
    equidistant, e.g. t[..., :C]).  sat: the saturation word (sat_word)."""
    assert x.dtype == torch.float32 and hi.dtype == torch.float16 and lo.dtype == torch.float16 and hi.shape == x.shape == lo.shape
    cols = x.shape[-1]
    rows = x.numel() // cols

    def ld(t):   # row stride of a [..., cols] view with uniformly spaced rows
        assert t.stride(-1) == 1
        lead = t.stride(-2) if t.dim() > 1 else cols
        for d in range(t.dim() - 2):   # leading dims must continue the same row spacing
            assert t.stride(d) == t.stride(d + 1) * t.shape[d + 1], "rows must be equidistant"
        return lead
    assert ld(hi) == ld(lo)
    call("mk_split_planes", ptr(x), rows, cols, ld(x), float(scale), ptr(hi), ptr(lo), ld(hi), sat_word(sat), stream())
    return hi, lo


def gemm_grouped_split(a, w, bias, out, groups, M, N, K, lda, ldc, stride_a, stride_w, stride_bias, stride_out, act=ACT_NONE,
                       w_scale=SPLIT_W_SCALE, sat=None):
    """mk_gemm_grouped_split: a = (hi, lo) fp16 planes [groups, M, lda] (one allocation: plane_pair), w fp16 [groups, N, 2 K]
    (weights.split_conv_weight); out fp32 or a (hi, lo) pair."""
    ah, al = a
    assert w.dtype == torch.float16 and w.shape[-1] == 2 * K
    if isinstance(out, (tuple, list)):
        oh, ol = out
    else:
        oh, ol = out, None
        assert out.dtype == torch.float32
    call("mk_gemm_grouped_split", ptr(ah), ptr(al), lda, stride_a, ptr(w), 2 * K, stride_w, ptr(bias), stride_bias, ptr(oh), ptr(ol),
         ldc, stride_out, groups, M, N, K, act, 1.0 / (SPLIT_ACT_SCALE * float(w_scale)), SPLIT_ACT_SCALE, sat_word(sat), stream())
    return out


def conv3x3_split(in1, C1, w, bias, out, Cout, groups, nimg, H, W, act=ACT_NONE, in2=None, C2=0, stride_in1=0, stride_in2=0,
                  stride_w=0, stride_bias=0, stride_out=0, out_bordered=False, w_scale=SPLIT_W_SCALE, sat=None):
    """mk_conv3x3_split: in1 / in2 = (hi, lo) pairs of bordered fp16 planes (each pair one allocation: plane_pair), w fp16
    [.., Cout, 2 K] (weights.split_conv_weight); out: an fp32 tensor, or a (hi, lo) pair of fp16 planes = the operand form of
    the next split conv (no fp32 round trip, no mk_split_planes pass).  in1 = (hi, None): the source is its hi plane (fp16
    features of an fp16 encoder): two products instead of three (then without in2)."""
    assert w.dtype == torch.float16
    h1, l1 = in1
    h2, l2 = in2 if in2 is not None else (None, None)
    if isinstance(out, (tuple, list)):
        oh, ol = out
        assert oh.dtype == torch.float16 and ol.dtype == torch.float16 and oh.shape == ol.shape
    else:
        oh, ol = out, None
        assert out.dtype == torch.float32
    call("mk_conv3x3_split", ptr(h1), ptr(l1), stride_in1, C1, ptr(h2), ptr(l2), stride_in2, C2, ptr(w), w.shape[-1], stride_w,
         ptr(bias), stride_bias, ptr(oh), ptr(ol), Cout, stride_out, groups, nimg, H, W, act, int(out_bordered),
         1.0 / (SPLIT_ACT_SCALE * float(w_scale)), SPLIT_ACT_SCALE, sat_word(sat), stream())
    return out


# ---- training: the heads' trainable 3x3 convolutions (mickey_hip.h: mk_conv_train_*, mk_conv_wgrad; train_heads.py) -----------
def absmax_scale(x, work=None):
    """mk_absmax_scale: fp32 4-d device tensor of any strides -> fp32 [2] device tensor (s, 1 / s), s the power-of-two plane
    scale that follows the tensor's abs-max.  Stays on the device: no synchronisation."""
    assert x.dtype == torch.float32 and x.dim() == 4 and x.numel() > 0
    if work is None:
        work = torch.empty(int(query("mk_absmax_scale_work_floats")), device=x.device, dtype=torch.float32)
    scale = torch.empty(2, device=x.device, dtype=torch.float32)
    if x.is_contiguous() or x.is_contiguous(memory_format=torch.channels_last):   # dense in memory: one flat sweep
        n = x.numel()
        dims, strides = (1, 1, 1, n), (n, n, n, 1)
    else:
        dims, strides = tuple(x.shape), tuple(x.stride())
    assert all(d < 2 ** 31 for d in dims), "mk_absmax_scale: a dimension of 2^31 elements or more"
    call("mk_absmax_scale", ptr(x), *dims, *strides, ptr(work), ptr(scale), stream())
    return scale


def conv_train_plane_buffer(nimg, H, W, C, device):
    """A zeroed (hi, lo) pair of training plane buffers (one allocation) and the views at bordered row 0 the kernels take:
    -> (buffer [2, mk_conv_train_plane_rows, C], hi, lo)."""
    lead, rows = int(query("mk_conv_train_lead_rows", W)), int(query("mk_conv_train_plane_rows", nimg, H, W))
    buf = torch.zeros((2, rows, C), device=device, dtype=torch.float16)
    return buf, buf[0, lead:], buf[1, lead:]


def conv_train_planes(x, scale, hi, lo):
    """mk_conv_train_planes: fp32 [nimg, C, H, W] of any strides -> the bordered (hi, lo) planes of x * scale[0]; hi / lo: the views
    of conv_train_plane_buffer, C <= their width."""
    nimg, C, H, W = x.shape
    assert x.dtype == torch.float32 and hi.dtype == torch.float16 and lo.dtype == torch.float16 and hi.stride() == lo.stride()
    call("mk_conv_train_planes", ptr(x), x.stride(0), x.stride(1), x.stride(2), x.stride(3), nimg, C, H, W, ptr(scale), ptr(hi),
         ptr(lo), hi.stride(0), stream())


def conv_train_weight_planes(w, w_scale, act_scale, transposed=False):
    """mk_conv_train_weight_planes: contiguous fp32 [Cout, Cin, 3, 3] -> (planes, acc_scale): the interleaved fp16 planes of the
    forward ([Cout, 2 * 9 Cin]) or, transposed, of the input gradient ([Cin, 2 * 9 Cp], Cp = Cout rounded up to 32), and the fp32
    [1] accumulator scale 1 / (s_w s_act) of the conv that uses them."""
    Cout, Cin = w.shape[:2]
    assert w.dtype == torch.float32 and w.is_contiguous() and tuple(w.shape[2:]) == (3, 3)
    Cp = (Cout + 31) // 32 * 32
    planes = torch.empty((Cin, 18 * Cp) if transposed else (Cout, 18 * Cin), device=w.device, dtype=torch.float16)
    acc = torch.empty(1, device=w.device, dtype=torch.float32)
    call("mk_conv_train_weight_planes", ptr(w), Cout, Cin, int(bool(transposed)), ptr(w_scale), ptr(act_scale), ptr(planes), ptr(acc),
         stream())
    return planes, acc


def conv3x3_split_dscale(in1, C1, w, out, Cout, nimg, H, W, acc_scale):
    """mk_conv3x3_split_dscale, the plain form the training convs use: in1 = (hi, lo) bordered planes, w = interleaved planes,
    out fp32 dense rows [nimg * H * W, Cout] = acc * acc_scale[0] with acc_scale a device tensor."""
    h1, l1 = in1
    assert w.dtype == torch.float16 and out.dtype == torch.float32 and acc_scale.dtype == torch.float32
    call("mk_conv3x3_split_dscale", ptr(h1), ptr(l1), C1, ptr(w), w.shape[-1], ptr(out), Cout, nimg, H, W, ptr(acc_scale), stream())
    return out


def conv_wgrad(gy, ldg, xp, Cout, Cin, nimg, H, W, gy_scale, x_scale, dw=None):
    """mk_conv_wgrad: gy / xp = (hi, lo) plane views (conv_train_plane_buffer) of gY [.., ldg] and X [.., Cin] -> dw fp32
    [Cout, Cin, 3, 3]."""
    if dw is None:
        dw = torch.empty((Cout, Cin, 3, 3), device=xp[0].device, dtype=torch.float32)
    assert dw.dtype == torch.float32 and dw.is_contiguous() and tuple(dw.shape) == (Cout, Cin, 3, 3)
    work = torch.empty(max(1, int(query("mk_conv_wgrad_work_floats", Cout, Cin, nimg, H, W))), device=dw.device, dtype=torch.float32)
    call("mk_conv_wgrad", ptr(gy[0]), ptr(gy[1]), ldg, ptr(xp[0]), ptr(xp[1]), Cout, Cin, nimg, H, W, ptr(gy_scale), ptr(x_scale),
         ptr(work), ptr(dw), stream())
    return dw


# ---- the heads' positional encoding (mk_heads.hip) and linear attention for inference (mickey_hip.h: mk_linattn_*; mk_linattn.hip) ----
def posenc_add(x, pe, xs, cat, groups, nimg, npix, C):
    call("mk_posenc_add", ptr(x), ptr(pe), ptr(xs), ptr(cat), cat.stride(-2), groups, nimg, npix, C, dtype_code(x.dtype),
         stream())


def linattn_work_floats(groups, nimg, L, C):
    return query("mk_linattn_work_floats", groups, nimg, L, C)


def linattn_kv(qkv, kv, work, groups, nimg, L, C):
    call("mk_linattn_kv", ptr(qkv), ptr(kv), ptr(work), groups, nimg, L, C, stream())


def linattn_apply(qkv, kv, out, ldo, groups, nimg, L, C):
    call("mk_linattn_apply", ptr(qkv), ptr(kv), ptr(out), ldo, groups, nimg, L, C, dtype_code(out.dtype), stream())


def linattn_kv_fused(x, qkv_w, kv, work, groups, nimg, L, C, lda=None):
    """mk_linattn_kv_fused: kv / work as gemm_grouped(x, qkv_w) -> linattn_kv leave them, without the fp32 qkv rows.  x lp [G, nimg * L,
    lda] (columns [0, C) are read), qkv_w lp [G, 3C, C]."""
    lda = x.stride(-2) if lda is None else lda
    call("mk_linattn_kv_fused", ptr(x), lda, x.stride(0), ptr(qkv_w), qkv_w.stride(-2), qkv_w.stride(0), ptr(kv), ptr(work), groups, nimg,
         L, C, dtype_code(x.dtype), stream())


def linattn_apply_fused(x, qkv_w, kv, out, groups, nimg, L, C, merge_w=None, ln_w=None, ln_b=None, eps=1e-5, lda=None):
    """mk_linattn_apply_fused: q projection + linattn_apply, and with merge_w / ln_w / ln_b also merge -> norm1 (gemm_ln128), in one
    launch.  out lp [G, nimg * L, ldo] (a view: its strides are passed on) receives the normalised rows, or msg without merge_w."""
    lda = x.stride(-2) if lda is None else lda
    mw = merge_w is not None
    call("mk_linattn_apply_fused", ptr(x), lda, x.stride(0), ptr(qkv_w), qkv_w.stride(-2), qkv_w.stride(0), ptr(kv), ptr(merge_w),
         merge_w.stride(-2) if mw else 0, merge_w.stride(0) if mw else 0, ptr(ln_w), ptr(ln_b), float(eps), ptr(out), out.stride(-2),
         out.stride(0), groups, nimg, L, C, dtype_code(x.dtype), stream())
    return out


# ---- training: the heads' linear attention (mickey_hip.h: mk_linattn_train_*, mk_linattn.hip beside the inference kernels;
# train_attention.py) ------------------------------------------------------------------------------------------------------------
def _attn_rows(t):
    """[N, T, H, 16] fp32 device tensor with dense last two dimensions -> (pointer, row stride, image stride); the stride of a
    dimension of size 1 means nothing and is replaced by the dense one."""
    N, T, H, D = t.shape
    assert t.dtype == torch.float32 and D == 16 and t.stride(3) == 1 and (H == 1 or t.stride(2) == 16)
    ld = t.stride(1) if T > 1 else H * 16
    return ptr(t), ld, t.stride(0) if N > 1 else T * ld


def linattn_train_fwd(q, k, v, eps):
    """mk_linattn_train_fwd: q [N, L, H, 16], k, v [N, S, H, 16] (rows of any stride) -> (out [N, L, H, 16] contiguous,
    kv [N * H, 272]: the M | ks block the backward reads)."""
    N, L, H, _ = q.shape
    S, C = k.shape[1], H * 16
    out = torch.empty((N, L, H, 16), device=q.device, dtype=torch.float32)
    kv = torch.empty((N * H, 272), device=q.device, dtype=torch.float32)
    work = torch.empty(int(query("mk_linattn_train_work_floats", N, L, S, C)), device=q.device, dtype=torch.float32)
    call("mk_linattn_train_fwd", *_attn_rows(q), *_attn_rows(k), *_attn_rows(v), float(eps), ptr(out), ptr(kv), ptr(work), N, L, S, C,
         stream())
    return out, kv


def linattn_train_bwd(q, k, v, kv, go, eps, need, out=None):
    """mk_linattn_train_bwd: go [N, L, H, 16] contiguous, need = (gq, gk, gv wanted) -> (gq, gk, gv), None where not wanted.
    out: optional contiguous buffers (gq, gk, gv) to write instead of new ones (e.g. three planes of one allocation)."""
    N, L, H, _ = q.shape
    S, C = k.shape[1], H * 16
    assert go.dtype == torch.float32 and go.is_contiguous() and tuple(go.shape) == (N, L, H, 16) and tuple(kv.shape) == (N * H, 272)
    if out is not None:
        assert all(o.is_contiguous() and o.dtype == torch.float32 and o.numel() == N * T * C for o, T in zip(out, (L, S, S)))
    new = lambda T, i: out[i] if out is not None else torch.empty((N, T, H, 16), device=q.device, dtype=torch.float32)   # noqa: E731
    gq = new(L, 0) if need[0] else None
    gk = new(S, 1) if need[1] else None
    gv = new(S, 2) if need[2] else None
    work = gkv = None
    if need[1] or need[2]:
        gkv = torch.empty((N * H, 272), device=q.device, dtype=torch.float32)
        work = torch.empty(int(query("mk_linattn_train_work_floats", N, L, S, C)), device=q.device, dtype=torch.float32)
    call("mk_linattn_train_bwd", *_attn_rows(q), *_attn_rows(k), *_attn_rows(v), ptr(kv), ptr(go), float(eps), ptr(work), ptr(gkv),
         ptr(gq), ptr(gk), ptr(gv), N, L, S, C, stream())
    return gq, gk, gv


# ---- training: the Linears and LayerNorms of the heads' EncoderLayer (mickey_hip.h: mk_train_linear_* / mk_train_ln128_*;
# train_layer.py).  Operands are 2-D fp32 device tensors whose rows are dense and 16-byte aligned (any row stride). ----------------
def _mat(t):
    """2-D fp32 tensor with dense rows -> (pointer, row stride); None -> (None, 0)."""
    if t is None:
        return None, 0
    assert t.dtype == torch.float32 and t.dim() == 2 and (t.shape[1] == 1 or t.stride(1) == 1)
    return ptr(t), (t.stride(0) if t.shape[0] > 1 else t.shape[1])


def _wsplit(w):
    """a weight, or a tuple of three equally shaped ones read as their row-wise concatenation -> (w, w2, w3, wsplit)"""
    if isinstance(w, (tuple, list)):
        a, b, c = w
        assert a.shape == b.shape == c.shape and all(x.is_contiguous() and x.dtype == torch.float32 for x in w)
        return ptr(a), ptr(b), ptr(c), a.shape[0]
    assert w.is_contiguous() and w.dtype == torch.float32
    return ptr(w), None, None, 0


def _gplanes(g):
    """a gradient [M, N], or planes [P, M, n] read as [M, P n] -> (pointer, row stride, plane stride, columns per plane, M, N)"""
    if g.dim() == 3:
        P, M, n = g.shape
        assert g.dtype == torch.float32 and g.stride(2) == 1
        return ptr(g), (g.stride(1) if M > 1 else n), (g.stride(0) if P > 1 else 0), n, M, P * n
    p, ld = _mat(g)
    return p, ld, 0, 0, g.shape[0], g.shape[1]


def train_chunks(M):
    """(rows per chunk, chunks) of an M-row weight gradient: a function of M alone."""
    return int(query("mk_train_rows_per_chunk", M)), int(query("mk_train_chunks", M))


def train_ln_steps(M):
    return int(query("mk_train_ln_steps", M))


def train_linear_fwd(a1, w, a2=None, relu=False, out=None):
    """mk_train_linear_fwd: out [M, N] = act([a1 | a2] . w^T); w [N, K1 + K2] or a tuple of three such matrices (rows concatenated)."""
    M, K1 = a1.shape
    K2 = 0 if a2 is None else a2.shape[1]
    pw, pw2, pw3, ws = _wsplit(w)
    N = 3 * ws if ws else w.shape[0]
    if out is None:
        out = torch.empty((M, N), device=a1.device, dtype=torch.float32)
    call("mk_train_linear_fwd", *_mat(a1), K1, *_mat(a2), K2, pw, pw2, pw3, ws, *_mat(out), M, N, int(bool(relu)), stream())
    return out


def train_linear_ln128_fwd(a1, w, gamma, beta, eps, a2=None, resid=None, want_saved=True):
    """mk_train_linear_ln128_fwd: LayerNorm_128([a1 | a2] . w^T) gamma + beta (+ resid) -> (out, xhat, rstd); xhat and rstd are None
    unless want_saved."""
    M, K1 = a1.shape
    K2 = 0 if a2 is None else a2.shape[1]
    assert w.is_contiguous() and tuple(w.shape) == (128, K1 + K2) and gamma.is_contiguous() and beta.is_contiguous()
    out = torch.empty((M, 128), device=a1.device, dtype=torch.float32)
    xhat = torch.empty_like(out) if want_saved else None
    rstd = torch.empty((M,), device=a1.device, dtype=torch.float32) if want_saved else None
    call("mk_train_linear_ln128_fwd", *_mat(a1), K1, *_mat(a2), K2, ptr(w), ptr(gamma), ptr(beta), float(eps), *_mat(resid), ptr(out),
         ptr(xhat), ptr(rstd), M, stream())
    return out, xhat, rstd


def train_linear_dgrad(g, w, o1, o2=None, mask=None, accumulate=0):
    """mk_train_linear_dgrad: [o1 | o2] (+)= (g . w), zero where mask <= 0.  g [M, N] or planes [P, M, N / P]; accumulate: bit 0 adds
    to o1, bit 1 to o2."""
    pg, ldg, gplane, gsplit, M, N = _gplanes(g)
    pw, pw2, pw3, ws = _wsplit(w)
    K1 = o1.shape[1]
    K2 = 0 if o2 is None else o2.shape[1]
    call("mk_train_linear_dgrad", pg, ldg, gplane, gsplit, pw, pw2, pw3, ws, *_mat(mask), *_mat(o1), K1, *_mat(o2), K2,
         int(accumulate), M, N, stream())


def train_linear_wgrad(g, a1, part, chunk_stride, rows_per_chunk, chunks, a2=None):
    """mk_train_linear_wgrad: per-chunk partials of g^T . [a1 | a2] into part (a 1-D view whose element 0 is chunk 0's [N, K])."""
    pg, ldg, gplane, gsplit, M, N = _gplanes(g)
    K1 = a1.shape[1]
    K2 = 0 if a2 is None else a2.shape[1]
    assert part.dtype == torch.float32 and part.is_contiguous() and part.numel() >= (chunks - 1) * chunk_stride + N * (K1 + K2)
    call("mk_train_linear_wgrad", pg, ldg, gplane, gsplit, *_mat(a1), K1, *_mat(a2), K2, ptr(part), chunk_stride, rows_per_chunk, chunks,
         M, N, stream())


def train_tail(wpart, wstride, wchunks, nw, lpart, lstride, lsteps, nl, out):
    """mk_train_tail: every chunk / step partial of a backward pass -> out [nw + nl], added in index order, one launch."""
    assert out.is_contiguous() and out.numel() >= nw + nl
    assert nw == 0 or wpart.numel() >= (wchunks - 1) * wstride + nw
    assert nl == 0 or lpart.numel() >= (lsteps - 1) * lstride + nl
    call("mk_train_tail", ptr(wpart) if nw else None, wstride, wchunks, nw, ptr(lpart) if nl else None, lstride, lsteps, nl, ptr(out),
         stream())


def train_ln128_fwd(u, gamma, beta, eps, resid=None, want_saved=True):
    """mk_train_ln128_fwd: u [M, 128] dense -> (out, xhat, rstd); xhat and rstd are None unless want_saved."""
    M = u.shape[0]
    assert u.is_contiguous() and u.shape[1] == 128 and gamma.is_contiguous() and beta.is_contiguous()
    out = torch.empty_like(u)
    xhat = torch.empty_like(u) if want_saved else None
    rstd = torch.empty((M,), device=u.device, dtype=torch.float32) if want_saved else None
    call("mk_train_ln128_fwd", ptr(u), ptr(gamma), ptr(beta), float(eps), *_mat(resid), ptr(out), ptr(xhat), ptr(rstd), M, stream())
    return out, xhat, rstd


def train_ln128_bwd(g, xhat, rstd, gamma, gu=None, part=None, part_stride=256):
    """mk_train_ln128_bwd: gu [M, 128] (None: not wanted) and the per-step column sums g xhat | g into part (None: not wanted)."""
    M = g.shape[0]
    assert g.is_contiguous() and xhat.is_contiguous() and g.shape[1] == 128 and (gu is None or gu.is_contiguous())
    assert part is None or part.numel() >= (train_ln_steps(M) - 1) * part_stride + 256
    call("mk_train_ln128_bwd", ptr(g), ptr(xhat), ptr(rstd), ptr(gamma), ptr(gu), ptr(part), part_stride, M, stream())


# ---- training: the head tails (mickey_hip.h: mk_train_headtail_* / mk_train_desc_l2norm_*; train_tails.py).  Features are 2-D fp32
# [nimg h w, C] tensors with dense, 16-byte aligned rows; outputs may be passed in (tests place them in guarded windows). ----------
TAIL_IDENTITY, TAIL_SIGMOID, TAIL_MASKED_SIGMOID, TAIL_SOFTMAX = (_native.MK_TAIL_IDENTITY, _native.MK_TAIL_SIGMOID,
                                                                  _native.MK_TAIL_MASKED_SIGMOID, _native.MK_TAIL_SOFTMAX)
HEADTAIL_CHUNK_ROWS = 208   # rows of one weight-gradient partial == mk_train_headtail_chunk_rows() (tests/test_train_tails_cpu.py)
TAIL_MIN_C, TAIL_MAX_C = 4, 256


def headtail_chunks(rows):
    """chunks of the weight gradient of a `rows`-row 1x1 tail: a function of the row count alone."""
    return -(-rows // HEADTAIL_CHUNK_ROWS) if rows > 0 else 0   # == mk_train_headtail_chunks(rows), without the call


def _dense(t):
    assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % 16 == 0
    return t


def train_headtail_fwd(feat, w, nimg, h, wd, act, scale=1.0, border=0, temperature=1.0, eps=0.0, out=None):
    """mk_train_headtail_fwd: feat [nimg h wd, C], w [Cout, C] -> out [nimg, Cout, h wd] (1 launch; 2 for TAIL_SOFTMAX)."""
    C, Cout = feat.shape[1], w.shape[0]
    assert feat.shape[0] == nimg * h * wd and w.shape[1] == C
    if out is None:
        out = torch.empty((nimg, Cout, h * wd), device=feat.device, dtype=torch.float32)
    assert out.is_contiguous() and out.numel() == nimg * Cout * h * wd
    call("mk_train_headtail_fwd", ptr(_dense(feat)), ptr(_dense(w)), ptr(out), nimg, h, wd, C, Cout, int(act), float(scale), int(border),
         float(temperature), float(eps), stream())
    return out


def train_headtail_bwd(g, y, feat, w, nimg, n, act, scale=1.0, temperature=1.0, want_gfeat=True, want_gw=True, gfeat=None, gw=None,
                       part=None):
    """mk_train_headtail_bwd: g, y [nimg, Cout, n] -> (gfeat [nimg n, C] or None, gw [Cout, C] or None); at most 3 launches, none of
    the weight-gradient work without want_gw, no pass over gfeat without want_gfeat."""
    Cout, C = w.shape
    dev = g.device
    assert g.is_contiguous() and g.dtype == torch.float32 and g.numel() == nimg * Cout * n and (y is None or y.is_contiguous())
    chunks = headtail_chunks(nimg * n) if want_gw else 0
    nw = Cout * C
    # one allocation for the work memory of a call: chunk partials | gw | the per-image dots of the softmax
    need = ((chunks * nw if part is None else 0) + (nw if gw is None else 0) if want_gw else 0) + (nimg if act == TAIL_SOFTMAX else 0)
    work = torch.empty((need,), device=dev, dtype=torch.float32) if need else None
    off = 0
    if want_gw:
        if part is None:
            part, off = work[:chunks * nw], chunks * nw
        if gw is None:
            gw, off = work[off:off + nw].view(Cout, C), off + nw
        assert part.is_contiguous() and part.numel() >= chunks * nw and part.data_ptr() % 16 == 0 and gw.is_contiguous() and gw.numel() == nw
        _dense(feat)
    dot = work[off:] if act == TAIL_SOFTMAX else None
    if want_gfeat and gfeat is None:
        gfeat = torch.empty((nimg * n, C), device=dev, dtype=torch.float32)
    call("mk_train_headtail_bwd", ptr(g), ptr(y), ptr(feat) if want_gw else None, ptr(_dense(w)), ptr(dot),
         ptr(_dense(gfeat)) if want_gfeat else None, ptr(part) if want_gw else None, ptr(gw) if want_gw else None, nimg, n, C, Cout,
         int(act), float(scale), float(temperature), stream())
    return (gfeat if want_gfeat else None), (gw if want_gw else None)


def train_desc_l2norm_fwd(x, nimg, n, eps, want_saved=True, out=None):
    """mk_train_desc_l2norm_fwd: x [nimg n, C] -> (y [nimg, C, n], rnorm [nimg n] or None)."""
    C = x.shape[1]
    assert x.shape[0] == nimg * n
    if out is None:
        out = torch.empty((nimg, C, n), device=x.device, dtype=torch.float32)
    assert out.is_contiguous() and out.numel() == nimg * C * n
    rnorm = torch.empty((nimg * n,), device=x.device, dtype=torch.float32) if want_saved else None
    call("mk_train_desc_l2norm_fwd", ptr(_dense(x)), ptr(out), ptr(rnorm), nimg, n, C, float(eps), stream())
    return out, rnorm


def train_desc_l2norm_bwd(g, y, rnorm, nimg, n, C, out=None):
    """mk_train_desc_l2norm_bwd: g, y [nimg, C, n], rnorm [nimg n] -> gx [nimg n, C]."""
    assert g.is_contiguous() and y.is_contiguous() and g.dtype == torch.float32 and g.numel() == y.numel() == nimg * C * n
    if out is None:
        out = torch.empty((nimg * n, C), device=g.device, dtype=torch.float32)
    assert out.is_contiguous() and out.numel() == nimg * n * C
    call("mk_train_desc_l2norm_bwd", ptr(g), ptr(y), ptr(rnorm), ptr(out), nimg, n, C, stream())
    return out


# ---- training: BatchNorm + residual + ReLU of the heads' BasicBlock (mickey_hip.h: mk_train_bn_*; train_block.py).  Operands are 2-D
# fp32 [M, C] device tensors with dense, 16-byte aligned rows (any row stride that is a multiple of 4); outputs may be passed in. ------
BN_CHUNK_ROWS = 256   # rows of one statistics partial == mk_train_bn_chunk_rows() (tests/test_train_block_cpu.py)
BN_MIN_C, BN_MAX_C = 4, 1024


def bn_chunks(M):
    """chunks of the per-channel sums over M rows: a function of M alone."""
    return -(-M // BN_CHUNK_ROWS) if M > 0 else 0   # == mk_train_bn_chunks(M), without the call


def _vec(t, C):
    assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == C and t.data_ptr() % 16 == 0
    return ptr(t)


def train_bn_fwd(x, gamma, beta, running_mean, running_var, num_batches_tracked, training, momentum, eps, resid=None, relu=True,
                 want_saved=True, out=None, stats=None, mask=None, work=None):
    """mk_train_bn_fwd: x [M, C] -> (y [M, C], stats [2, C] = mean | rstd or None, mask uint8 [M, C] or None); 2 launches in training
    (which also updates the running statistics), 1 in eval.  stats and mask are None unless want_saved (mask: and relu)."""
    M, C = x.shape
    dev = x.device
    if out is None:
        out = torch.empty((M, C), device=dev, dtype=torch.float32)
    if want_saved:
        if stats is None:
            stats = torch.empty((2, C), device=dev, dtype=torch.float32)
        if relu and mask is None:
            mask = torch.empty((M, C), device=dev, dtype=torch.uint8)
        assert stats.is_contiguous() and stats.numel() == 2 * C and (mask is None or (mask.is_contiguous() and mask.numel() == M * C))
    else:
        stats = mask = None
    if training and work is None:
        work = torch.empty((bn_chunks(M) * 2 * C,), device=dev, dtype=torch.float32)
    assert not training or (work.is_contiguous() and work.numel() >= bn_chunks(M) * 2 * C)
    assert num_batches_tracked is None or (num_batches_tracked.dtype == torch.int64 and num_batches_tracked.numel() == 1)
    call("mk_train_bn_fwd", *_mat(x), _vec(gamma, C), _vec(beta, C), *_mat(resid), _vec(running_mean, C), _vec(running_var, C),
         ptr(num_batches_tracked), float(momentum), float(eps), ptr(work) if training else None, *_mat(out),
         ptr(stats) if want_saved else None, ptr(stats[1]) if want_saved else None, ptr(mask), M, C, int(bool(relu)), int(bool(training)),
         stream())
    return out, stats, mask


def train_bn_bwd(g, x, gamma, stats, mask, training, eps, want_gx=True, want_gresid=False, want_affine=True, gx=None, gresid=None,
                 affine=None, work=None):
    """mk_train_bn_bwd: g, x [M, C], stats [2, C], mask uint8 [M, C] or None (no ReLU) -> (gx [M, C] or None, gresid [M, C] or None,
    affine [2, C] = dgamma | dbeta or None); 2 launches, none when nothing is wanted."""
    M, C = x.shape
    dev = g.device
    assert g.shape == x.shape and stats.is_contiguous() and stats.numel() == 2 * C and stats.data_ptr() % 16 == 0
    assert mask is None or (mask.dtype == torch.uint8 and mask.is_contiguous() and mask.numel() == M * C)
    if want_gx and gx is None:
        gx = torch.empty((M, C), device=dev, dtype=torch.float32)
    if want_gresid and gresid is None:
        gresid = torch.empty((M, C), device=dev, dtype=torch.float32)
    if want_affine and affine is None:
        affine = torch.empty((2, C), device=dev, dtype=torch.float32)
    if work is None:
        work = torch.empty((bn_chunks(M) * 8 * C,), device=dev, dtype=torch.float32)
    assert work.is_contiguous() and work.numel() >= bn_chunks(M) * 8 * C and work.data_ptr() % 16 == 0
    call("mk_train_bn_bwd", *_mat(g), *_mat(x), _vec(gamma, C), ptr(stats), ptr(stats[1]), ptr(mask), ptr(work),
         *_mat(gx if want_gx else None), *_mat(gresid if want_gresid else None), ptr(affine) if want_affine else None,
         ptr(affine[1]) if want_affine else None, float(eps), M, C, int(bool(training)), stream())
    return (gx if want_gx else None), (gresid if want_gresid else None), (affine if want_affine else None)


def head_tails(f_det, w_score, f_off, w_xy, f_dep, w_dep, f_dsc, nimg, h, w, C, Cd, border=3, use_softmax=True,
               use_depth_sigmoid=False, max_depth=60.0, norm_dsc=True, down=14.0):
    dev = f_det.device
    n = h * w
    scr = torch.empty((nimg, 1, n), device=dev, dtype=torch.float32)
    kps = torch.empty((nimg, 2, n), device=dev, dtype=torch.float32)
    depth = torch.empty((nimg, 1, n), device=dev, dtype=torch.float32)
    dsc = torch.empty((nimg, Cd, n), device=dev, dtype=torch.float32)
    call("mk_head_tails", ptr(f_det), ptr(w_score), ptr(f_off), ptr(w_xy), ptr(f_dep), ptr(w_dep), ptr(f_dsc), ptr(scr),
         ptr(kps), ptr(depth), ptr(dsc), nimg, h, w, C, Cd, border, int(use_softmax), int(use_depth_sigmoid), float(max_depth),
         int(norm_dsc), float(down), stream())
    return scr, kps, depth, dsc


def dual_softmax_split_ok(C, temperature):
    """Preconditions of mk_dual_softmax_split that can be checked on the host (the third, |dsc| <= 1, is the caller's)."""
    return C == 128 and temperature > 0 and LOG2E / float(temperature) <= 100.0


def check_keyframe_index(index, B, K):
    """Host validation of a pair -> keyframe map (keyframe mode, mickey_hip.h: the *_kf entry points): B integers in [0, K).
    Accepts a list, a numpy array or a CPU / device integer tensor (a device tensor is copied to the host: one synchronisation).
    Returns the map as a numpy int32 array; raises ValueError on a wrong length, a non-integer dtype, an entry out of range or
    more keyframes than pairs (K <= B is what the matchers' work sizes assume, mickey_hip.h)."""
    if torch.is_tensor(index):
        if index.dtype.is_floating_point or index.dtype.is_complex or index.dtype == torch.bool:
            raise ValueError("keyframe_index must hold integers, got %s" % index.dtype)
        a = index.detach().cpu().numpy()
    else:
        a = np.asarray(index)
        if a.size == 0 and a.dtype == np.float64:   # [] -> an empty integer map (the length check below decides)
            a = a.astype(np.int64)
        if a.dtype.kind not in "iu":
            raise ValueError("keyframe_index must hold integers, got %s" % a.dtype)
    if a.ndim != 1 or a.shape[0] != int(B):
        raise ValueError("keyframe_index must hold one entry per pair (%d), got shape %s" % (int(B), tuple(a.shape)))
    if not 0 < int(K) <= max(1, int(B)):
        raise ValueError("keyframe mode needs 1 <= K <= B keyframes (image0 has %d for %d pairs: a keyframe no pair uses is "
                         "wasted work)" % (int(K), int(B)))
    if a.size and (int(a.min()) < 0 or int(a.max()) >= int(K)):
        raise ValueError("keyframe_index entries must lie in [0, %d), got [%d, %d]" % (int(K), int(a.min()), int(a.max())))
    return a.astype(np.int32)


def _kf_arg(keyframe_index, B, K, dev):
    """-> (device int32 map or None, K for the ABI).  A contiguous int32 device tensor of B entries is passed as it is (the
    caller validated it: pipeline / model; a kernel skips a pair whose entry is outside [0, K) and reads nothing for it);
    anything else is validated on the host here and uploaded."""
    if keyframe_index is None:
        return None, B
    t = keyframe_index
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.dim() == 1 and t.shape[0] == B):
        t = torch.from_numpy(check_keyframe_index(t, B, K)).to(dev)
    return t, K


def check_pair_index(index, P, N):
    """Host validation of a pair list (pair-list mode, mickey_hip.h: the *_pairs entry points): [P, 2] integers, column 0 in
    [0, N0) and column 1 in [0, N1), where N is the size of the one image set both columns index or an (N0, N1) pair.  Accepts a
    list, a numpy array or a CPU / device integer tensor (a device tensor is copied to the host: one synchronisation).  Returns
    the list as a numpy int32 array [P, 2]; raises ValueError on a wrong shape, a non-integer dtype or an entry out of range.
    Duplicated pairs and self pairs (i, i) are legal, and so is an image no pair uses."""
    if torch.is_tensor(index):
        if index.dtype.is_floating_point or index.dtype.is_complex or index.dtype == torch.bool:
            raise ValueError("pair_index must hold integers, got %s" % index.dtype)
        a = index.detach().cpu().numpy()
    else:
        a = np.asarray(index)
        if a.size == 0 and a.dtype == np.float64:   # [] -> an empty integer list (the shape check below decides)
            a = a.astype(np.int64)
        if a.dtype.kind not in "iu":
            raise ValueError("pair_index must hold integers, got %s" % a.dtype)
    if a.ndim != 2 or a.shape != (int(P), 2):
        raise ValueError("pair_index must have shape [%d, 2] (one (image 0, image 1) row per pair), got %s" % (int(P), tuple(a.shape)))
    for side, n in enumerate(N if isinstance(N, (tuple, list)) else (N, N)):
        col = a[:, side]
        if int(n) <= 0:
            raise ValueError("pair-list mode needs at least one image on side %d, got %d" % (side, int(n)))
        if col.size and (int(col.min()) < 0 or int(col.max()) >= int(n)):
            raise ValueError("pair_index[:, %d] entries must lie in [0, %d), got [%d, %d]" % (side, int(n), int(col.min()), int(col.max())))
    return a.astype(np.int32)


def pair_maps(pair_index, P, N, dev):
    """[P, 2] pair list (anything check_pair_index takes, validated here on the host) -> the two contiguous int32 device maps
    (idx0, idx1) of the *_pairs entry points (mickey_hip.h)."""
    t = torch.from_numpy(np.ascontiguousarray(check_pair_index(pair_index, P, N).T)).to(dev)
    return t[0], t[1]


def _pair_arg(pair_index, N0, N1, dev, P=None):
    """-> (idx0, idx1, P) for the *_pairs entry points.  A 2-tuple (idx0, idx1) of contiguous int32 device maps -- either may be
    None = the identity on that side -- is passed as it is (the caller validated it: pipeline / model; a kernel skips a pair whose
    entry is outside its operand's rows and reads nothing for it).  Anything else is a [P, 2] list, validated on the host here
    (check_pair_index) and uploaded."""
    if isinstance(pair_index, tuple) and len(pair_index) == 2 and all(
            m is None or (torch.is_tensor(m) and m.is_cuda and m.dtype == torch.int32 and m.is_contiguous() and m.dim() == 1)
            for m in pair_index):
        i0, i1 = pair_index
        sizes = {int(m.shape[0]) for m in (i0, i1) if m is not None}
        sizes |= {int(n) for m, n in ((i0, N0), (i1, N1)) if m is None}   # an identity side has one row per pair
        if P is not None:
            sizes.add(int(P))
        if len(sizes) != 1:
            raise ValueError("pair maps, identity sides and the pair count disagree: %s" % sorted(sizes))
        return i0, i1, sizes.pop()
    n = len(pair_index) if P is None else int(P)
    i0, i1 = pair_maps(pair_index, n, (N0, N1), dev)
    return i0, i1, n


def _one_mode(keyframe_index, pair_index):
    if keyframe_index is not None and pair_index is not None:
        raise ValueError("keyframe_index and pair_index are mutually exclusive")


def _row_maps(keyframe_index, pair_index, rows0, rows1, dev, P=None):
    """The calling mode of a matcher / solver wrapper (plain, keyframe_index= or pair_index=; rows0 / rows1: the rows operand 0 /
    operand 1 hold; P: the pair count where the caller knows it) -> (suffix, maps, rows, P), with which the wrapper finishes the
    call without looking at the mode again: the entry point is the plain name + suffix, its trailing arguments are
    *map(ptr, maps), *rows, and P is the pair count.
        plain      "",        (),           (),             P = rows1
        keyframe   "_kf",     (map,),       (K,),           P = rows1                       (_kf_arg)
        pair list  "_pairs",  (idx0, idx1), (rows0, rows1), P = the maps' / the list's length (_pair_arg)
    The maps come back as tensors: they must live until the call is enqueued."""
    _one_mode(keyframe_index, pair_index)
    if pair_index is not None:
        i0, i1, P = _pair_arg(pair_index, rows0, rows1, dev, P)
        return "_pairs", (i0, i1), (rows0, rows1), P
    P = rows1 if P is None else P
    if keyframe_index is not None:
        kf, K = _kf_arg(keyframe_index, P, rows0, dev)
        return "_kf", (kf,), (K,), P
    return "", (), (), P


def _outs(out, shape, wants, dev):
    """The three [B, n0, n1] outputs of a matcher: fresh, or the caller's (out = (scores, kp_scores, final_scores), an entry
    None where not wanted: a chunked caller writes every chunk into its own buffers)."""
    if out is None:
        return [torch.empty(shape, device=dev, dtype=torch.float32) if w else None for w in wants]
    for o, w in zip(out, wants):
        if (o is not None) != bool(w) or (o is not None and not (o.is_cuda and o.dtype == torch.float32 and o.is_contiguous() and
                                                                   tuple(o.shape) == tuple(shape))):
            raise ValueError("out= must hold a contiguous fp32 device tensor %s exactly where an output is wanted" % (tuple(shape),))
    return list(out)


def dsc_split_planes(dsc):
    """mk_dsc_split_planes: fp32 [N, 128, n] unit-norm descriptors -> their split-fp16 operand planes (an opaque fp32 buffer),
    made once for a set that many pairs read (dual_softmax(..., planes=...))."""
    _chk(dsc, torch.float32)
    N, C, n = dsc.shape
    planes = torch.empty((query("mk_dsc_split_planes_floats", N, n),), device=dsc.device, dtype=torch.float32)
    call("mk_dsc_split_planes", ptr(dsc), ptr(planes), N, C, n, stream())
    return planes


# dual_softmax: (split, planes given, entry-point suffix of the mode) -> (work-size query, entry point)
_DUAL_SOFTMAX = {
    (False, False, ""): ("mk_dual_softmax_work_floats", "mk_dual_softmax"),
    (False, False, "_kf"): ("mk_dual_softmax_work_floats", "mk_dual_softmax_kf"),
    (False, False, "_pairs"): ("mk_dual_softmax_work_floats", "mk_dual_softmax_pairs"),
    (True, False, ""): ("mk_dual_softmax_split_work_floats", "mk_dual_softmax_split"),
    (True, False, "_kf"): ("mk_dual_softmax_split_work_floats", "mk_dual_softmax_split_kf"),
    (True, False, "_pairs"): ("mk_dual_softmax_split_pairs_work_floats", "mk_dual_softmax_split_pairs"),
    (True, True, "_pairs"): ("mk_dual_softmax_split_planes_work_floats", "mk_dual_softmax_split_planes"),
}


def dual_softmax(dsc0, dsc1, scr0=None, scr1=None, temperature=0.1, dustbin=None, want_scores=True, want_kp=True,
                 want_final=True, split=False, keyframe_index=None, pair_index=None, planes=None, out=None):
    """Returns (scores, kp_scores, final_scores) (None where not requested).  split: the correlation on the 16-bit matrix
    cores with split-fp16 operands (mk_dual_softmax_split; unit-norm descriptors only), else the exact fp32 MFMA.
    keyframe_index (keyframe mode): B pair -> keyframe entries; dsc0 / scr0 then hold the K keyframes, dsc1 / scr1 the B
    pairs' query frames, and pair b correlates dsc0[keyframe_index[b]] with dsc1[b] (mk_dual_softmax_kf / _split_kf).
    pair_index (pair-list mode, mk_dual_softmax_pairs / _split_pairs): [P, 2]; dsc0 / scr0 hold N0 images, dsc1 / scr1 N1 (the
    same tensors for one image set), and pair p correlates dsc0[pair_index[p, 0]] with dsc1[pair_index[p, 1]]; or the 2-tuple of
    device maps _pair_arg describes.  planes (split, pair-list mode): (planes0, planes1) of dsc_split_planes -- the passes run
    on them (mk_dual_softmax_split_planes) instead of making the planes in this call.  out: see _outs."""
    _one_mode(keyframe_index, pair_index)
    _chk(dsc0, torch.float32)
    _chk(dsc1, torch.float32)
    K, C, n0 = dsc0.shape
    B, n1 = dsc1.shape[0], dsc1.shape[2]
    dev = dsc0.device
    if pair_index is None:
        if planes is not None or out is not None:
            raise ValueError("planes= and out= belong to pair-list mode (pair_index=)")
        if keyframe_index is None:
            assert K == B, "dsc0 and dsc1 hold different batch counts (keyframe mode needs keyframe_index)"
    suffix, maps, rows, P = _row_maps(keyframe_index, pair_index, K, B, dev)
    scores, kp, fin = _outs(out, (P, n0, n1), (want_scores, want_kp and scr0 is not None, want_final and scr0 is not None), dev)
    wq, entry = _DUAL_SOFTMAX[bool(split), bool(split) and planes is not None, suffix]
    # what each work-size query takes after (P, n0, n1); shared: one image set on both sides, its planes are made once
    wq_args = {"mk_dual_softmax_work_floats": (int(scores is None and fin is None),),
               "mk_dual_softmax_split_pairs_work_floats": (K, B, int(dsc0.data_ptr() == dsc1.data_ptr() and n0 == n1 and K == B))}
    work = torch.empty((query(wq, P, n0, n1, *wq_args.get(wq, ())),), device=dev, dtype=torch.float32)
    # (the passes on ready planes take the planes for the descriptors, and no channel count)
    lead, dims = ((planes[0], planes[1]), (P, n0, n1)) if entry == "mk_dual_softmax_split_planes" else ((dsc0, dsc1), (P, C, n0, n1))
    call(entry, ptr(lead[0]), ptr(lead[1]), ptr(scr0), ptr(scr1), 1.0 / float(temperature), int(dustbin is not None),
         float(dustbin) if dustbin is not None else 0.0, ptr(scores), ptr(kp), ptr(fin), ptr(work), *dims, *map(ptr, maps), *rows, stream())
    return scores, kp, fin


def dual_softmax_train_fwd(dsc0, dsc1, scr0, scr1, temperature, dustbin, split):
    """mk_dual_softmax_train (the forward of mickey_amd.train_matcher.dual_softmax_train; arguments validated there) ->
    (final_scores, or scores when scr0 / scr1 are None; lse [B, 2, max(n0, n1)], log2 domain).  dustbin: None or a one-element
    fp32 device tensor, read on the device."""
    B, C, n0 = dsc0.shape
    n1 = dsc1.shape[2]
    dev = dsc0.device
    out = torch.empty((B, n0, n1), device=dev, dtype=torch.float32)
    lse = torch.empty((B, 2, max(n0, n1)), device=dev, dtype=torch.float32)
    work = torch.empty((query("mk_dual_softmax_train_work_floats", B, n0, n1, int(split)),), device=dev, dtype=torch.float32)
    has_kp = scr0 is not None
    call("mk_dual_softmax_train", ptr(dsc0), ptr(dsc1), ptr(scr0), ptr(scr1), 1.0 / float(temperature), ptr(dustbin),
         None if has_kp else ptr(out), None, ptr(out) if has_kp else None, ptr(lse), ptr(work), B, C, n0, n1, int(split), stream())
    return out, lse


def dual_softmax_bwd(dsc0, dsc1, scr0, scr1, temperature, dustbin, lse, G, split, need):
    """mk_dual_softmax_bwd: G = d loss / d (the output of dual_softmax_train_fwd) -> (g_dsc0, g_dsc1, g_scr0, g_scr1, g_dustbin
    [B] per pair); need: five booleans in that order, None where not needed."""
    B, C, n0 = dsc0.shape
    n1 = dsc1.shape[2]
    dev = dsc0.device
    shapes = ((B, C, n0), (B, C, n1), (B, n0), (B, n1), (B,))
    outs = [torch.empty(sh, device=dev, dtype=torch.float32) if want else None for sh, want in zip(shapes, need)]
    work = torch.empty((query("mk_dual_softmax_bwd_work_floats", B, n0, n1, int(split)),), device=dev, dtype=torch.float32)
    call("mk_dual_softmax_bwd", ptr(dsc0), ptr(dsc1), ptr(scr0), ptr(scr1), 1.0 / float(temperature), ptr(dustbin), ptr(lse),
         ptr(G), *[ptr(o) for o in outs], ptr(work), B, C, n0, n1, int(split), stream())
    return tuple(outs)


def sinkhorn(dsc0, dsc1, alpha, iters=10, scr0=None, scr1=None, want_scores=True, want_kp=False, want_final=False,
             keyframe_index=None, pair_index=None, out=None):
    """Returns scores, or (scores, kp_scores, final_scores) when scr0/scr1 are given.  keyframe_index: as in dual_softmax
    (mk_sinkhorn_kf); pair_index and out: as in dual_softmax (mk_sinkhorn_pairs)."""
    _one_mode(keyframe_index, pair_index)
    K, C, n0 = dsc0.shape
    B, n1 = dsc1.shape[0], dsc1.shape[2]
    dev = dsc0.device
    if pair_index is None:
        if out is not None:
            raise ValueError("out= belongs to pair-list mode (pair_index=)")
        if keyframe_index is None:
            assert K == B, "dsc0 and dsc1 hold different batch counts (keyframe mode needs keyframe_index)"
    suffix, maps, rows, P = _row_maps(keyframe_index, pair_index, K, B, dev)
    res, kp, fin = _outs(out, (P, n0, n1), (want_scores, want_kp and scr0 is not None, want_final and scr0 is not None), dev)
    work = torch.empty((query("mk_sinkhorn_work_floats", P, n0, n1),), device=dev, dtype=torch.float32)
    call("mk_sinkhorn" + suffix, ptr(dsc0), ptr(dsc1), ptr(scr0), ptr(scr1), float(alpha), int(iters), ptr(res), ptr(kp), ptr(fin),
         ptr(work), P, C, n0, n1, *map(ptr, maps), *rows, stream())
    return res if scr0 is None else (res, kp, fin)


def mutual_nn(scores):
    """Batched get_matches_list: returns (matches int32 [B, n0, 2], count int32 [B])."""
    _chk(scores, torch.float32)
    B, n0, n1 = scores.shape
    dev = scores.device
    matches = torch.zeros((B, n0, 2), device=dev, dtype=torch.int32)
    count = torch.zeros((B,), device=dev, dtype=torch.int32)
    work = torch.empty((2 * B * (n0 + n1),), device=dev, dtype=torch.int32)
    call("mk_mutual_nn", ptr(scores), ptr(matches), ptr(count), ptr(work), B, n0, n1, stream())
    return matches, count


# ---- solver ---------------------------------------------------------------------------------------

def counter_add(counter, inc):
    """counter (int64 CUDA tensor, 1 element) += inc on the current stream (see mk_counter_add)."""
    call("mk_counter_add", ptr(counter), int(inc), stream())


def dev_mfma_sustained(device, iters=400000, zero_operands=False, workgroups=None):
    """Measurement probe (mickey_hip_dev.h: mk_dev_mfma_sustained): TFLOP/s of back-to-back v_mfma_f32_16x16x32 (bf16) on
    register-resident operands, one 8-wave workgroup per CU, one warm launch + one timed launch (HIP events).  Not product code."""
    wg = workgroups or torch.cuda.get_device_properties(device).multi_processor_count
    scratch = torch.empty((wg * 512,), device=device, dtype=torch.float32)
    call("mk_dev_mfma_sustained", ptr(scratch), wg, max(1, iters // 8), int(zero_operands), stream())
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call("mk_dev_mfma_sustained", ptr(scratch), wg, iters, int(zero_operands), stream())
    e1.record()
    e1.synchronize()
    return wg * iters * 1048576.0 / (e0.elapsed_time(e1) * 1e-3) / 1e12


def exprace_work(B, rows_per_pair, k, ncell, device):
    """Workspace of mk_exprace_topk with its self-cleaning state zeroed (mickey_hip.h): allocate ONCE per shape and stream and
    hand it to every exprace_topk call -- a call leaves the state zero, so no zero-fill launch stands in front of the chain."""
    work = torch.empty((query("mk_exprace_topk_work_bytes", B, rows_per_pair, k, ncell),), device=device, dtype=torch.uint8)
    work[:query("mk_exprace_topk_state_bytes", B, rows_per_pair)].zero_()
    return work


def exprace_topk(p, rows_per_pair, k, noise=None, seed=0, offset=0, invalid=None, offset_dev=None, pair_base=0, work=None):
    """p fp32 [B, ncell] -> (idx int32 [B*rows_per_pair, k], cnt int32 [B*rows_per_pair]).  work: exprace_work(...) kept by the
    caller across calls (None: allocated and zeroed here -- one more launch).  A call that raises zeroes the state of `work`
    before the error propagates: the chain may have stopped between its launches (mickey_hip.h)."""
    p, noise = _c(p, noise)
    _chk(p, torch.float32)
    B, ncell = p.shape
    dev = p.device
    idx = torch.empty((B * rows_per_pair, k), device=dev, dtype=torch.int32)
    cnt = torch.empty((B * rows_per_pair,), device=dev, dtype=torch.int32)
    if work is None:
        work = exprace_work(B, rows_per_pair, k, ncell, dev)
    assert work.numel() >= query("mk_exprace_topk_work_bytes", B, rows_per_pair, k, ncell)
    try:
        call("mk_exprace_topk", ptr(p), ptr(noise), int(seed), int(offset), ptr(offset_dev), ptr(idx), ptr(cnt), ptr(invalid),
             ptr(work), B, rows_per_pair, ncell, k, int(pair_base), stream())
    except Exception:
        work[:query("mk_exprace_topk_state_bytes", B, rows_per_pair)].zero_()
        raise
    return idx, cnt


def _c(*ts):
    """Device pointers are handed to C with implied dense row-major strides: normalise views."""
    return [None if t is None else t.contiguous() for t in ts]


def gather_backproject(idx, final_scores, kps0, depth0, kps1, depth1, K0, K1, rows_per_pair, keyframe_index=None, pair_index=None):
    """keyframe_index (keyframe mode, mk_gather_backproject_kf): kps0 / depth0 hold the K keyframes, pair b reads row
    keyframe_index[b]; K0 stays per pair.  pair_index (pair-list mode, mk_gather_backproject_pairs; forms as in dual_softmax):
    kps0 / depth0 hold N0 images and kps1 / depth1 N1, pair p reads rows pair_index[p]; K0, K1 stay per pair."""
    _one_mode(keyframe_index, pair_index)
    idx, final_scores, kps0, depth0, kps1, depth1, K0, K1 = _c(idx, final_scores, kps0, depth0, kps1, depth1, K0, K1)
    B, n0, n1 = final_scores.shape
    R, k = idx.shape
    dev = idx.device
    suffix, maps, rows, _ = _row_maps(keyframe_index, pair_index, kps0.shape[0], kps1.shape[0], dev, P=B)
    X = torch.empty((R, k, 3), device=dev, dtype=torch.float32)
    Y = torch.empty((R, k, 3), device=dev, dtype=torch.float32)
    wts = torch.empty((R, k), device=dev, dtype=torch.float32)
    corr = torch.empty((R, k, 6), device=dev, dtype=torch.float32)
    call("mk_gather_backproject" + suffix, ptr(idx), ptr(final_scores), ptr(kps0), ptr(depth0), ptr(kps1), ptr(depth1), ptr(K0), ptr(K1),
         ptr(X), ptr(Y), ptr(wts), ptr(corr), B, rows_per_pair, k, n0, n1, *map(ptr, maps), *rows, stream())
    return X, Y, wts, corr


def ransac_hypotheses(X, Y, wts, it_ransac, th_soft, noise3=None, idx3_in=None, seed=0, offset=0, offset_dev=None, set_base=0):
    X, Y, wts, noise3, idx3_in = _c(X, Y, wts, noise3, idx3_in)
    nsets, k, _ = X.shape
    dev = X.device
    nh = nsets * it_ransac
    Rh = torch.empty((nh, 9), device=dev, dtype=torch.float32)
    th = torch.empty((nh, 3), device=dev, dtype=torch.float32)
    score = torch.empty((nh,), device=dev, dtype=torch.float32)
    idx3 = torch.empty((nh, 3), device=dev, dtype=torch.int32)
    call("mk_ransac_hypotheses", ptr(X), ptr(Y), ptr(wts), ptr(noise3), ptr(idx3_in), int(seed), int(offset), ptr(offset_dev),
         float(th_soft), ptr(Rh), ptr(th), ptr(score), ptr(idx3), nsets, it_ransac, k, int(set_base), stream())
    return Rh, th, score, idx3


def train_ransac_masks(X, Y, wts, it_ransac, th_ref, num_ref, num_corr, noise=None, idx_in=None, seed=0, offset=0,
                       offset_dev=None, set_base=0):
    """Training-time hypotheses + refinement (reference loss_class.py:141-184): X, Y [nsets, S, 3], wts [nsets, S] ->
    (inliers_final fp32 [nsets*it_ransac, S], drawn indices int32 [nsets*it_ransac, num_corr], rounds int32)."""
    X, Y, wts, noise, idx_in = _c(X, Y, wts, noise, idx_in)
    _chk(X, torch.float32)
    nsets, S, _ = X.shape
    dev = X.device
    nh = nsets * it_ransac
    if idx_in is not None:
        idx_in = idx_in.to(torch.int32)
    mask = torch.empty((nh, S), device=dev, dtype=torch.float32)
    idx = torch.empty((nh, num_corr), device=dev, dtype=torch.int32)
    rounds = torch.empty((nh,), device=dev, dtype=torch.int32)
    call("mk_train_ransac_masks", ptr(X), ptr(Y), ptr(wts), ptr(noise), ptr(idx_in), int(seed), int(offset), ptr(offset_dev),
         float(th_ref), int(num_ref), int(num_corr), ptr(mask), ptr(idx), ptr(rounds), nsets, it_ransac, S, int(set_base),
         stream())
    return mask, idx, rounds


def reinforce_scatter(idx, loss_value, B, it_matches, ncell):
    """REINFORCE bookkeeping (reference loss_class.py:251-261): idx int32 [B*it_matches, S], loss_value fp32 [B*it_matches]
    -> (gradients, gradients_b) fp32 [B, ncell]."""
    idx, loss_value = _c(idx.to(torch.int32), loss_value.to(torch.float32))
    S = idx.shape[1]
    dev = idx.device
    grads = torch.zeros((B, ncell), device=dev, dtype=torch.float32)
    grads_b = torch.zeros((B, ncell), device=dev, dtype=torch.float32)
    call("mk_reinforce_scatter", ptr(idx), ptr(loss_value), ptr(grads), ptr(grads_b), B, it_matches, S, ncell, stream())
    return grads, grads_b

def train_tail_fwd(X, Y, mask, Rgt, tgt, K0, K1, it_ransac, it_matches, th_soft, loss_type, soft_clip, img_h=720.0):
    """Forward of the differentiable RANSAC tail (mk_train_tail_fwd): -> (out [nhyp, 4], Rt [nhyp, 12], saved [nhyp, 32])."""
    X, Y, mask, Rgt, tgt, K0, K1 = _c(X, Y, mask, Rgt, tgt, K0, K1)
    nsets, S, _ = X.shape
    nh = nsets * it_ransac
    dev = X.device
    out = torch.empty((nh, 4), device=dev, dtype=torch.float32)
    Rt = torch.empty((nh, 12), device=dev, dtype=torch.float32)
    saved = torch.zeros((nh, 32), device=dev, dtype=torch.float32)
    call("mk_train_tail_fwd", ptr(X), ptr(Y), ptr(mask), ptr(Rgt), ptr(tgt), ptr(K0), ptr(K1), nsets, it_ransac, S, it_matches,
         float(th_soft), int(loss_type), int(soft_clip), float(img_h), ptr(out), ptr(Rt), ptr(saved), stream())
    return out, Rt, saved


def train_tail_bwd(X, Y, mask, Rgt, tgt, K0, K1, it_ransac, it_matches, th_soft, loss_type, soft_clip, Rt, saved, grad_out,
                   img_h=720.0):
    """Backward of the same (mk_train_tail_bwd): grad_out [nhyp, 2] = dL/d(loss_value, score) -> (dL/dX, dL/dY) [nsets, S, 3]."""
    X, Y, mask, Rgt, tgt, K0, K1, grad_out = _c(X, Y, mask, Rgt, tgt, K0, K1, grad_out)
    nsets, S, _ = X.shape
    dev = X.device
    work = torch.empty((nsets * it_ransac, 16), device=dev, dtype=torch.float32)
    gX, gY = torch.empty_like(X), torch.empty_like(Y)
    call("mk_train_tail_bwd", ptr(X), ptr(Y), ptr(mask), ptr(Rgt), ptr(tgt), ptr(K0), ptr(K1), nsets, it_ransac, S, it_matches,
         float(th_soft), int(loss_type), int(soft_clip), float(img_h), ptr(Rt), ptr(saved), ptr(grad_out), ptr(work), ptr(gX),
         ptr(gY), stream())
    return gX, gY


def train_aggregate_fwd(out, Rt, saved, B, it_matches, it_ransac, temperature, add_null, null_loss, null_score):
    """mk_train_aggregate_fwd: -> (loss_value [B*it_matches], per_pair [B, 3] = sums of (loss_value, rot, trans) over a pair's sets,
    coef [nhyp, 2] for the backward, flags int32 [2] = (any non-finite R / t, number of rank-one hypotheses))."""
    out, Rt, saved = _c(out, Rt, saved)
    dev = out.device
    loss_value = torch.empty((B * it_matches,), device=dev, dtype=torch.float32)
    per_pair = torch.empty((B, 3), device=dev, dtype=torch.float32)
    coef = torch.empty((B * it_matches * it_ransac, 2), device=dev, dtype=torch.float32)
    flags = torch.zeros((2,), device=dev, dtype=torch.int32)
    call("mk_train_aggregate_fwd", ptr(out), ptr(Rt), ptr(saved), B, it_matches, it_ransac, float(temperature), int(bool(add_null)),
         float(null_loss), float(null_score), ptr(loss_value), ptr(per_pair), ptr(coef), ptr(flags), stream())
    return loss_value, per_pair, coef, flags


def train_aggregate_bwd(coef, g_pair, B, it_matches, it_ransac):
    """mk_train_aggregate_bwd: dL/d(pair baseline) [B] -> dL/d(loss_k, score_k) [nhyp, 2] (the grad_out of train_tail_bwd)."""
    coef, g_pair = _c(coef, g_pair.float())
    g = torch.empty_like(coef)
    call("mk_train_aggregate_bwd", ptr(coef), ptr(g_pair), B, it_matches, it_ransac, ptr(g), stream())
    return g


def gather_backproject_bwd(idx, corr, gX, gY, K0, K1, B, rows_per_pair, n0, n1):
    """mk_gather_backproject_bwd: dL/dX, dL/dY [B*rows_per_pair, k, 3] -> (dL/dkps0 [B,2,n0], dL/ddepth0 [B,1,n0], dL/dkps1, dL/ddepth1)."""
    idx, corr, gX, gY, K0, K1 = _c(idx, corr, gX, gY, K0, K1)
    k = idx.shape[1]
    buf = torch.zeros((B * 3 * (n0 + n1),), device=idx.device, dtype=torch.float32)   # one zero-fill for the four accumulators
    gk0, gd0 = buf[:2 * B * n0].view(B, 2, n0), buf[2 * B * n0:3 * B * n0].view(B, 1, n0)
    o = 3 * B * n0
    gk1, gd1 = buf[o:o + 2 * B * n1].view(B, 2, n1), buf[o + 2 * B * n1:].view(B, 1, n1)
    call("mk_gather_backproject_bwd", ptr(idx), ptr(corr), ptr(gX), ptr(gY), ptr(K0), ptr(K1), ptr(gk0), ptr(gd0), ptr(gk1), ptr(gd1),
         B, rows_per_pair, k, n0, n1, stream())
    return gk0, gd0, gk1, gd1


def pose_finalize(R, t, conf, invalid):
    """mk_pose_finalize: the batch-level invalid rule -- every pose of R [B, 3, 3], t [B, 1, 3], conf [B, 1] is zeroed in place
    when the word `invalid` is set."""
    call("mk_pose_finalize", ptr(R), ptr(t), ptr(conf), ptr(invalid), R.shape[0], stream())


def refine_pose(X, Y, Rh, th, score, B, it_matches, it_ransac, th_inlier, num_ref, min_inliers, invalid=None, finalize=True):
    """finalize=False leaves mk_pose_finalize to the caller (a forward that solves its pairs in chunks applies the batch-level
    invalid rule once, over all of them: pose_finalize)."""
    X, Y, Rh, th, score = _c(X, Y, Rh, th, score)
    k = X.shape[1]
    dev = X.device
    R = torch.empty((B, 3, 3), device=dev, dtype=torch.float32)
    t = torch.empty((B, 1, 3), device=dev, dtype=torch.float32)
    conf = torch.empty((B, 1), device=dev, dtype=torch.float32)
    best = torch.empty((B,), device=dev, dtype=torch.int32)
    mask = torch.empty((B, k), device=dev, dtype=torch.uint8)
    rounds = torch.empty((B,), device=dev, dtype=torch.int32)
    if invalid is None:
        invalid = torch.zeros((1,), device=dev, dtype=torch.int32)
    call("mk_refine_pose", ptr(X), ptr(Y), ptr(Rh), ptr(th), ptr(score), float(th_inlier), int(num_ref), int(min_inliers),
         ptr(R), ptr(t), ptr(conf), ptr(best), ptr(mask), ptr(rounds), ptr(invalid), B, it_matches, it_ransac, k, stream())
    if finalize:
        call("mk_pose_finalize", ptr(R), ptr(t), ptr(conf), ptr(invalid), B, stream())
    return R, t, conf, best, mask, rounds, invalid


def pose_metrics(R, t, T_gt, K, conf, W, H, records, row0=0):
    """mk_pose_metrics: the records of the B pairs of R [B, 3, 3], t [B, 1, 3], T_gt [B, 4, 4], K [B, 3, 3], conf [B] (or None) into
    rows row0 .. row0 + B of records fp32 [capacity, 8] (in place; returns records)."""
    R, t, T_gt, K, conf = _c(R, t, T_gt, K, conf)
    _chk(records, torch.float32)
    call("mk_pose_metrics", ptr(R), ptr(t), ptr(T_gt), ptr(K), ptr(conf), float(W), float(H), ptr(records), int(row0),
         int(R.shape[0]), int(records.shape[0]), stream())
    return records


def pose_summary_tile():
    """Records of an LDS tile of mk_pose_summary's ranking launch."""
    return int(query("mk_pose_summary_tile"))


def pose_summary(records, N, failures, thresholds, losses=None, S=0, out=None, work=None):
    """mk_pose_summary over the first N rows of records fp32 [*, 8] (and the first S rows of losses fp32 [*, 3], or None) ->
    (out fp32 [16], work fp64 [ceil(N / tile) + 1, 16]: the partial rows, then the 16 results before their rounding)."""
    _chk(records, torch.float32)
    dev = records.device
    if losses is not None:
        _chk(losses, torch.float32)
    if out is None:
        out = torch.empty((16,), device=dev, dtype=torch.float32)
    if work is None:
        work = torch.empty((int(query("mk_pose_summary_work_doubles", int(N))) // 16, 16), device=dev, dtype=torch.float64)
    th = [float(v) for v in thresholds]
    call("mk_pose_summary", ptr(records), int(N), int(failures), th[0], th[1], th[2], th[3], th[4], ptr(losses), int(S), ptr(out),
         ptr(work), stream())
    return out, work
