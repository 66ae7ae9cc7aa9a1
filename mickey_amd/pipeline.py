"""Host-side orchestration of the HIP kernels for the MicKey hot path: which kernel runs on which
buffer, in which order.  All arithmetic is in libmickey_hip.so; torch provides device memory and
the stream only.  Mirrors (file:line under the reference):
  encoder   DINO_modules/dinov2.py:191-236, layers/block.py:105-106
  heads     mickey_extractor.py:53-58,126-140,166-178,202-218,237-251
  matcher   compute_correspondences.py:52-92, compute_pose.py:23
  solver    utils/probabilisticProcrustes.py:183-348
"""
import torch

from . import ops
from . import weights as wts_mod


class Workspace:
    """Per-shape device buffers, allocated once and reused across forward calls."""

    def __init__(self):
        self.bufs = {}
        self.sat_flag = None   # split-operand heads: the int32 [1] device word the plane-writing kernels report saturation into

    def get_planes(self, name, shape, device, zero=False):
        """(hi, lo) fp16 planes of a split-operand activation: the two halves of ONE buffer (the kernels address both planes of
        a source from one base pointer, mickey_hip.h)."""
        t = self.get(name, (2,) + tuple(shape), torch.float16, device, zero=zero)
        return t[0], t[1]

    def get(self, name, shape, dtype, device, zero=False):
        key = (name, tuple(shape), dtype)
        t = self.bufs.get(key)
        if t is None or t.device != device:
            t = (torch.zeros if zero else torch.empty)(tuple(shape), dtype=dtype, device=device)
            self.bufs[key] = t
        return t


def _encoder_trunk(W, ws, img):
    """Everything of the encoder up to its final norm (shared by encoder_forward and encoder_features: the same launches in
    the same order on the same workspace buffers).  -> (x fp32 [nimg * ntok, D] (a workspace buffer), nimg, gh, gw)."""
    imgs = list(img) if isinstance(img, (list, tuple)) else [img]
    img = imgs[0]
    dev, lp = img.device, W.lp
    _, _, H, Wd = img.shape
    assert all(t.shape[1:] == img.shape[1:] for t in imgs)
    nimg = sum(t.shape[0] for t in imgs)
    gh, gw = H // 14, Wd // 14
    npatch, D, heads = gh * gw, W.D, W.heads
    ntok = npatch + 1
    pad = (ntok + 63) // 64 * 64
    M = nimg * ntok
    pos = wts_mod.interp_pos_embed(W, gh, gw, dev)
    a = ws.get("im2col", (nimg * npatch, wts_mod.PATCH_K), lp, dev)
    r0 = 0
    for t in imgs:
        ops.im2col_patch14(t, gh, gw, wts_mod.PATCH_K, lp, out=a[r0:r0 + t.shape[0] * npatch])
        r0 += t.shape[0] * npatch
    x = ws.get("x", (M, D), torch.float32, dev)
    att = ws.get("att", (M, D), lp, dev)
    hid = ws.get("hid", (M, 4 * D), lp, dev)
    q = ws.get("q", (nimg, heads, pad, 64), lp, dev, zero=True)   # pad rows stay zero forever
    k = ws.get("k", (nimg, heads, pad, 64), lp, dev, zero=True)
    vt = ws.get("vt", (nimg, heads, 64, pad), lp, dev, zero=True)
    if getattr(W, "ln_fold", False):
        # norm1 / norm2 folded into the GEMMs around them (mickey_hip.h, mk_gemm_*_ln): the residual stream lives as two
        # 16-bit planes (x = xh + xl); whoever writes it also writes per-slot row statistics; qkv / fc1 read xh (raw) and
        # normalise in their epilogue.  The last block writes fp32 rows for the final norm.
        xh = ws.get("xh", (M, D), lp, dev)
        xl = ws.get("xl", (M, D), lp, dev)
        st = ws.get("ln_stats", (M, D // 64, 2), torch.float32, dev)
        # row centring (mickey_hip.h): every consumer publishes the rows' means, the producer after it takes them off -- the
        # stream stays centred (LayerNorm, its only reader, cannot tell), so the raw hi plane rounds x - mean, not x
        sh = ws.get("ln_shift", (M,), torch.float32, dev) if getattr(W, "ln_centre", True) else None
        ops.gemm_patch_embed_ln(a, W.patch_w, W.patch_b, pos, xh, xl, st, nimg, npatch)
        ops.cls_token_ln(W.cls, pos, xh, xl, st, nimg, ntok, D)
        if sh is not None:
            ops.recentre_split(xh, xl, st)   # the first consumer (qkv of block 0) meets centred rows too
        last = len(W.blocks) - 1
        for bi, blk in enumerate(W.blocks):
            ops.gemm_qkv_ln(xh, blk.qkv_wf, blk.qkv_bf, blk.qkv_cs, st, 1e-6, q, k, vt, nimg, ntok, pad, heads, shift_out=sh)
            ops.flash_attn(q, k, vt, att, nimg, heads, ntok, pad)
            ops.gemm_ls_residual_ln(att, blk.proj_w, blk.proj_b, blk.g1, xh, xl, st, shift=sh)
            ops.gemm_ln(xh, blk.fc1_wf, blk.fc1_bf, blk.fc1_cs, st, 1e-6, act=ops.ACT_GELU, out=hid, shift_out=sh)
            ops.gemm_ls_residual_ln(hid, blk.fc2_w, blk.fc2_b, blk.g2, xh, xl, st, x_out=x if bi == last else None, shift=sh)
    else:
        ops.gemm_patch_embed(a, W.patch_w, W.patch_b, pos, x, nimg, npatch)
        ops.cls_token(W.cls, pos, x, nimg, ntok, D)
        y = ws.get("y", (M, D), lp, dev)
        for blk in W.blocks:
            ops.layernorm(x, blk.n1w, blk.n1b, 1e-6, out=y)
            ops.gemm_qkv(y, blk.qkv_w, blk.qkv_b, q, k, vt, nimg, ntok, pad, heads)
            ops.flash_attn(q, k, vt, att, nimg, heads, ntok, pad)
            ops.gemm_ls_residual(att, blk.proj_w, blk.proj_b, blk.g1, x)
            ops.layernorm(x, blk.n2w, blk.n2b, 1e-6, out=y)
            ops.gemm(y, blk.fc1_w, blk.fc1_b, act=ops.ACT_GELU, out=hid)
            ops.gemm_ls_residual(hid, blk.fc2_w, blk.fc2_b, blk.g2, x)
    return x, nimg, gh, gw


def encoder_forward(W, ws, img):
    """img fp32 [nimg, 3, H, W] on device (already cropped view or not: the /14 crop is implicit in
    gh, gw), or a sequence of such tensors of one H x W (the two image sets of a pair batch: patched straight into one
    token matrix, no concatenated copy of the images).  Returns the final-norm patch tokens, lp, as a bordered feature map
    of nimg gh x gw grids."""
    x, nimg, gh, gw = _encoder_trunk(W, ws, img)
    dev, D = x.device, W.D
    npatch = gh * gw
    ntok = npatch + 1
    # the heads' operand type, as a BORDERED feature map (mickey_hip.h: what a 3x3 conv reads; border rows stay zero)
    # (bordered buffers are zeroed ONCE and only their pixel rows are ever written: the key carries the geometry, because two
    # geometries can share a row count while their border rows sit elsewhere)
    R = ops.bordered_rows(nimg, gh, gw)
    if W.heads_split:
        # split-operand heads: the final norm writes the convs' (hi, lo) fp16 operand planes directly (no fp32 feature map).
        # features_lp (AMD.FEATURES_LP; automatic behind an fp16 encoder): the reference's heads receive what its fp16 encoder
        # returns -- fp16 values, widened exactly by .float() (mickey_extractor.py:49-52) -- so only the hi plane is written (the rows
        # rounded to fp16) and the lo plane of this buffer, zeroed at allocation, stays zero: the first conv of every head then runs
        # two products instead of three (heads_forward)
        flp = W.features_lp
        feat = ws.get_planes("feat_hl%s_%d_%d_%d" % ("_lp" if flp else "", nimg, gh, gw), (R, D), dev, zero=True)
    else:
        feat = ws.get("feat_%d_%d_%d" % (nimg, gh, gw), (R, D), W.lp_heads, dev, zero=True)
    hi_only = W.heads_split and W.features_lp
    ops.layernorm(x, W.norm_w, W.norm_b, 1e-6, out=(feat[0], None) if hi_only else feat, rows_out=nimg * npatch, rows_per_img=ntok, skip=1,
                  bordered=(nimg, gh, gw), sat=ws.sat_flag)
    return feat, gh, gw


def encoder_features(W, ws, img, round_fp16=False):
    """The encoder for a torch consumer (the reference's trainable Conv2d heads in a training step, mickey_amd.train_encoder):
    the trunk of encoder_forward, then the final norm written channel-major by mk_layernorm_nchw.  img as encoder_forward takes
    it.  Returns fp32 [nimg, D, gh, gw] -- the values of dinov2.py:230-233 x_norm_patchtokens after
    mickey_extractor.py:49-52's permute / reshape / float(); round_fp16: rounded to fp16 on the way (what an fp16 encoder hands
    over).  The result is a FRESH tensor on every call, never a workspace buffer: a training step holds image 0's features while
    image 1 is encoded, and autograd holds both until the heads' backward."""
    x, nimg, gh, gw = _encoder_trunk(W, ws, img)
    npatch = gh * gw
    out = torch.empty((nimg, W.D, gh, gw), dtype=torch.float32, device=x.device)
    ops.layernorm_nchw(x, W.norm_w, W.norm_b, 1e-6, nimg, npatch, rows_per_img=npatch + 1, skip=1, round_fp16=bool(round_fp16), out=out)
    return out


# ---- the heads ("The heads' host code": what an activation is, the stride rules of the helpers, the launch record) ----
def _t(x):   # the tensor that carries the shape and strides of an activation (a tensor, or the (hi, lo) pair of its fp16 planes)
    return x[0] if isinstance(x, tuple) else x


def _sub(x, idx):   # x[idx] of an activation (of both planes)
    return tuple(p[idx] for p in x) if isinstance(x, tuple) else x[idx]


def _wscale(w):   # power-of-two scale of a split weight tensor's planes (set by weights.prepare on the tensor object)
    if getattr(w, "mk_scale", None) is None:
        raise RuntimeError("split-operand weight without its plane scale: the tensor is not the one weights.prepare made "
                           "(copied / moved weights must be re-prepared)")
    return w.mk_scale


def _bordered(W, ws, name, lead, C, grid, dev):
    """A bordered activation [*lead, bordered_rows, C] for a 3x3 conv to read (zeroed once; its key carries the geometry)."""
    shape, geo = tuple(lead) + (ops.bordered_rows(*grid), C), "_%d_%d_%d" % grid
    if W.heads_split:
        return ws.get_planes(name + "_hl" + geo, shape, dev, zero=True)
    return ws.get(name + geo, shape, W.lp_heads, dev, zero=True)


def _conv(x, w, bias, out, grid, act, short=None, has_sc=True, either=False, bordered=False, sat=None):
    """One 3x3 conv launch on grid = (nimg, gh, gw): out = act(conv(x, w) + bias + shortcut), out bordered or dense rows.
    short: the block input, carried by shortcut columns of w (has_sc: as in2) or added as it is (resid); either: a block that
    exists in both forms states the shortcut's stride for both."""
    def gs(t, grouped=3):   # [groups, rows, cols] (bias: [groups, cols]): .stride(0); no group dimension: 0 = shared by all groups
        return t.stride(0) if t is not None and t.dim() == grouped else 0
    xt, st = _t(x), _t(short)
    kw = dict(act=act, stride_in1=gs(xt), stride_w=gs(w), stride_bias=gs(bias, 2), stride_out=gs(_t(out)), out_bordered=bordered)
    if short is not None:
        kw.update(in2=short if has_sc else None, C2=st.shape[-1], stride_in2=gs(st))
    args = (xt.shape[-1], w, bias, out, w.shape[-2], w.shape[0] if w.dim() == 3 else 1) + tuple(grid)
    if isinstance(x, tuple):
        return ops.conv3x3_split(x, *args, w_scale=_wscale(w), sat=sat, **kw)
    if either:
        kw.update(resid=None if has_sc else short, stride_resid=gs(st))
    return ops.conv3x3(x, *args, **kw)


def _basic_block(x, blk, h, out, grid, sat, act=ops.ACT_RELU, bordered=False, hi_only=False, rb4=False):
    """BasicBlock (BatchNorm folded): conv -> ReLU -> h (bordered) -> conv + shortcut of x -> act -> out.  In split mode the
    epilogues write the next conv's operand planes directly (no fp32 round trip, no mk_split_planes pass).  hi_only: x's lo
    plane is identically zero -- the first conv reads the hi plane alone, two products instead of three.  rb4: shortcut columns
    or an identity shortcut by the checkpoint (blk.has_sc), and an fp32 output in front of the tails: no saturation word."""
    _conv((x[0], None) if hi_only else x, blk.w1, blk.b1, h, grid, ops.ACT_RELU, bordered=True, sat=sat)
    return _conv(h, blk.w2, blk.b2, out, grid, act, short=x, has_sc=blk.has_sc if rb4 else True, either=rb4, bordered=bordered,
                 sat=None if rb4 else sat)


def _linear(a, w, out, act=ops.ACT_NONE, sat=None):
    """out[g] = act(a[g] @ w[g]^T): a [G, M, K] (a column block of wider rows: its own row stride and pointer), w [G, N, K]
    (split: 2 K interleaved (hi | lo) columns, weights.split_conv_weight), out [G, M, N]; a / out tensors or plane pairs."""
    at, ot = _t(a), _t(out)
    G, M, N = at.shape[0], at.shape[1], w.shape[1]
    if isinstance(a, tuple):
        return ops.gemm_grouped_split(a, w, None, out, G, M, N, w.shape[2] // 2, at.stride(1), ot.stride(1), at.stride(0),
                                      w.stride(0), 0, ot.stride(0), act=act, w_scale=_wscale(w), sat=sat)
    return ops.gemm_grouped(a, w, None, out, G, M, N, w.shape[2], at.stride(1), w.stride(1), ot.stride(1), at.stride(0),
                            w.stride(0), 0, ot.stride(0), act=act)


def _conv_stack(W, ws, feat, grid):
    """resblock1-3 of the four heads (groups: det_head, det_offset, depth_head, dsc_head), all reading one feature map.
    -> dense rows [4, nimg * gh * gw, C] of the heads' type: what the row-wise attention kernels read."""
    x, dev, last = feat, _t(feat).device, len(W.rb) - 1
    for bi, rb in enumerate(W.rb):
        G, co = rb.w1.shape[:2]
        h = _bordered(W, ws, "rb%d_h" % bi, (G,), co, grid, dev)
        out = _bordered(W, ws, "rb%d_x" % bi, (G,), co, grid, dev) if bi < last else \
            ws.get("rb%d_x_%d_%d_%d" % ((bi,) + grid), (G, grid[0] * grid[1] * grid[2], co), W.lp_heads, dev)
        x = _basic_block(x, rb, h, out, grid, ws.sat_flag, bordered=bi < last, hi_only=bi == 0 and W.features_lp)
    return x


def _position_encoding(W, ws, x, grid, cfg):
    """x [G, M, C] -> (xs fp32 [G, M, C]: the layers' residual stream, cat lp [G, M, 2C]: x (+ pe) in its left half).  The
    keypoint heads (groups 0-2) and the descriptor head take the sine table or not by their own switches: two launches then."""
    G, M, C = x.shape
    xs = ws.get("att_xs", (G, M, C), torch.float32, x.device)
    cat = ws.get("att_cat", (G, M, 2 * C), W.lp_heads, x.device)
    pe = wts_mod.sine_pos_table(W, C, grid[1], grid[2], x.device)
    kp_pe, dsc_pe = bool(cfg["MICKEY"]["KP_HEADS"]["POS_ENCODING"]), bool(cfg["MICKEY"]["DSC_HEAD"]["POS_ENCODING"])
    for sl, on in [(slice(None), kp_pe)] if kp_pe == dsc_pe else [(slice(0, 3), kp_pe), (slice(3, None), dsc_pe)]:
        ops.posenc_add(x[sl], pe if on else None, xs[sl], cat[sl], x[sl].shape[0], grid[0], pe.shape[0], C)
    return xs, cat


def _attention_layers(W, ws, xs, cat, grid, cfg):
    """Transformer_self_att: the linear-attention encoder layers, residual stream xs in fp32.  -> the bordered activation
    [G, bordered_rows, C] that resblock4's convs read, written by the last layer's closing LayerNorm."""
    nimg, L = grid[0], grid[1] * grid[2]
    G, M, C = xs.shape
    dev, lp, split, sat = xs.device, W.lp_heads, W.heads_split, ws.sat_flag
    left, right = (Ellipsis, slice(0, C)), (Ellipsis, slice(C, None))   # cat's column halves: the layer input | norm1(message)
    # 16-bit operands: Linear(-> 128) + LayerNorm (+ residual) in one pass (mk_gemm_ln128), and with AMD.LINATTN_FUSED q | k | v are
    # projected inside the attention kernels (no fp32 qkv rows, no msg rows); off = the separate launches, the same bits (A/B runs)
    ln128 = not split and C == 128 and lp != torch.float32
    fused = ln128 and bool(cfg["AMD"].get("LINATTN_FUSED", True))
    kv = ws.get("att_kv", (G * nimg * (C // 16), 272), torch.float32, dev)
    kvw = ws.get("att_kvw", (ops.linattn_work_floats(G, nimg, L, C),), torch.float32, dev)
    qkv, msg = (None, None) if fused else (ws.get("att_qkv", (G, M, 3 * C), torch.float32, dev), ws.get("att_msg", (G, M, C), lp, dev))
    mrg, hid = ws.get("att_mrg", (G, M, C), torch.float32, dev), ws.get("att_hid", (G, M, 2 * C), lp, dev)
    out = _bordered(W, ws, "att_out", (G,), C, grid, dev)
    # c, m, h: the operand forms of cat / msg / hid.  split: the layers' small linears on split operands too (fp32 MFMA: 4.9 ms per
    # 32 pairs; split: the conversions below + 12 HBM-bound GEMMs) -- planes of `cat` (its two column halves are rewritten at
    # different times), of `msg`, and `hid` written as planes by the GEMM that produces it
    c, m, h = cat, msg, hid
    if split:
        c, m, h = (ws.get_planes("att_%s_hl" % nm, t.shape, dev) for nm, t in (("cat", cat), ("msg", msg), ("hid", hid)))
    for li, lay in enumerate(W.att):
        if fused:
            ops.linattn_kv_fused(cat, lay.qkv_w, kv, kvw, G, nimg, L, C)
            ops.linattn_apply_fused(cat, lay.qkv_w, kv, cat[right], G, nimg, L, C, merge_w=lay.merge_w, ln_w=lay.n1w, ln_b=lay.n1b)
        else:   # the separate launches; split: the same on plane operands, behind a conversion of what an fp32 kernel wrote
            if split and li == 0:   # (later layers: the previous layer's closing LayerNorm wrote these planes)
                ops.split_planes(cat[left], *_sub(c, left), sat=sat)
            _linear(_sub(c, left), lay.qkv_w, qkv, sat=sat)
            ops.linattn_kv(qkv, kv, kvw, G, nimg, L, C)
            ops.linattn_apply(qkv, kv, msg, msg.stride(1), G, nimg, L, C)
            if split:
                ops.split_planes(msg, *m, sat=sat)
            if ln128:
                ops.gemm_ln128(msg, lay.merge_w, lay.n1w, lay.n1b, 1e-5, cat[right], G, M, msg.shape[-1])
            else:
                _linear(m, lay.merge_w, mrg, sat=sat)
                ops.layernorm(mrg, lay.n1w, lay.n1b, 1e-5, out=_sub(c, right), wgroup_rows=M, sat=sat)
        _linear(c, lay.mlp0_w, h, act=ops.ACT_RELU, sat=sat)
        # mlp[2] + norm2 + the layer's residual -> the next layer's input columns, or (last) resblock4's bordered input
        o2, border = (out, grid) if li == len(W.att) - 1 else (_sub(c, left), None)
        if ln128:
            ops.gemm_ln128(hid, lay.mlp2_w, lay.n2w, lay.n2b, 1e-5, o2, G, M, hid.shape[-1], resid=xs, bordered=border)
        else:
            _linear(h, lay.mlp2_w, mrg, sat=sat)
            ops.layernorm(mrg, lay.n2w, lay.n2b, 1e-5, out=o2, resid=xs, wgroup_rows=M, bordered=border, sat=sat)
    return out


def _resblock4(W, ws, x, grid):
    """x: bordered [4, bordered_rows, C].  The three keypoint heads as one grouped block and the descriptor head as an ungrouped
    one (no ReLU behind it: relu=False, mickey_extractor.py:246) -> fp32 dense rows f4 [3, M, ck], fd [M, cd]."""
    kpw, dw, dev = W.rb4_kp, W.rb4_dsc, _t(x).device
    assert not W.heads_split or (kpw.has_sc and dw.has_sc)   # (weights.prepare gives the descriptor block identity shortcut columns)
    nk, M = kpw.w1.shape[0], grid[0] * grid[1] * grid[2]
    f4, fd = ws.get("rb4_f", (nk, M, kpw.cout), torch.float32, dev), ws.get("rb4_fd", (M, dw.cout), torch.float32, dev)
    h4, hd = _bordered(W, ws, "rb4_h", (nk,), kpw.cout, grid, dev), _bordered(W, ws, "rb4_hd", (), dw.cout, grid, dev)
    _basic_block(_sub(x, slice(0, nk)), kpw, h4, f4, grid, ws.sat_flag, rb4=True)
    return f4, _basic_block(_sub(x, nk), dw, hd, fd, grid, ws.sat_flag, act=ops.ACT_NONE, rb4=True)


def heads_forward(W, ws, feat, nimg, gh, gw, cfg):
    """feat lp, bordered feature map of nimg gh x gw grids [bordered_rows, D] (split-operand heads: its (hi, lo) fp16 planes)
    -> scr [nimg,1,n], kps [nimg,2,n] (absolute pixels), depth [nimg,1,n], dsc [nimg,Cd,n], all fp32.  Every activation a 3x3
    conv reads is bordered; what only row-wise kernels read is dense.  The plane-writing kernels report saturation / NaN into
    ws.sat_flag (per workspace = per model: no shared word)."""
    grid = (nimg, gh, gw)
    x = _conv_stack(W, ws, feat, grid)
    xs, cat = _position_encoding(W, ws, x, grid, cfg)
    x4 = _attention_layers(W, ws, xs, cat, grid, cfg)
    f4, fd = _resblock4(W, ws, x4, grid)
    mk, kh = cfg["MICKEY"], cfg["MICKEY"]["KP_HEADS"]
    return ops.head_tails(f4[0], W.w_score, f4[1], W.w_xy, f4[2], W.w_depth, fd, nimg, gh, gw, f4.shape[-1], fd.shape[-1], border=3,
                          use_softmax=bool(kh["USE_SOFTMAX"]), use_depth_sigmoid=bool(kh["USE_DEPTHSIGMOID"]),
                          max_depth=float(kh["MAX_DEPTH"]), norm_dsc=bool(mk["DSC_HEAD"]["NORM_DSC"]),
                          down=float(mk["DINOV2"]["DOWN_FACTOR"]))


def match_uses_split(cfg, C):
    """Does match() take the split-fp16 correlation for C-channel descriptors under this configuration?  AMD.MATCHER_CORR:
    'auto' = the split-fp16 correlation on the 16-bit matrix cores when its preconditions hold (L2-normalised 128-channel
    descriptors, mickey_hip.h: mk_dual_softmax_split), else the exact fp32 MFMA; 'fp32' | 'split16' (ValueError without them)."""
    fm = cfg["FEATURE_MATCHER"]
    if fm["TYPE"] != "DualSoftmax":
        return False
    mode = str(cfg["AMD"].get("MATCHER_CORR", "auto")).lower()
    can = bool(cfg["MICKEY"]["DSC_HEAD"]["NORM_DSC"]) and ops.dual_softmax_split_ok(C, float(fm["DUAL_SOFTMAX"]["TEMPERATURE"]))
    if mode == "split16" and not can:
        raise ValueError("AMD.MATCHER_CORR: split16 needs MICKEY.DSC_HEAD.NORM_DSC, 128 descriptor channels and T >= 0.0145")
    return can and mode != "fp32"


def match(W, cfg, dsc0, dsc1, scr0, scr1, lean=False, keyframe_index=None, pair_index=None, planes=None, out=None):
    """keyframe_index (keyframe mode): int32 device map pair -> row of dsc0 / scr0 (which then hold the K keyframes).
    pair_index (pair-list mode): the (idx0, idx1) device maps of a chunk of pairs into the image sets dsc0 / scr0 and dsc1 / scr1
    (ops._pair_arg); planes: the sets' split planes, made once per forward (ops.dsc_split_planes; only where match_uses_split);
    out: the chunk's (scores, kp_scores, final_scores) buffers (ops._outs)."""
    fm = cfg["FEATURE_MATCHER"]
    if fm["TYPE"] == "DualSoftmax":
        ds = fm["DUAL_SOFTMAX"]
        # the mode's keywords only where set: bench.py's stage profiler wraps ops.dual_softmax with a byte count that takes the
        # standard call's keywords and no others (the other three wrapped calls below and in solve() take any)
        mode = {k: v for k, v in (("keyframe_index", keyframe_index), ("pair_index", pair_index), ("planes", planes), ("out", out))
                if v is not None}
        return ops.dual_softmax(dsc0, dsc1, scr0, scr1, float(ds["TEMPERATURE"]), W.dustbin if ds["USE_DUSTBIN"] else None,
                                want_scores=not lean, want_kp=not lean, want_final=True, split=match_uses_split(cfg, dsc0.shape[1]),
                                **mode)
    if fm["TYPE"] == "Sinkhorn":
        # the reference's Sinkhorn branch is unreachable through featureMatcher.forward; the maths
        # restated is feature_matcher.py:125-137 with matching_mat(dsc0, dsc1, None)
        alpha = W.dustbin if W.dustbin is not None else float(fm["SINKHORN"]["DUSTBIN_SCORE_INIT"])
        return ops.sinkhorn(dsc0, dsc1, alpha, int(fm["SINKHORN"]["NUM_IT"]), scr0, scr1, want_scores=not lean,
                            want_kp=not lean, want_final=True, keyframe_index=keyframe_index, pair_index=pair_index, out=out)
    raise ValueError("feature matcher not recognized: %r" % (fm["TYPE"],))


def solve(cfg, final_scores, kps0, depth0, kps1, depth1, K0, K1, seed=0, offset=0, noise_outer=None, noise_inner=None,
          idx3_in=None, debug=False, offset_dev=None, pair_base=0, ws=None, keyframe_index=None, pair_index=None, invalid=None,
          finalize=True):
    """reference probabilisticProcrustes.py:183-348 on device.  Returns a dict with R [B,3,3], t [B,1,3],
    inliers [B,1] and the intermediates needed for the inlier list.  pair_base = global index of pair 0 (keys the
    Philox streams: sharding a batch over calls / GPUs does not change any pair's draws).  keyframe_index (keyframe mode):
    int32 device map pair -> row of kps0 / depth0 (which then hold the K keyframes); K0 stays per pair.  pair_index (pair-list
    mode): the (idx0, idx1) device maps of these pairs into the image sets kps0 / depth0 and kps1 / depth1; K0 / K1 stay per pair.
    invalid / finalize=False: a forward that solves its pairs in chunks hands every chunk the ONE invalid word of the forward and
    applies the batch-level rule itself, once (ops.pose_finalize)."""
    P = cfg["PROCRUSTES"]
    it_m, it_r, ns, k3 = int(P["IT_MATCHES"]), int(P["IT_RANSAC"]), int(P["NUM_SAMPLED_MATCHES"]), int(P["NUM_CORR_3D_3D"])
    if k3 != 3:
        raise ValueError("NUM_CORR_3D_3D must be 3 (the inference solver fits minimal 3-point samples)")
    B, n0, n1 = final_scores.shape
    dev = final_scores.device
    if invalid is None:
        invalid = torch.zeros((1,), device=dev, dtype=torch.int32)
    # the sampler's workspace lives in the model's Workspace (ws) like every other buffer of a forward: zeroed once, self-cleaning
    # afterwards (mickey_hip.h); one model is one forward at a time
    work = None
    if ws is not None:
        key = ("exprace_work", B, it_m, ns, n0 * n1)
        work = ws.bufs.get(key)
        if work is None or work.device != dev:
            work = ws.bufs[key] = ops.exprace_work(B, it_m, ns, n0 * n1, dev)
    idx, cnt = ops.exprace_topk(final_scores.reshape(B, n0 * n1), it_m, ns, noise=noise_outer, seed=seed, offset=offset,
                                invalid=invalid, offset_dev=offset_dev, pair_base=pair_base, work=work)
    X, Y, w, corr = ops.gather_backproject(idx, final_scores, kps0, depth0, kps1, depth1, K0, K1, it_m,
                                           keyframe_index=keyframe_index, pair_index=pair_index)
    Rh, th, score, idx3 = ops.ransac_hypotheses(X, Y, w, it_r, float(P["TH_SOFT_INLIER"]), noise3=noise_inner,
                                                idx3_in=idx3_in, seed=seed, offset=offset + 1, offset_dev=offset_dev,
                                                set_base=pair_base * it_m)
    R, t, conf, best, mask, rounds, invalid = ops.refine_pose(X, Y, Rh, th, score, B, it_m, it_r, float(P["TH_INLIER"]),
                                                              int(P["NUM_REFINEMENTS"]), k3, invalid=invalid, finalize=finalize)
    out = {"R": R, "t": t, "inliers": conf, "best": best, "mask": mask, "corr": corr, "weights": w, "invalid": invalid,
           "it_ransac": it_r, "it_matches": it_m}
    if debug:
        out.update(idx=idx, cnt=cnt, X=X, Y=Y, R_hyp=Rh, t_hyp=th, score=score, idx3=idx3, rounds=rounds)
    return out


def inliers_list(sol):
    """Per pair [m_i, 7] = (u0, v0, u1, v1, score, d0, d1) of the final hard inliers, sorted by score
    (descending): reference probabilisticProcrustes.py:306-327.  Only built on request (demo 3-D
    visualisation); a handful of torch index ops on <= 2048 rows per pair, outside the hot path."""
    B = sol["R"].shape[0]
    if int(sol["invalid"].item()) != 0:
        return [torch.zeros([0, 5])] * B
    k = sol["mask"].shape[1]
    sets = sol["best"].long() // sol["it_ransac"] + torch.arange(B, device=sol["best"].device) * sol["it_matches"]
    out = []
    for b in range(B):
        sel = sol["mask"][b] != 0
        c = sol["corr"][sets[b]][sel]
        w = sol["weights"][sets[b]][sel]
        order = torch.argsort(w, descending=True)
        c, w = c[order], w[order]
        out.append(torch.cat([c[:, 0:4], w[:, None], c[:, 4:6]], 1))
    return out
