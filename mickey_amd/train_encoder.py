"""The frozen DINOv2 encoder of a training step, on the HIP encoder kernels.

The reference trainer runs its encoder under torch.no_grad() on both images of every pair and hands the patch tokens to four
trainable torch Conv2d stacks (lib/models/MicKey/modules/mickey_extractor.py:43-58):

    feats = self.dinov2_vitl14.forward_features(x.to(self.amp_dtype))['x_norm_patchtokens']
    feats = feats.permute(0, 2, 1).reshape(B, C, H // 14, W // 14).float()

The encoder is frozen (requires_grad_(False), eval(), its weights dropped from every checkpoint, model.py:291-298), so it needs
no backward: the inference kernels serve it as they are (pipeline.encoder_features), with the final LayerNorm written as the
fp32 NCHW tensor the Conv2d stacks read (mk_layernorm_nchw) instead of this project's bordered token-major feature map.

    FrozenDinoV2(source)          nn.Module with the reference's forward_features contract; no parameters, no buffers
    encode_frozen(m, images)      functional form: both image sets of a batch in one pass
    use_hip_encoder(model)        swaps it into a reference-style model in place (next to train_matcher.use_hip_matcher)
"""
import collections.abc

import torch
from torch import nn

from . import _native, pipeline
from . import weights as wts_mod
from ._train_common import swap_modules

_DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
_TOP_KEYS = ("cls_token", "pos_embed", "patch_embed.proj.weight", "patch_embed.proj.bias", "norm.weight", "norm.bias")
_BLOCK_KEYS = ("norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias", "ls1.gamma",
               "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias", "ls2.gamma")
_IGNORED_KEYS = ("mask_token",)   # in the hub file, unused by forward_features without masks (dinov2.py:194-195)


def _block_shapes(D):
    return {"norm1.weight": (D,), "norm1.bias": (D,), "attn.qkv.weight": (3 * D, D), "attn.qkv.bias": (3 * D,),
            "attn.proj.weight": (D, D), "attn.proj.bias": (D,), "ls1.gamma": (D,), "norm2.weight": (D,), "norm2.bias": (D,),
            "mlp.fc1.weight": (4 * D, D), "mlp.fc1.bias": (4 * D,), "mlp.fc2.weight": (D, 4 * D), "mlp.fc2.bias": (D,),
            "ls2.gamma": (D,)}


def check_state_dict(sd):
    """Problems of a flat DINOv2 state dict (the hub file's key names) that keep it off the HIP encoder kernels, one line each,
    every line naming the offending key; [] = supported (ViT/14 with LayerScale and an MLP FFN, no register tokens, D % 64 == 0).
    Also returns the keys that are neither used nor known."""
    errs = []
    swiglu = [k for k in sd if ".mlp.w12." in k or ".mlp.w3." in k]
    errs += ["%s: register tokens are not supported by the HIP encoder" % k for k in sd
             if k == "register_tokens" or k.endswith(".register_tokens")]
    if swiglu:   # (every block has them: the first one names the architecture)
        errs.append("%s: the SwiGLU FFN is not supported by the HIP encoder (MLP FFN only)" % swiglu[0])
    chunked = [k for k in sd if k.startswith("blocks.") and len(k.split(".")) > 3 and k.split(".")[2].isdigit()]
    if chunked:
        errs.append("%s: chunked blocks (block_chunks > 0) are not supported; build the encoder with block_chunks=0" % chunked[0])
    missing_top = [k for k in _TOP_KEYS if k not in sd]
    errs += ["%s: missing key" % k for k in missing_top]
    if missing_top or errs:
        return errs, []
    D = int(sd["cls_token"].shape[-1])
    if D % 64 != 0:
        errs.append("cls_token: embedding width D=%d is not a multiple of 64 (head_dim 64)" % D)
    pw = tuple(sd["patch_embed.proj.weight"].shape)
    if len(pw) != 4 or pw[2:] != (14, 14):
        errs.append("patch_embed.proj.weight: patch size %s, the HIP encoder supports 14 x 14 only" % (pw[2:],))
    elif pw[:2] != (D, 3):
        errs.append("patch_embed.proj.weight: shape %s, expected %s" % (pw, (D, 3, 14, 14)))
    if errs:
        return errs, []
    have = sorted({int(k.split(".")[1]) for k in sd if k.startswith("blocks.") and k.split(".")[1].isdigit()})
    if not have:
        return ["blocks.0.norm1.weight: missing key"], []
    depth = have[-1] + 1
    expected = {"cls_token": (1, 1, D), "patch_embed.proj.bias": (D,), "norm.weight": (D,), "norm.bias": (D,)}
    for i in range(depth):
        for k, s in _block_shapes(D).items():
            expected["blocks.%d.%s" % (i, k)] = s
    for k, s in expected.items():
        if k not in sd:
            errs.append("%s: missing key" % k)
        elif tuple(sd[k].shape) != s:
            errs.append("%s: shape %s, expected %s" % (k, tuple(sd[k].shape), s))
    pe = tuple(sd["pos_embed"].shape)
    n = pe[1] - 1 if len(pe) == 3 else -1
    if len(pe) != 3 or pe[0] != 1 or pe[2] != D or n < 1 or int(round(n ** 0.5)) ** 2 != n:
        errs.append("pos_embed: shape %s, expected (1, 1 + g * g, %d)" % (pe, D))
    known = set(expected) | {"pos_embed", "patch_embed.proj.weight"} | set(_IGNORED_KEYS)
    return errs, [k for k in sd if k not in known]


def _looks_like_dinov2(module):
    """DINOv2's state-dict key structure (dinov2.py:88-150): recognised by what it holds, not by its class name."""
    try:
        keys = set(module.state_dict().keys())
    except Exception:
        return False
    return {"cls_token", "pos_embed", "patch_embed.proj.weight", "norm.weight"} <= keys and any(k.startswith("blocks.") for k in keys)


class FrozenDinoV2(nn.Module):
    """The reference's frozen `dinov2_vitl14` child on the HIP encoder kernels.

    source: a DINOv2 module (anything with its state-dict keys) or a flat state dict with the hub file's key names.
    dtype: 'auto' | 'bf16' | 'fp16' | 'fp32' -- operand type of the encoder's GEMMs and attention; 'auto' = fp16 when the
        source's weights are fp16 (the reference's MICKEY.DINOV2.FLOAT16), bf16 otherwise.
    ln_fold: norm1 / norm2 folded into the GEMMs around them (weights.prepare_encoder).
    features_lp: 'auto' | True | False -- round the features to fp16 on the way out, as an fp16 torch encoder followed by
        .float() hands them over (mickey_extractor.py:49-52); 'auto' = exactly when the encoder dtype is fp16.

    The module registers NO parameters and NO buffers: its state_dict() is empty, so a checkpoint is written without encoder
    keys (what the reference's on_save_checkpoint produces by deleting them, model.py:291-298) and such a checkpoint loads
    strictly.  A state dict that does carry keys below this module's prefix replaces the held weights.  The weights live on the
    host; their device image (weights.prepare_encoder) is made on first use and dropped by every .to() / .cuda() / .cpu().
    Everything runs under torch.no_grad() on the current stream; there is no CPU path (MickeyHipError)."""

    patch_size = 14

    def __init__(self, source, dtype="auto", ln_fold=True, features_lp="auto"):
        super().__init__()
        dev = torch.device("cpu")
        if isinstance(source, nn.Module):
            sd = source.state_dict()
            first = next(iter(sd.values()), None)
            if first is not None:
                dev = first.device
        elif isinstance(source, collections.abc.Mapping):
            sd = source
        else:
            raise TypeError("FrozenDinoV2: source must be a DINOv2 module or a state dict, got %s" % type(source).__name__)
        sd = {k: v.detach().to("cpu", copy=True) for k, v in sd.items() if torch.is_tensor(v)}   # its own copy: later edits of the source do not reach it
        errs, _ = check_state_dict(sd)
        if errs:
            raise ValueError("FrozenDinoV2: unsupported encoder -- " + "; ".join(errs[:8]))
        if dtype not in ("auto",) + tuple(_DTYPES):
            raise ValueError("FrozenDinoV2: dtype must be 'auto', 'bf16', 'fp16' or 'fp32', got %r" % (dtype,))
        if dtype == "auto":
            dtype = "fp16" if sd["blocks.0.attn.qkv.weight"].dtype == torch.float16 else "bf16"
        if features_lp not in ("auto", True, False):
            raise ValueError("FrozenDinoV2: features_lp must be 'auto', True or False, got %r" % (features_lp,))
        self.lp_dtype = _DTYPES[dtype]
        self.ln_fold = bool(ln_fold)
        self.round_fp16 = self.lp_dtype == torch.float16 if features_lp == "auto" else bool(features_lp)
        self._set_weights(sd)
        self._probe = torch.zeros(1, device=dev)   # a plain attribute (not a buffer) that follows _apply: the module's device
        self.requires_grad_(False)
        self.eval()

    def _set_weights(self, sd):
        self._sd = sd
        self.embed_dim = int(sd["cls_token"].shape[-1])
        self.depth = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
        self._dev_weights = None
        self._ws = pipeline.Workspace()

    def extra_repr(self):
        return "embed_dim=%d, depth=%d, dtype=%s, ln_fold=%s, round_fp16=%s" % (self.embed_dim, self.depth, self.lp_dtype, self.ln_fold,
                                                                             self.round_fp16)

    # ---- device / checkpoint contract ------------------------------------------------------------------------------
    def _apply(self, fn, *a, **k):
        self._dev_weights = None
        self._ws = pipeline.Workspace()
        self._probe = fn(self._probe)
        return super()._apply(fn, *a, **k)

    @property
    def device(self):
        return self._probe.device

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        mine = {k[len(prefix):]: v.detach().to("cpu", copy=True) for k, v in state_dict.items() if k.startswith(prefix) and torch.is_tensor(v)}
        if not mine:
            return   # a checkpoint saved without the frozen encoder: the held weights stay
        errs, unknown = check_state_dict(mine)
        if errs:
            error_msgs.extend("%s%s (FrozenDinoV2 keeps its current weights)" % (prefix, e) for e in errs)
            return
        if strict:
            unexpected_keys.extend(prefix + k for k in unknown)
        self._set_weights(mine)

    def device_weights(self):
        dev = self.device
        if dev.type != "cuda":
            raise _native.MickeyHipError("FrozenDinoV2 needs the module on a GPU (model.cuda()); mickey_amd has no CPU fallback")
        if self._dev_weights is None:
            self._dev_weights = wts_mod.prepare_encoder(self._sd, dev, self.lp_dtype, prefix="", ln_fold=self.ln_fold)
        return self._dev_weights

    # ---- forward ---------------------------------------------------------------------------------------------------
    def _encode(self, images, round_fp16=None):
        W = self.device_weights()
        sets = [_pixels(t, W.norm_w.device) for t in images]
        with torch.no_grad(), torch.cuda.device(W.norm_w.device):
            return pipeline.encoder_features(W, self._ws, sets if len(sets) > 1 else sets[0],
                                             round_fp16=self.round_fp16 if round_fp16 is None else round_fp16)

    def forward(self, x):
        """x [B, 3, H, W] fp32 / fp16 (H, W cropped to multiples of 14) -> fp32 [B, D, H // 14, W // 14]; requires no grad."""
        return self._encode([x])

    def forward_features(self, x, masks=None):
        """dinov2.py:221-236 for the one key the reference reads: {'x_norm_patchtokens': [B, n, D]}, a VIEW of the NCHW
        tensor the kernel wrote -- the caller's .permute(0, 2, 1).reshape(B, C, h, w).float() lands on that buffer again."""
        if masks is not None:
            raise ValueError("FrozenDinoV2.forward_features: masks are not supported")
        nchw = self._encode([x])
        B, D, gh, gw = nchw.shape
        return {"x_norm_patchtokens": nchw.view(B, D, gh * gw).permute(0, 2, 1)}


def _pixels(x, dev):
    if not torch.is_tensor(x) or x.dim() != 4 or x.shape[1] != 3:
        raise ValueError("FrozenDinoV2: images must be [B, 3, H, W] tensors, got %s" %
                         (tuple(x.shape) if torch.is_tensor(x) else type(x).__name__))
    if x.shape[0] < 1 or x.shape[2] < 14 or x.shape[3] < 14:
        raise ValueError("FrozenDinoV2: images must hold at least one 14 x 14 patch, got %s" % (tuple(x.shape),))
    if x.device != dev:
        raise _native.MickeyHipError("FrozenDinoV2: images on %s, the encoder on %s" % (x.device, dev))
    if x.dtype in (torch.float16, torch.bfloat16):
        x = x.float()   # the reference passes x.to(amp_dtype): the pixels are widened, not re-derived
    elif x.dtype != torch.float32:
        raise ValueError("FrozenDinoV2: images must be float32 or float16, got %s" % x.dtype)
    x = x.detach()
    return x if x.stride(3) == 1 else x.contiguous()


def encode_frozen(module_or_weights, images, round_fp16=None, ws=None):
    """Functional form for a custom training step.  module_or_weights: a FrozenDinoV2, or the DeviceWeights of
    weights.prepare_encoder.  images: one [B, 3, H, W] tensor -> fp32 [B, D, H // 14, W // 14]; or a sequence of image sets of
    one size (image 0 and image 1 of every pair) -> a list of such tensors, all sets encoded in ONE pass.  round_fp16: None =
    the module's setting (with bare weights: whether they are fp16).  ws (bare weights only): the pipeline.Workspace holding the
    encoder's intermediate buffers -- pass the model's own to share them with its inference path; None keeps one on the weights
    object (`_features_ws`, about 1 GB at 16 images of 540x720), allocated at the first call."""
    single = torch.is_tensor(images)
    sets = [images] if single else list(images)
    if isinstance(module_or_weights, FrozenDinoV2):
        if ws is not None:
            raise ValueError("encode_frozen: ws= goes with bare DeviceWeights; a FrozenDinoV2 owns its workspace")
        out = module_or_weights._encode(sets, round_fp16)
    else:
        W = module_or_weights
        if ws is None:
            ws = getattr(W, "_features_ws", None)
            if ws is None:
                ws = W._features_ws = pipeline.Workspace()
        dev = W.norm_w.device
        px = [_pixels(t, dev) for t in sets]
        with torch.no_grad(), torch.cuda.device(dev):
            out = pipeline.encoder_features(W, ws, px if len(px) > 1 else px[0],
                                            round_fp16=W.lp == torch.float16 if round_fp16 is None else round_fp16)
    return out if single else list(out.split([t.shape[0] for t in sets]))


def use_hip_encoder(model, dtype="auto", ln_fold=True, features_lp="auto"):
    """Replace every frozen DINOv2 child named `dinov2_vitl14` inside `model` (a reference-style training model:
    MicKey_Extractor.dinov2_vitl14, mickey_extractor.py:25-28) by a FrozenDinoV2 built from it, in place.  A child counts when
    it has a forward_features method and DINOv2's state-dict key structure, whatever its class.  An architecture the kernels do
    not cover (register tokens, SwiGLU FFN, patch size != 14, D % 64 != 0) raises ValueError instead of being skipped.  Returns
    the number of children swapped; a second call finds none."""
    def make(old):
        if not isinstance(old, FrozenDinoV2) and callable(getattr(old, "forward_features", None)) and _looks_like_dinov2(old):
            return FrozenDinoV2(old, dtype=dtype, ln_fold=ln_fold, features_lp=features_lp)   # (stays in eval mode, whatever old's)

    return swap_modules(model, make, name="dinov2_vitl14")
