"""Drop-in replacement of the reference's inference module.

Same contract as reference lib/models/MicKey/compute_pose.py::MickeyRelativePose:
``forward(data, return_inliers=False) -> (R [B,3,3], t [B,1,3])`` with the reference's in-place side
effects on ``data``, ``on_load_checkpoint`` / ``load_state_dict`` with the reference's key names,
``.e2e_Procrustes.num_samples_matches``, ``.compute_matches.{extractor,matcher}``, ``.parameters()``.
All arithmetic of ``forward`` runs in libmickey_hip.so on the module's device; there is no CPU / ATen
fallback (a CPU-resident module raises on forward).
"""
import collections
import copy
import os

import torch
import torch.nn as nn

from . import _native, pipeline, weights
from .config import as_cfg
from .synthetic import DINO_PREFIX, DUSTBIN_KEY, VIT_ARCH, expected_keys

_LP = {"bf16": torch.bfloat16, "fp16": torch.float16, "bfloat16": torch.bfloat16, "float16": torch.float16,
       "fp32": torch.float32, "float32": torch.float32}
# hub file the reference's extractor downloads in its constructor (reference mickey_extractor.py:14-17)
DINOV2_URL = "https://dl.fbaipublicfiles.com/dinov2/dinov2_vitl14/dinov2_vitl14_pretrain.pth"


def resolve_encoder_dtype(cfg):
    """AMD.ENCODER_DTYPE: 'bf16' | 'fp16' | 'fp32', or 'auto' = follow the reference's own precision switch
    MICKEY.DINOV2.FLOAT16 (reference mickey_extractor.py:31-35): True -> fp16 operands, False -> the exact-fp32 path."""
    v = str(cfg["AMD"].get("ENCODER_DTYPE", "auto")).lower()
    if v == "auto":
        v = "fp16" if bool(cfg["MICKEY"]["DINOV2"].get("FLOAT16", True)) else "fp32"
    if v not in _LP:
        raise ValueError("AMD.ENCODER_DTYPE must be auto | bf16 | fp16 | fp32, got %r" % v)
    return _LP[v]


def resolve_heads_dtype(cfg, encoder_dtype):
    """AMD.HEADS_DTYPE: operand type of the four head stacks (reference mickey_extractor.py:53-56 always runs them in fp32).
    'auto': fp16 beside a 16-bit encoder -- the heads' activations are BatchNorm outputs and the encoder's final-norm tokens
    (which the reference's shipped fp16 mode itself holds in fp16, mickey_extractor.py:49-51), fp16's 11 bits run at the bf16
    MFMA rate and take the heads' share of the bf16 mode's noise down 8x; fp32 beside the fp32 parity encoder.
    'same' = the encoder's type, or bf16 | fp16 | fp32 (exact: fp32 MFMA) | split (the fp32 pipeline with its 3x3 convolutions
    on split fp16 operands: fp32-grade products on the 16-bit matrix cores, resolve_heads_split)."""
    v = str(cfg["AMD"].get("HEADS_DTYPE", "auto")).lower()
    if v == "split":
        return torch.float32
    if v == "auto":
        return torch.float32 if encoder_dtype == torch.float32 else torch.float16
    if v == "same":
        return encoder_dtype
    if v not in _LP:
        raise ValueError("AMD.HEADS_DTYPE must be auto | same | bf16 | fp16 | fp32 | split, got %r" % v)
    if encoder_dtype == torch.float32 and _LP[v] != torch.float32:
        raise ValueError("AMD.HEADS_DTYPE: %s needs a 16-bit AMD.ENCODER_DTYPE (the fp32 parity mode runs everything in fp32)" % v)
    return _LP[v]


def resolve_features_lp(cfg, lp_dtype):
    """AMD.FEATURES_LP (split-operand heads only): the encoder's features reach the heads rounded to fp16, as in the reference, whose
    fp16 encoder RETURNS fp16 tensors that `.float()` widens exactly (mickey_extractor.py:49-52).  auto (default) = True behind an
    fp16 encoder (the reference's MICKEY.DINOV2.FLOAT16 data flow, literally), False otherwise; true / false force it (false: the
    final LayerNorm's fp32 rows as (hi, lo) planes -- more precise than the reference, and a third product in the first conv)."""
    v = str(cfg["AMD"].get("FEATURES_LP", "auto")).lower()
    if v not in ("auto", "true", "false", "1", "0"):
        raise ValueError("AMD.FEATURES_LP must be auto | true | false, got %r" % v)
    return lp_dtype == torch.float16 if v == "auto" else v in ("true", "1")


def resolve_heads_split(cfg):
    """AMD.HEADS_DTYPE: split -- the reference's precision split (fp32 heads behind a 16-bit encoder, mickey_extractor.py:49-56)
    at 16-bit matrix-core speed: head activations, LayerNorms and the small linears as in the fp32 mode, the 3x3
    convolutions (99 % of the heads' flops) as three fp16 MFMA products of hi / lo operand planes staged once (mk_conv3x3_split)."""
    return str(cfg["AMD"].get("HEADS_DTYPE", "auto")).lower() == "split"


class _SolverView:
    """Attribute view of the PROCRUSTES config (reference probabilisticProcrustes.py:12-20)."""

    def __init__(self, cfg):
        P = cfg["PROCRUSTES"]
        self.it_RANSAC = P["IT_RANSAC"]
        self.it_matches = P["IT_MATCHES"]
        self.num_samples_matches = P["NUM_SAMPLED_MATCHES"]
        self.num_corr_3d_3d = P["NUM_CORR_3D_3D"]
        self.num_refinements = P["NUM_REFINEMENTS"]
        self.th_inlier = P["TH_INLIER"]
        self.th_soft_inlier = P["TH_SOFT_INLIER"]


class _MatcherView:
    def __init__(self, owner):
        self._owner = owner

    def get_matches_list(self, scores, min_conf=0.0):
        """Mutual nearest neighbours with exp(score) > min_conf, sorted by score: reference feature_matcher.py:19-46
        (B = 1 there; batched here, returns the B = 1 tensor for a batch of one, a list otherwise)."""
        from . import ops
        scores = scores.contiguous()
        m, c = ops.mutual_nn(scores)
        outs = []
        for b in range(scores.shape[0]):
            mb = m[b, : int(c[b])].long()
            if min_conf > 0.0 and mb.numel():   # the kernel applies the reference's default threshold exp(s) > 0
                mb = mb[scores[b, mb[:, 0], mb[:, 1]].exp() > min_conf]
            outs.append(mb)
        return outs[0] if len(outs) == 1 else outs


class _ComputeMatchesView:
    def __init__(self, owner):
        self.matcher = _MatcherView(owner)
        self.extractor = owner
        self.down_factor = owner.cfg["MICKEY"]["DINOV2"]["DOWN_FACTOR"]
        self.dsc_dim = owner.cfg["MICKEY"]["DSC_HEAD"]["LAST_DIM"]


class MickeyRelativePose(nn.Module):
    def __init__(self, cfg, dinov2_weights=None):
        super().__init__()
        self.cfg = as_cfg(cfg)
        amd = self.cfg["AMD"]
        self.lp_dtype = resolve_encoder_dtype(self.cfg)
        self.heads_dtype = resolve_heads_dtype(self.cfg, self.lp_dtype)
        self.heads_split = resolve_heads_split(self.cfg)
        self.features_lp = self.heads_split and resolve_features_lp(self.cfg, self.lp_dtype)
        self.lean = bool(amd.get("LEAN", False))
        self.ln_fold = bool(amd.get("LN_FOLD", True))   # norm1 / norm2 folded into the GEMMs around them (16-bit modes)
        self.ln_centre = bool(amd.get("LN_CENTRE", True))   # ... with the residual stream kept row-centred
        self.seed = int(amd.get("SEED", 0))
        # hipGraph replay of the whole forward for launch-bound batches: "auto" (<= GRAPH_MAX_IMAGES images), True, False
        self.graph_mode = amd.get("GRAPH", "auto")
        self.graph_max_images = int(amd.get("GRAPH_MAX_IMAGES", 8))
        self.graph_cache_size = int(amd.get("GRAPH_CACHE", 4))   # captured input signatures kept (LRU)
        self._graphs = collections.OrderedDict()
        self._sat_flag = None   # split-operand heads: device word the plane-writing kernels report saturation into
        self._calls = 0
        self._ctr = None   # device-resident 2 * _calls: the Philox stream offset (read by the kernels, so a graph can advance it)
        # a single registered parameter carries the module's device (reference callers use
        # next(model.parameters()).device, lib/utils/data.py:7); the real weights live in _sd
        self._anchor = nn.Parameter(torch.zeros(1), requires_grad=False)
        self._sd = {}
        self._dev_weights = None
        self._ws = pipeline.Workspace()
        self.e2e_Procrustes = _SolverView(self.cfg)
        object.__setattr__(self, "compute_matches", _ComputeMatchesView(self))
        # the frozen encoder weights: an explicit dict, a local file (AMD.DINOV2_WEIGHTS / $MICKEY_DINOV2_WEIGHTS), or --
        # as the reference's extractor does in its constructor (mickey_extractor.py:14-17) -- the hub download; "none"
        # defers to a state_dict that carries them (tests, synthetic weights)
        if dinov2_weights is None:
            path = amd.get("DINOV2_WEIGHTS") or os.environ.get("MICKEY_DINOV2_WEIGHTS")
            if path and str(path).lower() != "none":
                dinov2_weights = torch.load(path, map_location="cpu")
        self._dino_injected = set()
        if dinov2_weights is not None:
            for k, v in dinov2_weights.items():
                self._sd[DINO_PREFIX + k] = v.detach().cpu()
                self._dino_injected.add(DINO_PREFIX + k)
        self.eval()

    # ---- checkpoint contract ---------------------------------------------------------------------
    def state_dict(self, *args, **kwargs):
        return dict(self._sd)

    def load_state_dict(self, state_dict, strict=True):
        """nn.Module.load_state_dict semantics against the reference's key layout: with strict=True
        missing / unexpected keys and shape mismatches raise; with strict=False they are returned.  Keys absent from
        `state_dict` keep their current value (so DINOv2 weights injected at construction survive a MicKey checkpoint
        that was saved without them, which is how the reference's checkpoints are written: model.py:291-298)."""
        new = {k: v.detach().cpu() for k, v in state_dict.items() if torch.is_tensor(v)}
        arch = str(self.cfg["AMD"].get("VIT", "vit_large"))
        if any(k.endswith("cls_token") for k in new):   # take the width from the checkpoint when it says otherwise
            D = [v.shape[-1] for k, v in new.items() if k.endswith("cls_token")][0]
            arch = {v[0]: k for k, v in VIT_ARCH.items()}.get(D, arch)
        expected = expected_keys(self.cfg, arch)
        if arch != "vit_large" or any(DINO_PREFIX + "blocks." in k for k in new):   # depth follows the checkpoint
            have = [int(k[len(DINO_PREFIX) + 7:].split(".")[0]) for k in new if k.startswith(DINO_PREFIX + "blocks.")]
            if have:
                depth = 1 + max(have)
                expected = {k: s for k, s in expected.items()
                            if not k.startswith(DINO_PREFIX + "blocks.") or int(k[len(DINO_PREFIX) + 7:].split(".")[0]) < depth}
        if not any("dinov2" in k for k in new) and not any("dinov2" in k for k in self._sd):
            self._fetch_dinov2()
        merged = dict(self._sd)
        merged.update(new)
        missing = [k for k in expected if k not in merged]
        unexpected = [k for k in new if k not in expected]
        bad_shape = ["%s: %s, expected %s" % (k, tuple(merged[k].shape), expected[k]) for k in expected
                     if k in merged and tuple(merged[k].shape) != expected[k] and merged[k].numel() != 1]
        if strict and (missing or unexpected or bad_shape):
            hint = ""
            if any(k.startswith(DINO_PREFIX) for k in missing):
                hint = ("\n(MicKey checkpoints are saved without the DINOv2 weights: pass dinov2_weights=, or set "
                        "AMD.DINOV2_WEIGHTS / $MICKEY_DINOV2_WEIGHTS to dinov2_vitl14_pretrain.pth; the hub download the "
                        "reference performs was %s)" % (getattr(self, "_hub_error", None) or "disabled (AMD.DINOV2_HUB: False)"))
            raise RuntimeError("Error(s) in loading state_dict for MickeyRelativePose:\n\tMissing key(s): %s\n\tUnexpected "
                               "key(s): %s\n\tsize mismatch: %s%s" % (missing[:8] + (["..."] if len(missing) > 8 else []),
                                                                     unexpected[:8], bad_shape[:8], hint))
        self._sd = merged
        self._dev_weights = None
        self._graphs.clear()
        return torch.nn.modules.module._IncompatibleKeys(missing, unexpected)

    def _fetch_dinov2(self):
        """The reference's extractor downloads dinov2_vitl14_pretrain.pth in its constructor (mickey_extractor.py:14-17);
        here the download is deferred to the moment a checkpoint WITHOUT encoder weights is loaded and none were given
        (dinov2_weights= / AMD.DINOV2_WEIGHTS / $MICKEY_DINOV2_WEIGHTS).  AMD.DINOV2_HUB: False forbids it."""
        if not bool(self.cfg["AMD"].get("DINOV2_HUB", True)):
            return False
        try:
            sd = torch.hub.load_state_dict_from_url(DINOV2_URL, map_location="cpu")
        except Exception as e:   # no network, proxy, disk ...: reported by the strict load with the hint below
            self._hub_error = "%s: %s" % (type(e).__name__, e)
            return False
        for k, v in sd.items():
            self._sd[DINO_PREFIX + k] = v.detach().cpu()
        return True

    def on_load_checkpoint(self, checkpoint):
        """MicKey checkpoints are saved without the frozen DINOv2 weights; re-inject them before
        load_state_dict (reference compute_pose.py:39-48)."""
        sd = checkpoint["state_dict"]
        if not any("dinov2" in k for k in self._sd) and not any("dinov2" in k for k in sd):
            self._fetch_dinov2()
        for k, v in self._sd.items():
            if "dinov2" in k:
                sd[k] = v

    def is_eval_model(self, is_eval):  # reference compute_pose.py:50-60; inference-only here
        if not is_eval:
            raise NotImplementedError("mickey_amd implements the inference path only")

    def _apply(self, fn, *a, **k):
        self._dev_weights = None
        self._graphs = collections.OrderedDict()
        self._ctr = None
        self._sat_flag = None
        return super()._apply(fn, *a, **k)

    @property
    def device(self):
        return self._anchor.device

    def device_weights(self):
        dev = self._anchor.device
        if dev.type != "cuda":
            raise _native.MickeyHipError("MickeyRelativePose.forward needs the module on a GPU (model.cuda()); "
                                         "mickey_amd has no CPU fallback")
        if self._dev_weights is None:
            if not self._sd:
                raise RuntimeError("no weights loaded")
            fm = self.cfg["FEATURE_MATCHER"]
            if fm["TYPE"] == "DualSoftmax" and fm["DUAL_SOFTMAX"]["USE_DUSTBIN"] and DUSTBIN_KEY not in self._sd:
                raise RuntimeError("FEATURE_MATCHER.DUAL_SOFTMAX.USE_DUSTBIN is set but the checkpoint has no %s (the "
                                   "reference's strict load fails on this too)" % DUSTBIN_KEY)
            self._dev_weights = weights.prepare(self._sd, self.cfg, dev, self.lp_dtype, heads_dtype=self.heads_dtype, heads_split=self.heads_split,
                                                ln_fold=self.ln_fold, ln_centre=self.ln_centre, features_lp=self.features_lp)
        return self._dev_weights

    # ---- forward ---------------------------------------------------------------------------------
    def _images(self, t):   # -> fp32 device tensor with a dense last dimension (the patch kernel takes any outer strides)
        t = t.to(device=self._anchor.device, dtype=torch.float32)
        return t if t.stride(3) == 1 else t.contiguous()

    def _arm_sat_flag(self):
        """Split-operand heads hold activations as x * 64 = hi + lo in fp16: a value beyond +-1023 is clamped.  The plane-writing
        kernels report it (and any NaN) into this word of the model's own workspace, never silently (split_saturated() reads it)."""
        if self.heads_split and self._sat_flag is None:
            self._sat_flag = torch.zeros((1,), device=self._anchor.device, dtype=torch.int32)
        self._ws.sat_flag = self._sat_flag if self.heads_split else None

    def _next_call(self):   # one call number per forward: its Philox stream offset = 2 * (forwards so far), kept on the device
        from . import ops
        if self._ctr is None:
            self._ctr = torch.full((1,), 2 * self._calls, device=self._anchor.device, dtype=torch.int64)
        self._calls += 1
        ops.counter_add(self._ctr, 2)

    def _keyframe_map(self, data):
        """Keyframe mode (data["keyframe_index"]): validate the pair -> keyframe map on the host (ValueError: wrong length, not
        integers, out of [0, K)) and return the model's device int32 copy of it (workspace).  A map given as a device tensor is
        copied to the host for the check: one synchronisation.  None without the key."""
        if "keyframe_index" not in data:
            return None
        from . import ops
        B, K = int(data["image1"].shape[0]), int(data["image0"].shape[0])
        host = torch.from_numpy(ops.check_keyframe_index(data["keyframe_index"], B, K))
        kf = self._ws.get("keyframe_index", (B,), torch.int32, self._anchor.device)
        kf.copy_(host)
        return kf

    @torch.no_grad()
    def compute_correspondences(self, data, _kf=None):
        """reference compute_correspondences.py:52-92 + compute_pose.py:23: fills the data dict.  Keyframe mode
        (data["keyframe_index"], README): image0 holds K distinct keyframes, image1 one query frame per pair; the per-keyframe
        outputs (kps0, depth_kp0, scr0, dsc0, depth0_map) get K rows, the per-pair ones B."""
        if _kf is None:
            _kf = self._keyframe_map(data)   # validated before anything is launched
        W = self.device_weights()
        dev = self._anchor.device
        im0, im1 = self._images(data["image0"]), self._images(data["image1"])
        B = im0.shape[0]
        same = im0.shape == im1.shape
        if _kf is not None:   # K keyframes + B queries: one pass over K + B images when the frame sizes agree
            same = im0.shape[1:] == im1.shape[1:]
        rows = (B, B) if _kf is None else (B, im1.shape[0])   # rows of the image-0 / image-1 outputs
        # one 2B-image pass when shapes agree (the two image sets are patched into one token matrix: no copy of the images)
        imgs = [(im0, im1)] if same else [(im0,), (im1,)]
        outs = []
        self._arm_sat_flag()
        for im in imgs:
            feat, gh, gw = pipeline.encoder_forward(W, self._ws, im)
            scr, kps, depth, dsc = pipeline.heads_forward(W, self._ws, feat, sum(t.shape[0] for t in im), gh, gw, self.cfg)
            outs.append((scr, kps, depth, dsc, gh, gw))
        if same:
            scr, kps, depth, dsc, gh, gw = outs[0]
            parts = [(scr[:B], kps[:B], depth[:B], dsc[:B], gh, gw), (scr[B:], kps[B:], depth[B:], dsc[B:], gh, gw)]   # (B = image0's rows: K in keyframe mode)
        else:
            parts = outs
        for i, (scr, kps, depth, dsc, gh, gw) in enumerate(parts):
            data["kps%d_shape" % i] = [gh, gw]
            data["depth%d_map" % i] = depth.reshape(rows[i], 1, gh, gw)
            data["kps%d" % i] = kps.contiguous()
            data["depth_kp%d" % i] = depth.contiguous()
            data["scr%d" % i] = scr.contiguous()
            data["dsc%d" % i] = dsc.contiguous()
        data["down_factor"] = self.cfg["MICKEY"]["DINOV2"]["DOWN_FACTOR"]
        scores, kp, fin = pipeline.match(W, self.cfg, data["dsc0"], data["dsc1"], data["scr0"], data["scr1"], self.lean,
                                         keyframe_index=_kf)
        if scores is not None:
            data["scores"] = scores
            data["kp_scores"] = kp
        data["final_scores"] = fin
        return data["kps0"], data["dsc0"], data["kps1"], data["dsc1"]

    def split_saturated(self, reset=False):
        """AMD.HEADS_DTYPE: split only: did any head activation since the last reset exceed the range of its fp16 operand planes
        (|x| > 1023) and get clamped?  Synchronises the device.  Always False in the other modes."""
        if self._sat_flag is None:
            return False
        v = bool(int(self._sat_flag.item()))
        if reset:
            self._sat_flag.zero_()
        return v

    @torch.no_grad()
    def estimate_pose(self, data, return_inliers=False, _kf=None):
        if _kf is None:
            _kf = self._keyframe_map(data)
        dev = self._anchor.device
        K0 = data["K_color0"].to(device=dev, dtype=torch.float32).contiguous()
        K1 = data["K_color1"].to(device=dev, dtype=torch.float32).contiguous()
        self._next_call()
        # data["pair_base"] (optional, int): global index of this batch's first pair -- a rank of a sharded batch passes its
        # shard offset so that the poses do not depend on the sharding (mickey_amd.distributed.shard_batch sets it)
        sol = pipeline.solve(self.cfg, data["final_scores"], data["kps0"], data["depth_kp0"], data["kps1"], data["depth_kp1"],
                             K0, K1, seed=self.seed, offset=0, offset_dev=self._ctr, pair_base=int(data.get("pair_base", 0)),
                             ws=self._ws, keyframe_index=_kf)
        if return_inliers:
            return sol["R"], sol["t"], sol["inliers"], pipeline.inliers_list(sol)
        return sol["R"], sol["t"], sol["inliers"]

    # ---- pair-list mode ---------------------------------------------------------------------------
    def _pairlist_inputs(self, data):
        """Pair-list mode (data["pair_index"]): every host check of the mode, before anything is launched (ValueError).  A pair
        list given as a device tensor is copied to the host for the check: one synchronisation.  -> (pair list as a numpy int32
        array [P, 2], N, P)."""
        from . import ops
        for k in ("image0", "image1", "keyframe_index"):
            if k in data:
                raise ValueError("pair-list mode (data['pair_index']) takes data['images'], not data[%r]" % k)
        for k in ("images", "K_color"):
            if not torch.is_tensor(data.get(k)):
                raise ValueError("pair-list mode needs the tensor data[%r]" % k)
        images, K = data["images"], data["K_color"]
        if images.dim() != 4 or images.shape[1] != 3 or images.shape[0] == 0:
            raise ValueError("data['images'] must be [N, 3, H, W] with N >= 1 (one size for the whole set), got %s" % (tuple(images.shape),))
        N = int(images.shape[0])
        if tuple(K.shape) != (N, 3, 3):
            raise ValueError("data['K_color'] must hold one 3x3 matrix per image [%d, 3, 3], got %s" % (N, tuple(K.shape)))
        pi = data["pair_index"]
        P = int(pi.shape[0]) if hasattr(pi, "shape") and len(pi.shape) else len(pi)
        if P == 0:
            raise ValueError("pair_index holds no pair")
        int(data.get("pair_base", 0))
        return ops.check_pair_index(pi, P, N), N, P

    @torch.no_grad()
    def _forward_pairlist(self, data, return_inliers=False):
        """Pair-list mode (README "Pair-list mode"): data["images"] [N, 3, H, W] are encoded ONCE (chunks of
        AMD.IMAGE_CHUNK images; an image no pair uses is still encoded), then pair p = (images[pair_index[p, 0]],
        images[pair_index[p, 1]]) is matched and solved (chunks of AMD.PAIR_CHUNK pairs on one chunk-sized workspace).  Every
        pair's result is, bit for bit, that of the standard forward on the materialised batch: one Philox call number for the
        whole forward, chunk c keyed by its global pair index, one invalid word and one mk_pose_finalize over all P poses."""
        import numpy as np
        from . import ops
        host, N, P = self._pairlist_inputs(data)
        W = self.device_weights()
        dev, amd = self._anchor.device, self.cfg["AMD"]
        ichunk, pchunk = max(1, int(amd.get("IMAGE_CHUNK", 64))), max(1, int(amd.get("PAIR_CHUNK", 32)))
        keep = bool(amd.get("PAIRLIST_SCORES", False))
        images = self._images(data["images"])
        K = data["K_color"].to(device=dev, dtype=torch.float32).contiguous()
        maps = torch.from_numpy(np.ascontiguousarray(host.T)).to(dev)   # [2, P]: the two maps of the *_pairs entry points
        self._arm_sat_flag()
        parts = []
        for lo in range(0, N, ichunk):
            im = images[lo:lo + ichunk]
            feat, gh, gw = pipeline.encoder_forward(W, self._ws, im)
            parts.append(pipeline.heads_forward(W, self._ws, feat, im.shape[0], gh, gw, self.cfg))   # fresh tensors, not workspace
        scr, kps, depth, dsc = parts[0] if len(parts) == 1 else tuple(torch.cat(c, 0) for c in zip(*parts))
        data["kps_shape"] = [gh, gw]
        data["depth_map"] = depth.reshape(N, 1, gh, gw)
        data["kps"], data["depth_kp"], data["scr"], data["dsc"] = kps, depth, scr, dsc
        data["down_factor"] = self.cfg["MICKEY"]["DINOV2"]["DOWN_FACTOR"]
        K0, K1 = K.index_select(0, maps[0].long()), K.index_select(0, maps[1].long())
        data["K_color0"], data["K_color1"] = K0, K1
        n = dsc.shape[2]
        planes = None
        if pipeline.match_uses_split(self.cfg, dsc.shape[1]):   # the set's split planes: once, not per chunk of pairs
            planes = (ops.dsc_split_planes(dsc),) * 2
        # the dense matrices: [P, n, n] outputs under AMD.PAIRLIST_SCORES, else only final_scores, in a chunk-sized buffer
        names = ("scores", "kp_scores", "final_scores")
        wants = (keep and not self.lean, keep and not self.lean, True)
        if keep:
            full = [torch.empty((P, n, n), device=dev, dtype=torch.float32) if w else None for w in wants]
        else:
            full = [self._ws.get("pairlist_" + nm, (min(pchunk, P), n, n), torch.float32, dev) if w else None for nm, w in zip(names, wants)]
        self._next_call()   # ONE call number for the forward, as one standard forward over the P pairs takes
        invalid = torch.zeros((1,), device=dev, dtype=torch.int32)
        pair_base = int(data.get("pair_base", 0))
        sols = []
        for c0 in range(0, P, pchunk):
            c1 = min(P, c0 + pchunk)
            out = tuple(None if t is None else (t[c0:c1] if keep else t[:c1 - c0]) for t in full)
            pi = (maps[0, c0:c1], maps[1, c0:c1])
            fin = pipeline.match(W, self.cfg, dsc, dsc, scr, scr, not wants[0], pair_index=pi, planes=planes, out=out)[2]
            sol = pipeline.solve(self.cfg, fin, kps, depth, kps, depth, K0[c0:c1], K1[c0:c1], seed=self.seed, offset=0,
                                 offset_dev=self._ctr, pair_base=pair_base + c0, ws=self._ws, pair_index=pi, invalid=invalid,
                                 finalize=False)
            sols.append(sol if return_inliers else {k: sol[k] for k in ("R", "t", "inliers")})
        R, t, conf = (sols[0][k] if len(sols) == 1 else torch.cat([s[k] for s in sols], 0) for k in ("R", "t", "inliers"))
        ops.pose_finalize(R, t, conf, invalid)   # the batch-level rule of the standard forward: any invalid pair zeroes all P poses
        if keep:
            data.update({nm: t_ for nm, t_ in zip(names, full) if t_ is not None})
        if return_inliers:
            data["inliers_list"] = [m for s in sols for m in pipeline.inliers_list(s)]
        data["R"], data["t"], data["inliers"] = R, t, conf
        return R, t

    def _forward_eager(self, data, return_inliers=False):
        if "pair_index" in data:
            return self._forward_pairlist(data, return_inliers)
        kf = self._keyframe_map(data)   # keyframe mode: the map is checked on the host before any launch
        self.compute_correspondences(data, _kf=kf)   # a missing / failing HIP library raises _native.MickeyHipError: never papered over
        res = self.estimate_pose(data, return_inliers, _kf=kf)
        if return_inliers:
            data["inliers_list"] = res[3]
        data["R"], data["t"], data["inliers"] = res[0], res[1], res[2]
        return res[0], res[1]

    def reseed(self, seed=None, calls=0):
        """Restart the on-device sampler streams: call number `calls` + 1 comes next (optionally with a new Philox seed).
        Two modules with equal weights, seed and call count produce bit-identical poses."""
        if seed is not None:
            if int(seed) != self.seed:
                self._graphs.clear()   # the seed is a kernel argument baked into captured graphs
            self.seed = int(seed)
        self._calls = int(calls)
        if self._ctr is not None:
            self._ctr.fill_(2 * self._calls)

    _GRAPH_INPUTS = ("image0", "image1", "K_color0", "K_color1")
    _LEAN_KEYS = ("R", "t", "inliers", "final_scores", "depth0_map", "depth1_map", "scr0", "scr1", "kps0", "kps1", "depth_kp0",
                  "depth_kp1", "kps0_shape", "kps1_shape", "down_factor")

    def _wants_graph(self, data, return_inliers):
        mode = self.graph_mode
        if mode is False or str(mode).lower() in ("false", "0", "off") or return_inliers:
            return False
        if "keyframe_index" in data:   # keyframe mode runs eager (K == B would pass the shape test below)
            return False
        if "pair_index" in data:   # pair-list mode runs eager too
            return False
        if self._anchor.device.type != "cuda" or not all(torch.is_tensor(data.get(k)) for k in self._GRAPH_INPUTS):
            return False
        if data["image0"].shape != data["image1"].shape:
            return False
        if mode is True or str(mode).lower() in ("true", "1", "on"):
            return True
        return 2 * data["image0"].shape[0] <= self.graph_max_images   # "auto": the launch-bound regime

    def _forward_graphed(self, data):
        """One hipGraph per input signature: ~330 kernel launches replayed with a single submission (a single 540x720
        pair: 7.9 -> 7.3 ms).  Inputs are copied into static buffers and everything written into `data` is cloned out of
        the graph's memory pool, so results never alias a later call."""
        dev = self._anchor.device
        key = tuple((k, tuple(data[k].shape)) for k in self._GRAPH_INPUTS) + (("pair_base", int(data.get("pair_base", 0))),)
        entry = self._graphs.get(key)
        if entry is None:
            static = {k: torch.empty(data[k].shape, device=dev, dtype=torch.float32) for k in self._GRAPH_INPUTS}
            for k in self._GRAPH_INPUTS:
                static[k].copy_(data[k])
            if "pair_base" in data:
                static["pair_base"] = int(data["pair_base"])   # a kernel argument: part of the captured graph (and of its key)
            # warm-up outside the capture (lazy weight preparation, workspace allocation, kernel attributes) without
            # consuming random-stream positions
            calls = self._calls
            self._forward_eager(dict(static))
            self._calls = calls
            self._ctr.fill_(2 * calls)
            torch.cuda.synchronize(dev)
            graph = torch.cuda.CUDAGraph()
            gdata = dict(static)
            with torch.cuda.graph(graph):
                self._forward_eager(gdata)
            self._calls = calls
            entry = (graph, static, gdata)
            self._graphs[key] = entry
            while len(self._graphs) > max(1, self.graph_cache_size):   # each entry owns a private memory pool: bound it
                self._graphs.popitem(last=False)
        self._graphs.move_to_end(key)
        graph, static, gdata = entry
        # the four inputs go into the static buffers in ONE multi-tensor launch when they are fp32 device tensors already (the
        # common case; a one-pair forward is ~330 kernels of 5.4 ms: every stray 5-us launch around the replay shows)
        srcs = [data[k] for k in self._GRAPH_INPUTS]
        if all(t.is_cuda and t.dtype == torch.float32 and t.device == dev for t in srcs):
            torch._foreach_copy_([static[k] for k in self._GRAPH_INPUTS], srcs)
        else:
            for k in self._GRAPH_INPUTS:
                static[k].copy_(data[k], non_blocking=True)
        self._calls += 1
        graph.replay()
        # everything the forward wrote is cloned out of the graph's pool (a later replay overwrites it); in LEAN mode only
        # what the inference callers read (submission.py:40-45, demo_inference.py:120-123): poses, confidence, depth / score
        # maps and keypoints, plus final_scores (the one [B, n, n] matrix LEAN keeps) -- not the descriptors.  The tensor
        # copies are ONE multi-tensor launch per dtype instead of one launch per output (17 of them in the full mode)
        keep = self._LEAN_KEYS if self.lean else None
        names, outs = [], []
        for k, v in gdata.items():
            if k not in self._GRAPH_INPUTS and (keep is None or k in keep):
                if torch.is_tensor(v):
                    names.append(k)
                    outs.append(v)
                else:
                    data[k] = copy.copy(v)
        fresh = [torch.empty_like(v) for v in outs]
        torch._foreach_copy_(fresh, outs)
        for k, t in zip(names, fresh):
            data[k] = t
        return data["R"], data["t"]

    def forward(self, data, return_inliers=False):
        if self._wants_graph(data, return_inliers):
            return self._forward_graphed(data)
        return self._forward_eager(data, return_inliers)


def build_model(cfg, checkpoint="", dinov2_weights=None):
    """reference lib/models/builder.py:5-18."""
    cfg = as_cfg(cfg)
    if cfg["MODEL"] != "MicKey":
        raise NotImplementedError()
    model = MickeyRelativePose(cfg, dinov2_weights=dinov2_weights)
    ckpt = torch.load(checkpoint, map_location="cpu", weights_only=False)  # Lightning checkpoints are pickles
    ckpt = {"state_dict": dict(ckpt["state_dict"])}
    model.on_load_checkpoint(ckpt)
    model.load_state_dict(ckpt["state_dict"])
    if torch.cuda.is_available():
        model = model.cuda()
    model.eval()
    return model
