"""CPU (no GPU): the frozen-encoder hand-over for training steps -- pipeline.encoder_features' launch sequence, the argument
checks of mk_layernorm_nchw, FrozenDinoV2's checkpoint / device contract and use_hip_encoder's recognition rules."""
import os

import pytest
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def nv():
    from mickey_amd import build, _native
    if not os.path.exists(build.lib_path()):
        build.build(verbose=False)
    _native.load()
    return _native


def _record_encoder(monkeypatch, entry, fold):
    """Run pipeline.<entry> on CPU with recording stand-ins for every kernel wrapper; -> (calls, result, workspace)."""
    from mickey_amd import ops, pipeline, synthetic as syn, weights
    calls = []

    def rec(name, ret=None):
        def f(*a, **k):
            calls.append((name, a, k))
            return ret(*a, **k) if callable(ret) else ret
        return f

    def im2col(img, gh, gw, ldo, dtype, out=None):
        calls.append(("im2col", (), {}))
        return out if out is not None else torch.zeros((img.shape[0] * gh * gw, ldo), dtype=dtype)

    for nm in ("gemm_patch_embed", "cls_token", "gemm_qkv", "flash_attn", "gemm_ls_residual", "gemm", "gemm_patch_embed_ln",
               "cls_token_ln", "gemm_qkv_ln", "gemm_ls_residual_ln", "gemm_ln", "recentre_split"):
        monkeypatch.setattr(ops, nm, rec(nm))
    monkeypatch.setattr(ops, "im2col_patch14", im2col)
    monkeypatch.setattr(ops, "layernorm", rec("layernorm", lambda x, w, b, eps, out=None, **k: out))
    monkeypatch.setattr(ops, "layernorm_nchw", rec("layernorm_nchw", lambda x, w, b, eps, nimg, npix, out=None, **k: out))
    sd = syn.dinov2_state_dict("vit_tiny_test", seed=1)
    W = weights.prepare_encoder(sd, torch.device("cpu"), torch.bfloat16, prefix="", ln_fold=fold)
    ws = pipeline.Workspace()
    img = torch.rand((2, 3, 84, 126))
    res = getattr(pipeline, entry)(W, ws, img)
    return calls, res, ws


@pytest.mark.parametrize("fold", [True, False])
def test_encoder_features_launch_sequence(monkeypatch, fold):
    """encoder_features = encoder_forward's launches in encoder_forward's order on the same workspace buffers, with ONE
    mk_layernorm_nchw in place of the bordered final norm; its result is a fresh tensor, never a workspace buffer."""
    ref_calls, _, ref_ws = _record_encoder(monkeypatch, "encoder_forward", fold)
    calls, out, ws = _record_encoder(monkeypatch, "encoder_features", fold)
    names, ref_names = [c[0] for c in calls], [c[0] for c in ref_calls]
    assert ref_names[-1] == "layernorm" and names == ref_names[:-1] + ["layernorm_nchw"]
    assert all("bordered" not in c[2] for c in calls)
    # the same workspace buffers (names, shapes, dtypes) except the feature map, which encoder_features never allocates there
    assert set(ws.bufs) == {k for k in ref_ws.bufs if not k[0].startswith("feat")}
    last = calls[-1]
    nimg, npix = last[1][4], last[1][5]
    assert (nimg, npix) == (2, 54) and last[2]["skip"] == 1 and last[2]["rows_per_img"] == 55 and not last[2]["round_fp16"]
    x = last[1][0]
    assert x.dtype == torch.float32 and x.shape == (2 * 55, 128) and any(x is b for b in ws.bufs.values())
    if fold:   # the final norm reads the fp32 rows the last residual GEMM wrote
        assert x is [c for c in calls if c[0] == "gemm_ls_residual_ln"][-1][2]["x_out"]
    assert out is last[2]["out"] and out.shape == (2, 128, 6, 9) and out.dtype == torch.float32 and out.is_contiguous()
    assert all(out.data_ptr() != b.data_ptr() for b in ws.bufs.values())
    # ... and a second call hands out another tensor (a training step keeps image 0's features while image 1 is encoded)
    from mickey_amd import pipeline, synthetic as syn, weights
    W = weights.prepare_encoder(syn.dinov2_state_dict("vit_tiny_test", seed=1), torch.device("cpu"), torch.bfloat16, prefix="", ln_fold=fold)
    a = pipeline.encoder_features(W, ws, torch.rand((2, 3, 84, 126)), round_fp16=True)
    b = pipeline.encoder_features(W, ws, [torch.rand((1, 3, 84, 126)), torch.rand((1, 3, 84, 126))])
    assert a is not b and a.data_ptr() != b.data_ptr() and a.shape == b.shape == (2, 128, 6, 9)
    ln = [c for c in calls if c[0] == "layernorm_nchw"]
    assert len(ln) == 3 and ln[1][2]["round_fp16"] is True and ln[2][1][4] == 2   # two image sets of one: one pass over 2 images


def test_layernorm_nchw_rejects_bad_arguments_without_a_device(nv):
    lib = nv.load()
    assert "mk_layernorm_nchw" in nv.SIGNATURES and nv.missing_symbols() == []
    assert lib.mk_layernorm_nchw(None, 0, None, None, 1e-6, None, 0, 0, 0, 0, 0, 0, None) == 1
    assert b"layernorm_nchw" in lib.mk_last_error()
    fake = 0x100000   # never dereferenced: every call below fails its argument checks before any launch
    for nimg, npix, D, rpi, skip, ldx in ((1, 4, 130, 5, 1, 132), (1, 4, 4096, 5, 1, 4096), (0, 4, 128, 5, 1, 128), (1, 0, 128, 5, 1, 128),
                                          (1, 4, 128, 4, 1, 128), (1, 4, 128, 5, -1, 128), (1, 4, 128, 5, 1, 64), (1, 4, 128, 5, 1, 130)):
        assert lib.mk_layernorm_nchw(fake, ldx, fake, fake, 1e-6, fake, nimg, npix, D, rpi, skip, 0, None) == 1, (nimg, npix, D, rpi, skip, ldx)
        assert b"layernorm_nchw" in lib.mk_last_error()


def _tiny_sd(seed=3):
    from mickey_amd import synthetic as syn
    return syn.dinov2_state_dict("vit_tiny_test", seed=seed)


def test_frozen_dinov2_holds_no_parameters_and_validates_its_source(nv):
    from mickey_amd import train_encoder as te
    sd = _tiny_sd()
    m = te.FrozenDinoV2(sd)
    assert list(m.parameters()) == [] and list(m.buffers()) == [] and m.state_dict() == {} and not m.training
    assert m.lp_dtype == torch.bfloat16 and m.round_fp16 is False and (m.embed_dim, m.depth) == (128, 2)
    half = te.FrozenDinoV2({k: v.half() for k, v in sd.items()})
    assert half.lp_dtype == torch.float16 and half.round_fp16 is True             # 'auto': the reference's DINOV2.FLOAT16
    assert te.FrozenDinoV2(sd, dtype="fp16", features_lp=False).round_fp16 is False
    assert te.FrozenDinoV2(sd, dtype="fp32").lp_dtype == torch.float32
    # every rejected architecture names its key
    def bad(change, key):
        d = dict(sd)
        change(d)
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            te.FrozenDinoV2(d)
    bad(lambda d: d.update(register_tokens=torch.zeros(1, 4, 128)), "register_tokens")
    bad(lambda d: d.update({"blocks.0.mlp.w12.weight": torch.zeros(8, 128)}), "blocks.0.mlp.w12.weight")
    bad(lambda d: d.update({"patch_embed.proj.weight": torch.zeros(128, 3, 16, 16)}), "patch_embed.proj.weight")
    bad(lambda d: d.pop("blocks.1.ls2.gamma"), "blocks.1.ls2.gamma")
    bad(lambda d: d.pop("norm.bias"), "norm.bias")
    d96 = {k: (v[..., :96] if v.shape[-1] == 128 else v) for k, v in sd.items()}
    with pytest.raises(ValueError, match="cls_token"):
        te.FrozenDinoV2(d96)
    with pytest.raises(ValueError, match="dtype"):
        te.FrozenDinoV2(sd, dtype="int8")
    # no CPU path
    with pytest.raises(nv.MickeyHipError):
        m(torch.rand(1, 3, 28, 28))
    with pytest.raises(nv.MickeyHipError):
        m.forward_features(torch.rand(1, 3, 28, 28))
    with pytest.raises(nv.MickeyHipError):
        te.encode_frozen(m, [torch.rand(1, 3, 28, 28), torch.rand(1, 3, 28, 28)])


def test_frozen_dinov2_load_state_dict():
    from mickey_amd import train_encoder as te
    sd, other = _tiny_sd(3), _tiny_sd(4)
    m = te.FrozenDinoV2(sd)
    m._dev_weights = "stale"
    assert m.load_state_dict(other, strict=True).missing_keys == []
    assert m._dev_weights is None and torch.equal(m._sd["norm.weight"], other["norm.weight"])
    assert not torch.equal(m._sd["norm.weight"], sd["norm.weight"])
    assert m.load_state_dict({}, strict=True) is not None and torch.equal(m._sd["norm.weight"], other["norm.weight"])
    # one missing key / one misshapen key: reported by name, the held weights stay
    part = dict(sd)
    del part["blocks.0.attn.proj.bias"]
    with pytest.raises(RuntimeError, match=r"blocks\.0\.attn\.proj\.bias"):
        m.load_state_dict(part, strict=True)
    with pytest.raises(RuntimeError, match=r"blocks\.0\.attn\.proj\.bias"):
        m.load_state_dict(part, strict=False)    # never silently
    wrong = dict(sd)
    wrong["blocks.1.mlp.fc1.weight"] = torch.zeros(3, 128)
    with pytest.raises(RuntimeError, match=r"blocks\.1\.mlp\.fc1\.weight"):
        m.load_state_dict(wrong)
    assert torch.equal(m._sd["norm.weight"], other["norm.weight"])
    extra = dict(sd, **{"head.weight": torch.zeros(3)})
    with pytest.raises(RuntimeError, match=r"head\.weight"):
        m.load_state_dict(extra, strict=True)


class _TinyEncoder(nn.Module):
    """A module with DINOv2's state-dict keys and a forward_features, written for this test (not the reference's class)."""

    def __init__(self, sd):
        super().__init__()
        for k, v in sd.items():
            parts = k.split(".")
            mod = self
            for p in parts[:-1]:
                if p not in mod._modules:
                    mod.add_module(p, nn.Module())
                mod = mod._modules[p]
            mod.register_parameter(parts[-1], nn.Parameter(v.clone()))

    def forward_features(self, x):
        raise AssertionError("the torch encoder must not run after the swap")


class _Other(nn.Module):
    def __init__(self):
        super().__init__()
        self.proj = nn.Linear(4, 4)

    def forward_features(self, x):
        return {"x_norm_patchtokens": x}


class _Extractor(nn.Module):
    def __init__(self, enc):
        super().__init__()
        self.dinov2_vitl14 = enc
        self.head = nn.Conv2d(128, 8, 3, padding=1)


class _Model(nn.Module):
    def __init__(self, sd):
        super().__init__()
        self.extractor = _Extractor(_TinyEncoder(sd))
        self.unrelated = _Extractor(_Other())      # a `dinov2_vitl14` child WITHOUT the key structure
        self.side = _Other()


def test_use_hip_encoder_swaps_by_structure():
    from mickey_amd import train_encoder as te
    sd = _tiny_sd()
    model = _Model(sd)
    assert any("dinov2" in k for k in model.state_dict())
    other, side = model.unrelated.dinov2_vitl14, model.side
    model.extractor.dinov2_vitl14.half()
    assert te.use_hip_encoder(model) == 1
    enc = model.extractor.dinov2_vitl14
    assert isinstance(enc, te.FrozenDinoV2) and enc.lp_dtype == torch.float16 and enc.round_fp16   # 'auto' follows the fp16 source
    assert torch.equal(enc._sd["blocks.1.attn.qkv.weight"], sd["blocks.1.attn.qkv.weight"].half())
    assert model.unrelated.dinov2_vitl14 is other and model.side is side
    assert te.use_hip_encoder(model) == 0
    keys = set(model.state_dict())
    assert not any("extractor.dinov2" in k for k in keys) and "extractor.head.weight" in keys
    # a checkpoint saved without encoder keys loads strictly; one that carries them replaces the held weights
    ck = {k: v.clone() for k, v in model.state_dict().items()}
    assert model.load_state_dict(ck, strict=True).unexpected_keys == []
    new = _tiny_sd(5)
    ck.update({"extractor.dinov2_vitl14." + k: v for k, v in new.items()})
    model.load_state_dict(ck, strict=True)
    assert torch.equal(enc._sd["norm.bias"], new["norm.bias"])
    # the reference's device moves / train() calls pass through
    model.train()
    model.to("cpu")
    assert enc.device.type == "cpu" and enc._dev_weights is None
    # dtype override, and an unsupported architecture raises instead of being skipped
    m2 = _Model(sd)
    assert te.use_hip_encoder(m2, dtype="bf16") == 1 and m2.extractor.dinov2_vitl14.lp_dtype == torch.bfloat16
    bad = dict(sd)
    bad["register_tokens"] = torch.zeros(1, 4, 128)
    with pytest.raises(ValueError, match="register_tokens"):
        te.use_hip_encoder(_Model(bad))


def test_use_hip_encoder_recognises_the_reference_encoder():
    """Only where the reference checkout is present: its own DinoVisionTransformer at the tiny test arch."""
    from oracle import ref_shim
    if not ref_shim.available():
        pytest.skip("no reference checkout")
    import sys
    from mickey_amd import train_encoder as te
    before = set(sys.modules)
    ref_shim.install()
    try:
        from lib.models.MicKey.modules.DINO_modules.dinov2 import DinoVisionTransformer
        vit = DinoVisionTransformer(img_size=518, patch_size=14, embed_dim=128, depth=2, num_heads=2, mlp_ratio=4, init_values=1.0,
                                    ffn_layer="mlp", block_chunks=0)
    finally:
        ref_shim.uninstall()
        for name in ("cv2", "pytorch_lightning"):   # the shim's stub modules: not left behind for other tests
            if name not in before:
                sys.modules.pop(name, None)
    sd = _tiny_sd()
    vit.load_state_dict(sd, strict=True)
    vit.requires_grad_(False).eval()
    holder = nn.Module()
    holder.dinov2_vitl14 = vit
    assert te.use_hip_encoder(holder) == 1 and isinstance(holder.dinov2_vitl14, te.FrozenDinoV2)
    assert holder.dinov2_vitl14.lp_dtype == torch.bfloat16 and holder.state_dict() == {}
    for k, v in sd.items():
        if k != "mask_token":
            assert torch.equal(holder.dinov2_vitl14._sd[k], v), k
