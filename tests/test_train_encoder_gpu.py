"""-m gpu: the frozen encoder of a training step on the HIP kernels -- mk_layernorm_nchw against mk_layernorm bit for bit, the
golden tokens of the reference's DinoVisionTransformer, equality with the inference encoder, the module's calling contract
inside a reference-style extractor with a trainable torch head, and the in-place swap."""
import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _dense_nchw(x, w, b, nimg, npix, D, skip):
    """what mk_layernorm_nchw replaces: mk_layernorm, fp32, dense rows, then torch's transposition"""
    from mickey_amd import ops
    dense = ops.layernorm(x, w, b, 1e-6, out_dtype=torch.float32, rows_out=nimg * npix, rows_per_img=npix + skip, skip=skip)
    return dense.view(nimg, npix, D).permute(0, 2, 1).reshape(nimg, D, npix).contiguous()


CASES = [(1, 1, 1, 128), (2, 6, 9, 128), (3, 8, 8, 384), (5, 7, 19, 768), (2, 13, 14, 1024), (2, 38, 51, 1024)]


@pytest.mark.parametrize("skip", [0, 1])
@pytest.mark.parametrize("nimg,gh,gw,D", CASES)
def test_layernorm_nchw_equals_layernorm_bit_for_bit(nimg, gh, gw, D, skip):
    from mickey_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(100 * D + gh * gw + skip)
    npix = gh * gw
    rows = nimg * (npix + skip)
    x = (torch.randn((rows, D), generator=g) * 1.7 + 0.4 * torch.randn((rows, 1), generator=g)).to(dev)
    w = (1 + 0.2 * torch.randn((D,), generator=g)).to(dev)
    b = (0.3 * torch.randn((D,), generator=g)).to(dev)
    ref = _dense_nchw(x, w, b, nimg, npix, D, skip)
    out = ops.layernorm_nchw(x, w, b, 1e-6, nimg, npix, npix + skip, skip=skip)
    assert out.shape == (nimg, D, npix) and out.dtype == torch.float32
    assert torch.equal(out, ref)
    # round_fp16: tensor.half().float() of the same values
    lp = ops.layernorm_nchw(x, w, b, 1e-6, nimg, npix, npix + skip, skip=skip, round_fp16=True)
    assert torch.equal(lp, ref.half().float())
    # `out` inside a larger buffer, at an address that is not 16-byte aligned: nothing outside it is written
    n = nimg * D * npix
    buf = torch.full((n + 4096,), 12345.0, device=dev)
    off = 1027
    ops.layernorm_nchw(x, w, b, 1e-6, nimg, npix, npix + skip, skip=skip, out=buf[off:off + n])
    assert torch.equal(buf[off:off + n].view(nimg, D, npix), ref)
    assert bool((buf[:off] == 12345.0).all()) and bool((buf[off + n:] == 12345.0).all())
    if npix < 2:
        return
    # non-finite rows: one with a NaN, one with 1e30 (its squares overflow) -- the same elements as the dense kernel's are
    # non-finite, every other row is untouched
    xb = x.clone()
    r_nan, r_big = skip + 0, (nimg - 1) * (npix + skip) + skip + npix - 1    # first pixel of image 0, last pixel of the last image
    xb[r_nan, D // 3] = float("nan")
    xb[r_big, D - 1] = 1e30
    refb = _dense_nchw(xb, w, b, nimg, npix, D, skip)
    for rnd in (False, True):
        outb = ops.layernorm_nchw(xb, w, b, 1e-6, nimg, npix, npix + skip, skip=skip, round_fp16=rnd)
        want, clean = (refb.half().float(), ref.half().float()) if rnd else (refb, ref)
        assert torch.equal(torch.isfinite(outb), torch.isfinite(want)) and torch.equal(torch.isnan(outb), torch.isnan(want))
        assert torch.equal(torch.nan_to_num(outb), torch.nan_to_num(want))
        bad = torch.zeros((nimg, npix), dtype=torch.bool, device=dev)
        bad[0, 0] = bad[nimg - 1, npix - 1] = True
        keep = ~bad[:, None, :].expand(nimg, D, npix)
        assert not bool(torch.isfinite(outb[0, :, 0]).any()) and bool(torch.isfinite(outb[keep]).all())
        assert torch.equal(outb[keep], clean[keep])


def test_layernorm_nchw_round_fp16_overflows_to_inf():
    """values beyond fp16's range become inf as tensor.half() makes them (no saturation), subnormals survive"""
    from mickey_amd import ops
    dev = _dev()
    D, npix = 128, 70
    x = torch.randn((npix, D), generator=torch.Generator().manual_seed(5)).to(dev)
    w = torch.full((D,), 1.0, device=dev)
    w[:8] = 1e5
    w[8:16] = 1e-6
    b = torch.zeros((D,), device=dev)
    ref = _dense_nchw(x, w, b, 1, npix, D, 0)
    out = ops.layernorm_nchw(x, w, b, 1e-6, 1, npix, npix, skip=0, round_fp16=True)
    assert torch.equal(out, ref.half().float())
    assert bool(torch.isinf(out[0, :8]).any()) and bool(((out[0, 8:16] != 0) & (out[0, 8:16].abs() < 6.2e-5)).any())


def test_frozen_dinov2_golden(golden):
    """FrozenDinoV2 on the tiny arch against the reference's own DinoVisionTransformer outputs (tests/golden/vit_tiny.npz): the
    setup, dtypes and bounds of test_model_gpu.test_vit_tiny_encoder_golden."""
    from mickey_amd import synthetic as syn, train_encoder as te
    dev = _dev()
    g = golden("vit_tiny")
    sd = syn.dinov2_state_dict("vit_tiny_test", seed=3)
    img = torch.rand((2, 3, 84, 126), generator=torch.Generator().manual_seed(11)).to(dev)
    for name, tol in (("bf16", 1.5e-2), ("fp16", 2.5e-3), ("fp32", 2e-5)):
        m = te.FrozenDinoV2(sd, dtype=name).to(dev)
        tok = m.forward_features(img)["x_norm_patchtokens"]
        assert tok.shape == (2, 54, 128) and tok.dtype == torch.float32 and not tok.requires_grad
        e = rel(tok, g["tokens"])
        print("FrozenDinoV2 %s vs the reference's tokens: %.3e (bound %.1e)" % (name, e, tol))
        assert e < tol, (name, e)
        nchw = m(img)
        assert nchw.shape == (2, 128, 6, 9) and torch.equal(nchw.view(2, 128, 54).permute(0, 2, 1), tok)


@pytest.fixture(scope="module")
def vitl_sd():
    from mickey_amd import synthetic as syn
    return syn.dinov2_state_dict("vit_large", seed=2)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("fold", [True, False])
def test_same_numbers_as_the_inference_encoder(vitl_sd, dtype, fold):
    """ViT-L: encode_frozen's NCHW tensor, cast to the encoder's 16-bit type, equals the pixels of encoder_forward's bordered map
    (which is pinned against the reference and the oracle at these sizes) -- and two calls agree bit for bit."""
    from mickey_amd import ops, pipeline, train_encoder as te
    dev = _dev()
    m = te.FrozenDinoV2(vitl_sd, dtype=dtype, ln_fold=fold).to(dev)
    W = m.device_weights()
    assert W.ln_fold == fold and W.lp == m.lp_dtype
    for nimg, H, Wd in ((4, 182, 196), (2, 540, 720)):
        img = torch.rand((nimg, 3, H, Wd), generator=torch.Generator().manual_seed(H)).to(dev)
        feat, gh, gw = pipeline.encoder_forward(W, pipeline.Workspace(), img)
        want = feat[ops.bordered_index(nimg, gh, gw, dev)]                       # [nimg * gh * gw, D] lp
        out = te.encode_frozen(m, img, round_fp16=False)
        assert out.shape == (nimg, 1024, gh, gw) and out.dtype == torch.float32
        got = out.view(nimg, 1024, gh * gw).permute(0, 2, 1).reshape(-1, 1024).to(m.lp_dtype)
        assert torch.equal(got, want), (dtype, fold, H, rel(got.float(), want.float()))
        again = te.encode_frozen(m, img, round_fp16=False)
        assert again.data_ptr() != out.data_ptr() and torch.equal(again, out)
        if dtype == "fp16":   # the module's own default behind an fp16 encoder: the same values rounded to fp16
            assert torch.equal(m(img), out.half().float())
        else:
            assert torch.equal(m(img), out)


class _KeyedEncoder(nn.Module):
    """A torch module with DINOv2's state-dict keys and a forward_features -- written for this test, not the reference's class;
    its forward must never run once the swap has happened."""

    def __init__(self, sd):
        super().__init__()
        for k, v in sd.items():
            mod, parts = self, k.split(".")
            for p in parts[:-1]:
                if p not in mod._modules:
                    mod.add_module(p, nn.Module())
                mod = mod._modules[p]
            mod.register_parameter(parts[-1], nn.Parameter(v, requires_grad=False))

    def forward_features(self, x):
        raise AssertionError("the torch encoder ran")


class _Extractor(nn.Module):
    """The calling contract of the reference's extractor (mickey_extractor.py:43-58) in this test's own words: crop to a multiple
    of 14, forward_features on the amp-typed pixels under no_grad, permute / reshape / float, then a trainable torch head."""

    def __init__(self, enc, channels, amp_dtype=torch.float32):
        super().__init__()
        self.dinov2_vitl14 = enc
        self.channels, self.amp_dtype = channels, amp_dtype
        self.head = nn.Conv2d(channels, 8, 3, padding=1)
        self.features = None

    def forward(self, x):
        B, _, H, W = x.shape
        x = x[:, :, :14 * (H // 14), :14 * (W // 14)]
        with torch.no_grad():
            f = self.dinov2_vitl14.forward_features(x.to(self.amp_dtype))["x_norm_patchtokens"]
            f = f.permute(0, 2, 1).reshape(B, self.channels, H // 14, W // 14).float()
        self.features = f
        return self.head(f)


def test_module_contract_inside_an_extractor(monkeypatch):
    from mickey_amd import _native, pipeline, synthetic as syn, train_encoder as te
    dev = _dev()
    sd = syn.dinov2_state_dict("vit_tiny_test", seed=3)
    torch.manual_seed(0)
    ext = _Extractor(te.FrozenDinoV2(sd), 128).to(dev)
    made = []
    real = pipeline.encoder_features
    monkeypatch.setattr(pipeline, "encoder_features", lambda *a, **k: made.append(real(*a, **k)) or made[-1])
    g = torch.Generator().manual_seed(21)
    im0 = torch.rand((2, 3, 90, 130), generator=g).to(dev).requires_grad_(True)
    im1 = torch.rand((2, 3, 90, 130), generator=g).to(dev)
    y0 = ext(im0)
    f0 = ext.features
    # the head's input IS the kernel's output buffer: no copy between them, nothing to differentiate
    assert len(made) == 1 and f0.data_ptr() == made[0].data_ptr() and f0.shape == (2, 128, 6, 9) and f0.is_contiguous()
    assert not f0.requires_grad and f0.dtype == torch.float32
    keep = f0.clone()
    y1 = ext(im1)
    f1 = ext.features
    assert f1.data_ptr() != f0.data_ptr() and f1.untyped_storage().data_ptr() != f0.untyped_storage().data_ptr()
    assert torch.equal(f0, keep) and not torch.equal(f0, f1)
    (y0.square().mean() + y1.square().mean()).backward()
    gw = ext.head.weight.grad
    assert gw is not None and bool(torch.isfinite(gw).all()) and float(gw.abs().max()) > 0 and im0.grad is None
    assert ext.state_dict().keys() == {"head.weight", "head.bias"}
    # fp16 pixels (the reference's x.to(amp_dtype) with DINOV2.FLOAT16) are widened, not re-derived
    ext.amp_dtype = torch.float16
    ext(im0.detach())
    fh = ext.features
    ext.amp_dtype = torch.float32
    ext(im0.detach().half().float())
    assert torch.equal(fh, ext.features)
    # device moves: no CPU path, and the weights come back after .cuda()
    ext.cpu()
    with pytest.raises(_native.MickeyHipError):
        ext(im0.detach())
    ext.to(dev)
    ext(im0.detach())
    assert torch.equal(ext.features, f0)


def test_swap_end_to_end(vitl_sd):
    """use_hip_encoder on a stand-in training model with ViT-L weights, 2 pairs of 540x720."""
    from mickey_amd import train_encoder as te
    dev = _dev()

    class Model(nn.Module):
        def __init__(self):
            super().__init__()
            self.extractor = _Extractor(_KeyedEncoder(vitl_sd), 1024)

    model = Model().to(dev)
    assert te.use_hip_encoder(model) == 1 and te.use_hip_encoder(model) == 0
    enc = model.extractor.dinov2_vitl14
    assert isinstance(enc, te.FrozenDinoV2) and enc.lp_dtype == torch.bfloat16 and enc.device == dev
    assert not any("dinov2" in k for k in model.state_dict())
    g = torch.Generator().manual_seed(7)
    im0, im1 = (torch.rand((2, 3, 540, 720), generator=g).to(dev) for _ in range(2))
    model.extractor(im0)
    f0 = model.extractor.features
    model.extractor(im1)
    f1 = model.extractor.features
    a0, a1 = te.encode_frozen(enc, im0), te.encode_frozen(enc, im1)
    assert f0.shape == (2, 1024, 38, 51) and torch.equal(f0, a0) and torch.equal(f1, a1)
    # both image sets in ONE pass: row for row the two single calls.  Two calls on the same images agree bit for bit at this size
    # (test_same_numbers_as_the_inference_encoder), and nothing in the encoder ties an image's rows to the image count: a GEMM
    # output's K order does not depend on M, attention is per image, the row statistics are per row.  No dependence on the image
    # count has been observed, so the weaker bf16 bound that such a dependence would call for is not used.
    b0, b1 = te.encode_frozen(enc, [im0, im1])
    assert b0.shape == a0.shape and b1.shape == a1.shape
    print("one pass over 4 images vs two passes over 2: relative difference %.3e, %.3e" % (rel(b0, a0), rel(b1, a1)))
    assert torch.equal(b0, a0) and torch.equal(b1, a1)
