"""CPU (no GPU): host logic and the C-ABI surface -- the library loads and exports every symbol
include/mickey_hip.h declares, argument validation works without a device, config / checkpoint
contract, BatchNorm folding, the lib.* drop-in import paths."""
import copy
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def nv():
    from mickey_amd import build, _native
    if not os.path.exists(build.lib_path()):
        build.build(verbose=False)
    _native.load()
    return _native


def test_abi_exports_every_declared_symbol(nv):
    hdr = open(os.path.join(ROOT, "include", "mickey_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)   # declarations only
    declared = set(re.findall(r"\b(mk_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(nv.SIGNATURES), declared ^ set(nv.SIGNATURES)
    # the dev knobs are declared in their own header, not in the drop-in ABI
    dev = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mickey_hip_dev.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(mk_[a-z0-9_]+)\s*\(", dev)) == set(nv.DEV_SIGNATURES)
    assert not (declared & set(nv.DEV_SIGNATURES))
    assert nv.missing_symbols() == []
    assert nv.query("mk_version") >= 100
    # arity of every binding == arity of the C declaration
    for name, (_, args) in nv.SIGNATURES.items():
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, hdr, re.S)
        assert m, name
        params = [p for p in m.group(1).split(",") if p.strip() and p.strip() != "void"]
        assert len(params) == len(args), (name, len(params), len(args))


def test_abi_rejects_bad_arguments_without_a_device(nv):
    lib = nv.load()
    assert lib.mk_gemm(None, 0, None, 0, None, None, 0, 0, 0, 0, 0, 0, 0, None) == 1
    assert b"gemm" in lib.mk_last_error()
    assert lib.mk_layernorm(None, 0, None, None, 1e-6, None, 0, 0, None, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, None) == 1
    assert nv.query("mk_bordered_rows", 2, 9, 7) == (2 * 10 + 1) * 8 + 1
    assert lib.mk_conv3x3(None, 0, 64, None, 0, 0, None, 0, 0, None, 0, None, 0, None, 64, 0, 1, 1, 4, 4, 0, 3, 0, None) == 1   # out_kind 3
    # row partials (4 column chunks) + column partials (1 row block) + final LSE vectors + pad + the stored correlation
    assert nv.query("mk_dual_softmax_work_floats", 2, 10, 12, 1) == 2 * 4 * 10 * 2 + 2 * 1 * 12 * 2 + 2 * 2 * 12 + 4 + 2 * 10 * 12
    assert nv.query("mk_dual_softmax_work_floats", 2, 10, 12, 0) == 2 * 4 * 10 * 2 + 2 * 1 * 12 * 2 + 2 * 2 * 12 + 4
    assert nv.query("mk_exprace_topk_work_bytes", 1, 20, 2048, 1938 * 1938) > 20 * 8192 * 8 + 1938 * 1938 // 16 * 4
    with pytest.raises(nv.MickeyHipError):
        nv.call("mk_flash_attn_fwd", None, None, None, None, 0, 0, 0, 0, 0, 0, None)


def test_missing_library_fails_loudly(monkeypatch):
    from mickey_amd import _native
    monkeypatch.setattr(_native, "_lib", None)
    monkeypatch.setenv("MICKEY_HIP_LIB", "/nonexistent/libmickey_hip.so")
    with pytest.raises(_native.MickeyHipError):
        _native.load()


def test_cfg_access_styles(cfg):
    from mickey_amd.config import as_cfg, CfgDict
    assert cfg.PROCRUSTES.IT_RANSAC == 100 and cfg["PROCRUSTES"]["IT_MATCHES"] == 20
    assert cfg.MICKEY.DINOV2.CHANNEL_DIM == 1024 and cfg["FEATURE_MATCHER"]["TYPE"] == "DualSoftmax"
    # yacs-style schema: None everywhere must not clobber defaults; real overrides win
    c = as_cfg({"MODEL": "MicKey", "PROCRUSTES": {"IT_RANSAC": 10, "IT_MATCHES": None}, "TRAINING": {"LR": None}})
    assert c.PROCRUSTES.IT_RANSAC == 10 and c.PROCRUSTES.IT_MATCHES == 20 and isinstance(c.PROCRUSTES, CfgDict)
    d = copy.deepcopy(c)
    d.PROCRUSTES.IT_RANSAC = 3
    assert c.PROCRUSTES.IT_RANSAC == 10


def test_bn_fold_matches_basic_block(cfg):
    """weights.fold_basic_block + a conv == the oracle's conv-BN-ReLU-conv-BN-add block."""
    from mickey_amd import synthetic as syn, weights
    from oracle import mickey_oracle as O
    sd = syn.heads_state_dict(cfg, seed=1)
    p = "compute_matches.extractor.det_head.resblock3."
    x = torch.randn((2, 256, 7, 6), generator=torch.Generator().manual_seed(0))
    ref = O.basic_block(sd, p, x)
    w1, b1, w2, b2, has_sc = weights.fold_basic_block(sd, p)
    assert has_sc and w1.shape == (128, 9 * 256) and w2.shape == (128, 9 * 128 + 256)
    def conv(inp, wflat, cin):
        w = wflat.reshape(wflat.shape[0], 3, 3, cin).permute(0, 3, 1, 2)
        return F.conv2d(inp, w, padding=1)
    h = F.relu(conv(x, w1, 256) + b1.view(1, -1, 1, 1))
    y = conv(h, w2[:, : 9 * 128], 128) + F.conv2d(x, w2[:, 9 * 128:].reshape(128, 256, 1, 1)) + b2.view(1, -1, 1, 1)
    assert torch.allclose(F.relu(y), ref, rtol=1e-4, atol=1e-4)


def test_checkpoint_contract_and_dropin_imports(cfg, tmp_path):
    from mickey_amd import synthetic as syn
    from lib.models.builder import build_model
    from lib.models.MicKey.compute_pose import MickeyRelativePose
    sd = syn.mickey_state_dict(cfg, arch="vit_tiny_test")
    dino = {k.split("dinov2_vitl14.", 1)[1]: v for k, v in sd.items() if "dinov2_vitl14." in k}
    mickey_only = {k: v for k, v in sd.items() if "dinov2" not in k}      # what a MicKey .ckpt holds
    ck = tmp_path / "mickey.ckpt"
    torch.save({"state_dict": mickey_only, "pytorch-lightning_version": "2.0"}, ck)
    model = build_model(cfg, str(ck), dinov2_weights=dino)
    assert isinstance(model, MickeyRelativePose) and not model.training
    assert set(model.state_dict()) == set(sd)
    assert model.e2e_Procrustes.num_samples_matches == 2048
    assert next(model.parameters()).device.type == "cpu"
    # (lib.utils.data.data_to_model_device stays the reference's own file: it only needs next(model.parameters()).device)
    with pytest.raises(RuntimeError):
        MickeyRelativePose(cfg).load_state_dict(mickey_only)   # no DINOv2 weights anywhere
    with pytest.raises(NotImplementedError):
        bad = copy.deepcopy(cfg)
        bad["MODEL"] = "other"
        build_model(bad, str(ck))


def test_planted_pose_generator_is_consistent():
    from mickey_amd import synthetic as syn
    from oracle import mickey_oracle as O
    data, R, t = syn.planted_pose_problem(B=1, h=20, w=16, seed=3)
    fs = data["final_scores"][0]
    i, j = torch.nonzero(fs > 1e-7, as_tuple=True)
    assert len(i) > 50
    X = O.backproject(data["kps0"][0, :, i].t()[None], data["depth_kp0"][0, 0, i][None, :, None], data["K_color0"])
    Y = O.backproject(data["kps1"][0, :, j].t()[None], data["depth_kp1"][0, 0, j][None, :, None], data["K_color1"])
    assert float(O.point_dist(X, Y, R, t).max()) < 2e-3


def test_intrinsics_rescale_matches_the_reference_formula():
    """mickey_amd.input_pipeline.correct_intrinsic_scale == reference lib/datasets/utils.py:86-99 (restated in
    oracle/input_oracle.py; identical when imported from the reference tree where it exists)."""
    import numpy as np
    import torch
    from mickey_amd import input_pipeline as ip
    from oracle import input_oracle as IO
    K = torch.tensor([[549.7018, 0.0, 268.6665], [0.0, 549.7018, 351.8357], [0.0, 0.0, 1.0]])
    for sx, sy in ((1.0, 1.0), (0.5, 0.5), (196 / 540, 182 / 720), (2.0, 1.5)):
        assert torch.equal(ip.correct_intrinsic_scale(K, sx, sy), IO.correct_intrinsic_scale(K, sx, sy))
    # the oracle's cv2-exact resize (pinned in tests/test_input_oracle_cpu.py): identity and constant images
    img = np.full((7, 9, 3), 37, np.uint8)
    assert np.array_equal(IO.resize_u8(img, 9, 7), img)
    assert (IO.resize_u8(img, 20, 15) == 37).all()


def test_no_product_kernel_spills_registers():
    """Per-kernel register report of the build (hipcc -Rpass-analysis=kernel-resource-usage -> build/resource_usage.json).
    All epilogues of a GEMM kernel share ONE register allocation: a variant over 256 VGPRs makes hipcc spill the
    accumulators of every tile of every launch (it happened: +25 % on all GEMMs of the forward, profiles/README.md, round 2).
    No kernel of the library is exempt.  The report is written by build(); a checkout whose objects were built elsewhere
    (no json) skips."""
    import glob
    import os
    from mickey_amd import build as B
    usage = B.resource_usage()
    srcs = [os.path.basename(p) for p in glob.glob(os.path.join(B.CSRC, "*.hip"))]
    if any(s not in usage for s in srcs):
        pytest.skip("no register report for %s (run python -m mickey_amd.build --force)" % [s for s in srcs if s not in usage])
    seen = 0
    for src, kernels in usage.items():
        for k in kernels:
            seen += 1
            # SGPR spills go to spare VGPR lanes (v_writelane), not to memory: a few dozen in cold kernels are tolerated; the one
            # large case is named -- lse_partial_kernel<false>, the exact-fp32 matcher for descriptor widths != 128 (its 64
            # operand registers per side leave the scalar unit no VGPR-free bookkeeping): not on the benchmarked path
            # ... and the persistent instantiations of the 256x256 GEMM (tile loop around K loop + epilogue: the kernel arguments and
            # the tile walk stay in scalar registers across both; none of the lane reads sits in the steady-state K loop)
            allowed = 400 if "lse_partial_kernelILb0E" in k["name"] else 64
            if "gemm_pp64_kernel" in k["name"]:
                # template arguments parsed out of the mangled name -- <T, AMODE, KIND, PERSIST, SP, SP2> -- and a signature change must
                # fail HERE, not move a kernel into another bucket silently (round 5 keyed on the substring 'ELb1E')
                m = re.search(r"gemm_pp64_kernelI(DF16b|DF16_)Li(\d)ELi(\d)ELb([01])ELb([01])ELb([01])EE", k["name"])
                assert m, "gemm_pp64_kernel's template signature changed: update this parser (%s)" % k["name"]
                persist = m.group(4) == "1"
                allowed = 144 if persist else 64   # measured: 68 - 137 in the persistent instantiations (tile loop around K loop +
                #                                    epilogue), 0 in the others
            assert k.get("sgpr_spill", 0) <= allowed, (src, k)
            assert k.get("vgpr_spill", 0) == 0, (src, k)
            # no private memory at all (round 3 had 32 B / lane in every GEMM kernel: SROA kept a 16-byte slice of the by-value
            # GemmParams -- qscale | pos | npatch -- as an alloca because `f32x4 *= p.qscale` loaded it as <1 x float>)
            assert k.get("scratch", 0) == 0, (src, k)
    assert seen > 40 and any("gemm_pp64_kernel" in k["name"] for k in usage.get("mk_gemm_pp64.hip", []))


def test_fold_layernorm_is_an_identity():
    """weights.fold_layernorm: LN(x) @ W^T + b == rstd * (x @ W'^T) - rstd * mean * colsum + b' (what mk_gemm_ln evaluates),
    checked with un-rounded folded weights; with the 16-bit rounding of W' the difference stays at that rounding."""
    import torch
    import torch.nn.functional as F
    from mickey_amd import weights
    g = torch.Generator().manual_seed(3)
    M, D, N = 40, 128, 96
    x = (torch.randn((M, D), generator=g) * 2 + 1.3).double()
    x[:, 5] += 30
    lw, lb = (1 + 0.3 * torch.randn((D,), generator=g)).double(), (0.2 * torch.randn((D,), generator=g)).double()
    W, b = (torch.randn((N, D), generator=g) / D ** 0.5).double(), torch.randn((N,), generator=g).double()
    ref = F.layer_norm(x, (D,), lw, lb, 1e-6) @ W.t() + b
    mean = x.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(x.var(1, unbiased=False, keepdim=True) + 1e-6)
    wf, cs, bf = weights.fold_layernorm(W, b, lw, lb, torch.float64)
    out = rstd * (x @ wf.t()) - rstd * mean * cs + bf
    assert float((out - ref).abs().max()) < 1e-5   # the fold itself works in fp32
    wf16, cs16, bf16 = weights.fold_layernorm(W.float(), b.float(), lw.float(), lb.float(), torch.bfloat16)
    assert wf16.dtype == torch.bfloat16 and torch.equal(cs16, wf16.float().sum(1))   # colsum of the ROUNDED weights
    out16 = rstd * (x @ wf16.double().t()) - rstd * mean * cs16.double() + bf16.double()
    assert float((out16 - ref).norm() / ref.norm()) < 2 ** -8


def test_encoder_launch_sequence_with_and_without_the_fold(monkeypatch):
    """pipeline.encoder_forward wiring on CPU with recording stand-ins for the kernels: with the LayerNorm fold the block is
    qkv_ln -> attention -> residual_ln -> gemm_ln(GELU) -> residual_ln, fed from the split stream, the LAST residual GEMM
    writes fp32 rows for the final norm and no LayerNorm kernel runs inside a block; without it the plain sequence."""
    import torch
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
    sd = syn.dinov2_state_dict("vit_tiny_test", seed=1)
    img = torch.rand((2, 3, 84, 126))
    for fold in (True, False):
        W = weights.prepare_encoder(sd, torch.device("cpu"), torch.bfloat16, prefix="", ln_fold=fold)
        assert W.ln_fold == fold and hasattr(W.blocks[0], "qkv_wf") == fold
        calls.clear()
        feat, gh, gw = pipeline.encoder_forward(W, pipeline.Workspace(), img)
        names = [c[0] for c in calls]
        assert (gh, gw) == (6, 9) and feat.shape == (ops.bordered_rows(2, 6, 9), 128)   # bordered feature map
        assert calls[-1][2]["bordered"] == (2, 6, 9)
        if fold:
            assert names == ["im2col", "gemm_patch_embed_ln", "cls_token_ln", "recentre_split"] + \
                ["gemm_qkv_ln", "flash_attn", "gemm_ls_residual_ln", "gemm_ln", "gemm_ls_residual_ln"] * W.depth + ["layernorm"]
            res = [c for c in calls if c[0] == "gemm_ls_residual_ln"]
            assert [c[2].get("x_out") is not None for c in res] == [False] * (2 * W.depth - 1) + [True]
            xh = calls[1][1][4]
            assert all(c[1][0] is xh for c in calls if c[0] in ("gemm_qkv_ln", "gemm_ln"))    # consumers read the hi plane
            assert calls[-1][1][0] is res[-1][2]["x_out"]                                     # the final norm reads the fp32 rows
            # row centring: every consumer publishes into the buffer every producer reads
            sh = res[0][2]["shift"]
            assert sh is not None and sh.shape == (2 * 55,) and all(c[2]["shift"] is sh for c in res)
            assert all(c[2]["shift_out"] is sh for c in calls if c[0] in ("gemm_qkv_ln", "gemm_ln"))
            # bench.py's work / byte accounting accepts exactly these call signatures (a mismatch only shows on the GPU box)
            import bench
            prof = bench.StageProfiler()

            class _Ops:
                pass
            fake = _Ops()
            for nm in ("gemm", "gemm_ls_residual", "gemm_qkv", "gemm_patch_embed", "gemm_ln", "gemm_qkv_ln", "gemm_ls_residual_ln",
                       "gemm_patch_embed_ln", "flash_attn", "conv3x3", "conv3x3_split", "split_planes", "gemm_grouped_split", "gemm_grouped", "gemm_ln128",
                           "layernorm",
                       "dual_softmax", "sinkhorn",
                       "exprace_topk", "gather_backproject", "ransac_hypotheses", "refine_pose"):
                setattr(fake, nm, lambda *a, **k: None)
            ev = type("E", (), {"record": lambda self: None, "elapsed_time": lambda self, o: 1.0})
            monkeypatch.setattr(torch.cuda, "Event", lambda enable_timing=True: ev())
            prof.wrap(fake)
            prof.on = True
            for nm, a, k in calls:
                if hasattr(fake, nm):
                    getattr(fake, nm)(*a, **k)
            stages, by = prof.summary(1)
            assert by["encoder_gemm"]["launches"] == 1 + 4 * W.depth and by["encoder_gemm"]["bytes"] > 0
        else:
            assert names == ["im2col", "gemm_patch_embed", "cls_token"] + \
                ["layernorm", "gemm_qkv", "flash_attn", "gemm_ls_residual", "layernorm", "gemm", "gemm_ls_residual"] * W.depth + ["layernorm"]
    # fp32 operands never fold (the exact parity mode keeps LayerNorm as its own kernel)
    assert not weights.prepare_encoder(sd, torch.device("cpu"), torch.float32, prefix="", ln_fold=True).ln_fold


def test_bordered_index_matches_the_library():
    """the torch-side index helper (tests, tools) and mk_bordered_rows describe the same layout"""
    from mickey_amd import ops
    for nimg, H, W in ((1, 1, 1), (2, 9, 7), (3, 4, 11)):
        idx = ops.bordered_index(nimg, H, W, "cpu")
        assert idx.shape == (nimg * H * W,) and len(set(idx.tolist())) == idx.numel()
        R = ops.bordered_rows(nimg, H, W)
        assert R == (nimg * (H + 1) + 1) * (W + 1) + 1
        # every 3x3 neighbour of every pixel is inside the buffer and is either a pixel of the same image or a border row
        pix = set(idx.tolist())
        for i, r in enumerate(idx.tolist()):
            b, y, x = i // (H * W), (i // W) % H, i % W
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    n = r + dy * (W + 1) + dx
                    assert 0 <= n < R
                    inside = 0 <= y + dy < H and 0 <= x + dx < W
                    assert (n in pix) == inside
                    if inside:
                        assert n == idx[(b * H + y + dy) * W + x + dx]


def test_split_operand_scheme_is_fp32_grade():
    """The arithmetic behind mk_conv3x3_split / mk_gemm_grouped_split / mk_dual_softmax_split, emulated on the CPU with the
    host-side preparation the product uses (weights.split_conv_weight): x * 64 and w * scale as hi + lo fp16 planes, the three
    products hi.hi + lo.hi + hi.lo with fp32-or-better accumulation, scaled back by 1 / (64 scale).  The dropped lo.lo term and
    the planes' rounding leave ~22 bits: <= 2e-6 relative against the exact fp64 product -- also for weights so large
    (BatchNorm folded over a tiny variance) that the plane scale has to come down, and for activations near the planes' range."""
    import torch
    from mickey_amd import ops, weights
    g = torch.Generator().manual_seed(0)
    for wmag, xmag in ((0.05, 1.0), (30.0, 1.0), (0.05, 150.0)):   # |x| * 64 stays inside fp16 (the planes clamp beyond +-1023)
        K, Cout, M = 1152, 96, 200
        w = torch.randn((Cout, K), generator=g) * wmag
        x = torch.randn((M, K), generator=g) * xmag
        sw = weights.split_weight_scale(w)
        assert sw == 2.0 ** round(math.log2(sw)) and float(w.abs().max()) * sw <= 32768.0
        planes = weights.split_conv_weight(w, sw)                 # [Cout, 2K]: per 32 columns, 32 hi then 32 lo values
        assert planes.shape == (Cout, 2 * K) and planes.dtype == torch.float16
        w_hi, w_lo = (t.double() for t in weights.split_conv_weight_planes(planes))
        assert torch.equal(planes[:, 64:96], w_hi[:, 32:64].half()) and torch.equal(planes[:, 96:128], w_lo[:, 32:64].half())
        assert torch.equal(w_hi.float(), (w * sw).half().float())
        xs = x * ops.SPLIT_ACT_SCALE
        x_hi = xs.clamp(-65504.0, 65504.0).to(torch.float16)
        x_lo = (xs - x_hi.float()).to(torch.float16)
        acc = x_lo.double() @ w_hi.t() + x_hi.double() @ w_lo.t() + x_hi.double() @ w_hi.t()
        out = acc / (ops.SPLIT_ACT_SCALE * sw)
        ref = x.double() @ w.double().t()
        err = float((out - ref).norm() / ref.norm())
        assert err < 2e-6, (wmag, xmag, err)


def test_natural_batch_statistics_and_determinism():
    """synthetic.natural_batch (bench.py's `natural` leg): images in [0, 1] with a 1/f amplitude spectrum -- neighbouring pixels
    correlated, unlike synthetic_batch's white noise -- same intrinsics, deterministic in the seed."""
    import torch
    from mickey_amd import synthetic as syn
    a = syn.natural_batch(B=2, H=126, W=98, seed=7)
    b = syn.natural_batch(B=2, H=126, W=98, seed=7)
    c = syn.synthetic_batch(B=2, H=126, W=98, seed=7)
    assert set(a) == set(c) and a["image0"].shape == (2, 3, 126, 98) and torch.equal(a["K_color0"], c["K_color0"])
    assert torch.equal(a["image0"], b["image0"]) and not torch.equal(a["image0"], a["image1"])
    assert float(a["image0"].min()) >= 0.0 and float(a["image0"].max()) <= 1.0 and 0.3 < float(a["image0"].mean()) < 0.6

    def neighbour_corr(img):
        x = img[:, :, :, :-1].reshape(-1) - img.mean()
        y = img[:, :, :, 1:].reshape(-1) - img.mean()
        return float((x * y).mean() / (x.std() * y.std()))
    assert neighbour_corr(a["image0"]) > 0.6 and abs(neighbour_corr(c["image0"])) < 0.05


def test_features_lp_resolution():
    """AMD.FEATURES_LP: auto = fp16 features behind an fp16 encoder with split heads only (the reference's data flow,
    mickey_extractor.py:49-52); explicit true / false; anything else is refused."""
    import copy
    import torch
    from mickey_amd.config import default_cfg
    from mickey_amd.model import MickeyRelativePose, resolve_features_lp
    cfg = default_cfg()
    assert resolve_features_lp(cfg, torch.float16) and not resolve_features_lp(cfg, torch.bfloat16)
    for enc, heads, flp, want in (("fp16", "split", None, True), ("bf16", "split", None, False), ("fp16", "auto", None, False),
                                  ("fp16", "split", False, False), ("bf16", "split", True, True)):
        c = copy.deepcopy(cfg)
        c["AMD"]["ENCODER_DTYPE"], c["AMD"]["HEADS_DTYPE"] = enc, heads
        if flp is not None:
            c["AMD"]["FEATURES_LP"] = flp
        assert MickeyRelativePose(c).features_lp == want, (enc, heads, flp)
    c = copy.deepcopy(cfg)
    c["AMD"]["FEATURES_LP"] = "sometimes"
    with pytest.raises(ValueError):
        resolve_features_lp(c, torch.float16)


# ---- the binding is derived from the headers (mickey_amd/_native.py: parse_header) --------------------------------------------
_ABI_PROBE = r"""
#include <cstdio>
#include <type_traits>
#include "mickey_hip.h"
#include "mickey_hip_dev.h"
template <class T> constexpr char code(bool result) {
  return result && std::is_same<T, const char*>::value ? 's'
       : std::is_pointer<T>::value ? 'p'
       : std::is_same<T, int>::value ? 'i'
       : std::is_same<T, long long>::value ? 'l'
       : std::is_same<T, float>::value ? 'f'
       : std::is_same<T, unsigned long long>::value ? 'u' : '?';
}
template <class R, class... A> void show(const char* name, R (*)(A...)) {
  const char args[] = {code<A>(false)..., 0};
  std::printf("%s %c %s\n", name, code<R>(true), args);
}
int main() {
@SHOWS@
  return 0;
}
"""


def _host_cxx():
    """the first of c++ on PATH and the clang++ that hipcc drives (present wherever the library can be built)"""
    import shutil
    from mickey_amd import build
    hipcc = shutil.which(build.hipcc()) or build.hipcc()
    bindir = os.path.dirname(os.path.realpath(hipcc))
    for c in (shutil.which("c++"), os.path.join(bindir, "clang++"), os.path.join(bindir, "..", "lib", "llvm", "bin", "clang++"),
              os.path.join(os.path.dirname(hipcc), "..", "lib", "llvm", "bin", "clang++")):
        if c and os.path.exists(c):
            return c
    pytest.fail("no host C++ compiler: neither c++ on PATH nor a clang++ beside %s" % hipcc)


def test_abi_binding_matches_the_compilers_view(tmp_path):
    """Every letter code of SIGNATURES / DEV_SIGNATURES against what a C++ compiler makes of the same headers: decltype(&mk_name)
    taken apart with <type_traits>.  Types only -- nothing is linked -- and no regular expression shared with the parser."""
    import subprocess
    from mickey_amd import _native
    table = {**_native.SIGNATURES, **_native.DEV_SIGNATURES}
    assert len(table) == len(_native.SIGNATURES) + len(_native.DEV_SIGNATURES) > 100
    src, exe = tmp_path / "abi_probe.cpp", tmp_path / "abi_probe"
    src.write_text(_ABI_PROBE.replace("@SHOWS@", "\n".join('  show("%s", static_cast<decltype(&%s)>(nullptr));' % (n, n) for n in table)))
    subprocess.run([_host_cxx(), "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout
    seen = {}
    for line in out.splitlines():
        name, res, *args = line.split(" ")
        seen[name] = (res, "".join(args))
    assert set(seen) == set(table)
    for name in table:
        assert seen[name] == table[name], (name, seen[name], table[name])
        assert len(_native.PARAM_NAMES[name]) == len(table[name][1]) and all(_native.PARAM_NAMES[name]), name


def test_abi_parser_is_strict():
    from mickey_amd import _native
    P, E = _native.parse_header, _native.MickeyHipError
    ok = P('#ifdef __cplusplus\nextern "C" {\n#endif\ntypedef void* mk_stream_t; /* a stream */\nenum { MK_A = 0, MK_B = 3 };\n'
           "#define MK_C 7\ntypedef struct mk_row { float *p, *g; long long n; double lr; } mk_row;\n"
           "const char* mk_text(void);\nlong long mk_f(const char* name, const unsigned char* src, unsigned long long seed,\n"
           "                  float eps, long long n, int k, mk_stream_t stream);\n#ifdef __cplusplus\n}\n#endif\n")
    assert ok.signatures == {"mk_text": ("s", ""), "mk_f": ("l", "ppuflip")}   # a const char* PARAMETER is a pointer
    assert ok.params["mk_f"] == ("name", "src", "seed", "eps", "n", "k", "stream") and ok.params["mk_text"] == ()
    assert ok.constants == {"MK_A": 0, "MK_B": 3, "MK_C": 7}
    assert ok.structs == {"mk_row": [("p", "q"), ("g", "q"), ("n", "q"), ("lr", "d")]}
    for bad, quoted in (("int mk_f(short n);", "short n"),                                   # a scalar outside the set
                        ("int mk_f(unsigned n);", "unsigned n"),
                        ("short mk_f(int n);", "short mk_f"),
                        ("void mk_f(int n);", "void mk_f"),
                        ("int mk_f(int n, float);", "float"),                                # parameters without a name
                        ("int mk_f(const float*, int n);", "const float*"),
                        ("int mk_f(long long);", "long long"),
                        ("int mk_f(int n);\nint mk_f(int n);", "mk_f"),                      # a duplicate prototype
                        ("enum { MK_A = 0 };\nenum { MK_A = 1 };", "MK_A"),
                        ("#define MK_A 0\nenum { MK_A = 1 };", "MK_A"),
                        ("#define MK_A (1 << 2)\nint mk_f(int n);", "MK_A"),                 # constants are plain integers
                        ("enum { MK_A, MK_B };", "MK_A"),
                        ("int mk_f(int n);\nint mk_count;", "mk_count"),                     # statements that are no prototype
                        ("typedef int mk_int;\nint mk_f(int n);", "typedef int mk_int"),
                        ("int mk_f(int n);\nstatic int helper(void);", "helper"),
                        ("int mk_f(int (*cb)(int));", "cb"),
                        ("int mk_f(int n)", "mk_f"),                                         # (no terminating semicolon)
                        ("typedef struct mk_row { float* p; int flags; } mk_row;", "int flags"),   # a struct field of unknown type
                        ("typedef struct mk_row { float x; } mk_row;", "float x")):
        with pytest.raises(E) as err:
            P(bad)
        assert quoted in str(err.value), (bad, str(err.value))


def test_abi_recentre_split_rows_are_long_long():
    """the one entry the hand-written table had wrong: (..., long long rows, int D, int dtype, stream)"""
    from mickey_amd import _native
    assert _native.SIGNATURES["mk_recentre_split"] == ("i", "pppliip")
    assert _native.PARAM_NAMES["mk_recentre_split"] == ("xh", "xl", "stats", "rows", "D", "dtype", "stream")


def test_abi_constants_come_from_the_headers():
    from mickey_amd import _native, ops, train_optim
    found = {}
    for h in ("mickey_hip.h", "mickey_hip_dev.h"):
        raw = open(os.path.join(ROOT, "include", h)).read()
        found.update((k, int(v)) for k, v in re.findall(r"\b(MK_[A-Z0-9_]+) = (\d+)", raw) + re.findall(r"#define (MK_[A-Z0-9_]+) (\d+)", raw))
    assert len(found) >= 22 and found == _native.CONSTANTS
    for name, value in found.items():
        assert getattr(_native, name) is _native.CONSTANTS[name] and getattr(_native, name) == value, name
    for mod, alias, c_name in [(_native, "MK_" + k, "MK_" + k) for k in ("BF16", "F16", "F32")] + \
            [(m, "ACT_" + k, "MK_ACT_" + k) for m in (_native, ops) for k in ("NONE", "RELU", "GELU")] + \
            [(ops, "CONV_OUT_" + k, "MK_CONV_OUT_" + k) for k in ("DENSE", "BORDERED", "F32")] + \
            [(ops, "TAIL_" + k, "MK_TAIL_" + k) for k in ("IDENTITY", "SIGMOID", "MASKED_SIGMOID", "SOFTMAX")] + \
            [(train_optim, "FLAG_" + k, "MK_OPTIM_" + k) for k in ("NORM", "PARAM")]:
        assert getattr(mod, alias) is _native.CONSTANTS[c_name], (mod.__name__, alias)
    # the values the kernels were built against
    assert (_native.MK_BF16, _native.MK_F16, _native.MK_F32) == (0, 1, 2) and (ops.ACT_NONE, ops.ACT_RELU, ops.ACT_GELU) == (0, 1, 2)
    assert (ops.CONV_OUT_DENSE, ops.CONV_OUT_BORDERED, ops.CONV_OUT_F32) == (0, 1, 2)
    assert (ops.TAIL_IDENTITY, ops.TAIL_SIGMOID, ops.TAIL_MASKED_SIGMOID, ops.TAIL_SOFTMAX) == (0, 1, 2, 3)
    assert (train_optim.FLAG_NORM, train_optim.FLAG_PARAM) == (1, 2)
    assert train_optim._ROW.format == "=qqqqqqdddddq" and [f for f, _ in _native.STRUCTS["mk_optim_row"]] == \
        ["p", "g", "m", "v", "step", "numel", "lr", "beta1", "beta2", "eps", "weight_decay", "flags"]


def test_abi_call_names_the_c_parameter_and_query_checks_exports(nv, monkeypatch):
    with pytest.raises(nv.MickeyHipError, match=r"mk_layernorm: argument 13 'rows_per_img'"):
        nv.call("mk_layernorm", None, 0, None, None, 1e-6, None, 0, 0, None, 0, 0, 0, "seven", 0, 0, 0, 0, 0, 0, None)
    monkeypatch.setattr(nv, "_missing", {"mk_bordered_rows"})   # a stale library: the symbol is declared, not exported
    for fn in (nv.call, nv.query):
        with pytest.raises(nv.MickeyHipError, match="does not export mk_bordered_rows"):
            fn("mk_bordered_rows", 1, 1, 1)
