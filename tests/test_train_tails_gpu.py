"""mickey_amd.train_tails on the GPU: the four trainable head tails (forward and every gradient), the ops under guard windows, the
invariances the module promises, and the swap.

The yardstick is the *_formula of mickey_amd.train_tails (the in-repo restatement of mickey_extractor.py:98-124,134-140,172-176,
211-216,248-249, checked against the reference's own fp64 autograd by tests/test_train_tails_cpu.py) under fp64 autograd on the
device, on the same inputs.  For every output and every gradient

    e = max |x - x64| / max |x64|   <=   max(2 * e_torch32, 2e-6)

e_torch32 = the same error of the same formula run by torch in fp32 on the same GPU; 2e-6 = the project's fp32-grade bound
(DESIGN.md section 4).  No element is left out.  Every measured figure goes to profiles/train_tails_parity.txt.

Inputs: relu(randn) features (channels_last), weights randn / sqrt(C), a randn gradient.  A weight gradient sums rows in chunks of
ops.HEADTAIL_CHUNK_ROWS: the shapes below include one row less, exactly that many and one more, and 3876 rows (19 chunks).

Two detector shapes are degenerate and are stated as conditions, not tolerances: (1, 7, 7) has ONE interior pixel -- the softmax is
1 there and 0 elsewhere, the true gradient is cancellation noise at the 1e-19 level, and torch fp32's own relative error on it is
1.0 -- and (1, 6, 8) has none: output and gradients are exact zeros."""
import copy
import os

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from tests.helpers.guarded import guarded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FLOOR = 2e-6
RESULTS = []
VARIANTS = ("softmax", "masked_sigmoid", "offset", "depth", "depth_sigmoid")
COUT = {"offset": 2}


@pytest.fixture(scope="module")
def tt():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mickey_amd import train_tails
    yield train_tails
    if RESULTS:
        try:
            with open(os.path.join(ROOT, "profiles", "train_tails_parity.txt"), "w") as f:
                f.write("# tests/test_train_tails_gpu.py: max |x - x64| / max |x64| against the *_formula of mickey_amd.train_tails under fp64 autograd;\n")
                f.write("# bound: max(2 * e_torch32, 2e-6), e_torch32 = the same formula in torch fp32 on the same GPU\n")
                f.write("# %-44s %-12s %12s %12s %12s\n" % ("case", "tensor", "e_hip", "e_torch32", "bound"))
                for r in RESULTS:
                    f.write("%-46s %-12s %12.3e %12.3e %12.3e\n" % r)
        except OSError:
            pass   # a read-only checkout: the assertions have run all the same


def _fns(tt, variant):
    """(the HIP op, the plain-torch formula) of a 1x1 tail variant, both (feat, weight) -> out"""
    if variant == "softmax":
        return (lambda f, w: tt.score_tail_train(f, w)), (lambda f, w: tt.score_tail_formula(f, w))
    if variant == "masked_sigmoid":
        return (lambda f, w: tt.score_tail_train(f, w, use_softmax=False)), (lambda f, w: tt.score_tail_formula(f, w, use_softmax=False))
    if variant == "offset":
        return tt.offset_tail_train, tt.offset_tail_formula
    if variant == "depth":
        return tt.depth_tail_train, tt.depth_tail_formula
    return (lambda f, w: tt.depth_tail_train(f, w, True, 60.0)), (lambda f, w: tt.depth_tail_formula(f, w, True, 60.0))


def _draw(variant, B, C, H, W, seed=0):
    """(feat channels_last [B, C, H, W], weight [Cout, C, 1, 1], go [B, Cout, H, W]) on the device"""
    g = torch.Generator().manual_seed(1000 * seed + 7 * B + 31 * H + 131 * W + C + VARIANTS.index(variant))
    cout = COUT.get(variant, 1)
    feat = torch.relu(torch.randn((B, C, H, W), generator=g)).cuda().contiguous(memory_format=torch.channels_last)
    w = (torch.randn((cout, C, 1, 1), generator=g) / C ** 0.5).cuda()
    go = torch.randn((B, cout, H, W), generator=g).cuda()
    return feat, w, go


def _draw_desc(B, C, H, W, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + 7 * B + 31 * H + 131 * W + C)
    x = torch.randn((B, C, H, W), generator=g).cuda().contiguous(memory_format=torch.channels_last)
    return x, torch.randn((B, C, H, W), generator=g).cuda()


def _run(fn, ins, go, dtype=torch.float32):
    """(out, the gradient of every input) of fn(*ins) in `dtype`"""
    leaves = [t.detach().to(dtype).requires_grad_(True) for t in ins]   # (fp32: the very storage, its layout is part of the test)
    out = fn(*leaves)
    return (out.detach(),) + tuple(torch.autograd.grad(out, leaves, go.to(dtype)))


def _err(a, ref):
    ref = ref.detach().double()
    return float((a.detach().double() - ref).abs().max() / ref.abs().max())


def _check(case, names, got, ref, t32):
    """Prints and records every figure, then asserts the bound of the module docstring."""
    assert len(names) == len(got) == len(ref) == len(t32)
    rows = []
    for name, g, r, t in zip(names, got, ref, t32):
        assert g.shape == r.shape and g.dtype == torch.float32, (case, name)
        e_hip, e_t = _err(g, r), _err(t, r)
        rows.append((case, name, e_hip, e_t, max(2 * e_t, FLOOR)))
        print("%s %s: e_hip %.3e  e_torch32 %.3e  bound %.3e" % rows[-1])
    RESULTS.extend(rows)
    for case, name, e_hip, e_t, bound in rows:
        assert e_hip <= bound, (case, name, e_hip, e_t, bound)


def _chunk_shapes():
    """one row less than a weight-gradient chunk, exactly one chunk, one row more -- read from ops, not guessed"""
    from mickey_amd import ops
    R = ops.HEADTAIL_CHUNK_ROWS
    shapes = []
    for rows in (R - 1, R, R + 1):
        h = next(h for h in range(7, 24) if rows % h == 0 and rows // h >= 7)   # (both sides keep interior pixels)
        shapes.append((1, h, rows // h))
    return shapes


# ---- 1: parity of every tail --------------------------------------------------------------------------------------------------
SHAPES = [(2, 8, 9, 64), (1, 7, 9, 64), (3, 9, 7, 64), (2, 38, 51, 64), (2, 8, 9, 4), (2, 8, 9, 128), (2, 8, 9, 256)]


@pytest.mark.parametrize("B,H,W,C", SHAPES)
def test_tail_parity_per_shape(tt, B, H, W, C):
    for variant in VARIANTS:
        hip, formula = _fns(tt, variant)
        feat, w, go = _draw(variant, B, C, H, W)
        got = _run(hip, (feat, w), go)
        assert got[0].shape == (B, COUT.get(variant, 1), H, W) and got[2].shape == w.shape
        _check("%s B%d %dx%d C%d" % (variant, B, H, W, C), ("out", "gfeat", "gw"), got, _run(formula, (feat, w), go, torch.float64),
               _run(formula, (feat, w), go))


def test_tail_parity_either_side_of_a_weight_gradient_chunk(tt):
    from mickey_amd import ops
    shapes = _chunk_shapes()
    assert [b * h * w for b, h, w in shapes] == [ops.HEADTAIL_CHUNK_ROWS - 1, ops.HEADTAIL_CHUNK_ROWS, ops.HEADTAIL_CHUNK_ROWS + 1]
    assert [ops.headtail_chunks(b * h * w) for b, h, w in shapes] == [1, 1, 2]
    for B, H, W in shapes:
        for variant in VARIANTS:
            hip, formula = _fns(tt, variant)
            feat, w, go = _draw(variant, B, 64, H, W)
            _check("%s B%d %dx%d C64 (%d rows)" % (variant, B, H, W, B * H * W), ("out", "gfeat", "gw"), _run(hip, (feat, w), go),
                   _run(formula, (feat, w), go, torch.float64), _run(formula, (feat, w), go))


@pytest.mark.parametrize("B,H,W,C", [(2, 7, 9, 128), (1, 8, 8, 128), (1, 5, 13, 128), (2, 38, 51, 128), (2, 5, 13, 64)])   # n = 63, 64, 65: the tile is 64 pixels
def test_desc_l2norm_parity(tt, B, H, W, C):
    x, go = _draw_desc(B, C, H, W)
    got = _run(tt.desc_l2norm_train, (x,), go)
    assert got[0].shape == (B, C, H, W) and got[0].is_contiguous() and got[0].view(B, C, H * W).is_contiguous()
    _check("desc B%d %dx%d C%d" % (B, H, W, C), ("out", "gx"), got, _run(tt.desc_l2norm_formula, (x,), go, torch.float64),
           _run(tt.desc_l2norm_formula, (x,), go))


def test_parity_on_the_golden_fixture(tt):
    import numpy as np
    z = np.load(os.path.join(ROOT, "tests", "golden", "head_tails_grad.npz"))
    for case, variant in (("score_softmax", "softmax"), ("score_sigmoid", "masked_sigmoid"), ("offset", "offset"), ("depth", "depth"),
                          ("depth_sigmoid", "depth_sigmoid")):
        hip, formula = _fns(tt, variant)
        feat, w, go = (torch.from_numpy(z[k + case]).cuda() for k in ("x_", "w_", "go_"))
        stored = tuple(torch.from_numpy(z[k + case]).cuda() for k in ("out_", "gx_", "gw_"))   # the reference's own autograd
        _check("golden " + case, ("out", "gfeat", "gw"), _run(hip, (feat, w), go), stored, _run(formula, (feat, w), go))
    x, go = torch.from_numpy(z["x_desc"]).cuda(), torch.from_numpy(z["go_desc"]).cuda()
    stored = tuple(torch.from_numpy(z[k + "desc"]).cuda() for k in ("out_", "gx_"))
    _check("golden desc", ("out", "gx"), _run(tt.desc_l2norm_train, (x,), go), stored, _run(tt.desc_l2norm_formula, (x,), go))


# ---- 2: the two degenerate detector shapes ------------------------------------------------------------------------------------
def test_one_interior_pixel(tt):
    feat, w, go = _draw("softmax", 1, 64, 7, 7)
    out, gfeat, gw = _run(_fns(tt, "softmax")[0], (feat, w), go)
    want = torch.zeros((1, 1, 7, 7), device="cuda")
    want[0, 0, 3, 3] = 1
    assert float((out - want).abs().max()) <= 1e-6 and float(out.sum() - out[0, 0, 3, 3]) == 0.0
    assert bool(torch.isfinite(gfeat).all()) and bool(torch.isfinite(gw).all())
    assert float(gfeat.abs().max()) <= 1e-6 * float(go.abs().max()) * float(w.abs().max())


def test_no_interior_pixel(tt):
    for variant in ("softmax", "masked_sigmoid"):
        feat, w, go = _draw(variant, 1, 64, 6, 8)
        for t in _run(_fns(tt, variant)[0], (feat, w), go):
            assert not bool(torch.isnan(t).any()) and float(t.abs().max()) == 0.0, variant


# ---- 3: the ops inside guard windows ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,C", [(1, 7, 9, 64), (2, 8, 9, 4)])   # 63 rows: a ragged last wave; C = 4: one lane of a row's sixteen
def test_tail_ops_stay_inside_their_outputs(tt, B, H, W, C):
    from mickey_amd import ops
    n = H * W
    acts = {"softmax": (ops.TAIL_SOFTMAX, 1.0), "masked_sigmoid": (ops.TAIL_MASKED_SIGMOID, 1.0), "offset": (ops.TAIL_SIGMOID, 1.0),
            "depth": (ops.TAIL_IDENTITY, 1.0), "depth_sigmoid": (ops.TAIL_SIGMOID, 60.0)}
    for variant in VARIANTS:
        hip, _ = _fns(tt, variant)
        feat, w, go = _draw(variant, B, C, H, W)
        want = _run(hip, (feat, w), go)
        act, scale = acts[variant]
        cout = w.shape[0]
        rows2d, w2d = feat.permute(0, 2, 3, 1).reshape(B * n, C), w.view(cout, C)
        out, chk_out = guarded(B * cout, n, torch.float32, "cuda")
        ops.train_headtail_fwd(rows2d, w2d, B, H, W, act, scale, 3, 100.0, 1e-16, out=out)
        chk_out()
        assert torch.equal(out.view(B, cout, H, W), want[0]), variant
        chunks = ops.headtail_chunks(B * n)
        gfeat, chk_gf = guarded(B * n, C, torch.float32, "cuda")
        gw, chk_gw = guarded(cout, C, torch.float32, "cuda")
        part, chk_part = guarded(chunks, cout * C, torch.float32, "cuda")
        ops.train_headtail_bwd(go.contiguous(), out, rows2d, w2d, B, n, act, scale, 100.0, gfeat=gfeat, gw=gw, part=part.view(-1))
        for chk in (chk_gf, chk_gw, chk_part, chk_out):
            chk()
        assert torch.equal(gfeat.view(B, H, W, C).permute(0, 3, 1, 2), want[1]) and torch.equal(gw.view(w.shape), want[2]), variant
        assert chunks == 1 and torch.equal(part[0], gw.view(-1))


@pytest.mark.parametrize("B,H,W,C", [(2, 5, 13, 128), (1, 5, 13, 4), (1, 7, 9, 256)])   # n = 65 and 63; C = 4; two channel slabs
def test_desc_ops_stay_inside_their_outputs(tt, B, H, W, C):
    from mickey_amd import ops
    n = H * W
    x, go = _draw_desc(B, C, H, W)
    want = _run(tt.desc_l2norm_train, (x,), go)
    rows2d = x.permute(0, 2, 3, 1).reshape(B * n, C)
    y, chk_y = guarded(B * C, n, torch.float32, "cuda")
    _, rnorm = ops.train_desc_l2norm_fwd(rows2d, B, n, 1e-10, out=y)
    chk_y()
    assert torch.equal(y.view(B, C, H, W), want[0]) and rnorm.shape == (B * n,)
    gx, chk_gx = guarded(B * n, C, torch.float32, "cuda")
    ops.train_desc_l2norm_bwd(go.contiguous(), y, rnorm, B, n, C, out=gx)
    chk_gx()
    chk_y()
    assert torch.equal(gx.view(B, H, W, C).permute(0, 3, 1, 2), want[1])
    _check("desc B%d %dx%d C%d" % (B, H, W, C), ("out", "gx"), want, _run(tt.desc_l2norm_formula, (x,), go, torch.float64),
           _run(tt.desc_l2norm_formula, (x,), go))


# ---- 4: determinism and invariances ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_tail_invariances(tt, variant):
    hip, _ = _fns(tt, variant)
    B, C, H, W = 3, 64, 9, 8
    feat, w, go = _draw(variant, B, C, H, W)
    out, gfeat, gw = _run(hip, (feat, w), go)
    for a, b in zip((out, gfeat, gw), _run(hip, (feat, w), go)):
        assert torch.equal(a, b)                                                  # two runs: the same bits
    for i in range(B):                                                            # image i alone: its forward and gfeat bits
        o1, g1, _ = _run(hip, (feat[i:i + 1], w), go[i:i + 1])
        assert torch.equal(o1[0], out[i]) and torch.equal(g1[0], gfeat[i]), i
    for scale in (2.0 ** -40, 2.0 ** 20):                                         # bit-linear in the incoming gradient
        _, gs, ws = _run(hip, (feat, w), go * scale)
        assert torch.equal(gs, gfeat * scale) and torch.equal(ws, gw * scale), scale
    _, g0, w0 = _run(hip, (feat, w), torch.zeros_like(go))
    assert float(g0.abs().max()) == 0.0 and float(w0.abs().max()) == 0.0          # a zero gradient: exact zeros
    bad = go.clone()
    bad[1, :, 4, 4] = float("nan")                                                # an interior pixel of image 1
    _, gn, wn = _run(hip, (feat, w), bad)
    assert bool(torch.isnan(wn).all())
    assert bool(torch.isnan(gn[1, :, 4, 4]).all()) and (variant != "softmax" or bool(torch.isnan(gn[1]).all()))
    assert torch.equal(gn[0], gfeat[0]) and torch.equal(gn[2], gfeat[2])          # the other images: bit for bit


def test_desc_invariances(tt):
    B, C, H, W = 3, 128, 5, 13
    x, go = _draw_desc(B, C, H, W)
    out, gx = _run(tt.desc_l2norm_train, (x,), go)
    for a, b in zip((out, gx), _run(tt.desc_l2norm_train, (x,), go)):
        assert torch.equal(a, b)
    for i in range(B):
        o1, g1 = _run(tt.desc_l2norm_train, (x[i:i + 1],), go[i:i + 1])
        assert torch.equal(o1[0], out[i]) and torch.equal(g1[0], gx[i]), i
    for scale in (2.0 ** -40, 2.0 ** 20):
        assert torch.equal(_run(tt.desc_l2norm_train, (x,), go * scale)[1], gx * scale), scale
    assert float(_run(tt.desc_l2norm_train, (x,), torch.zeros_like(go))[1].abs().max()) == 0.0
    bad = go.clone()
    bad[1, 5, 2, 3] = float("nan")
    gn = _run(tt.desc_l2norm_train, (x,), bad)[1]
    assert bool(torch.isnan(gn[1, :, 2, 3]).all())
    keep = torch.ones((B, H, W), dtype=torch.bool, device="cuda")
    keep[1, 2, 3] = False
    assert torch.equal(gn.permute(0, 2, 3, 1)[keep], gx.permute(0, 2, 3, 1)[keep])   # every other pixel row: bit for bit


# ---- 5: layouts -------------------------------------------------------------------------------------------------------------------
def test_layouts(tt):
    B, C, H, W = 2, 64, 8, 9
    for variant in VARIANTS:
        hip, _ = _fns(tt, variant)
        feat, w, go = _draw(variant, B, C, H, W)
        assert feat.is_contiguous(memory_format=torch.channels_last) and not feat.is_contiguous()
        leaf = feat.detach().requires_grad_(True)
        out = hip(leaf, w.detach().requires_grad_(True))
        saved = out.grad_fn.saved_tensors
        assert saved[0].data_ptr() == feat.data_ptr() and saved[0].shape == feat.shape          # read in place, kept as it is
        assert saved[1].data_ptr() == w.data_ptr() and len(saved) == (2 if variant == "depth" else 3)
        (gfeat,) = torch.autograd.grad(out, [leaf], go)
        assert gfeat.is_contiguous(memory_format=torch.channels_last)
        want = _run(hip, (feat, w), go)
        nchw = feat.contiguous()
        assert nchw.is_contiguous() and torch.equal(nchw, feat)
        for a, b in zip(_run(hip, (nchw, w), go), want):
            assert torch.equal(a, b), variant                                                 # a contiguous NCHW input: the same bits
    x, go = _draw_desc(B, 128, H, W)
    leaf = x.detach().requires_grad_(True)
    out = tt.desc_l2norm_train(leaf)
    assert out.is_contiguous() and out.view(B, 128, H * W).is_contiguous()
    saved = out.grad_fn.saved_tensors
    assert len(saved) == 2 and saved[0].data_ptr() == out.data_ptr() and tuple(saved[1].shape) == (B * H * W,)
    (gx,) = torch.autograd.grad(out, [leaf], go)
    assert gx.is_contiguous(memory_format=torch.channels_last)
    for a, b in zip(_run(tt.desc_l2norm_train, (x.contiguous(),), go), (out.detach(), gx)):
        assert torch.equal(a, b)


# ---- 6: needs_input_grad, no_grad ---------------------------------------------------------------------------------------------
def test_only_the_gradients_asked_for(tt, monkeypatch):
    from mickey_amd import ops
    calls = []
    orig = ops.train_headtail_bwd

    def spy(*a, **k):
        res = orig(*a, **k)
        calls.append((k["want_gfeat"], k["want_gw"], res[0] is None, res[1] is None))
        return res
    monkeypatch.setattr(ops, "train_headtail_bwd", spy)
    for variant in VARIANTS:
        hip, _ = _fns(tt, variant)
        feat, w, go = _draw(variant, 2, 64, 8, 9)
        _, gfeat, gw = _run(hip, (feat, w), go)
        del calls[:]
        f = feat.detach().requires_grad_(True)                                   # a frozen weight: no weight-gradient work
        (g,) = torch.autograd.grad(hip(f, w.detach()), [f], go)
        assert torch.equal(g, gfeat) and calls == [(True, False, False, True)], (variant, calls)
        del calls[:]
        ww = w.detach().requires_grad_(True)                                     # a feature map without grad: no gfeat pass
        (g,) = torch.autograd.grad(hip(feat.detach(), ww), [ww], go)
        assert torch.equal(g, gw) and calls == [(False, True, True, False)], (variant, calls)
        packed = []
        with torch.autograd.graph.saved_tensors_hooks(lambda t: packed.append(t) or t, lambda t: t):
            with torch.no_grad():
                out = hip(feat.detach().requires_grad_(True), w.detach().requires_grad_(True))
            assert out.grad_fn is None and not out.requires_grad and packed == []
            out = hip(feat.detach(), w.detach())                                 # nothing asks for a gradient: nothing kept
            assert out.grad_fn is None and packed == []
    x, _ = _draw_desc(2, 128, 8, 9)
    packed = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: packed.append(t) or t, lambda t: t):
        with torch.no_grad():
            out = tt.desc_l2norm_train(x.detach().requires_grad_(True))
        assert out.grad_fn is None and packed == []
        out = tt.desc_l2norm_train(x.detach().requires_grad_(True))
        assert out.grad_fn is not None and len(packed) == 2


# ---- 7: the training forward against the inference kernels ------------------------------------------------------------------------
@pytest.mark.parametrize("use_softmax,use_depth_sigmoid", [(True, False), (False, True)])
def test_forward_agrees_with_the_inference_tails(tt, use_softmax, use_depth_sigmoid):
    from mickey_amd import ops
    B, H, W, C, Cd, down = 2, 38, 51, 64, 128, 14.0
    n = H * W
    f_det, w_sc, _ = _draw("softmax", B, C, H, W, seed=1)
    f_off, w_xy, _ = _draw("offset", B, C, H, W, seed=1)
    f_dep, w_d, _ = _draw("depth", B, C, H, W, seed=1)
    f_dsc, _ = _draw_desc(B, Cd, H, W, seed=1)
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(B * n, t.shape[1])   # noqa: E731
    scr, kps, depth, dsc = ops.head_tails(rows(f_det), w_sc.view(-1), rows(f_off), w_xy.view(2, C), rows(f_dep), w_d.view(-1), rows(f_dsc), B, H, W,
                                          C, Cd, border=3, use_softmax=use_softmax, use_depth_sigmoid=use_depth_sigmoid, max_depth=60.0,
                                          norm_dsc=True, down=down)
    with torch.no_grad():
        t_scr = tt.score_tail_train(f_det, w_sc, 3, use_softmax)
        t_off = tt.offset_tail_train(f_off, w_xy)
        t_dep = tt.depth_tail_train(f_dep, w_d, use_depth_sigmoid, 60.0)
        t_dsc = tt.desc_l2norm_train(f_dsc)
    cell = torch.stack([torch.arange(W, device="cuda").repeat(H), torch.arange(H, device="cuda").repeat_interleave(W)]).float()   # x row, y row
    t_kps = (t_off.view(B, 2, n) + cell) * down       # the absolute-coordinate step of the inference kernel
    for name, a, b in (("scr", t_scr.view(B, 1, n), scr), ("kps", t_kps, kps), ("depth", t_dep.view(B, 1, n), depth)):
        e = _err(a, b)
        print("train vs inference %s (softmax %s, depth sigmoid %s): %.3e" % (name, use_softmax, use_depth_sigmoid, e))
        assert e <= 1e-6, (name, e)
    assert torch.equal(t_dsc.view(B, Cd, n), dsc)     # the descriptors: bit for bit


# ---- 8: the swap, end to end ------------------------------------------------------------------------------------------------------
class _Stub(nn.Module):
    """stands in for a BasicBlock: smooth, so that no kink separates the precisions"""
    def __init__(self, cin, cout):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, cout, 1, bias=False)

    def forward(self, x, relu=True):
        x = self.conv1(x)
        return F.softplus(x) if relu else x


class _Att(nn.Module):
    def forward(self, x):
        return x


class _Head(nn.Module):
    """A head with the reference's attribute names and none of its code; its forward restates the tail with the formulas."""
    def __init__(self, kind):
        super().__init__()
        self.kind_ = kind
        self.resblock1, self.resblock2, self.resblock3 = _Stub(32, 32), _Stub(32, 32), _Stub(32, 32)
        self.resblock4 = _Stub(32, 128 if kind == "desc" else 64)
        self.sigmoid = nn.Sigmoid()
        if kind in ("softmax", "masked_sigmoid"):
            self.score = nn.Conv2d(64, 1, 1, bias=False)
            self.use_softmax, self.tmp_softmax = kind == "softmax", 100
            self.eps = nn.Parameter(torch.tensor(1e-16), requires_grad=False)
            self.offset_par1 = nn.Parameter(torch.tensor(0.5), requires_grad=False)
            self.offset_par2 = nn.Parameter(torch.tensor(2.), requires_grad=False)
            self.ones_kernel = nn.Parameter(torch.ones((1, 1, 3, 3)), requires_grad=False)
        elif kind == "offset":
            self.xy_offset = nn.Conv2d(64, 2, 1, bias=False)
        elif kind in ("depth", "depth_sigmoid"):
            self.depth = nn.Conv2d(64, 1, 1, bias=False)
            self.use_depth_sigmoid, self.max_depth = kind == "depth_sigmoid", 60
        else:
            self.norm_desc = True
        self.att_layer = _Att()

    def forward(self, x):
        from mickey_amd import train_tails as tt
        x = self.att_layer(self.resblock3(self.resblock2(self.resblock1(x))))
        if self.kind_ == "desc":
            return tt.desc_l2norm_formula(self.resblock4(x, relu=False))
        x = self.resblock4(x)
        if self.kind_ in ("softmax", "masked_sigmoid"):
            return tt.score_tail_formula(x, self.score.weight, 3, self.use_softmax, self.tmp_softmax, float(self.eps))
        if self.kind_ == "offset":
            return tt.offset_tail_formula(x, self.xy_offset.weight)
        return tt.depth_tail_formula(x, self.depth.weight, self.use_depth_sigmoid, self.max_depth)


@pytest.mark.parametrize("kind", VARIANTS + ("desc",))
def test_swapped_head_matches_the_unswapped_module(tt, kind):
    torch.manual_seed(VARIANTS.index(kind) if kind in VARIANTS else 9)
    holder = nn.ModuleDict({"head": _Head(kind)}).cuda()
    g = torch.Generator().manual_seed(3)
    x = torch.randn((2, 32, 8, 9), generator=g).cuda()
    go = torch.randn((2, {"offset": 2, "desc": 128}.get(kind, 1), 8, 9), generator=g).cuda()

    def run(module, dtype):
        module = module.to(dtype)
        params = [p for p in module.parameters() if p.requires_grad]
        out = module(x.to(dtype))
        return (out.detach(),) + tuple(torch.autograd.grad(out, params, go.to(dtype)))
    ref = run(copy.deepcopy(holder["head"]), torch.float64)
    t32 = run(holder["head"], torch.float32)
    names = ("out",) + tuple("g:" + n for n, p in holder["head"].named_parameters() if p.requires_grad)
    keys = list(holder.state_dict().keys())
    assert tt.use_hip_tails(holder) == 1 and type(holder["head"]) is tt.HipHead and list(holder.state_dict().keys()) == keys
    got = run(holder["head"], torch.float32)
    assert got[0].is_contiguous() or kind != "desc"
    _check("swapped head " + kind, names, got, ref, t32)
