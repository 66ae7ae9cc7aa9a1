"""mickey_amd.train_heads on the GPU: forward, input gradient and weight gradient of the trainable 3x3 convolutions against
torch's own F.conv2d (what the reference calls, utils/extractor_utils.py:18-31).

The yardstick is F.conv2d's fp64 autograd on the same inputs (on the device; on the CPU if the device has no fp64 convolution).
Bounds, relative Frobenius:
    forward          <= 2e-6                      the project's fp32-grade bound of the split conv
    gX, dW           <= max(2 * e_torch32, 2e-6)  e_torch32 = the error of torch's fp32 autograd against the same fp64 result on that
                                                  case; 2 = the margin between two fp32 summation orders of equal length
Every measured pair goes to profiles/train_conv_parity.txt."""
import copy
import os

import pytest
import torch
import torch.nn.functional as F
from torch import nn

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD_BOUND = 2e-6
RESULTS = []


@pytest.fixture(scope="module")
def th():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mickey_amd import train_heads
    yield train_heads
    if RESULTS:
        try:
            with open(os.path.join(ROOT, "profiles", "train_conv_parity.txt"), "w") as f:
                f.write("# tests/test_train_heads_gpu.py: relative Frobenius errors against F.conv2d's fp64 autograd\n")
                f.write("# bound: forward 2e-6; gradients max(2 * e_torch32, 2e-6)\n")
                f.write("# %-44s %-8s %12s %12s %12s\n" % ("case", "tensor", "e_hip", "e_torch32", "bound"))
                for r in RESULTS:
                    f.write("%-46s %-8s %12.3e %12.3e %12.3e\n" % r)
        except OSError:
            pass   # a read-only checkout: the assertions have run all the same


def _rel(a, b):
    b = b.double().cpu()
    return float((a.detach().double().cpu() - b).norm() / (b.norm() + 1e-300))


def _ref64(x, w, gy):
    """F.conv2d forward and autograd in fp64 -> (y, gX, dW) on the CPU."""
    last = None
    for dev in (x.device, torch.device("cpu")):
        try:
            xd = x.detach().to(dev, torch.float64).requires_grad_(True)
            wd = w.detach().to(dev, torch.float64).requires_grad_(True)
            y = F.conv2d(xd, wd, padding=1)
            gx, dw = torch.autograd.grad(y, (xd, wd), gy.detach().to(dev, torch.float64))
            return y.detach().cpu(), gx.cpu(), dw.cpu()
        except RuntimeError as e:   # no fp64 convolution on this device
            last = e
    raise last


def _torch32(x, w, gy):
    xd, wd = x.detach().clone().requires_grad_(True), w.detach().clone().requires_grad_(True)
    y = F.conv2d(xd, wd, padding=1)
    gx, dw = torch.autograd.grad(y, (xd, wd), gy)
    return y.detach(), gx, dw


def _hip(th, x, w, gy, x_grad=True):
    xd, wd = x.detach().requires_grad_(x_grad), w.detach().clone().requires_grad_(True)
    y = th.conv3x3_train(xd, wd)
    grads = torch.autograd.grad(y, (xd, wd) if x_grad else (wd,), gy)
    return (y.detach(), grads[0], grads[1]) if x_grad else (y.detach(), None, grads[0])


def _inputs(Cin, Cout, B, H, W, seed=0):
    g = torch.Generator().manual_seed(seed + Cin * 7 + Cout)
    x = torch.randn((B, Cin, H, W), generator=g).cuda()
    w = (torch.randn((Cout, Cin, 3, 3), generator=g) / (9 * Cin) ** 0.5).cuda()
    gy = torch.randn((B, Cout, H, W), generator=g).cuda()
    return x, w, gy


def _check(case, got, ref, t32):
    """Prints and records every figure, then asserts the bounds of the module docstring."""
    rows = []
    for name, g, r, t in zip(("y", "gX", "dW"), got, ref, t32):
        if g is None:
            continue
        e_hip, e_t = _rel(g, r), _rel(t, r)
        bound = FWD_BOUND if name == "y" else max(2 * e_t, 2e-6)
        rows.append((case, name, e_hip, e_t, bound))
        print("%s %s: e_hip %.3e  e_torch32 %.3e  bound %.3e" % rows[-1])
    RESULTS.extend(rows)
    for case, name, e_hip, e_t, bound in rows:
        assert e_hip <= bound, (case, name, e_hip, e_t, bound)


@pytest.mark.parametrize("Cin,Cout,B,H,W", [(32, 4, 1, 3, 3), (64, 64, 3, 7, 9), (128, 64, 2, 13, 5), (512, 256, 8, 38, 51),
                                            (1024, 512, 8, 38, 51)])
def test_parity_per_shape(th, Cin, Cout, B, H, W):
    x, w, gy = _inputs(Cin, Cout, B, H, W)
    got = _hip(th, x, w, gy)
    assert got[0].shape == (B, Cout, H, W) and got[0].dtype == torch.float32 and got[0].stride(1) == 1   # channels_last rows
    assert got[1].shape == x.shape and got[1].stride(1) == 1 and got[2].shape == w.shape and got[2].is_contiguous()
    _check("%d->%d %dx%dx%d" % (Cin, Cout, B, H, W), got, _ref64(x, w, gy), _torch32(x, w, gy))


@pytest.mark.parametrize("Cin,Cout,B,H,W", [(64, 64, 3, 7, 9), (64, 64, 8, 38, 51), (256, 128, 2, 13, 5)])
def test_two_runs_are_bit_identical(th, Cin, Cout, B, H, W):
    from mickey_amd import _native
    # (the first two cases take the split-K path of the weight gradient: more than one slab of partial sums)
    if Cin == 64:
        assert _native.query("mk_conv_wgrad_work_floats", Cout, Cin, B, H, W) > Cout * 9 * Cin
    x, w, gy = _inputs(Cin, Cout, B, H, W, seed=3)
    a = _hip(th, x, w, gy)
    torch.cuda.synchronize()
    b = _hip(th, x, w, gy)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_gradient_magnitude_zero_and_non_finite(th):
    Cin, Cout, B, H, W = 64, 32, 2, 9, 7
    x, w, gy = _inputs(Cin, Cout, B, H, W, seed=5)
    ref, t32 = _ref64(x, w, gy), _torch32(x, w, gy)
    base = _hip(th, x, w, gy)
    for k in (-40, 20):
        s = 2.0 ** k
        got = _hip(th, x, w, gy * s)
        # the same relative bounds at any magnitude of the incoming gradient ...
        _check("64->32 2x9x7 gY*2^%d" % k, (None, got[1] / s, got[2] / s), ref, t32)
        # ... because the plane scale follows the tensor: the results are the scaled bits
        assert torch.equal(got[1], base[1] * s) and torch.equal(got[2], base[2] * s)
    z = _hip(th, x, w, torch.zeros_like(gy))
    assert float(z[1].abs().max()) == 0.0 and float(z[2].abs().max()) == 0.0
    assert bool(torch.isfinite(z[1]).all()) and bool(torch.isfinite(z[2]).all())
    for bad in (float("nan"), float("inf")):
        g = gy.clone()
        g[1, 5, 3, 2] = bad
        got = _hip(th, x, w, g)
        assert not bool(torch.isfinite(got[2]).all()), bad
        assert not bool(torch.isfinite(got[1]).all()), bad
    # the forward stays finite and untouched by all of this
    assert torch.equal(_hip(th, x, w, gy)[0], base[0])


def test_needs_input_grad(th):
    x, w, gy = _inputs(128, 32, 2, 6, 10, seed=7)
    full = _hip(th, x, w, gy)
    only_w = _hip(th, x, w, gy, x_grad=False)
    assert only_w[1] is None and torch.equal(only_w[2], full[2]) and torch.equal(only_w[0], full[0])
    # through .backward(): no gradient lands on an input that does not require one
    xd, wd = x.detach(), w.detach().clone().requires_grad_(True)
    th.conv3x3_train(xd, wd).backward(gy)
    assert xd.grad is None and torch.equal(wd.grad, full[2])
    # a frozen weight: the input gradient alone
    xd, wd = x.detach().requires_grad_(True), w.detach()
    th.conv3x3_train(xd, wd).backward(gy)
    assert torch.equal(xd.grad, full[1])
    with torch.no_grad():
        y = th.conv3x3_train(x, w.detach().requires_grad_(True))
    assert y.grad_fn is None and torch.equal(y, full[0])


def test_layouts_give_identical_results(th):
    Cin, Cout, B, H, W = 64, 32, 2, 9, 7
    x, w, gy = _inputs(Cin, Cout, B, H, W, seed=9)
    base = _hip(th, x, w, gy)
    cl = x.contiguous(memory_format=torch.channels_last)
    assert cl.stride(1) == 1
    big = torch.randn((B, Cin + 5, H + 3, W + 4), device="cuda")
    big[:, 2:2 + Cin, 1:1 + H, 3:3 + W] = x
    sliced = big[:, 2:2 + Cin, 1:1 + H, 3:3 + W]
    assert not sliced.is_contiguous() and torch.equal(sliced, x)
    gbig = torch.zeros((B, H + 1, W, Cout + 3), device="cuda")
    gbig[:, :H, :, 1:1 + Cout] = gy.permute(0, 2, 3, 1)
    gy_sliced = gbig[:, :H, :, 1:1 + Cout].permute(0, 3, 1, 2)
    assert torch.equal(gy_sliced, gy) and not gy_sliced.is_contiguous()
    assert all(torch.equal(u, v) for u, v in zip(_hip(th, x, w, gy.contiguous()), base))
    for xin, gin in ((cl, gy), (sliced, gy), (x, gy.contiguous(memory_format=torch.channels_last)), (cl, gy_sliced),
                     (x, gy.sum(dim=(0, 2, 3), keepdim=True).expand_as(gy))):
        ref = _hip(th, x, w, gin.contiguous())
        got = _hip(th, xin, w, gin)
        for u, v in zip(got, ref):
            assert torch.equal(u, v)


def test_wrong_arguments_raise_before_any_launch(th):
    from mickey_amd import _native
    x, w, _ = _inputs(32, 4, 1, 3, 3)
    with pytest.raises(ValueError):
        th.conv3x3_train(x.half(), w)
    with pytest.raises(ValueError):
        th.conv3x3_train(x, w.double())
    with pytest.raises(ValueError):
        th.conv3x3_train(x[:, :16], w[:, :16])
    with pytest.raises(ValueError):
        th.conv3x3_train(x, w[:3])
    with pytest.raises(ValueError):
        th.conv3x3_train(x[0], w)
    with pytest.raises(ValueError):
        th.conv3x3_train(x, w[:, :, :2])
    with pytest.raises(_native.MickeyHipError):
        th.conv3x3_train(x.cpu(), w)


class _BasicBlock(nn.Module):
    """The reference's BasicBlock (utils/extractor_utils.py:18-52), restated from torch modules: conv3x3 - BN - ReLU - conv3x3 -
    BN, a 1x1 conv + BN shortcut where the channel count changes, ReLU."""

    def __init__(self, cin, cout):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, cout, 3, stride=1, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(cout)
        self.conv2 = nn.Conv2d(cout, cout, 3, stride=1, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(cout)
        self.shortcut = nn.Sequential()
        if cin != cout:
            self.shortcut = nn.Sequential(nn.Conv2d(cin, cout, 1, bias=False), nn.BatchNorm2d(cout))

    def forward(self, x):
        out = F.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        return F.relu(out + self.shortcut(x))


class _Head(nn.Module):
    def __init__(self):
        super().__init__()
        self.resblock1 = _BasicBlock(128, 64)
        self.resblock2 = _BasicBlock(64, 64)
        self.resblock3 = _BasicBlock(64, 32)
        self.score = nn.Conv2d(32, 1, 1, bias=False)

    def forward(self, x):
        return self.score(self.resblock3(self.resblock2(self.resblock1(x))))


def test_head_stack_end_to_end_and_adam_step(th):
    torch.manual_seed(11)
    ref32 = _Head().cuda().train()
    with torch.no_grad():   # BatchNorm away from its identity initialisation
        for m in ref32.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.3, 0.3)
    hip = copy.deepcopy(ref32)
    opt = torch.optim.Adam(hip.parameters(), lr=1e-2)   # made BEFORE the swap: it must keep working
    before = {n: p for n, p in hip.named_parameters()}
    assert th.use_hip_convs(hip) == 6
    assert all(p is before[n] for n, p in hip.named_parameters()) and list(hip.state_dict()) == list(ref32.state_dict())
    assert type(hip.score) is nn.Conv2d and type(hip.resblock1.shortcut[0]) is nn.Conv2d
    x = torch.randn((4, 128, 12, 10), device="cuda")
    gy = torch.randn((4, 1, 12, 10), device="cuda")

    def run(model, xin, gin):
        model.zero_grad(set_to_none=True)
        y = model(xin)
        y.backward(gin)
        return y.detach(), {n: p.grad.detach().clone() for n, p in model.named_parameters()}

    y_hip, g_hip = run(hip, x, gy)
    y_32, g_32 = run(ref32, x, gy)
    last = None
    for dev in (x.device, torch.device("cpu")):
        try:
            ref64 = copy.deepcopy(ref32).to(dev).double().train()
            y_64, g_64 = run(ref64, x.to(dev).double(), gy.to(dev).double())
            break
        except RuntimeError as e:
            last = e
    else:
        raise last
    rows = [("head stack 128->64->64->32", "y", _rel(y_hip, y_64), _rel(y_32, y_64))]
    rows += [("head stack " + n, "grad", _rel(g_hip[n], g_64[n]), _rel(g_32[n], g_64[n])) for n in g_64]
    rows = [r + (max(2 * r[3], 2e-6),) for r in rows]
    for r in rows:
        print("%s %s: e_hip %.3e  e_torch32 %.3e  bound %.3e" % r)
    RESULTS.extend(rows)
    for case, name, e_hip, e_t, bound in rows:
        assert e_hip <= bound, (case, name, e_hip, e_t, bound)
    # one Adam step updates the shared Parameters, and the swapped modules read the new values
    w_before = hip.resblock1.conv1.weight.detach().clone()
    opt.step()
    assert hip.resblock1.conv1.weight is before["resblock1.conv1.weight"]
    assert not torch.equal(hip.resblock1.conv1.weight.detach(), w_before)
    assert len(opt.state) == len(before)
    with torch.no_grad():
        y2 = hip(x)
    assert bool(torch.isfinite(y2).all()) and not torch.equal(y2, y_hip)
