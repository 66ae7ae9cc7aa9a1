"""mickey_amd.train_heads without a GPU: the formulas the kernels implement against fp64 autograd, the weight-plane layout, the
swap contract of use_hip_convs and the C ABI's argument checks."""
import os
import re

import pytest
import torch
import torch.nn.functional as F
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ("mk_conv3x3_split_dscale", "mk_absmax_scale_work_floats", "mk_absmax_scale", "mk_conv_train_lead_rows",
               "mk_conv_train_plane_rows", "mk_conv_train_planes", "mk_conv_train_weight_planes", "mk_conv_wgrad_work_floats",
               "mk_conv_wgrad")


@pytest.fixture(scope="module")
def nv():
    from mickey_amd import build, _native
    if not os.path.exists(build.lib_path()):
        build.build(verbose=False)
    _native.load()
    return _native


def _autograd64(x, w, gy):
    x = x.clone().requires_grad_(True)
    w = w.clone().requires_grad_(True)
    y = F.conv2d(x, w, padding=1)
    gx, dw = torch.autograd.grad(y, (x, w), gy)
    return y.detach(), gx, dw


@pytest.mark.parametrize("B,Cin,Cout,H,W", [(1, 3, 2, 3, 3), (2, 5, 4, 4, 7), (3, 8, 6, 6, 5), (1, 4, 4, 1, 1)])
def test_formulas_match_fp64_autograd(B, Cin, Cout, H, W):
    from mickey_amd import train_heads as th
    g = torch.Generator().manual_seed(B * 100 + Cin)
    x = torch.randn((B, Cin, H, W), generator=g, dtype=torch.float64)
    w = torch.randn((Cout, Cin, 3, 3), generator=g, dtype=torch.float64)
    gy = torch.randn((B, Cout, H, W), generator=g, dtype=torch.float64)
    _, gx, dw = _autograd64(x, w, gy)
    # dgrad: a plain 3x3 convolution of gY with the flipped / transposed weight
    wt = th.dgrad_weight(w)
    assert tuple(wt.shape) == (Cin, Cout, 3, 3)
    assert float((F.conv2d(gy, wt, padding=1) - gx).abs().max()) <= 1e-12 * max(1.0, float(gx.abs().max()))
    # wgrad: the sum over ALL bordered rows, one row shift per tap
    got = th.wgrad_bordered(x, gy)
    assert tuple(got.shape) == (Cout, Cin, 3, 3)
    assert float((got - dw).abs().max()) <= 1e-12 * max(1.0, float(dw.abs().max()))


def test_bordered_map_is_the_library_layout(nv):
    from mickey_amd import ops, train_heads as th
    B, C, H, W = 2, 3, 4, 5
    x = torch.arange(B * C * H * W, dtype=torch.float64).reshape(B, C, H, W) + 1
    xb = th.bordered_map(x)
    assert xb.shape[0] == nv.query("mk_bordered_rows", B, H, W)
    idx = ops.bordered_index(B, H, W, "cpu")
    assert torch.equal(xb[idx], x.permute(0, 2, 3, 1).reshape(-1, C))
    mask = torch.ones(xb.shape[0], dtype=torch.bool)
    mask[idx] = False
    assert float(xb[mask].abs().max()) == 0.0
    # the plane buffers of the training kernels: Wd + 2 rows in front, whole K steps of 32 rows + Wd + 2 behind
    R = (B * (H + 1) + 1) * (W + 1) + 1
    assert nv.query("mk_conv_train_lead_rows", W) == W + 2
    assert nv.query("mk_conv_train_plane_rows", B, H, W) == (W + 2) + (R + 31) // 32 * 32 + (W + 2)


def test_weight_planes_are_split_conv_weight_of_the_tap_major_weight():
    from mickey_amd import train_heads as th, weights
    g = torch.Generator().manual_seed(5)
    w = torch.randn((8, 64, 3, 3), generator=g)
    pl = th.weight_planes(w, 256.0)
    assert pl.dtype == torch.float16 and tuple(pl.shape) == (8, 2 * 9 * 64)
    tap_major = w.permute(0, 2, 3, 1).reshape(8, 9 * 64)   # column tap * Cin + ci, as weights.fold_basic_block lays them out
    assert torch.equal(pl, weights.split_conv_weight(tap_major, 256.0))
    hi, lo = weights.split_conv_weight_planes(pl)
    assert float(((hi.double() + lo.double()) / 256.0 - tap_major.double()).abs().max()) < 2.0 ** -20
    # transposed: the planes of the input gradient's conv, Cout padded to 32 with zero columns
    plt = th.weight_planes(w, 256.0, transposed=True)
    assert tuple(plt.shape) == (64, 2 * 9 * 32)
    hi, lo = weights.split_conv_weight_planes(plt)
    back = ((hi.double() + lo.double()) / 256.0).reshape(64, 3, 3, 32)
    assert float(back[..., 8:].abs().max()) == 0.0
    wt = th.dgrad_weight(w.double())   # [Cin, Cout, 3, 3]
    assert float((back[..., :8].permute(0, 3, 1, 2) - wt).abs().max()) < 2.0 ** -20


class _Block(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(64, 32, 3, padding=1, bias=False)      # taken
        self.bn1 = nn.BatchNorm2d(32)
        self.conv2 = nn.Conv2d(32, 4, 3, padding=1, bias=False)       # taken (Cout % 4)
        self.shortcut = nn.Conv2d(64, 4, 1, bias=False)               # 1x1: left
        self.biased = nn.Conv2d(32, 32, 3, padding=1, bias=True)      # bias: left
        self.strided = nn.Conv2d(32, 32, 3, stride=2, padding=1, bias=False)
        self.rgb = nn.Conv2d(3, 32, 3, padding=1, bias=False)         # Cin = 3: left
        self.odd = nn.Conv2d(32, 6, 3, padding=1, bias=False)         # Cout % 4 != 0: left
        self.dilated = nn.Conv2d(32, 32, 3, padding=1, dilation=1, groups=2, bias=False)   # groups: left
        self.reflect = nn.Conv2d(32, 32, 3, padding=1, bias=False, padding_mode="reflect")
        self.nopad = nn.Conv2d(32, 32, 3, padding=0, bias=False)
        self.inner = nn.Sequential(nn.Conv2d(128, 64, 3, padding=1, bias=False), nn.ReLU())   # nested: taken


def test_swap_contract():
    from mickey_amd import train_heads as th
    m = _Block()
    keys = list(m.state_dict().keys())
    params = {n: p for n, p in m.named_parameters()}
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    assert th.use_hip_convs(m) == 3
    assert isinstance(m.conv1, th.Conv3x3) and isinstance(m.conv2, th.Conv3x3) and isinstance(m.inner[0], th.Conv3x3)
    for name in ("shortcut", "biased", "strided", "rgb", "odd", "dilated", "reflect", "nopad"):
        assert type(getattr(m, name)) is nn.Conv2d, name
    assert type(m.bn1) is nn.BatchNorm2d and type(m.inner[1]) is nn.ReLU
    # the SAME Parameter objects: optimiser state and checkpoints stay valid
    assert list(m.state_dict().keys()) == keys
    for n, p in m.named_parameters():
        assert p is params[n], n
    assert {id(p) for grp in opt.param_groups for p in grp["params"]} == {id(p) for p in m.parameters()}
    c = m.conv1
    assert (c.in_channels, c.out_channels, c.kernel_size, c.padding, c.stride) == (64, 32, (3, 3), (1, 1), (1, 1))
    assert c.bias is None and tuple(c.weight.shape) == (32, 64, 3, 3)
    assert th.use_hip_convs(m) == 0   # idempotent
    # a checkpoint of the un-swapped model loads strictly
    m.load_state_dict(_Block().state_dict(), strict=True)
    # a fresh module initialises like nn.Conv2d and refuses channel counts the kernels do not cover
    fresh = th.Conv3x3(32, 8)
    assert list(fresh.state_dict().keys()) == ["weight"] and float(fresh.weight.detach().abs().max()) <= (1.0 / (32 * 9)) ** 0.5 + 1e-6
    with pytest.raises(ValueError):
        th.Conv3x3(3, 8)


def test_cpu_tensors_and_bad_arguments_raise_before_any_launch():
    from mickey_amd import _native, train_heads as th
    m = th.Conv3x3(32, 4)
    with pytest.raises(_native.MickeyHipError):
        m(torch.zeros(1, 32, 3, 3))
    with pytest.raises(_native.MickeyHipError):
        th.conv3x3_train(torch.zeros(1, 32, 3, 3), torch.zeros(4, 32, 3, 3))
    with pytest.raises((ValueError, _native.MickeyHipError)):
        th.conv3x3_train(torch.zeros(1, 32, 3, 3, dtype=torch.float16), torch.zeros(4, 32, 3, 3))


def test_abi_argument_checks(nv):
    lib = nv.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mickey_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mk_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW_SYMBOLS:
        assert name in declared and name in nv.SIGNATURES and hasattr(lib, name), name
    assert nv.missing_symbols() == []
    # every new entry point cites the reference's conv
    raw = open(os.path.join(ROOT, "include", "mickey_hip.h")).read()
    for name in ("mk_conv3x3_split_dscale", "mk_absmax_scale", "mk_conv_train_planes", "mk_conv_train_weight_planes", "mk_conv_wgrad"):
        decl = raw.index("int %s(" % name)
        comment = raw.rfind("/*", 0, decl)
        assert "utils/extractor_utils.py:18-31" in raw[comment:decl], name
    one = 16   # any non-null, aligned address: argument checks come before every launch and never touch it
    # wgrad: Cin % 32, Cout % 4, null pointers, non-positive sizes
    ok = dict(gy_hi=one, gy_lo=one, ldg=32, x_hi=one, x_lo=one, Cout=4, Cin=32, nimg=1, H=3, W=3, gs=one, xs=one, work=one, dw=one)

    def wgrad(**kw):
        a = dict(ok, **kw)
        return lib.mk_conv_wgrad(a["gy_hi"], a["gy_lo"], a["ldg"], a["x_hi"], a["x_lo"], a["Cout"], a["Cin"], a["nimg"], a["H"], a["W"],
                                 a["gs"], a["xs"], a["work"], a["dw"], None)
    for bad in (dict(Cin=48), dict(Cout=6), dict(gy_hi=None), dict(x_lo=None), dict(work=None), dict(dw=None), dict(gs=None),
                dict(nimg=0), dict(H=-1), dict(W=0), dict(Cout=0), dict(ldg=16), dict(ldg=0), dict(x_hi=8)):
        assert wgrad(**bad) == 1, bad
        assert b"mk_conv_wgrad" in lib.mk_last_error()
    assert lib.mk_conv_train_weight_planes(one, 4, 48, 0, one, one, one, one, None) == 1
    assert lib.mk_conv_train_weight_planes(one, 6, 32, 0, one, one, one, one, None) == 1
    assert lib.mk_conv_train_weight_planes(None, 4, 32, 0, one, one, one, one, None) == 1
    assert lib.mk_conv_train_weight_planes(one, 4, 32, 1, one, one, one, None, None) == 1
    assert lib.mk_conv_train_planes(None, 1, 1, 1, 1, 1, 4, 3, 3, one, one, one, 4, None) == 1
    assert lib.mk_conv_train_planes(one, 1, 1, 1, 1, 1, 6, 3, 3, one, one, one, 8, None) == 1     # C % 4
    assert lib.mk_conv_train_planes(one, 1, 1, 1, 1, 1, 8, 3, 3, one, one, one, 4, None) == 1     # ld < C
    assert lib.mk_conv_train_planes(one, 1, 1, 1, 1, 0, 8, 3, 3, one, one, one, 8, None) == 1     # nimg
    assert lib.mk_absmax_scale(None, 1, 1, 1, 1, 1, 1, 1, 1, one, one, None) == 1
    assert lib.mk_absmax_scale(one, 1, 0, 1, 1, 1, 1, 1, 1, one, one, None) == 1
    assert lib.mk_conv3x3_split_dscale(one, one, 32, one, 576, one, 4, 1, 3, 3, None, None) == 1     # no device scale
    assert lib.mk_conv3x3_split_dscale(one, one, 48, one, 864, one, 4, 1, 3, 3, one, None) == 1      # C1 % 32
    assert lib.mk_conv3x3_split_dscale(one, one, 32, one, 576, one, 6, 1, 3, 3, one, None) == 1      # Cout % 4
    assert lib.mk_conv3x3_split_dscale(one, None, 32, one, 576, one, 4, 1, 3, 3, one, None) == 1
    assert lib.mk_conv3x3_split_dscale(one, one, 32, one, 576, one, 4, 0, 3, 3, one, None) == 1
    # work sizes: whole partial-sum slabs, at least one; a function of the shape alone
    assert nv.query("mk_absmax_scale_work_floats") >= 256
    for Cout, Cin, nimg, H, W in ((4, 32, 1, 3, 3), (64, 64, 8, 38, 51), (512, 1024, 8, 38, 51), (256, 256, 24, 38, 51)):
        n = nv.query("mk_conv_wgrad_work_floats", Cout, Cin, nimg, H, W)
        assert n >= Cout * 9 * Cin and n % (Cout * 9 * Cin) == 0 and n == nv.query("mk_conv_wgrad_work_floats", Cout, Cin, nimg, H, W)
    # the small layers do not fill the part with output tiles alone: their K is split
    assert nv.query("mk_conv_wgrad_work_floats", 64, 64, 8, 38, 51) > 64 * 9 * 64
    assert nv.query("mk_conv_wgrad_work_floats", 0, 64, 8, 38, 51) == 0
