"""-m gpu: the heads' 3x3 convolutions -- 99 % of the heads' flops -- ELEMENT by element against fp64, on both code paths:
  * training, all of mk_train_conv.hip: mk_absmax_scale, mk_conv_train_planes (both instantiations), mk_conv_train_weight_planes,
    mk_conv_wgrad (+ its reduce) and mk_conv3x3_split_dscale (+ its scale pass), called directly as ops.py calls them;
  * inference, the A_CONV3 stager of mk_gemm_common.hpp under the three forced schedules (128x128, 64x128, 256x256 ping-pong) with
    the dense, bordered, fp32 and (hi, lo)-plane epilogues: ops.conv3x3 and ops.conv3x3_split;
at the smallest shapes that reach every loop edge (tests/helpers/conv_refs.py names them, tests/test_conv_edges_cpu.py asserts that
each has its edge).  Every output -- dw, work, out, scale, acc_scale, weight planes, plane buffers -- sits in a guarded window
(tests/helpers/guarded.py); the guards are checked after each call and every wanted element is found overwritten.

Three levels (derivations: tests/helpers/conv_refs.py; tests/test_conv_edges_cpu.py shows that a correct fp32 evaluation meets every
bound in two summation orders and that subtly wrong references fail on a single tile-edge element):
  1. exact, as integers: scales against the header's contract, planes against hi = fp16(fl32(x s)), lo = fp16(fl32(x s - hi)) with
     everything else of a sentinel-filled buffer untouched, weight planes against train_heads.weight_planes;
  2. a kernel given its planes: fp64 sums of the products of the planes' actual bits, |err| <= gamma(n) sum |terms| x 1.01;
  3. end to end: train_heads.conv3x3_train against fp64 autograd, level 2 plus what the planes cannot represent.
A case passes when |got - ref64| / bound <= 1 on every element.  Measured worst ratios: profiles/conv_edges_parity.txt."""
import time

import pytest
import torch

from tests.helpers import conv_refs as R
from tests.helpers.guarded import bits, guarded, sentinel_bits

pytestmark = pytest.mark.gpu

WORST = {}       # (kernel, output) -> largest |error| / bound seen in this process
EXACT = {}       # (kernel, output) -> number of bit-exact comparisons made
RAN = [0]
F16, F32 = torch.float16, torch.float32
NAN16 = 0x7E00


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _nv():
    from mickey_amd import _native
    return _native


@pytest.fixture(scope="module", autouse=True)
def _report_and_reset():
    t0 = time.perf_counter()
    yield
    if torch.cuda.is_available():
        from mickey_amd import ops
        ops.gemm_set_tile(0)
    for (kernel, what), r in sorted(WORST.items()):
        print("conv edges worst |err| / bound: %-30s %-16s %.3f" % (kernel, what, r))
    for (kernel, what), n in sorted(EXACT.items()):
        print("conv edges bit-exact comparisons: %-28s %-16s %d" % (kernel, what, n))
    print("conv edges: %d tests in %.1f s" % (RAN[0], time.perf_counter() - t0))


@pytest.fixture(autouse=True)
def _count():
    yield
    RAN[0] += 1


def _written(t):
    return not bool((bits(t) == sentinel_bits(t.dtype)).any())


def _untouched(t):
    return bool((bits(t) == sentinel_bits(t.dtype)).all())


def _exact(kernel, what, got, want, msg):
    """got (device) and want (CPU) hold the same bits; names the first element that does not"""
    g, w = bits(got).cpu().reshape(-1), (want if want.dtype in (torch.int16, torch.int32) else bits(want)).reshape(-1)
    assert g.shape == w.shape, (g.shape, w.shape)
    ne = g != w
    EXACT[(kernel, what)] = EXACT.get((kernel, what), 0) + 1
    if bool(ne.any()):
        i = int(torch.nonzero(ne)[0])
        cols = got.shape[-1]
        raise AssertionError("%s %s, %s: %d of %d elements differ, first at (row %d, column %d): got bits 0x%x, want 0x%x"
                             % (kernel, what, msg, int(ne.sum()), ne.numel(), i // cols, i % cols, int(g[i]) & 0xffffffff,
                                int(w[i]) & 0xffffffff))


def _within(kernel, what, got, ref, bound, msg, where=None):
    got = got.detach().double().cpu().reshape(ref.shape)
    worst, i = R.ratio(got, ref, bound)
    WORST[(kernel, what)] = max(WORST.get((kernel, what), 0.0), worst)
    if not worst <= 1.0:
        e = (got - ref).abs().reshape(-1)
        outside = int((e > bound.reshape(-1)).sum() + (~torch.isfinite(got)).sum())
        cols = ref.shape[-1]
        at = where(i) if where else "(row %d, column %d) = row %d of its 64-row tile, column %d of its 128-column tile" % (
            i // cols, i % cols, (i // cols) % 64, (i % cols) % 128)
        raise AssertionError("%s %s, %s: |err| / bound = %.3g at %s: got %r, fp64 %r, bound %.3g; %d of %d elements outside"
                             % (kernel, what, msg, worst, at, float(got.reshape(-1)[i]), float(ref.reshape(-1)[i]),
                                float(bound.reshape(-1)[i]), outside, e.numel()))


# ---- the entry points on guarded buffers, called as ops.py calls them -----------------------------------------------------------
def _absmax(x):
    """mk_absmax_scale as ops.absmax_scale calls it, `work` and `scale` in guarded windows -> the fp32 [2] scale (device)"""
    nv = _nv()
    work, c1 = guarded(1, int(nv.query("mk_absmax_scale_work_floats")), F32, x.device)
    scale, c2 = guarded(1, 2, F32, x.device)
    if x.is_contiguous() or x.is_contiguous(memory_format=torch.channels_last):
        n = x.numel()
        dims, strides = (1, 1, 1, n), (n, n, n, 1)
    else:
        dims, strides = tuple(x.shape), tuple(x.stride())
    nv.call("mk_absmax_scale", nv.ptr(x), *dims, *strides, nv.ptr(work), nv.ptr(scale), nv.stream())
    torch.cuda.synchronize()
    c1()
    c2()
    assert _written(scale), "mk_absmax_scale left an element of `scale` unwritten"
    return scale[0]


def _check_scale(x_cpu, scale, msg):
    want = R.scale_ref(x_cpu)
    got = scale.cpu().tolist()
    EXACT[("absmax", "scale")] = EXACT.get(("absmax", "scale"), 0) + 1
    assert R.same_scale(got, want), "mk_absmax_scale, %s: got (%r, %r), the contract gives (%r, %r)" % (msg, got[0], got[1], want[0], want[1])
    return want


def _plane_windows(nimg, H, W, ld, dev, fill):
    """(hi, lo) whole training plane buffers [plane_rows, ld] pre-set to `fill` (None: the sentinel), in ONE guarded window -- the
    split conv wants the planes of a source within 2 GiB of each other -- with four sentinel rows between them"""
    rows = int(_nv().query("mk_conv_train_plane_rows", nimg, H, W))
    assert rows == R.plane_rows(nimg, H, W)
    win, chk = guarded(2 * rows + 4, ld, F16, dev)
    hi, gap, lo = win[:rows], win[rows:rows + 4], win[rows + 4:]
    if fill is not None:
        hi.fill_(fill)
        lo.fill_(fill)

    def check():
        chk()
        assert _untouched(gap), "the rows between the hi and the lo buffer were written"

    return hi, lo, (check,)


def _planes(src, scale, hi, lo, W):
    """mk_conv_train_planes as ops.conv_train_planes calls it; hi / lo: whole buffers (_plane_windows)"""
    nv = _nv()
    nimg, C, H, Wd = src.shape
    assert Wd == W
    lead = int(nv.query("mk_conv_train_lead_rows", W))
    nv.call("mk_conv_train_planes", nv.ptr(src), src.stride(0), src.stride(1), src.stride(2), src.stride(3), nimg, C, H, W, nv.ptr(scale),
            nv.ptr(hi[lead:]), nv.ptr(lo[lead:]), hi.stride(0), nv.stream())
    torch.cuda.synchronize()


def _made_planes(x_cpu, ld, dev, msg):
    """scale + planes of x_cpu by the kernels, in zero-filled guarded buffers; both checked exactly (level 1) -> (scale, hi, lo)"""
    nimg, C, H, W = x_cpu.shape
    xd = x_cpu.to(dev)
    scale = _absmax(xd)
    s = _check_scale(x_cpu, scale, msg)
    hi, lo, checks = _plane_windows(nimg, H, W, ld, dev, 0.0)
    _planes(xd, scale, hi, lo, W)
    for c in checks:
        c()
    wh, wl = R.plane_buffer(nimg, H, W, C, ld, *R.planes_ref(x_cpu, s[0]), fill=0)
    _exact("planes", "hi (chain)", hi, wh, msg)
    _exact("planes", "lo (chain)", lo, wl, msg)
    return scale, hi, lo


def _weight_planes(w_dev, sw, sa, transposed):
    """mk_conv_train_weight_planes as ops.conv_train_weight_planes calls it, planes and acc_scale in guarded windows"""
    nv = _nv()
    Cout, Cin = w_dev.shape[:2]
    Cp = (Cout + 31) // 32 * 32
    rows, cols = (Cin, 18 * Cp) if transposed else (Cout, 18 * Cin)
    planes, c1 = guarded(rows, cols, F16, w_dev.device)
    acc, c2 = guarded(1, 1, F32, w_dev.device)
    nv.call("mk_conv_train_weight_planes", nv.ptr(w_dev), Cout, Cin, int(transposed), nv.ptr(sw), nv.ptr(sa), nv.ptr(planes), nv.ptr(acc),
            nv.stream())
    torch.cuda.synchronize()
    c1()
    c2()
    assert _written(acc), "acc_scale left unwritten"
    return planes, acc[0]


# ================================================================ mk_absmax_scale ===============================================
@pytest.mark.parametrize("where", ["first", "last", "strided view, last"])
def test_absmax_finds_the_maximum_at_the_ends(where):
    dev = _dev()
    g = R.gen("absmax", where)
    if where == "strided view, last":
        big = torch.randn((2, 4, 6, 10), generator=g)
        big[:, :, 1::2, :] = 1e6      # everything between the view's elements is larger than its maximum
        big[:, :, :, 1::2] = 1e6
        bd = big.to(dev)
        x, xd = big[:, :, ::2, ::2], bd[:, :, ::2, ::2]
        x[-1, -1, -1, -1] = -37.5
        xd[-1, -1, -1, -1] = -37.5
        assert not xd.is_contiguous() and tuple(xd.shape) == (2, 4, 3, 5)
    else:
        x = torch.randn((2, 4, 3, 5), generator=g)
        x.view(-1)[0 if where == "first" else -1] = -37.5
        xd = x.to(dev)
    want = _check_scale(x, _absmax(xd), where)
    assert want == (2.0 ** 9, 2.0 ** -9)


def test_absmax_grid_stride_second_sweep():
    """1024 blocks x 1024 elements + 1: the last element is the only one of the loop's second trip, and it is the maximum"""
    dev = _dev()
    n = 1024 * 1024 + 1
    x = torch.rand((1, 1, 1, n), generator=R.gen("absmax", "sweep")) * 0.9
    x[0, 0, 0, -1] = 3.0
    want = _check_scale(x, _absmax(x.to(dev)), "1024 * 1024 + 1 elements")
    assert want == (2.0 ** 13, 2.0 ** -13)


def test_absmax_of_an_expanded_gradient():
    dev = _dev()
    v = torch.randn((1, 8, 1, 1), generator=R.gen("absmax", "expand"))
    v[0, 5] = 100.0
    xd = v.to(dev).expand(2, 8, 3, 5)
    assert xd.stride() == (0, 1, 0, 0)
    want = _check_scale(v.expand(2, 8, 3, 5), _absmax(xd), "stride-0 expand")
    assert want == (2.0 ** 8, 2.0 ** -8)


@pytest.mark.parametrize("m,k", [(2.0 ** -149, 100), (2.0 ** -126, 100), (1.5 * 2.0 ** -87, 100), (2.0 ** -86, 100), (2.0 ** 114, -100),
                                 (2.0 ** 115, -100), (3.4028234663852886e38, -100)])
def test_absmax_exponent_clamps(m, k):
    """the maxima on both sides of the two clamps (2^-86 and 2^114 are the last unclamped ones) and the ends of fp32's range"""
    dev = _dev()
    x = torch.zeros((1, 4, 2, 2))
    x.view(-1)[3] = m * 0.5
    x.view(-1)[-1] = -m
    want = _check_scale(x, _absmax(x.to(dev)), "max %g" % m)
    assert want == (2.0 ** k, 2.0 ** -k)
    if m in (2.0 ** -86, 2.0 ** 114):
        assert 2.0 ** 14 <= m * want[0] < 2.0 ** 15


@pytest.mark.parametrize("v", [0.0, float("inf"), float("-inf"), float("nan")])
def test_absmax_zero_and_non_finite(v):
    dev = _dev()
    x = torch.zeros((2, 4, 3, 5)) if v == 0.0 else torch.randn((2, 4, 3, 5), generator=R.gen("absmax", "nf"))
    x.view(-1)[-1] = v
    scale = _absmax(x.to(dev))
    _check_scale(x, scale, "last element %r" % v)
    got = scale.cpu()
    assert float(got[0]) == 1.0 and (float(got[1]) == 1.0 if v == 0.0 else bool(torch.isnan(got[1])))


# ================================================================ mk_conv_train_planes ==========================================
def _layout(x, layout, dev):
    """device tensor with the values of x [nimg, C, H, W] in the given memory layout; everything around a slice is NaN"""
    nimg, C, H, W = x.shape
    if layout == "contiguous":
        return x.to(dev)
    if layout == "channels_last":
        return x.to(dev).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    if layout == "slice":
        big = torch.full((nimg + 1, C + 4, H + 2, W + 3), float("nan"), device=dev)
        v = big[1:, 2:2 + C, 1:1 + H, 2:2 + W]
    elif layout == "slice_channels_last":
        big = torch.full((nimg + 1, H + 2, W + 3, C + 4), float("nan"), device=dev)
        v = big[1:, 1:1 + H, 2:2 + W, 2:2 + C].permute(0, 3, 1, 2)
    else:
        raise AssertionError(layout)
    v.copy_(x)
    return v


@pytest.mark.parametrize("layout", R.PLANES_LAYOUTS)
@pytest.mark.parametrize("C", R.PLANES_C)
@pytest.mark.parametrize("nimg,H,W", R.PLANES_PIX)
def test_planes_exact_and_nothing_else_touched(nimg, H, W, C, layout):
    """both instantiations (stride_c == 1: CFAST) at npix % 64 in {1, 63, 0}, W = 1, H = 1, C % 32 in {4, 0}: the pixel rows hold the
    reference bits; every border row, every lead / tail row and every column C .. ld - 1 of the sentinel-filled buffers keep the
    sentinel"""
    dev = _dev()
    ld = (C + 31) // 32 * 32
    if layout == "expand":
        v = R.spread((1, C, 1, 1), ("planes", C), ())
        v[0, 0] = 3.0
        x = v.expand(nimg, C, H, W)
        xd = v.to(dev).expand(nimg, C, H, W)
        assert all(st == 0 for st, n in zip(xd.stride(), xd.shape) if n > 1 and st != 1)
    else:
        x = R.spread((nimg, C, H, W), ("planes", layout), (0, 2, 3), zeros=0.1)
        x[0, 0, 0, 0] = 3.0
        xd = _layout(x, layout, dev)
    cfast = xd.stride(1) == 1
    assert cfast == (layout in ("channels_last", "slice_channels_last", "expand") or (layout == "contiguous" and H * W == 1))
    msg = "%dx%dx%d, C %d, %s (%s)" % (nimg, H, W, C, layout, "CFAST" if cfast else "pixel-fast")
    scale = _absmax(xd)
    s = _check_scale(x, scale, msg)
    hi, lo, checks = _plane_windows(nimg, H, W, ld, dev, None)
    _planes(xd, scale, hi, lo, W)
    for c in checks:
        c()
    sent = sentinel_bits(F16)
    assert sent == R.F16_SENTINEL
    wh, wl = R.plane_buffer(nimg, H, W, C, ld, *R.planes_ref(x, s[0]), fill=sent)
    kernel = "planes CFAST" if cfast else "planes pixel-fast"
    _exact(kernel, "hi", hi, wh, msg)
    _exact(kernel, "lo", lo, wl, msg)
    idx = (R.bordered_index(nimg, H, W) + R.lead_rows(W)).to(dev)
    assert _written(hi[idx][:, :C]) and _written(lo[idx][:, :C]), msg + ": a wanted element kept the sentinel"


# ================================================================ mk_conv_train_weight_planes ===================================
@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("Cout,Cin", R.WEIGHT_SHAPES)
def test_weight_planes_exact(Cout, Cin, transposed):
    from mickey_amd import train_heads as th
    dev = _dev()
    w = torch.randn((Cout, Cin, 3, 3), generator=R.gen("wplanes", Cout, Cin)) / (9 * Cin) ** 0.5
    w[0, 0, 0, 0] = 0.0
    wd = w.to(dev)
    sw = _absmax(wd)
    s = _check_scale(w, sw, "weight")
    act = torch.tensor([2.0 ** -7, 2.0 ** 7], device=dev)
    planes, acc = _weight_planes(wd, sw, act, transposed)
    msg = "%d -> %d%s" % (Cin, Cout, ", transposed" if transposed else "")
    assert _written(planes), msg + ": a plane element kept the sentinel"
    _exact("weight_planes", "transposed" if transposed else "forward", planes, th.weight_planes(w, s[0], transposed=transposed), msg)
    _exact("weight_planes", "acc_scale", acc.reshape(1, 1), torch.tensor([[s[1] * 2.0 ** 7]], dtype=F32), msg)
    if transposed:
        Cp = (Cout + 31) // 32 * 32
        hi, lo = R.split_weight_planes(planes.cpu())
        pad = torch.arange(9 * Cp) % Cp >= Cout
        assert Cp > Cout and bool((bits(hi[:, pad]) == 0).all()) and bool((bits(lo[:, pad]) == 0).all()), msg + ": co >= Cout is not +0"


# ================================================================ mk_conv_wgrad =================================================
def _wgrad(gh, gl, ldg, xh, xl, Cout, Cin, nimg, H, W, sg, sx):
    """mk_conv_wgrad as ops.conv_wgrad calls it (gh .. xl: whole plane buffers), `work` sized exactly, `dw` and `work` guarded"""
    nv = _nv()
    lead = int(nv.query("mk_conv_train_lead_rows", W))
    floats = int(nv.query("mk_conv_wgrad_work_floats", Cout, Cin, nimg, H, W))
    assert floats == R.wgrad_split(Cout, Cin, nimg, H, W)[2] * Cout * 9 * Cin
    work, c1 = guarded(1, floats, F32, gh.device)
    dw, c2 = guarded(Cout, Cin * 9, F32, gh.device)
    nv.call("mk_conv_wgrad", nv.ptr(gh[lead:]), nv.ptr(gl[lead:]), ldg, nv.ptr(xh[lead:]), nv.ptr(xl[lead:]), Cout, Cin, nimg, H, W,
            nv.ptr(sg), nv.ptr(sx), nv.ptr(work), nv.ptr(dw), nv.stream())
    torch.cuda.synchronize()
    c1()
    c2()
    assert _written(dw), "mk_conv_wgrad left an element of dw unwritten"
    assert _written(work), "mk_conv_wgrad left an element of its partials unwritten"
    return dw


@pytest.mark.parametrize("name,nimg,H,W,Cout,Cin", R.wgrad_cases())
def test_wgrad_elementwise(name, nimg, H, W, Cout, Cin):
    """planes made by the kernels (checked exactly on the way); dw against the fp64 sum of the planes' products; the same case again
    (bit-identical) and once more with finite sentinels where the contract allows anything finite -- X's rows outside the bordered
    map, gY's columns Cout .. ldg - 1 -- (bit-identical again)"""
    dev = _dev()
    x, _, gy = R.train_inputs(nimg, H, W, Cin, Cout, "gpu")
    msg = "%s: %dx%dx%d, %d -> %d" % (name, nimg, H, W, Cin, Cout)
    ldg = (Cout + 31) // 32 * 32
    sx, xh, xl = _made_planes(x, Cin, dev, msg + ", X")
    sg, gh, gl = _made_planes(gy, ldg, dev, msg + ", gY")
    args = (ldg, xh, xl, Cout, Cin, nimg, H, W, sg, sx)
    dw = _wgrad(gh, gl, *args)
    inv = R.scale_ref(x)[1] * R.scale_ref(gy)[1]
    ref, ab = R.wgrad_ref(gh.cpu(), gl.cpu(), xh.cpu(), xl.cpu(), nimg, H, W, Cout, Cin, inv)
    chunk, nsteps, ksplit = R.wgrad_split(Cout, Cin, nimg, H, W)

    def where(i):
        co, ci, tap = i // (9 * Cin), (i // 9) % Cin, i % 9
        n = tap * Cin + ci
        return ("dw[%d, %d, %d, %d] = row %d of M tile %d, column %d of N tile %d (%d chunks of %d steps, %d steps)"
                % (co, ci, tap // 3, tap % 3, co % 128, co // 128, n % 128, n // 128, ksplit, chunk, nsteps))

    _within("wgrad", "dw", dw, ref, R.wgrad_bound(ab, Cout, Cin, nimg, H, W), msg, where)
    _exact("wgrad", "second run", _wgrad(gh, gl, *args), bits(dw).cpu(), msg)
    lead, rows = R.lead_rows(W), R.bordered_rows(nimg, H, W)
    sent = sentinel_bits(F16)
    for p in (xh, xl):
        bits(p)[:lead] = sent
        bits(p)[lead + rows:] = sent
    if ldg > Cout:
        bits(gh)[:, Cout:] = sent
        bits(gl)[:, Cout:] = sent
    _exact("wgrad", "finite surroundings", _wgrad(gh, gl, *args), bits(dw).cpu(), msg)


# ================================================================ mk_conv3x3_split_dscale =======================================
def _dscale(ih, il, C1, wpl, Cout, nimg, H, W, acc, tile):
    """mk_conv3x3_split_dscale as ops.conv3x3_split_dscale calls it under a forced schedule; ih / il at bordered row 0"""
    from mickey_amd import ops
    nv = _nv()
    out, chk = guarded(nimg * H * W, Cout, F32, ih.device)
    ops.gemm_set_tile(tile)
    try:
        nv.call("mk_conv3x3_split_dscale", nv.ptr(ih), nv.ptr(il), C1, nv.ptr(wpl), wpl.shape[-1], nv.ptr(out), Cout, nimg, H, W,
                nv.ptr(acc), nv.stream())
        torch.cuda.synchronize()
    finally:
        ops.gemm_set_tile(0)
    chk()
    assert _written(out), "mk_conv3x3_split_dscale left an output element unwritten"
    return out


def _dscale_setup(nimg, H, W, Cout, Cin, transposed, dev, msg):
    """-> (conv input channels, conv output channels, input plane buffers, weight planes, acc_scale) of the forward conv (x's
    planes, W) or of the input gradient (gY's planes [.., Cp], W transposed), every operand made by the kernels.  The rows of the
    plane buffers outside the bordered map are NaN: the conv has no business there."""
    x, w, gy = R.train_inputs(nimg, H, W, Cin, Cout, "gpu")
    wd = w.to(dev)
    sw = _absmax(wd)
    _check_scale(w, sw, msg)
    src, ld = (gy, (Cout + 31) // 32 * 32) if transposed else (x, Cin)
    sa, ih, il = _made_planes(src, ld, dev, msg)
    lead, rows = R.lead_rows(W), R.bordered_rows(nimg, H, W)
    for p in (ih, il):
        bits(p)[:lead] = NAN16
        bits(p)[lead + rows:] = NAN16
    wpl, acc = _weight_planes(wd, sw, sa, transposed)
    return ld, (Cin if transposed else Cout), ih[lead:], il[lead:], wpl, acc, rows


@pytest.mark.parametrize("nimg,H,W,Cout,Cin,tile,transposed", R.dscale_cases())
def test_split_dscale_elementwise(nimg, H, W, Cout, Cin, tile, transposed):
    dev = _dev()
    msg = "%dx%dx%d (M = %d), %d -> %d%s, schedule %d" % (nimg, H, W, nimg * H * W, Cin, Cout, ", input gradient" if transposed else "", tile)
    C1, N, ih, il, wpl, acc, rows = _dscale_setup(nimg, H, W, Cout, Cin, transposed, dev, msg)
    out = _dscale(ih, il, C1, wpl, N, nimg, H, W, acc.reshape(1), tile)
    ref, e = R.split_conv_ref(ih[:rows].cpu(), il[:rows].cpu(), wpl.cpu(), nimg, H, W, float(acc))
    _within("split_dscale", "dgrad" if transposed else "forward", out, ref, e, msg)


def test_split_dscale_nan_scale_poisons_every_output():
    dev = _dev()
    nimg, H, W, Cout, Cin = 2, 5, 7, 132, 32
    C1, N, ih, il, wpl, acc, _ = _dscale_setup(nimg, H, W, Cout, Cin, 0, dev, "NaN acc_scale")
    out = _dscale(ih, il, C1, wpl, N, nimg, H, W, torch.full((1,), float("nan"), device=dev), 0)
    assert bool(torch.isnan(out).all())


# ================================================================ level 3: train_heads.conv3x3_train ============================
@pytest.mark.parametrize("nimg,H,W,Cin,Cout", R.E2E_CASES)
def test_conv3x3_train_end_to_end(nimg, H, W, Cin, Cout):
    from mickey_amd import train_heads as th
    dev = _dev()
    x, w, gy = R.train_inputs(nimg, H, W, Cin, Cout, "gpu")
    xd, wd = x.to(dev).requires_grad_(True), w.to(dev).requires_grad_(True)
    y = th.conv3x3_train(xd, wd)
    gx, dw = torch.autograd.grad(y, (xd, wd), gy.to(dev))
    torch.cuda.synchronize()
    want = R.e2e_ref(x, w, gy)
    msg = "%dx%dx%d, %d -> %d" % (nimg, H, W, Cin, Cout)

    def where_of(shape):
        def where(i):
            idx = []
            for s in reversed(shape):
                idx.append(i % s)
                i //= s
            return "index %s" % (tuple(reversed(idx)),)
        return where

    for k, got in (("y", y), ("gx", gx), ("dw", dw)):
        ref, bound = want[k]
        _within("conv3x3_train", k, got, ref.contiguous(), bound.contiguous(), msg, where_of(tuple(ref.shape)))


# ================================================================ the inference forms of the A_CONV3 stager ======================
def _rows_check(out, full_rows, pixel_rows, msg):
    """out [G, rows, Cout] (a guarded window's view): the pixel rows are written, all other rows keep the sentinel"""
    assert _written(out[:, pixel_rows]), msg + ": an output element kept the sentinel"
    if full_rows > pixel_rows.numel():
        rest = torch.ones(full_rows, dtype=torch.bool, device=out.device)
        rest[pixel_rows] = False
        assert _untouched(out[:, rest]), msg + ": a border row was written"


@pytest.mark.parametrize("kind,tile,form,M,Cout,C2,resid,groups,relu", R.inference_cases())
def test_inference_conv_elementwise(kind, tile, form, M, Cout, C2, resid, groups, relu):
    """ops.conv3x3 (bf16, fp16) and ops.conv3x3_split (three products; two on a lone hi plane) under a forced schedule: every group's
    every element against fp64; a bordered output's border rows are guard rows (they keep the sentinel)"""
    from mickey_amd import ops, weights
    dev = _dev()
    assert (ops.SPLIT_ACT_SCALE, ops.SPLIT_W_SCALE) == (R.ACT_SCALE, R.W_SCALE)
    nimg, H, W = R.INF_PIX[M]
    Rb = R.bordered_rows(nimg, H, W)
    assert Rb == ops.bordered_rows(nimg, H, W)
    split = kind.startswith("split")
    C1 = 32 if split else 64
    K = 9 * C1 + C2
    bord = form.endswith("bordered")
    rows = Rb if bord else M
    idx = R.bordered_index(nimg, H, W).to(dev) if bord else torch.arange(M, device=dev)
    msg = "%s, schedule %d, %s, M %d, Cout %d, C2 %d, resid %d, %d groups, relu %d" % (kind, tile, form, M, Cout, C2, resid, groups, relu)
    act = ops.ACT_RELU if relu else ops.ACT_NONE
    kernel = "conv3x3 " + kind
    ops.gemm_set_tile(tile)
    try:
        if not split:
            dtype = torch.bfloat16 if kind == "bf16" else F16
            c = R.lp_conv_inputs(nimg, H, W, C1, C2, Cout, groups, dtype, "gpu")
            odt = F32 if form == "f32" else dtype
            win, chk = guarded(groups * rows, Cout, odt, dev)
            out = win.view(groups, rows, Cout)
            a, a2, rs = c["a"].to(dev), None if C2 == 0 else c["a2"].to(dev), c["resid"].to(dev) if resid else None
            ops.conv3x3(a, C1, c["w"].to(dev), c["bias"].to(dev), out, Cout, groups, nimg, H, W, act=act, in2=a2, C2=C2, resid=rs,
                        stride_in1=Rb * C1, stride_in2=0, stride_w=Cout * K, stride_bias=Cout, stride_out=rows * Cout,
                        stride_resid=Rb * Cout, out_bordered=bord)
            torch.cuda.synchronize()
            chk()
            _rows_check(out, rows, idx, msg)
            for g in range(groups):
                ref, e = R.lp_conv_ref(c["a"][g], c["w"][g], nimg, H, W, dtype, form == "f32", a2=c["a2"], bias=c["bias"][g],
                                       resid=c["resid"][g] if resid else None, relu=bool(relu))
                _within(kernel, form, out[g, idx], ref, e, msg + ", group %d" % g)
            return
        v = R.inference_inputs(nimg, H, W, C1, C2, Cout, groups, "gpu")
        xb = torch.stack([R.bordered(r, nimg, H, W) for r in v["x"]]).to(dev)
        h1, l1 = ops.split_planes(xb, *ops.plane_pair(xb.shape, dev))
        in2 = None
        if C2:
            x2b = R.bordered(v["x2"], nimg, H, W).to(dev)
            in2 = ops.split_planes(x2b, *ops.plane_pair(x2b.shape, dev))
        wpl = weights.split_conv_weight(v["w"], R.W_SCALE).contiguous()
        planes_out = form.startswith("planes")
        wins = [guarded(groups * rows, Cout, F16 if planes_out else F32, dev) for _ in range(2 if planes_out else 1)]
        outs = [wn.view(groups, rows, Cout) for wn, _ in wins]
        ops.conv3x3_split((h1, l1 if kind == "split3" else None), C1, wpl.to(dev), v["bias"].to(dev), tuple(outs) if planes_out else outs[0],
                          Cout, groups, nimg, H, W, act=act, in2=in2, C2=C2, stride_in1=Rb * C1, stride_in2=0, stride_w=Cout * 2 * K,
                          stride_bias=Cout, stride_out=rows * Cout, out_bordered=bord, w_scale=R.W_SCALE)
        torch.cuda.synchronize()
        for o, (_, chk) in zip(outs, wins):
            chk()
            _rows_check(o, rows, idx, msg)
        h1c, l1c = h1.cpu(), l1.cpu()
        a2c = None if in2 is None else (in2[0].cpu(), in2[1].cpu())
        for g in range(groups):
            ref, e = R.split_conv_ref(h1c[g], l1c[g] if kind == "split3" else None, wpl[g], nimg, H, W, 1.0 / (R.ACT_SCALE * R.W_SCALE),
                                      a2=a2c, bias=v["bias"][g], relu=bool(relu))
            if not planes_out:
                _within(kernel, form, outs[0][g, idx], ref, e, msg + ", group %d" % g)
                continue
            bh, bs = R.planes_bounds(ref, e, R.ACT_SCALE)
            hi, lo = outs[0][g, idx].double(), outs[1][g, idx].double()
            _within(kernel, form + " hi", hi, ref * R.ACT_SCALE, bh, msg + ", group %d" % g)
            _within(kernel, form + " hi+lo", hi + lo, ref * R.ACT_SCALE, bs, msg + ", group %d" % g)
    finally:
        ops.gemm_set_tile(0)
