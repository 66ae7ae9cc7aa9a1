"""tests/helpers/conv_refs.py without a GPU: the references of the 3x3 convolution edge tests agree with fp64 autograd and with the
formulas of mickey_amd.train_heads, the restated K split agrees with the library, every designed shape has the edge it is named
for, every bound admits a correct fp32 evaluation in two summation orders (what keeps tests/test_conv_edges_gpu.py honest), no
designed input leaves an element with a zero bound, and subtly wrong references are rejected on ONE tile-edge element."""
import os

import pytest
import torch
import torch.nn.functional as F

from tests.helpers import conv_refs as R


@pytest.fixture(scope="module")
def nv():
    from mickey_amd import build, _native
    if not os.path.exists(build.lib_path()):
        build.build(verbose=False)
    _native.load()
    return _native


def _autograd64(x, w, gy):
    x = x.double().requires_grad_(True)
    w = w.double().requires_grad_(True)
    y = F.conv2d(x, w, padding=1)
    gx, dw = torch.autograd.grad(y, (x, w), gy.double())
    return dict(y=y.detach(), gx=gx, dw=dw)


def _planes_cpu(nimg, H, W, Cin, Cout, key="cpu"):
    """the training chain's operand planes as a correct implementation leaves them -> dict of fp16 buffers, scales, inputs"""
    x, w, gy = R.train_inputs(nimg, H, W, Cin, Cout, key)
    sx, sg = R.scale_ref(x), R.scale_ref(gy)
    ldg = (Cout + 31) // 32 * 32
    xh, xl = (b.view(torch.float16) for b in R.plane_buffer(nimg, H, W, Cin, Cin, *R.planes_ref(x, sx[0])))
    gh, gl = (b.view(torch.float16) for b in R.plane_buffer(nimg, H, W, Cout, ldg, *R.planes_ref(gy, sg[0])))
    return dict(x=x, w=w, gy=gy, xh=xh, xl=xl, gh=gh, gl=gl, inv=sx[1] * sg[1], sx=sx, sg=sg, geom=(nimg, H, W, Cout, Cin))


def _one(mut, ref, elem):
    """ref with the single element `elem` taken from the mutant"""
    got = ref.clone()
    got[elem] = mut[elem]
    return got


# ---- the references are the operation ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nimg,H,W,Cin,Cout", [(2, 3, 4, 32, 4), (1, 1, 1, 32, 8), (3, 4, 1, 32, 4), (1, 1, 5, 64, 36)])
def test_references_agree_with_fp64_autograd_and_train_heads(nimg, H, W, Cin, Cout):
    from mickey_amd import ops, train_heads as th
    x, w, gy = R.train_inputs(nimg, H, W, Cin, Cout, "agree")
    want = _autograd64(x, w, gy)
    got = R.e2e_ref(x, w, gy)
    for k in ("y", "gx", "dw"):
        ref, bound = got[k]
        assert ref.shape == want[k].shape == bound.shape
        assert float((ref - want[k]).abs().max()) <= 1e-12 * max(1.0, float(want[k].abs().max())), k
    # ... and the project's own statements of the same formulas
    x64, g64 = x.double(), gy.double()
    assert torch.equal(R.bordered(R.dense_rows(x64), nimg, H, W), th.bordered_map(x64))
    assert torch.equal(R.bordered_index(nimg, H, W), ops.bordered_index(nimg, H, W, "cpu"))
    assert float((th.wgrad_bordered(x64, g64) - got["dw"][0]).abs().max()) <= 1e-12 * float(want["dw"].abs().max())
    gx2 = F.conv2d(g64, th.dgrad_weight(w.double()), padding=1)
    assert float((gx2 - got["gx"][0]).abs().max()) <= 1e-12 * float(want["gx"].abs().max())
    # level 2 on exact planes (the fp64 values themselves as `hi`, zero `lo`) is the same number again
    z = torch.zeros
    rows = R.plane_rows(nimg, H, W)
    xb, gb = z((rows, Cin), dtype=torch.float64), z((rows, Cout), dtype=torch.float64)
    idx = R.bordered_index(nimg, H, W) + R.lead_rows(W)
    xb[idx], gb[idx] = R.dense_rows(x64), R.dense_rows(g64)
    dw2, _ = R.wgrad_ref(gb, z(gb.shape, dtype=torch.float64), xb, z(xb.shape, dtype=torch.float64), nimg, H, W, Cout, Cin, 1.0)
    assert float((dw2 - want["dw"]).abs().max()) <= 1e-12 * float(want["dw"].abs().max())


def test_weight_plane_reference_splits_back():
    from mickey_amd import train_heads as th, weights
    w = torch.randn((36, 32, 3, 3), generator=R.gen("wp"))
    for tr in (False, True):
        pl = th.weight_planes(w, 256.0, transposed=tr)
        hi, lo = R.split_weight_planes(pl)
        hi2, lo2 = weights.split_conv_weight_planes(pl)
        assert torch.equal(hi, hi2) and torch.equal(lo, lo2)
        wt = F.pad(th.dgrad_weight(w), (0, 0, 0, 0, 0, 28)) if tr else w
        assert float(((hi.double() + lo.double()) / 256.0 - R.tap_major(wt).double()).abs().max()) < 2.0 ** -20


# ---- the K split and the designed shapes -----------------------------------------------------------------------------------------
def test_restated_split_is_the_library_split(nv):
    seen = set()
    for _, nimg, H, W, Cout, Cin in R.wgrad_cases() + [("e2e", a, b, c, e, d) for a, b, c, d, e in R.E2E_CASES] + \
            [("big", 32, 51, 38, 256, 512), ("big", 8, 102, 76, 64, 128), ("big", 1, 1, 1, 1024, 1024)]:
        chunk, nsteps, ksplit = R.wgrad_split(Cout, Cin, nimg, H, W)
        floats = nv.query("mk_conv_wgrad_work_floats", Cout, Cin, nimg, H, W)
        assert floats == ksplit * Cout * 9 * Cin, (nimg, H, W, Cout, Cin, floats, ksplit)
        assert nsteps == (nv.query("mk_bordered_rows", nimg, H, W) + 31) // 32
        assert nv.query("mk_conv_train_plane_rows", nimg, H, W) == R.plane_rows(nimg, H, W)
        assert nv.query("mk_conv_train_lead_rows", W) == R.lead_rows(W)
        seen.add(ksplit)
    assert {1, 2, 5} <= seen


def test_designed_shapes_have_their_edges():
    rows = {k: R.bordered_rows(*v) for k, v in R.WGRAD_ROWS.items()}
    lens = {k: R.chunk_lengths(4, 32, *v) for k, v in R.WGRAD_ROWS.items()}
    assert rows["7 rows, one step"] == 7 and lens["7 rows, one step"] == [1]
    assert rows["rows % 32 == 31"] % 32 == 31 and lens["rows % 32 == 31"] == [1]
    assert rows["rows % 32 == 0, nk = 2"] == 64 and lens["rows % 32 == 0, nk = 2"] == [2]
    assert rows["rows % 32 == 1, W = 1"] % 32 == 1 and R.WGRAD_ROWS["rows % 32 == 1, W = 1"][2] == 1
    assert lens["one chunk of 3 steps"] == [3]
    assert lens["chunks of 5 and 4"] == [5, 4]
    assert lens["5 chunks, the last of one step"] == [5, 5, 5, 5, 1]
    assert lens["chunks of 6 and 5"] == [6, 5]
    assert lens["5 chunks, a pixel in the last"] == [5, 5, 5, 5, 1]
    # whether the last K step sees a pixel of gY at all: the last W + 2 rows of a bordered map are border rows
    for name, (nimg, H, W) in R.WGRAD_ROWS.items():
        last_pixel = int(R.bordered_index(nimg, H, W)[-1])
        assert last_pixel == rows[name] - 1 - (W + 2)
        if len(lens[name]) > 1:
            assert (last_pixel >= 32 * (sum(lens[name]) - 1)) == (name in ("chunks of 6 and 5", "5 chunks, a pixel in the last")), name
    # the split of these shapes does not depend on the channel counts of the file: the tile count never limits it
    for name, nimg, H, W, Cout, Cin in R.wgrad_cases():
        assert R.chunk_lengths(Cout, Cin, nimg, H, W) == lens[name]
    # tile remainders: M tiles of 128 output channels, N tiles of 128 of the 9 Cin columns
    assert [(c + 127) // 128 for c in R.WGRAD_COUT] == [1, 1, 1, 2, 3] and [c % 128 for c in R.WGRAD_COUT] == [4, 124, 0, 4, 4]
    assert (132 + 31) // 32 * 32 == 160
    assert [9 * c % 128 for c in R.WGRAD_CIN] == [32, 64, 96, 32] and (9 * 160 + 127) // 128 == 12
    cases = R.wgrad_cases()
    assert {(c[0], c[4]) for c in cases} == {(n, co) for n in R.WGRAD_ROWS for co in R.WGRAD_COUT}
    assert {(c[0], c[5]) for c in cases} == {(n, ci) for n in R.WGRAD_ROWS for ci in R.WGRAD_CIN}
    assert {(c[4], c[5]) for c in cases} == {(co, ci) for co in R.WGRAD_COUT for ci in R.WGRAD_CIN}
    # planes: 64 pixels x 32 channels a block
    assert [a * b * c % 64 for a, b, c in R.PLANES_PIX[:3]] == [1, 63, 0]
    assert any(p[2] == 1 and p[1] > 1 for p in R.PLANES_PIX) and any(p[1] == 1 and p[2] > 1 for p in R.PLANES_PIX)
    # the split conv: M-tile edges of the 64-, 128- and 256-row schedules
    assert [a * b * c for a, b, c in R.DSCALE_PIX] == [1, 63, 65, 70, 135]
    assert R.DSCALE_PIX[1][2] == 1 and R.DSCALE_PIX[2][1] == 1
    d = R.dscale_cases()
    for col, vals in ((3, R.DSCALE_COUT), (4, R.DSCALE_C1), (5, R.TILES), (6, [0, 1])):
        assert {(c[:3], c[col]) for c in d} == {(p, v) for p in R.DSCALE_PIX for v in vals}
    assert any(c[0] * c[1] * c[2] * c[3] // 4 % 256 != 0 for c in d)      # scale_rows_kernel: a ragged last block
    assert {(a * b * c) for a, b, c in R.INF_PIX.values()} == {70, 135, 257}
    assert {c[4] for c in R.E2E_CASES} == {132, 36, 4} and (1, 1, 21, 32, 4) in R.E2E_CASES and all(c[3] % 32 == 0 for c in R.E2E_CASES)


def test_inference_cases_are_a_pairwise_cover():
    cases = R.inference_cases()
    assert len(set(cases)) == len(cases)
    kinds, tiles = R.INF_KINDS, R.TILES
    for kind in kinds:
        mine = [c for c in cases if c[0] == kind]
        assert {(c[1], c[2]) for c in mine} == {(t, f) for t in tiles for f in R.INF_OUTS[kind]}
        assert {c[3] for c in mine} == {70, 135, 257} and {c[4] for c in mine} == set(R.INF_COUT)
        assert {c[7] for c in mine} == {1, 3} and {c[8] for c in mine} == {0, 1}
        assert {c[5] > 0 for c in mine} == ({False} if kind == "split2" else {False, True})
        assert {c[6] for c in mine} == ({0, 1} if kind in ("bf16", "fp16") else {0})
    for tile in tiles:
        mine = [c for c in cases if c[1] == tile]
        assert {c[3] for c in mine} == {70, 135, 257} and {c[4] for c in mine} == set(R.INF_COUT)
        assert {c[5] > 0 for c in mine} == {False, True} and {c[6] for c in mine} == {0, 1}
        assert {c[7] for c in mine} == {1, 3} and {c[8] for c in mine} == {0, 1}
    assert {(c[3], c[4]) for c in cases} == {(m, co) for m in (70, 135, 257) for co in R.INF_COUT}


# ---- every bound admits a correct fp32 evaluation --------------------------------------------------------------------------------
@pytest.mark.parametrize("name,Cout,Cin", [("7 rows, one step", 4, 32), ("rows % 32 == 31", 132, 64), ("chunks of 5 and 4", 124, 96),
                                           ("5 chunks, the last of one step", 260, 32), ("chunks of 6 and 5", 128, 160)])
def test_wgrad_bound_admits_fp32_in_two_orders(name, Cout, Cin):
    p = _planes_cpu(*R.WGRAD_ROWS[name], Cin, Cout)
    ref, ab = R.wgrad_ref(p["gh"], p["gl"], p["xh"], p["xl"], *p["geom"], p["inv"])
    bound = R.wgrad_bound(ab, Cout, Cin, *R.WGRAD_ROWS[name])
    assert torch.equal((bound > 0).all(0).all(0), R.live_taps(*R.WGRAD_ROWS[name][1:])), "a zero bound where a tap has terms"
    for order in (0, 1):
        got = R.wgrad_fp32(p["gh"], p["gl"], p["xh"], p["xl"], *p["geom"], p["inv"], order)
        worst, _ = R.ratio(got, ref, bound)
        assert worst <= 1.0, (order, worst)
    # the level-3 bound holds the level-2 reference (what the planes cannot represent) and a plain fp32 evaluation of the fp32 inputs
    e2e = R.e2e_ref(p["x"], p["w"], p["gy"])
    assert R.ratio(ref, *e2e["dw"])[0] <= 1.0
    assert torch.equal((e2e["dw"][1] > 0).all(0).all(0), R.live_taps(*R.WGRAD_ROWS[name][1:]))
    x32 = p["x"].clone().requires_grad_(True)
    w32 = p["w"].clone().requires_grad_(True)
    gx32, dw32 = torch.autograd.grad(F.conv2d(x32, w32, padding=1), (x32, w32), p["gy"])
    assert R.ratio(dw32, *e2e["dw"])[0] <= 1.0 and R.ratio(gx32, *e2e["gx"])[0] <= 1.0
    assert R.ratio(F.conv2d(p["x"], p["w"], padding=1), *e2e["y"])[0] <= 1.0


@pytest.mark.parametrize("nimg,H,W,C1,Cout", [(1, 1, 1, 32, 4), (2, 5, 7, 96, 132), (3, 21, 1, 32, 132)])
def test_split_conv_bound_admits_fp32_in_two_orders(nimg, H, W, C1, Cout):
    from mickey_amd import train_heads as th
    x, w, _ = R.train_inputs(nimg, H, W, C1, Cout, "splitcpu")
    sx, sw = R.scale_ref(x), R.scale_ref(w)
    ah, al = (R.bordered(p, nimg, H, W) for p in R.planes_ref(x, sx[0]))
    wpl = th.weight_planes(w, sw[0])
    ref, e = R.split_conv_ref(ah, al, wpl, nimg, H, W, sx[1] * sw[1])
    assert float(e.min()) > 0.0
    for order in (0, 1):
        assert R.ratio(R.split_conv_fp32(ah, al, wpl, nimg, H, W, sx[1] * sw[1], order), ref, e)[0] <= 1.0
    y, by = R.e2e_ref(x, w, torch.ones((nimg, Cout, H, W)))["y"]
    assert R.ratio(ref, R.dense_rows(y), R.dense_rows(by))[0] <= 1.0
    # planes of the result: a correct fp32 value, split as the epilogue does, meets both plane bounds
    v32 = R.split_conv_fp32(ah, al, wpl, nimg, H, W, sx[1] * sw[1], 1)
    sv = v32 * R.ACT_SCALE
    hi = sv.half()
    lo = (sv - hi.float()).half()
    bh, bs = R.planes_bounds(ref, e, R.ACT_SCALE)
    assert R.ratio(hi, ref * R.ACT_SCALE, bh)[0] <= 1.0 and R.ratio(hi.double() + lo.double(), ref * R.ACT_SCALE, bs)[0] <= 1.0


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("out_f32", [True, False])
def test_lp_conv_bound_admits_fp32_in_two_orders(dtype, out_f32):
    nimg, H, W, C1, C2, Cout = 2, 5, 7, 64, 64, 132
    c = R.lp_conv_inputs(nimg, H, W, C1, C2, Cout, 1, dtype, "lpcpu")
    a, a2, w2d, bias, resid = c["a"][0], c["a2"], c["w"][0], c["bias"][0], c["resid"][0]
    ref, e = R.lp_conv_ref(a, w2d, nimg, H, W, dtype, out_f32, a2=a2, bias=bias, resid=resid, relu=True)
    assert float(e.min()) > 0.0
    cols = R.im2col(a, nimg, H, W, a2).float()
    r = resid[R.bordered_index(nimg, H, W)].float()
    for order in (0, 1):
        if order == 0:
            v = cols @ w2d.float().t() + bias + r
        else:
            v = r + bias
            cf, wf = cols.flip(1), w2d.float().flip(1)
            for k in range(0, cf.shape[1], 48):
                v = v + cf[:, k:k + 48] @ wf[:, k:k + 48].t()
        v = v.clamp_min(0.0)
        got = v if out_f32 else v.to(dtype)
        assert R.ratio(got, ref, e)[0] <= 1.0, order


def test_designed_inputs_leave_no_zero_bound():
    for name, nimg, H, W, Cout, Cin in R.wgrad_cases()[::3]:
        p = _planes_cpu(nimg, H, W, Cin, Cout, "gpu")
        _, ab = R.wgrad_ref(p["gh"], p["gl"], p["xh"], p["xl"], nimg, H, W, Cout, Cin, p["inv"])
        assert torch.equal((ab > 0).all(0).all(0), R.live_taps(H, W)), (name, Cout, Cin)
        assert bool((p["x"] == 0).any()) == (nimg * H * W >= 8)      # exact zeros wherever a sum keeps other terms
    x, _, _ = R.train_inputs(3, 7, 25, 32, 4, "gpu")
    mags = x.abs().amax(1)
    assert float(mags.max() / mags[mags > 0].min()) > 100.0      # the per-pixel magnitude spread


# ---- mutants ---------------------------------------------------------------------------------------------------------------------
def _wgrad_mutant(name, Cout, Cin, elem, **mutation):
    nimg, H, W = R.WGRAD_ROWS[name]
    p = _planes_cpu(nimg, H, W, Cin, Cout, "mutant")
    args = (p["gh"], p["gl"], p["xh"], p["xl"], nimg, H, W, Cout, Cin, p["inv"])
    ref, ab = R.wgrad_ref(*args)
    bound = R.wgrad_bound(ab, Cout, Cin, nimg, H, W)
    mut, _ = R.wgrad_ref(*args, **mutation)
    assert R.ratio(ref, ref, bound)[0] == 0.0
    worst, at = R.ratio(_one(mut, ref, elem), ref, bound)
    assert worst > 1.0, (mutation, worst)
    return worst


def test_mutant_tap_shift_off_by_one_row():
    # tap 0 (ky = kx = 0) reads one bordered grid row too low: the last output channel of a 132-wide tile, the last input channel
    _wgrad_mutant("chunks of 5 and 4", 132, 32, (131, 31, 0, 0), shift_tap=(0, 1))
    _wgrad_mutant("rows % 32 == 1, W = 1", 4, 32, (3, 31, 2, 1), shift_tap=(7, -1))   # (W = 1: the taps kx != 1 have no term)


def test_mutant_last_step_of_a_chunk_dropped():
    _wgrad_mutant("chunks of 5 and 4", 4, 32, (3, 31, 1, 1), drop_step=0)
    _wgrad_mutant("chunks of 6 and 5", 132, 32, (131, 0, 1, 1), drop_step=1)


def test_mutant_one_partial_dropped():
    _wgrad_mutant("5 chunks, the last of one step", 4, 32, (0, 31, 1, 1), drop_chunk=3)   # (the chunk of one step holds border rows only)
    _wgrad_mutant("chunks of 5 and 4", 260, 32, (259, 31, 1, 1), drop_chunk=1)
    _wgrad_mutant("5 chunks, a pixel in the last", 4, 32, (3, 31, 1, 1), drop_chunk=4)   # one pixel row, one term


def test_mutant_gl_xh_product_dropped():
    # the product is 2^-12 of its term: seen where few terms are summed (gamma(97) = 2^-17.4), as a norm never could
    _wgrad_mutant("7 rows, one step", 4, 32, (3, 31, 1, 1), drop_glxh=True)
    _wgrad_mutant("rows % 32 == 31", 132, 32, (131, 31, 1, 1), drop_glxh=True)


def test_mutant_channel_128_from_channel_0():
    _wgrad_mutant("rows % 32 == 31", 132, 32, (128, 0, 1, 1), alias_128=True)


def test_mutant_nonzero_border_row_of_x():
    nimg, H, W = R.WGRAD_ROWS["chunks of 5 and 4"]
    Cout, Cin = 4, 32
    p = _planes_cpu(nimg, H, W, Cin, Cout, "mutant")
    ref, ab = R.wgrad_ref(p["gh"], p["gl"], p["xh"], p["xl"], nimg, H, W, Cout, Cin, p["inv"])
    bound = R.wgrad_bound(ab, Cout, Cin, nimg, H, W)
    xh = p["xh"].clone()
    border = int(R.bordered_index(nimg, H, W)[W - 1]) + 1 + R.lead_rows(W)   # the shared column behind the first grid row
    assert float(xh[border].abs().max()) == 0.0
    xh[border] = xh[border - 1]                    # a plane kernel that wrote the last pixel of the grid row once more, one row on
    mut, _ = R.wgrad_ref(p["gh"], p["gl"], xh, p["xl"], nimg, H, W, Cout, Cin, p["inv"])
    # seen by ONE element of tap (1, 2), whose gY row is the pixel left of the border row
    co, ci = int(p["gh"][border - 1, :Cout].abs().argmax()), int(xh[border].abs().argmax())
    assert R.ratio(_one(mut, ref, (co, ci, 1, 2)), ref, bound)[0] > 1.0


def test_mutant_dgrad_weight_not_flipped():
    nimg, H, W, Cin, Cout = 2, 5, 7, 32, 4
    x, w, gy = R.train_inputs(nimg, H, W, Cin, Cout, "mutant")
    ref, bound = R.e2e_ref(x, w, gy)["gx"]
    mut, _ = R.e2e_ref(x, w, gy, unflipped=True)["gx"]
    for elem in ((0, 0, 0, 0), (nimg - 1, Cin - 1, H - 1, W - 1)):
        assert R.ratio(_one(mut, ref, elem), ref, bound)[0] > 1.0


def test_mutant_conv_tap_shift_at_the_first_and_last_image_row():
    from mickey_amd import train_heads as th
    nimg, H, W, C1, Cout = 2, 5, 7, 32, 132
    x, w, _ = R.train_inputs(nimg, H, W, C1, Cout, "mutant")
    sx, sw = R.scale_ref(x), R.scale_ref(w)
    ah, al = (R.bordered(p, nimg, H, W) for p in R.planes_ref(x, sx[0]))
    wpl = th.weight_planes(w, sw[0])
    ref, e = R.split_conv_ref(ah, al, wpl, nimg, H, W, sx[1] * sw[1])
    M = nimg * H * W
    for tap, d, elem in ((1, 1, (0, Cout - 1)), (7, -1, (M - 1, 128)), (4, 1, (M - 1, 0))):
        mut, _ = R.split_conv_ref(ah, al, wpl, nimg, H, W, sx[1] * sw[1], shift_tap=(tap, d))
        assert R.ratio(_one(mut, ref, elem), ref, e)[0] > 1.0, (tap, d)
