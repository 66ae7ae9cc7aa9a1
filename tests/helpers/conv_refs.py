"""References, input builders, bounds and the case lists of the 3x3 convolution edge tests (tests/test_conv_edges_cpu.py checks
them here on the CPU, tests/test_conv_edges_gpu.py runs the kernels against them): the inference forms of the A_CONV3 stager
(mk_conv3x3, mk_conv3x3_split) and the whole training chain of mk_train_conv.hip.  Pure torch on the CPU.

Every value reference is fp64; a case passes when |got - ref64| / bound <= 1 on EVERY element, and every part of a bound is
derived here, before any kernel ran (u = 2^-24, gamma(n) = n u / (1 - n u), SLACK = 1.01 for the second-order terms; all from
tests/helpers/heads_refs.py).  Three levels:

  1. EXACT, compared as integers: the plane scale (scale_ref: the contract of mickey_hip.h), the operand planes (planes_ref:
     hi = fp16(fl32(x s)), lo = fp16(fl32(x s - hi)) -- x s is exact for a power-of-two s short of fp32's range ends, and
     x s - hi is exact always, so a correct kernel has no freedom), the weight planes (train_heads.weight_planes).
  2. A KERNEL GIVEN ITS PLANES: the reference is the fp64 sum of the products of the planes' actual bits.  A product of two fp16
     values has 22 significant bits and an exponent inside fp32's range: it is EXACT in fp32, on the matrix cores as in torch.
     The only error is the fp32 summation, in whatever order and grouping: gamma(n) sum |terms| for n terms.
  3. END TO END: train_heads.conv3x3_train against fp64 autograd on the fp32 inputs; the level-2 bound plus what the planes
     cannot represent, propagated through sum |terms| (product_bound)."""
import math

import torch
import torch.nn.functional as F

from tests.helpers.heads_refs import SLACK, U, U_OUT, UNDERFLOW, bordered_index, bordered_rows, gam, gen, planes_bounds, ratio  # noqa: F401

F16_SENTINEL = 0x7AB7        # tests/helpers/guarded.py: the finite fp16 sentinel (5.5e4), as bits
ACT_SCALE, W_SCALE = 64.0, 1024.0   # ops.SPLIT_ACT_SCALE, ops.SPLIT_W_SCALE (asserted equal in the GPU module)


# ================================================================ geometry =====================================================
def lead_rows(W):
    """rows in front of bordered row 0 in a training plane buffer (mk_conv_train_lead_rows)"""
    return W + 2


def plane_rows(nimg, H, W):
    """rows of a training plane buffer (mk_conv_train_plane_rows)"""
    return (W + 2) + (bordered_rows(nimg, H, W) + 31) // 32 * 32 + (W + 2)


def tap_shift(tap, W):
    """the row shift of tap = 3 ky + kx in a bordered feature map"""
    return (tap // 3 - 1) * (W + 1) + tap % 3 - 1


def live_taps(H, W):
    """bool [3, 3]: the taps of the weight gradient that have a term at all -- with H = 1 (W = 1) the taps of the rows above and
    below (the columns left and right) pair every pixel with padding: their sums are exactly 0, bound 0, and a kernel must return 0"""
    ky = torch.tensor([H > 1, True, H > 1])
    kx = torch.tensor([W > 1, True, W > 1])
    return ky[:, None] & kx[None, :]


def wgrad_split(Cout, Cin, nimg, H, W):
    """-> (chunk, nsteps, ksplit): the K split of mk_conv_wgrad, restated from the comment at the head of mk_train_conv.hip -- K steps
    of 32 bordered rows; about 512 workgroups (two per CU of a 256-CU part) but never fewer than 4 steps a chunk; chunks of equal
    length, the last one shorter.  tests/test_conv_edges_cpu.py holds it against mk_conv_wgrad_work_floats."""
    nsteps = (bordered_rows(nimg, H, W) + 31) // 32
    tiles = ((Cout + 127) // 128) * ((9 * Cin + 127) // 128)
    ks = max(1, min(512 // tiles, nsteps // 4))
    chunk = (nsteps + ks - 1) // ks
    return chunk, nsteps, (nsteps + chunk - 1) // chunk


def chunk_lengths(Cout, Cin, nimg, H, W):
    chunk, nsteps, ksplit = wgrad_split(Cout, Cin, nimg, H, W)
    return [min(chunk, nsteps - c * chunk) for c in range(ksplit)]


# ================================================================ the designed shapes ==========================================
# name -> (nimg, H, W): the row shapes of the weight gradient, each named for the edge it is there for (asserted in
# tests/test_conv_edges_cpu.py::test_designed_shapes_have_their_edges).  The last W + 2 rows of a bordered map are border rows: a
# last K step holds pixels of gY only where rows % 32 > W + 2 -- the last two shapes (W = 3, W = 1) are built for that: without
# them a reduce that forgets its last partial, or a last chunk that forgets its last step, would change nothing.
WGRAD_ROWS = {
    "7 rows, one step": (1, 1, 1),
    "rows % 32 == 31": (1, 1, 9),
    "rows % 32 == 0, nk = 2": (1, 1, 20),
    "rows % 32 == 1, W = 1": (3, 4, 1),
    "one chunk of 3 steps": (1, 1, 21),
    "chunks of 5 and 4": (3, 2, 25),
    "5 chunks, the last of one step": (3, 7, 25),
    "chunks of 6 and 5": (2, 40, 3),
    "5 chunks, a pixel in the last": (3, 106, 1),
}
WGRAD_COUT = [4, 124, 128, 132, 260]     # ldg = 160 at 132; three M tiles at 260
WGRAD_CIN = [32, 64, 96, 160]            # 9 Cin % 128 = 32, 64, 96; 12 N tiles (32 left over) at 160


def wgrad_cases():
    """(name, nimg, H, W, Cout, Cin): every row shape with every Cout, Cin rotating so that every (row shape, Cin) and every
    (Cout, Cin) pair occurs too -- a pairwise cover in 45 cases instead of the 180 of the full product"""
    out = []
    for i, (name, (nimg, H, W)) in enumerate(WGRAD_ROWS.items()):
        for j, cout in enumerate(WGRAD_COUT):
            out.append((name, nimg, H, W, cout, WGRAD_CIN[(i + j) % 4]))
    return out


PLANES_PIX = [(1, 1, 1), (1, 3, 21), (1, 4, 16), (2, 5, 1), (2, 1, 5)]   # npix % 64 = 1, 63, 0; W = 1; H = 1
PLANES_C = [4, 32, 36, 68]
PLANES_LAYOUTS = ["contiguous", "channels_last", "slice", "slice_channels_last", "expand"]

WEIGHT_SHAPES = [(4, 32), (36, 32), (132, 64)]

# M = nimg H W of the split conv's M-tile edges: 1, 63 (W = 1), 65 (H = 1), 70, 135
DSCALE_PIX = [(1, 1, 1), (3, 21, 1), (1, 1, 65), (2, 5, 7), (3, 5, 9)]
DSCALE_COUT, DSCALE_C1, TILES = [4, 132], [32, 96], [1, 2, 7]


def dscale_cases():
    """(nimg, H, W, Cout, Cin, tile, transposed): pixels x schedule x direction x Cout in full, Cin rotating against all four"""
    out = []
    for i, pix in enumerate(DSCALE_PIX):
        for t, tile in enumerate(TILES):
            for tr in (0, 1):
                for j, cout in enumerate(DSCALE_COUT):
                    out.append(pix + (cout, DSCALE_C1[(i + t + tr + j) % 2], tile, tr))
    return out


# (nimg, H, W, Cin, Cout) of the end-to-end runs; Cin is a multiple of 32 (the op refuses anything else), so the 132- and the 36-wide
# tile remainders come in as Cout: gY's planes are then [.., 160] and [.., 64] wide and the input gradient contracts over the padding
E2E_CASES = [(3, 7, 25, 64, 132), (2, 5, 7, 96, 36), (1, 1, 21, 32, 4)]

# the inference forms of the stager: M = 70, 135, 257
INF_PIX = {70: (2, 5, 7), 135: (3, 5, 9), 257: (1, 1, 257)}
INF_KINDS = ["bf16", "fp16", "split3", "split2"]
INF_OUTS = {"bf16": ["f32", "lp", "lp_bordered"], "fp16": ["f32", "lp", "lp_bordered"],
            "split3": ["f32", "f32_bordered", "planes", "planes_bordered"], "split2": ["f32", "f32_bordered", "planes", "planes_bordered"]}
INF_COUT = [4, 132, 260]


def inference_cases():
    """(kind, tile, out, M, Cout, C2, resid, groups, relu).  kind x tile x output form in full (42 cases); M, Cout, the shortcut
    source, the residual, the groups and the activation rotate with different periods, so that every value of each meets every
    kind, every schedule and -- over the file -- every value of the others.  The identity residual exists for 16-bit operands
    only and the second source not with a lone hi plane (mickey_hip.h)."""
    out, i = [], 0
    for kind in INF_KINDS:
        for t, tile in enumerate(TILES):
            for form in INF_OUTS[kind]:
                M = [70, 135, 257][(i + t) % 3]
                cout = INF_COUT[(i // 3 + t) % 3]
                c2 = 0 if kind == "split2" else [0, 64 if kind in ("bf16", "fp16") else 32][(i + i // 2) % 2]
                resid = kind in ("bf16", "fp16") and (i // 2) % 2 == 1
                groups = [1, 3][(i + i // 4) % 2]
                relu = (i // 3) % 2
                out.append((kind, tile, form, M, cout, c2, int(resid), groups, relu))
                i += 1
    return out


# ================================================================ inputs =======================================================
def spread(shape, key, pixel_dim, sigma=1.5, zeros=0.1, clamp=900.0):
    """randn with a per-pixel log-normal magnitude spread (`pixel_dim`: the dimensions that share a magnitude are all others) and
    some exact zeros, as test_conv3x3_split_is_fp32_grade uses: the lo planes reach fp16's subnormals, post-ReLU zeros occur"""
    g = gen("spread", key, tuple(shape))
    x = torch.randn(shape, generator=g)
    mshape = [s if d in pixel_dim else 1 for d, s in enumerate(shape)]
    x = x * torch.exp(sigma * torch.randn(mshape, generator=g))
    x = torch.where(torch.rand(shape, generator=g) < zeros, torch.zeros(()), x)
    return x.clamp_(-clamp, clamp)


def train_inputs(nimg, H, W, Cin, Cout, key="train"):
    """x [nimg, Cin, H, W], w [Cout, Cin, 3, 3], gy [nimg, Cout, H, W] fp32.  The gradient is small (a REINFORCE gradient has no
    known magnitude), the weight has nn.Conv2d's scale; no tensor is all zero (a zero is replaced at element 0)."""
    zeros = 0.1 if nimg * H * W >= 8 else 0.0   # a handful of pixels: an exact zero would leave whole sums without a term
    x = spread((nimg, Cin, H, W), (key, "x"), (0, 2, 3), zeros=zeros)
    gy = spread((nimg, Cout, H, W), (key, "gy"), (0, 2, 3), sigma=1.0, zeros=zeros) * 2.0 ** -9
    w = torch.randn((Cout, Cin, 3, 3), generator=gen(key, "w", Cout, Cin)) / math.sqrt(9 * Cin)
    for t in (x, gy):
        if float(t.abs().max()) == 0.0:
            t.view(-1)[0] = 1.0
    return x, w, gy


def inference_inputs(nimg, H, W, C1, C2, Cout, groups, key="inf"):
    """fp32 values of one inference conv: x [G, M, C1] (spread, post-ReLU zeros), x2 [M, C2] or None (shared by the groups), w [G,
    Cout, 9 C1 + C2] tap-major, bias [G, Cout], resid [G, M, Cout]"""
    M, K = nimg * H * W, 9 * C1 + C2
    g = gen("inference", key, nimg, H, W, C1, C2, Cout, groups)
    x = spread((groups, M, C1), (key, "x"), (0, 1), sigma=1.0)
    x2 = torch.randn((M, C2), generator=g) * 3.0 if C2 else None
    w = torch.randn((groups, Cout, K), generator=g) / math.sqrt(K)
    bias = torch.randn((groups, Cout), generator=g)
    resid = torch.randn((groups, M, Cout), generator=g)
    return dict(x=x, x2=x2, w=w, bias=bias, resid=resid)


def lp_conv_inputs(nimg, H, W, C1, C2, Cout, groups, dtype, key="inf"):
    """the same, rounded to `dtype` and laid out as mk_conv3x3 takes them: a [G, R, C1], a2 [R, C2] or None, w [G, Cout, K], bias fp32
    [G, Cout], resid [G, R, Cout] (bordered maps with zero border rows)"""
    v = inference_inputs(nimg, H, W, C1, C2, Cout, groups, key)
    b = lambda rows: bordered(rows.to(dtype), nimg, H, W)   # noqa: E731
    return dict(a=torch.stack([b(r) for r in v["x"]]), a2=None if v["x2"] is None else b(v["x2"]), w=v["w"].to(dtype), bias=v["bias"],
                resid=torch.stack([b(r) for r in v["resid"]]))


# ================================================================ level 1: exact ===============================================
def scale_ref(x):
    """(s, 1 / s) of mk_absmax_scale as python floats, from the header's contract alone: s = 2^k with max|x| 2^k in [2^14, 2^15), k
    clamped to [-100, 100]; an all-zero tensor (1, 1); a non-finite element (1, NaN)."""
    if not bool(torch.isfinite(x).all()):
        return 1.0, float("nan")
    m = float(x.abs().max())
    if m == 0.0:
        return 1.0, 1.0
    k = 14 - (math.frexp(m)[1] - 1)      # frexp: m = f 2^e, f in [0.5, 1): floor(log2 m) = e - 1 (exact for subnormals too)
    k = max(-100, min(100, k))
    return 2.0 ** k, 2.0 ** -k


def same_scale(got, want):
    """got: fp32 [2] as the kernel left it; want: scale_ref's pair.  Bit-equal, NaN matching any NaN."""
    g0, g1 = torch.tensor(got[0], dtype=torch.float32), torch.tensor(got[1], dtype=torch.float32)
    w0, w1 = torch.tensor(want[0], dtype=torch.float32), torch.tensor(want[1], dtype=torch.float32)
    ok0 = bool(g0.view(torch.int32) == w0.view(torch.int32))
    ok1 = bool(torch.isnan(g1)) if math.isnan(want[1]) else bool(g1.view(torch.int32) == w1.view(torch.int32))
    return ok0 and ok1


def planes_ref(x, s):
    """x fp32 [nimg, C, H, W] (any strides) -> (hi, lo) fp16 dense rows [nimg H W, C]: hi = fp16(fl32(x s)), lo = fp16(fl32(x s - hi)),
    round to nearest even, subnormals kept, no clamping"""
    v = x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).float() * torch.tensor(s, dtype=torch.float32)
    hi = v.half()
    return hi, (v - hi.float()).half()


def plane_buffer(nimg, H, W, C, ld, hi, lo, fill=0):
    """The training plane buffers [plane_rows, ld] a correct kernel leaves when it starts from buffers filled with the fp16 bit
    pattern `fill`: pixel rows, columns < C hold (hi, lo); everything else keeps `fill`.  -> int16 (bits) hi, lo."""
    rows = plane_rows(nimg, H, W)
    out = []
    idx = bordered_index(nimg, H, W) + lead_rows(W)
    for p in (hi, lo):
        b = torch.full((rows, ld), fill, dtype=torch.int16)
        b[idx, :C] = p.view(torch.int16)
        out.append(b)
    return out


# ================================================================ level 2: a kernel given its planes ===========================
def wgrad_ref(gh, gl, xh, xl, nimg, H, W, Cout, Cin, inv, shift_tap=None, drop_step=None, drop_chunk=None, drop_glxh=False,
              alias_128=False):
    """mk_conv_wgrad from the planes' bits.  gh, gl [plane_rows, ldg], xh, xl [plane_rows, Cin]: the WHOLE buffers (bordered row 0 is
    row lead_rows(W)) as fp16; inv = (1 / s_g)(1 / s_x), a power of two.  -> (dw64, abs64) [Cout, Cin, 3, 3]:
      dw[co, ci, tap] = inv sum over the 32 nsteps rows r the kernel sweeps of gh[r, co] xh[r + shift, ci] + gl[r, co] xh[r + shift, ci]
                        + gh[r, co] xl[r + shift, ci]
    and abs64 the same sum of the |products|.  Every product is exact in fp32 (module docstring), the multiplication by inv is exact,
    so wgrad_bound is the whole error of a correct kernel.
    The switches are the MUTANTS of tests/test_conv_edges_cpu.py: shift_tap = (tap, rows): that tap's shift off by `rows` bordered
    rows of X; drop_step = c: the last 32-row step of chunk c left out; drop_chunk = c: the partial of chunk c left out; drop_glxh:
    no gl . xh product; alias_128: output channel 128 computed from gY's column 0."""
    lead = lead_rows(W)
    chunk, nsteps, ksplit = wgrad_split(Cout, Cin, nimg, H, W)
    keep = torch.ones(32 * nsteps, dtype=torch.float64)
    if drop_step is not None:
        last = min(chunk * (drop_step + 1), nsteps) - 1
        keep[32 * last:32 * (last + 1)] = 0
    if drop_chunk is not None:
        keep[32 * chunk * drop_chunk:32 * min(chunk * (drop_chunk + 1), nsteps)] = 0
    sweep = slice(lead, lead + 32 * nsteps)
    G, Gl = gh[sweep, :Cout].double() * keep[:, None], gl[sweep, :Cout].double() * keep[:, None]
    if alias_128:
        G, Gl = G.clone(), Gl.clone()
        G[:, 128], Gl[:, 128] = G[:, 0], Gl[:, 0]
    dw, ab = [], []
    for tap in range(9):
        s = tap_shift(tap, W) + (shift_tap[1] * (W + 1) if shift_tap is not None and shift_tap[0] == tap else 0)
        rows = slice(lead + s, lead + s + 32 * nsteps)
        X, Xl = xh[rows].double(), xl[rows].double()
        mid = 0.0 if drop_glxh else Gl.t() @ X
        dw.append(G.t() @ X + mid + G.t() @ Xl)
        ab.append(G.abs().t() @ X.abs() + Gl.abs().t() @ X.abs() + G.abs().t() @ Xl.abs())
    return torch.stack(dw, -1).reshape(Cout, Cin, 3, 3) * inv, torch.stack(ab, -1).reshape(Cout, Cin, 3, 3) * inv


def wgrad_terms(Cout, Cin, nimg, H, W):
    """the number of fp32 additions behind one element: 3 products x the rows swept (whole steps of 32) + the ksplit partials of
    the reduce"""
    _, nsteps, ksplit = wgrad_split(Cout, Cin, nimg, H, W)
    return 3 * 32 * nsteps + ksplit


def wgrad_bound(abs64, Cout, Cin, nimg, H, W):
    return gam(wgrad_terms(Cout, Cin, nimg, H, W)) * abs64 * SLACK


def wgrad_fp32(gh, gl, xh, xl, nimg, H, W, Cout, Cin, inv, order=0):
    """A correct fp32 implementation of the same sums.  order 0: one torch matmul per product, added; order 1: the kernel's own
    grouping -- per chunk, per 32-row step, rows reversed, the three products of a step added to a running sum -- then the chunks"""
    lead = lead_rows(W)
    chunk, nsteps, ksplit = wgrad_split(Cout, Cin, nimg, H, W)
    G, Gl = gh[lead:lead + 32 * nsteps, :Cout].float(), gl[lead:lead + 32 * nsteps, :Cout].float()
    out = []
    for tap in range(9):
        s = tap_shift(tap, W)
        X, Xl = xh[lead + s:lead + s + 32 * nsteps].float(), xl[lead + s:lead + s + 32 * nsteps].float()
        if order == 0:
            out.append(G.t() @ X + Gl.t() @ X + G.t() @ Xl)
            continue
        total = torch.zeros((Cout, Cin))
        for c in range(ksplit):
            acc = torch.zeros((Cout, Cin))
            for st in range(c * chunk, min((c + 1) * chunk, nsteps)):
                r = slice(32 * st, 32 * st + 32)
                g, g2, x, x2 = G[r].flip(0), Gl[r].flip(0), X[r].flip(0), Xl[r].flip(0)
                acc = acc + g.t() @ x
                acc = acc + g2.t() @ x
                acc = acc + g.t() @ x2
            total = total + acc
        out.append(total)
    return torch.stack(out, -1).reshape(Cout, Cin, 3, 3) * torch.tensor(inv, dtype=torch.float32)


def im2col(xb, nimg, H, W, untapped=None, shift_tap=None):
    """bordered map [R, C] -> [nimg H W, 9 C], column tap C + c = xb[row(pixel) + shift(tap), c]; untapped: a second bordered map
    [R, C2] whose pixel rows are appended (the 1x1 shortcut source).  shift_tap = (tap, rows): the MUTANT with one tap's shift off
    by `rows` bordered rows (clamped into the map)."""
    idx = bordered_index(nimg, H, W)
    R = xb.shape[0]
    cols = []
    for tap in range(9):
        s = tap_shift(tap, W) + (shift_tap[1] * (W + 1) if shift_tap is not None and shift_tap[0] == tap else 0)
        cols.append(xb[(idx + s).clamp(0, R - 1)])
    if untapped is not None:
        cols.append(untapped[idx])
    return torch.cat(cols, 1)


def split_weight_planes(wpl):
    """interleaved (32 hi | 32 lo) planes [.., 2 K] -> (hi, lo) [.., K] (weights.split_conv_weight_planes, restated for fp64 use)"""
    lead = tuple(wpl.shape[:-1])
    v = wpl.reshape(lead + (wpl.shape[-1] // 64, 2, 32))
    return v[..., 0, :].reshape(lead + (-1,)), v[..., 1, :].reshape(lead + (-1,))


def split_conv_ref(ah, al, wpl, nimg, H, W, acc_scale, a2=None, bias=None, relu=False, shift_tap=None):
    """mk_conv3x3_split / mk_conv3x3_split_dscale from the planes' bits.  ah, al: bordered fp16 planes [R, C1] (al None: the
    two-product form on a lone hi plane), a2: None or the (hi, lo) planes [R, C2] of the shortcut source, wpl: fp16 [Cout, 2 K]
    interleaved, K = 9 C1 (+ C2).  -> (ref64, e32) [nimg H W, Cout]:
      acc = sum_k ah wh + ah wl + al wh        3 K exact products (2 K without al), fp32 sums: gamma(3 K) sum |products|
      v = acc acc_scale (+ bias)               a power of two: exact; the bias one more term and one more rounding
      relu                                     1-Lipschitz: the bound carries over
    n = 3 K + 3 terms and roundings at the most."""
    wh, wl = (t.double() for t in split_weight_planes(wpl))
    Ah = im2col(ah, nimg, H, W, None if a2 is None else a2[0], shift_tap).double()
    K = Ah.shape[1]
    acc = Ah @ (wh + wl).t()
    ab = Ah.abs() @ (wh.abs() + wl.abs()).t()
    if al is not None:
        Al = im2col(al, nimg, H, W, None if a2 is None else a2[1], shift_tap).double()
        acc = acc + Al @ wh.t()
        ab = ab + Al.abs() @ wh.abs().t()
    ref, ab = acc * acc_scale, ab * acc_scale
    if bias is not None:
        ref, ab = ref + bias.double(), ab + bias.double().abs()
    e = gam(3 * K + 3) * ab * SLACK
    return (ref.clamp_min(0.0) if relu else ref), e


def split_conv_fp32(ah, al, wpl, nimg, H, W, acc_scale, order=0):
    """A correct fp32 implementation of split_conv_ref's sums (no shortcut source, no bias); order 1: K reversed, blocks of 32 added
    to a running sum, product by product"""
    wh, wl = (t.float() for t in split_weight_planes(wpl))
    Ah, Al = im2col(ah, nimg, H, W).float(), im2col(al, nimg, H, W).float()
    if order == 0:
        acc = Ah @ wh.t() + Ah @ wl.t() + Al @ wh.t()
    else:
        Ah, Al, wh, wl = Ah.flip(1), Al.flip(1), wh.flip(1), wl.flip(1)
        acc = torch.zeros((Ah.shape[0], wh.shape[0]))
        for k in range(0, Ah.shape[1], 32):
            k2 = slice(k, k + 32)
            acc = acc + Ah[:, k2] @ wh[:, k2].t()
            acc = acc + Ah[:, k2] @ wl[:, k2].t()
            acc = acc + Al[:, k2] @ wh[:, k2].t()
    return acc * torch.tensor(acc_scale, dtype=torch.float32)


def lp_conv_ref(a, w2d, nimg, H, W, dtype, out_f32, a2=None, bias=None, resid=None, relu=False, shift_tap=None):
    """mk_conv3x3 on 16-bit operands: a bordered [R, C1], a2 None or bordered [R, C2], w2d [Cout, K], bias fp32 [Cout], resid None or
    bordered [R, Cout] -> (ref64, bound) [nimg H W, Cout].  Products of two 16-bit values are exact in fp32; K of them, the bias and
    the residual are summed in fp32: gamma(K + 3) sum |terms|; a 16-bit output is rounded once: U_OUT |ref| + UNDERFLOW (its
    second-order part, U_OUT x the fp32 error, is inside SLACK: 2^-8 < 0.01)."""
    cols = im2col(a, nimg, H, W, a2, shift_tap).double()
    K = cols.shape[1]
    ref = cols @ w2d.double().t()
    ab = cols.abs() @ w2d.double().abs().t()
    if bias is not None:
        ref, ab = ref + bias.double(), ab + bias.double().abs()
    if resid is not None:
        r = resid[bordered_index(nimg, H, W)].double()
        ref, ab = ref + r, ab + r.abs()
    if relu:
        ref = ref.clamp_min(0.0)
    e = gam(K + 3) * ab * SLACK
    if not out_f32:
        e = e + U_OUT[dtype] * ref.abs() + UNDERFLOW[dtype]
    return ref, e


# ================================================================ level 3: end to end ==========================================
def rep_err(v, s):
    """What a plane pair of scale s cannot represent of v, element-wise: |(hi + lo) / s - v| <= 2^-22 |v| + 2^-25 / s (hi carries 11
    bits, lo 11 more -- relative 2^-22 -- unless lo falls into fp16's subnormals, spacing 2^-24: 2^-25 absolute on v s; as
    planes_bounds in tests/helpers/heads_refs.py).  An exact zero has exact planes."""
    v = v.double().abs()
    return torch.where(v > 0, 2.0 ** -22 * v + 2.0 ** -25 / s, torch.zeros_like(v))


def product_bound(A, dA, B, dB, n):
    """Bound of sum_k A[i, k] B[k, j] computed by a split kernel from the planes of A and B, against the exact product of the fp32
    values; A [I, K], B [K, J] fp64, dA / dB = rep_err of them, n the number of fp32 terms:
      gamma(n) sum |A| |B|            the level-2 summation error; the three kept products |hi hi| + |lo hi| + |hi lo| are within
                                      (1 + 2^-11)^2 of |A| |B|, inside SLACK
      sum |A| dB + dA |B| + dA dB     the representation errors of the operands
      2^-22 sum |A| |B|               the dropped lo . lo product: |lo| <= 2^-11 |v s| on both sides"""
    A, B = A.abs(), B.abs()
    ab = A @ B
    return (gam(n) * ab + A @ dB + dA @ B + dA @ dB + 2.0 ** -22 * ab) * SLACK


def dense_rows(x):
    """[B, C, H, W] -> [B H W, C]"""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])


def tap_major(w):
    """[Cout, Cin, 3, 3] -> [Cout, 9 Cin], column tap Cin + ci"""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)


def bordered(rows, nimg, H, W):
    """dense rows [nimg H W, C] -> bordered map [R, C], zeros elsewhere"""
    out = rows.new_zeros((bordered_rows(nimg, H, W), rows.shape[1]))
    out[bordered_index(nimg, H, W)] = rows
    return out


def e2e_ref(x, w, gy, unflipped=False):
    """fp64 (y, gX, dW) of the 3x3 convolution, by the formulas the kernels implement (bordered maps, one row shift per tap; held
    against F.conv2d autograd in tests/test_conv_edges_cpu.py), with the level-3 bound of each.  unflipped: the MUTANT whose input
    gradient uses W[co, ci, ky, kx] in place of W[co, ci, 2 - ky, 2 - kx]."""
    nimg, Cin, H, W = x.shape
    Cout = w.shape[0]
    sx, sw, sg = scale_ref(x)[0], scale_ref(w)[0], scale_ref(gy)[0]
    x64, w64, g64 = x.double(), w.double(), gy.double()
    xb, gb = bordered(dense_rows(x64), nimg, H, W), bordered(dense_rows(g64), nimg, H, W)
    dxb, dgb = bordered(rep_err(dense_rows(x64), sx), nimg, H, W), bordered(rep_err(dense_rows(g64), sg), nimg, H, W)
    cx, dcx = im2col(xb, nimg, H, W), im2col(dxb, nimg, H, W)
    # forward: [M, 9 Cin] x [9 Cin, Cout]
    wf = tap_major(w64).t()
    y = cx @ wf
    by = product_bound(cx, dcx, wf, rep_err(wf, sw), 3 * 9 * Cin + 3)
    # input gradient: the same conv of gY with W'[ci, co, ky, kx] = W[co, ci, 2 - ky, 2 - kx]
    wt = (w64 if unflipped else w64.flip(2, 3)).transpose(0, 1)
    wb = tap_major(wt).t()
    cg, dcg = im2col(gb, nimg, H, W), im2col(dgb, nimg, H, W)
    Cp = (Cout + 31) // 32 * 32
    gx = cg @ wb
    bgx = product_bound(cg, dcg, wb, rep_err(wb, sw), 3 * 9 * Cp + 3)
    # weight gradient: gY^T [Cout, M] x im2col(X) [M, 9 Cin]; border rows of gY are zero: the pixels are all the terms
    gr = dense_rows(g64).t()
    dw = gr @ cx
    bdw = product_bound(gr, rep_err(gr, sg), cx, dcx, wgrad_terms(Cout, Cin, nimg, H, W))
    to_nchw = lambda r, C: r.reshape(nimg, H, W, C).permute(0, 3, 1, 2)   # noqa: E731
    to_w = lambda r: r.reshape(Cout, 3, 3, Cin).permute(0, 3, 1, 2)       # noqa: E731
    return dict(y=(to_nchw(y, Cout), to_nchw(by, Cout)), gx=(to_nchw(gx, Cin), to_nchw(bgx, Cin)), dw=(to_w(dw), to_w(bdw)))
