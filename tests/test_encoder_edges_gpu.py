"""-m gpu: the encoder's GEMM family and attention kernels, ELEMENT by element against fp64 on the same rounded operands, at the
smallest shapes where a ragged tile, a schedule threshold or an epilogue store can go wrong -- and every output inside guard
rows (tests/helpers/guarded.py), so that a store past M, past N or into a pad row is seen.

Every tolerance below is one of: an a-priori rounding bound (u = 2^-24, gamma(n) = n u / (1 - n u): a length-n fp32 sum or dot
product in ANY order is within gamma(n) * sum |terms| of the exact one), a number the suite already asserts
(test_flash_attention's 6e-2 / 8e-3), or E_ACT (measured, below)."""
import math

import pytest
import torch

from tests.helpers.guarded import bits, guarded, pad_mask, sentinel_bits, vt_perm

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
U_OUT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
# below the smallest normal a 16-bit store rounds on the subnormal grid: half its spacing, absolute.  It matters for fp16 only (2^-25
# = 3e-8: the lo plane of any |x| < 2^-3 is subnormal); every 16-bit bound carries it.
UNDERFLOW = {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25}
LN2 = 0.6931471805599453
GELU_LIP = 1.13          # sup |gelu'| = 1.1290
# Pointwise error of the kernels' gelu_erf4 against fp64 erf-GELU: E_ACT is 2 x the maximum measured on the device by
# test_gelu_pointwise_error, which re-measures it on every run (the kernel is deterministic; the 16-bit operand types are swept
# exhaustively, the factor covers the fp32 grid).
E_ACT_MEASURED = 2.94e-7   # measured on an MI355X: bf16 2.490e-7 (x = 4.03125), fp16 2.773e-7 (x = 4.00390625), fp32 2.937e-7 (x = 4.00291)
E_ACT = 2 * E_ACT_MEASURED
E_ACT_FINDING = 4e-7     # a larger measured error is a finding about the kernel, not a reason for a wider tolerance

WORST = {}               # (entry, dtype) -> largest |error| / bound seen in this process


def gam(n):
    return n * U / (1 - n * U)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def g(seed):
    return torch.Generator().manual_seed(seed)


@pytest.fixture(autouse=True)
def _auto_tile():
    yield
    if torch.cuda.is_available():
        from mickey_amd import ops
        ops.gemm_set_tile(0)
        ops.gemm_set_tile(400)   # tile order back to automatic
        ops.gemm_set_tile(602)   # persistent tile loop: the default (producers only)
        ops.attn_set_mode(0)


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    for (entry, dt), r in sorted(WORST.items()):
        print("edges worst |err| / bound: %-28s %-9s %.3f" % (entry, dt, r))


def _name(dtype):
    return str(dtype).replace("torch.", "")


# (schedule, persistent loop): the forced tile forms, and the ping-pong kernel once more with the persistent loop wherever it
# applies (more workgroups than tiles at these sizes); fp32 operands have one schedule
def _schedules(dtype):
    return [(0, 602)] if dtype == torch.float32 else [(0, 602), (1, 602), (2, 602), (7, 602), (7, 600)]


def _set(ops, sched):
    ops.gemm_set_tile(sched[0])
    ops.gemm_set_tile(sched[1])


def _poisoned(t, dev, extra_cols=8, extra_rows=4):
    """Device copy of the 2-D operand t as a view into a NaN buffer with `extra_cols` more columns per row and `extra_rows` more
    rows: whatever a kernel reads past K or past M shows in its outputs."""
    r, c = t.shape
    buf = torch.full((r + extra_rows, c + extra_cols), float("nan"), dtype=t.dtype, device=dev)
    buf[:r, :c] = t.to(dev)
    return buf[:r, :c]


def _rows(v):
    """[rows, ld] view of the same rows (ops.gemm takes the leading dimension from the shape)."""
    return torch.as_strided(v, (v.shape[0], v.stride(0)), (v.stride(0), 1), v.storage_offset())


def _written(t):
    """every element of a guarded window was overwritten"""
    return not bool((bits(t) == sentinel_bits(t.dtype)).any())


def _untouched(t):
    return bool((bits(t) == sentinel_bits(t.dtype)).all())


def _within(entry, dtype, got, ref, bound, what=""):
    """|got - ref| <= bound element-wise (fp64 CPU tensors); on failure the worst ratio, where it is, and where in a tile."""
    got, ref, bound = got.double().cpu(), ref.double(), bound.double()
    if got.dim() == 1:
        got, ref, bound = got[:, None], ref[:, None], bound[:, None]
    got, ref, bound = got.reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1]), bound.reshape(-1, bound.shape[-1])
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    finite = torch.isfinite(got)
    err = (got - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    ratio = torch.where(finite, ratio, torch.full_like(ratio, float("inf")))
    worst = float(ratio.max())
    key = (entry, _name(dtype))
    WORST[key] = max(WORST.get(key, 0.0), worst)
    if not worst <= 1.0:
        i = int(ratio.argmax())
        r, c = i // got.shape[1], i % got.shape[1]
        raise AssertionError("%s %s %s: |err| / bound = %.3g at (row %d, column %d) = tile position (%d, %d): got %r, fp64 %r, bound %.3g; "
                             "%d of %d elements outside" % (entry, _name(dtype), what, worst, r, c, r % 256, c % 256, float(got[r, c]),
                                                           float(ref[r, c]), float(bound[r, c]), int((ratio > 1).sum()), ratio.numel()))


def _b16(e, ref, dtype):
    """16-bit output: a round-to-nearest of something within e of ref"""
    return (e + U_OUT[dtype] * (ref.abs() + e)) * 1.01 + UNDERFLOW[dtype]


def _gelu64(x):
    return 0.5 * x * torch.special.erfc(-x / math.sqrt(2.0))


# ---- shapes: nothing workload-sized.  N = 192 is ragged for the 128- and the 256-wide tile; M walks over 1, the automatic
# schedule's M > 64 switch and every tile height +- 1; K = 64 is the ping-pong kernel's fallback (K < 2 BK) ----
MS = [1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513]
SHAPES = [(M, 192, 128) for M in MS] + [(257, N, 128) for N in (64, 128, 256, 320)] + [(257, 192, K) for K in (64, 192)]
SHAPES_F32 = [(M, 192, 128) for M in MS] + [(257, N, 128) for N in (64, 128, 256, 320)] + [(257, 192, K) for K in (32, 96)]   # K step 32
LP = [torch.bfloat16, torch.float16]


def _cases(extra=()):
    """(dtype, M, N, K): the 16-bit shapes for both 16-bit types, the fp32 kernel's for fp32; `extra`: further (M, N, K) for all three"""
    return [(dt,) + s_ for dt in LP for s_ in SHAPES + list(extra)] + [(torch.float32,) + s_ for s_ in SHAPES_F32 + list(extra)]


def _operands(M, N, K, dtype):
    a = (torch.randn((M, K), generator=g(1000 + M)) * 0.5).to(dtype)
    w = (torch.randn((N, K), generator=g(2000 + N + K)) / math.sqrt(K)).to(dtype)
    bias = torch.randn((N,), generator=g(3000 + N))
    return a, w, bias


# ---- gelu_erf4 on the device ------------------------------------------------------------------------------------------------
def _gelu_sweep(dtype):
    """Operand values for the GELU measurement: 16-bit types -- EVERY representable value of magnitude <= 8 (signed zeros, subnormals
    and the smallest normals included); fp32 -- 2^18 evenly spaced values plus the signed zeros, the smallest normal magnitudes of
    all three operand types and the fp32 neighbourhood of the +-6 clamp."""
    if dtype != torch.float32:
        pat = torch.arange(0, 0x8000, dtype=torch.int32)
        v = torch.cat([pat, pat - 0x8000]).to(torch.int16).view(dtype)   # pat - 0x8000: the same patterns with the sign bit set
        v = v[torch.isfinite(v.float()) & (v.float().abs() <= 8.0)]
    else:
        six = torch.tensor(6.0)
        near = [six]
        for _ in range(8):
            near.append(torch.nextafter(near[-1], torch.tensor(7.0)))
        lo = six
        for _ in range(8):
            lo = torch.nextafter(lo, torch.tensor(5.0))
            near.append(lo)
        near = torch.stack(near)
        tiny = torch.tensor([0.0, 2.0 ** -126, 2.0 ** -14, 2.0 ** -125, 2.0 ** -13])
        v = torch.cat([torch.linspace(-8.0, 8.0, 2 ** 18), near, -near, tiny, -tiny])
    n = (v.numel() + 255) // 256 * 256
    return torch.cat([v, torch.zeros(n - v.numel(), dtype=dtype)])


def test_gelu_pointwise_error():
    """E_act: ops.gemm(identity block, w, no bias, GELU, fp32 out) returns gelu(w) of every w exactly as the epilogue computes it
    (products with 1 and 0, fp32 sums of one non-zero term).  Measured against fp64 erf-GELU; mk_common.hpp claims 9.8e-8."""
    from mickey_amd import ops
    dev = _dev()
    worst = 0.0
    for dtype in (torch.bfloat16, torch.float16, torch.float32):
        v = _gelu_sweep(dtype)
        w = v.reshape(-1, 64)                                   # [N, 64]: out[i, n] = w[n, i]
        eye = torch.eye(64, dtype=dtype)
        wd = _poisoned(w, dev)
        out, check = guarded(64, w.shape[0], torch.float32, dev, ld=w.shape[0] + 8)
        ops.gemm(_rows(_poisoned(eye, dev)), _rows(wd), None, act=ops.ACT_GELU, out=out, lda=72, K=64)
        check()
        assert _written(out)
        got = out.cpu().double().t()
        ident, _ = guarded(64, w.shape[0], torch.float32, dev, ld=w.shape[0] + 8)
        ops.gemm(_rows(_poisoned(eye, dev)), _rows(wd), None, act=ops.ACT_NONE, out=ident, lda=72, K=64)
        assert torch.equal(ident.cpu().t(), w.float()), "the identity block must hand w through bit for bit"
        err = (got - _gelu64(w.double())).abs()
        assert bool(torch.isfinite(got).all())
        e = float(err.max())
        i = int(err.argmax())
        print("gelu_erf4 %s: max |err| vs fp64 erf-GELU %.4g at x = %r over %d values" % (_name(dtype), e, float(w.reshape(-1)[i]), w.numel()))
        worst = max(worst, e)
    print("gelu_erf4: measured E_act = %.4g (constant in this file: %.4g measured, E_ACT = %.4g)" % (worst, E_ACT_MEASURED, E_ACT))
    assert worst <= E_ACT_FINDING, worst
    assert worst <= E_ACT_MEASURED * 1.0001, "E_ACT_MEASURED is stale: %.6g measured" % worst


# ---- mk_gemm ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,M,N,K", _cases(extra=[(257, 132, 128)]))   # N = 132: N % 4 == 0 is all mk_gemm asks
def test_gemm_elementwise(M, N, K, dtype):
    """ops.gemm, act none / relu / gelu, fp32 and 16-bit output, with and without bias, every schedule."""
    from mickey_amd import ops
    dev = _dev()
    a, w, bias = _operands(M, N, K, dtype)
    ad, wd, bd = _rows(_poisoned(a, dev)), _rows(_poisoned(w, dev)), bias.to(dev)
    G = a.double() @ w.double().t()
    absG = a.double().abs() @ w.double().abs().t()
    for has_bias in (True, False):
        pre = G + bias.double() if has_bias else G
        acc = gam(K + 2) * (absG + bias.double().abs() if has_bias else absG)
        acts = ((ops.ACT_NONE, "none"), (ops.ACT_RELU, "relu"), (ops.ACT_GELU, "gelu")) if has_bias else ((ops.ACT_NONE, "none"),)
        for act, aname in acts:
            ref = pre if act == ops.ACT_NONE else (pre.clamp_min(0.0) if act == ops.ACT_RELU else _gelu64(pre))
            e = GELU_LIP * acc + E_ACT if act == ops.ACT_GELU else acc
            for sched in _schedules(dtype):
                _set(ops, sched)
                for odt in ((torch.float32,) if dtype == torch.float32 else (torch.float32, dtype)):
                    out, check = guarded(M, N, odt, dev, ld=N + 8)
                    ops.gemm(ad, wd, bd if has_bias else None, act=act, out=out, lda=K + 8, K=K)
                    check()
                    what = "%s bias=%d out=%s sched=%s M=%d N=%d K=%d" % (aname, has_bias, _name(odt), sched, M, N, K)
                    assert _written(out), what
                    bound = e + 2 * U * ref.abs() if odt == torch.float32 else _b16(e, ref, dtype)
                    _within("gemm->" + ("f32" if odt == torch.float32 else "lp"), dtype, out, ref, bound, what)


# ---- mk_gemm_ls_residual ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,M,N,K", _cases())
def test_gemm_ls_residual_elementwise(M, N, K, dtype):
    """x += gamma * (a @ w^T + bias) in place on a guarded fp32 x with ldx = N + 8."""
    from mickey_amd import ops
    dev = _dev()
    a, w, bias = _operands(M, N, K, dtype)
    gm = torch.randn((N,), generator=g(4)) * 0.7
    x0 = torch.randn((M, N), generator=g(5)) * 2 + 0.7
    ad, wd = _poisoned(a, dev), _poisoned(w, dev)
    pre = a.double() @ w.double().t() + bias.double()
    acc = gam(K + 2) * (a.double().abs() @ w.double().abs().t() + bias.double().abs())
    ref = x0.double() + gm.double() * pre
    bound = gm.double().abs() * acc + 2 * U * ref.abs() + 2 * U * x0.double().abs()
    for sched in _schedules(dtype):
        _set(ops, sched)
        x, check = guarded(M, N, torch.float32, dev, ld=N + 8, fill=x0)
        ops.gemm_ls_residual(ad, wd, bias.to(dev), gm.to(dev), x)
        check()
        _within("gemm_ls_residual", dtype, x, ref, bound, "sched=%s M=%d N=%d K=%d" % (sched, M, N, K))


# ---- the folded LayerNorm: consumers -------------------------------------------------------------------------------------------
def _slot_sums(x64):
    M, N = x64.shape
    xs = x64.reshape(M, N // 64, 64)
    return xs.sum(-1), (xs * xs).sum(-1), xs.abs().sum(-1)


def _ln_inputs(M, K, N, dtype, seed=0):
    """Rows of a spread of scales with a mean of the order of their spread, the hi plane, fp32 per-slot statistics of the fp32
    rows (what a producer leaves), folded weights, their fp32 column sums and a bias."""
    x = torch.randn((M, K), generator=g(11 + seed)) * (0.5 + 2 * torch.rand((M, 1), generator=g(12 + seed))) + 0.8 * torch.randn((M, 1), generator=g(13 + seed))
    s, q, _ = _slot_sums(x.double())
    stats = torch.stack([s, q], -1).float()
    w = (torch.randn((N, K), generator=g(2000 + N + K)) / math.sqrt(K)).to(dtype)
    colsum = w.float().sum(1)
    bias = torch.randn((N,), generator=g(3000 + N)) * 0.3
    return x.to(dtype), stats, w, colsum, bias


def _ln_reference(a, stats, w, colsum, bias, eps):
    """y = rstd (a @ w^T) - rstd mean colsum + bias in fp64 from the operands AS PASSED (16-bit a and w, fp32 statistics, colsum and
    bias), and an a-priori bound on what the kernel's fp32 evaluation of it may differ by.  With ns = K / 64 slots, S1 / S2 the
    fp64 sums of the slot sums / sums of squares, A1 = sum |slot sums| / K:
      the fp32 slot totals:        |ds| <= gamma(ns) K A1,   |dq| <= gamma(ns) S2
      mean = s / K:                |dmean| <= gamma(ns) A1 + u |mean|  (its fp32 rounding)            =: mu
      var = q / K - mean^2 (fp64): |dvar| <= gamma(ns) (S2 / K + 2 |mean| A1)
      rstd = 1 / sqrt(var + eps):  relative error <= dvar / (2 (var + eps)) + 8u  (rounding var, the sum, sqrt, reciprocal: <= 2u each)  =: rho
      acc = a @ w^T in fp32:       |dacc| <= gamma(K) |a| @ |w|^T
      v = acc * rstd + (colsum * (-mean rstd) + bias): three more roundings of partial results, <= 3u (|rstd G| + |rstd mean colsum| + |bias|)
    -> e = rstd gamma(K + 2) |a||w|^T + (rho + 3u) rstd |G| + rstd |colsum| (mu + |mean| (rho + 3u)) + 3u |bias|, x 1.01 for the second-order terms.
    Also returns the fp64 mean and the bound of shift_out: gamma(K / 64 + 2) sum |slot sums| / K."""
    M, K = a.shape
    ns = K // 64
    st = stats.double()
    S1, S2, A1 = st[..., 0].sum(1), st[..., 1].sum(1), st[..., 0].abs().sum(1) / K
    mean = S1 / K
    var = (S2 / K - mean * mean).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + eps)
    G = a.double() @ w.double().t()
    absG = a.double().abs() @ w.double().abs().t()
    cs, b = colsum.double(), bias.double()
    y = rstd[:, None] * G - (rstd * mean)[:, None] * cs + b
    mu = gam(ns) * A1 + U * mean.abs()
    rho = gam(ns) * (S2 / K + 2 * mean.abs() * A1) / (2 * (var + eps)) + 8 * U
    e = (rstd[:, None] * gam(K + 2) * absG + ((rho + 3 * U) * rstd)[:, None] * G.abs()
         + rstd[:, None] * cs.abs() * (mu + mean.abs() * (rho + 3 * U))[:, None] + 3 * U * b.abs()) * 1.01
    return y, e, mean, gam(ns + 2) * A1


LN_SHAPES = [(M, 192, 128) for M in MS] + [(257, N, 128) for N in (64, 128, 256, 320)] + [(257, 192, K) for K in (64, 192)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("M,N,K", LN_SHAPES)
def test_gemm_ln_elementwise(M, N, K, dtype):
    """ops.gemm_ln (act none / gelu, with shift_out): lda == K is required, so only the rows past M are poisoned."""
    from mickey_amd import ops
    dev = _dev()
    eps = 1e-6
    a, stats, w, colsum, bias = _ln_inputs(M, K, N, dtype)
    y, e, mean, eshift = _ln_reference(a, stats, w, colsum, bias, eps)
    ad, wd = _poisoned(a, dev, extra_cols=0), _poisoned(w, dev)
    sd = _poisoned(stats.reshape(M, -1), dev, extra_cols=0).reshape(M, K // 64, 2)
    for act, aname in ((ops.ACT_NONE, "none"), (ops.ACT_GELU, "gelu")):
        ref = _gelu64(y) if act == ops.ACT_GELU else y
        ee = GELU_LIP * e + E_ACT if act == ops.ACT_GELU else e
        for sched in _schedules(dtype):
            _set(ops, sched)
            out, check = guarded(M, N, dtype, dev, ld=N + 8)
            sh, sh_check = guarded(1, M, torch.float32, dev)
            ops.gemm_ln(ad, wd, bias.to(dev), colsum.to(dev), sd, eps, act=act, out=out, shift_out=sh[0])
            check()
            sh_check()
            what = "%s sched=%s M=%d N=%d K=%d" % (aname, sched, M, N, K)
            assert _written(out) and _written(sh), what
            _within("gemm_ln", dtype, out, ref, _b16(ee, ref, dtype), what)
            _within("gemm_ln shift_out", dtype, sh[0], mean, eshift, what)


def _qkv_check(ops, entry, dtype, what, q, k, vt, checks, ref, e, nimg, ntok, pad, heads):
    """q / k / vt against the [M, 3D] fp64 reference with bound e; pad rows of q and k and pad columns of vt bit-untouched."""
    D = heads * 64
    for c in checks:
        c()
    qs = (64.0 ** -0.5) * ops.LOG2E
    r = ref.reshape(nimg, ntok, 3, heads, 64).permute(2, 0, 3, 1, 4)     # [3, nimg, heads, ntok, 64]
    eb = e.reshape(nimg, ntok, 3, heads, 64).permute(2, 0, 3, 1, 4)
    q4, k4, vt4 = q.reshape(nimg, heads, pad, 64), k.reshape(nimg, heads, pad, 64), vt.reshape(nimg, heads, 64, pad)
    eq = qs * eb[0] + 2 * U * (qs * r[0]).abs()                           # one more fp32 multiply
    _within(entry + " q", dtype, q4[:, :, :ntok], qs * r[0], _b16(eq, qs * r[0], dtype), what)
    _within(entry + " k", dtype, k4[:, :, :ntok], r[1], _b16(eb[1], r[1], dtype), what)
    cols = torch.tensor([vt_perm(t) for t in range(ntok)])
    _within(entry + " vt", dtype, vt4.cpu()[:, :, :, cols], r[2].transpose(-1, -2), _b16(eb[2].transpose(-1, -2), r[2].transpose(-1, -2), dtype), what)
    if pad > ntok:
        padc = torch.tensor(sorted(pad_mask(ntok, pad)))
        assert _untouched(q4[:, :, ntok:]), what + ": q pad rows written"
        assert _untouched(k4[:, :, ntok:]), what + ": k pad rows written"
        assert _untouched(vt4.cpu()[:, :, :, padc]), what + ": vt pad columns written"
    # ... and everything else was written
    assert _written(q4[:, :, :ntok]) and _written(k4[:, :, :ntok]) and _written(vt4.cpu()[:, :, :, cols]), what


def _qkv_buffers(dtype, dev, nimg, heads, pad):
    """q / k / vt with front and back guards, everything (pad rows and columns too) holding the sentinel"""
    q, cq = guarded(nimg * heads * pad, 64, dtype, dev)
    k, ck = guarded(nimg * heads * pad, 64, dtype, dev)
    vt, cv = guarded(nimg * heads * 64, pad, dtype, dev)
    return q, k, vt, (cq, ck, cv)


QKV_TOK = [(1, 64), (63, 64), (64, 64), (65, 128), (65, 192), (333, 384)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("nimg", [1, 2])
def test_gemm_qkv_elementwise(nimg, heads, dtype):
    """ops.gemm_qkv and ops.gemm_qkv_ln: K = D = 64 heads (heads = 1: K < 2 BK, the ping-pong launcher's fallback)."""
    from mickey_amd import ops
    dev = _dev()
    D, eps = 64 * heads, 1e-6
    for ntok, pad in QKV_TOK:
        M = nimg * ntok
        # plain
        a, w, bias = _operands(M, 3 * D, D, dtype)
        ad, wd = _poisoned(a, dev), _poisoned(w, dev)
        ref = a.double() @ w.double().t() + bias.double()
        e = gam(D + 2) * (a.double().abs() @ w.double().abs().t() + bias.double().abs())
        # folded LayerNorm
        a2, stats, w2, colsum, bias2 = _ln_inputs(M, D, 3 * D, dtype, seed=ntok)
        y, e2, mean, eshift = _ln_reference(a2, stats, w2, colsum, bias2, eps)
        a2d, w2d = _poisoned(a2, dev, extra_cols=0), _poisoned(w2, dev)
        sd = _poisoned(stats.reshape(M, -1), dev, extra_cols=0).reshape(M, D // 64, 2)
        for sched in _schedules(dtype):
            _set(ops, sched)
            what = "sched=%s nimg=%d heads=%d ntok=%d pad=%d" % (sched, nimg, heads, ntok, pad)
            q, k, vt, checks = _qkv_buffers(dtype, dev, nimg, heads, pad)
            ops.gemm_qkv(ad, wd, bias.to(dev), q, k, vt, nimg, ntok, pad, heads)
            _qkv_check(ops, "gemm_qkv", dtype, what, q, k, vt, checks, ref, e, nimg, ntok, pad, heads)
            q, k, vt, checks = _qkv_buffers(dtype, dev, nimg, heads, pad)
            sh, sh_check = guarded(1, M, torch.float32, dev)
            ops.gemm_qkv_ln(a2d, w2d, bias2.to(dev), colsum.to(dev), sd, eps, q, k, vt, nimg, ntok, pad, heads, shift_out=sh[0])
            sh_check()
            assert _written(sh), what
            _qkv_check(ops, "gemm_qkv_ln", dtype, what, q, k, vt, checks, y, e2, nimg, ntok, pad, heads)
            _within("gemm_qkv_ln shift_out", dtype, sh[0], mean, eshift, what)


# ---- the folded LayerNorm: producers -------------------------------------------------------------------------------------------
def _split(x, dtype):
    hi = x.to(dtype)
    return hi, (x - hi.float()).to(dtype)


def _check_planes_and_stats(entry, dtype, what, xh, xl, stats, ref, bx):
    """hi + lo (fp64) within bx + u_out^2 |ref| (+ the lo plane's underflow) of ref, hi alone a 16-bit rounding of it; per-slot statistics of the new rows:
    sum within sum(bx) + gamma(64) sum |x|, sum of squares within sum(2 |x| bx + bx^2) + gamma(65) sum x^2."""
    uo = U_OUT[dtype]
    _within(entry + " hi+lo", dtype, xh.double().cpu() + xl.double().cpu(), ref, bx + uo * uo * ref.abs() * 1.01 + UNDERFLOW[dtype], what)
    _within(entry + " hi", dtype, xh, ref, _b16(bx, ref, dtype), what)
    M, N = ref.shape
    s, q, sa = _slot_sums(ref)
    bs = bx.reshape(M, N // 64, 64)
    xa = ref.abs().reshape(M, N // 64, 64)
    st = stats.reshape(M, N // 64, 2).double().cpu()
    _within(entry + " stats sum", dtype, st[..., 0], s, bs.sum(-1) + gam(64) * sa, what)
    _within(entry + " stats sumsq", dtype, st[..., 1], q, (2 * xa * bs + bs * bs).sum(-1) + gam(65) * q, what)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("M,N,K", [s for s in SHAPES if s[1] % 64 == 0])
def test_gemm_ls_residual_ln_elementwise(M, N, K, dtype):
    """ops.gemm_ls_residual_ln: plane + statistics form and x_out form, each with and without shift."""
    from mickey_amd import ops
    dev = _dev()
    a, w, bias = _operands(M, N, K, dtype)
    gm = torch.randn((N,), generator=g(4)) * 0.7
    hi0, lo0 = _split(torch.randn((M, N), generator=g(5)) * 2 + 0.7, dtype)
    x0 = hi0.double() + lo0.double()
    shift = torch.randn((M,), generator=g(6)) * 0.3
    ad, wd = _poisoned(a, dev), _poisoned(w, dev)
    pre = a.double() @ w.double().t() + bias.double()
    acc = gam(K + 2) * (a.double().abs() @ w.double().abs().t() + bias.double().abs())
    for use_shift in (False, True):
        sh = shift.double()[:, None] if use_shift else torch.zeros((M, 1), dtype=torch.float64)
        ref = x0 + gm.double() * pre - sh
        # fp32 rows: the accumulation, the rounding of x + gamma v and of the difference with shift
        bx = gm.double().abs() * acc + 2 * U * ref.abs() + 2 * U * x0.abs() + 2 * U * sh.abs()
        shd = _poisoned(shift[:, None], dev, extra_cols=0)[:, 0] if use_shift else None
        for sched in _schedules(dtype):
            _set(ops, sched)
            what = "shift=%d sched=%s M=%d N=%d K=%d" % (use_shift, sched, M, N, K)
            # plane form
            xh, ch = guarded(M, N, dtype, dev, ld=N + 8, fill=hi0)
            xl, cl = guarded(M, N, dtype, dev, ld=N + 8, fill=lo0)
            st, cs = guarded(M, N // 64 * 2, torch.float32, dev)
            spare, cspare = guarded(M, N, torch.float32, dev, ld=N + 8)      # an x_out-sized buffer that is NOT passed
            ops.gemm_ls_residual_ln(ad, wd, bias.to(dev), gm.to(dev), xh, xl, st.view(M, N // 64, 2), shift=shd)
            for c in (ch, cl, cs, cspare):
                c()
            assert _written(st) and _untouched(spare), what
            _check_planes_and_stats("gemm_ls_residual_ln", dtype, what, xh, xl, st, ref, bx)
            # x_out form: fp32 rows out, planes and statistics left alone
            xh, ch = guarded(M, N, dtype, dev, ld=N + 8, fill=hi0)
            xl, cl = guarded(M, N, dtype, dev, ld=N + 8, fill=lo0)
            st, cs = guarded(M, N // 64 * 2, torch.float32, dev)
            xo, co = guarded(M, N, torch.float32, dev, ld=N + 8)
            ops.gemm_ls_residual_ln(ad, wd, bias.to(dev), gm.to(dev), xh, xl, st.view(M, N // 64, 2), x_out=xo, shift=shd)
            for c in (ch, cl, cs, co):
                c()
            assert _written(xo) and _untouched(st), what
            assert torch.equal(bits(xh).cpu(), bits(hi0)) and torch.equal(bits(xl).cpu(), bits(lo0)), what + ": planes written in the x_out form"
            _within("gemm_ls_residual_ln x_out", dtype, xo, ref, bx, what)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("nimg", [1, 3])
@pytest.mark.parametrize("npatch", [1, 35, 420])
def test_patch_embed_and_cls_elementwise(npatch, nimg, dtype):
    """gemm_patch_embed + cls_token (fp32 rows) and gemm_patch_embed_ln + cls_token_ln (split planes + statistics), D = 128,
    K = 640: the GEMM leaves row 0 of every image alone, the cls kernels every other row."""
    from mickey_amd import ops
    dev = _dev()
    D, K, ntok = 128, 640, npatch + 1
    M = nimg * npatch
    a, w, bias = _operands(M, D, K, dtype)
    bias = bias * 0.1
    pos = torch.randn((ntok, D), generator=g(7)) * 0.1
    cls = torch.randn((D,), generator=g(8)) * 0.1
    ad, wd = _poisoned(a, dev), _poisoned(w, dev)
    pre = (a.double() @ w.double().t() + bias.double()).reshape(nimg, npatch, D)
    acc = (gam(K + 2) * (a.double().abs() @ w.double().abs().t() + bias.double().abs())).reshape(nimg, npatch, D)
    ref = torch.empty((nimg, ntok, D), dtype=torch.float64)
    ref[:, 1:] = pre + pos.double()[1:]
    ref[:, 0] = cls.double() + pos.double()[0]
    bx = torch.empty_like(ref)
    bx[:, 1:] = acc + 2 * U * ref[:, 1:].abs()
    bx[:, 0] = 2 * U * ref[:, 0].abs()
    ref2, bx2 = ref.reshape(nimg * ntok, D), bx.reshape(nimg * ntok, D)
    for sched in _schedules(dtype):
        _set(ops, sched)
        what = "sched=%s nimg=%d npatch=%d" % (sched, nimg, npatch)
        x, cx = guarded(nimg * ntok, D, torch.float32, dev)
        x3 = x.view(nimg, ntok, D)
        ops.gemm_patch_embed(ad, wd, bias.to(dev), pos.to(dev), x3, nimg, npatch)
        cx()
        assert _untouched(x3[:, 0]) and _written(x3[:, 1:]), what + ": gemm_patch_embed and row 0"
        before = x3[:, 1:].clone()
        ops.cls_token(cls.to(dev), pos.to(dev), x3, nimg, ntok, D)
        cx()
        assert _written(x3[:, 0]) and torch.equal(bits(before), bits(x3[:, 1:])), what + ": cls_token and rows 1.."
        _within("gemm_patch_embed+cls", dtype, x, ref2, bx2, what)
        # split planes
        xh, ch = guarded(nimg * ntok, D, dtype, dev)
        xl, cl = guarded(nimg * ntok, D, dtype, dev)
        st, cs = guarded(nimg * ntok, D // 64 * 2, torch.float32, dev)
        h3, l3, s3 = xh.view(nimg, ntok, D), xl.view(nimg, ntok, D), st.view(nimg, ntok, D // 32)
        ops.gemm_patch_embed_ln(ad, wd, bias.to(dev), pos.to(dev), xh, xl, st.view(nimg * ntok, D // 64, 2), nimg, npatch)
        for c in (ch, cl, cs):
            c()
        assert _untouched(h3[:, 0]) and _untouched(l3[:, 0]) and _untouched(s3[:, 0]), what + ": gemm_patch_embed_ln and row 0"
        assert _written(h3[:, 1:]) and _written(l3[:, 1:]) and _written(s3[:, 1:]), what
        before = [t[:, 1:].clone() for t in (h3, l3, s3)]
        ops.cls_token_ln(cls.to(dev), pos.to(dev), xh, xl, st.view(nimg * ntok, D // 64, 2), nimg, ntok, D)
        for c in (ch, cl, cs):
            c()
        assert _written(h3[:, 0]) and _written(l3[:, 0]) and _written(s3[:, 0]), what
        for b_, t in zip(before, (h3, l3, s3)):
            assert torch.equal(bits(b_), bits(t[:, 1:])), what + ": cls_token_ln and rows 1.."
        _check_planes_and_stats("gemm_patch_embed_ln+cls_ln", dtype, what, xh, xl, st, ref2, bx2)


# ---- attention ------------------------------------------------------------------------------------------------------------------
ATTN_NTOK = [1, 31, 32, 33, 63, 64, 65, 96, 97, 128, 129, 255, 256, 257, 288, 289]
ATTN_EMAX = {torch.bfloat16: 6e-2, torch.float16: 8e-3}     # test_flash_attention's element-wise bounds at this input scale


def _attn_inputs(dtype, ntok, nimg, heads, pad, LOG2E):
    """q, k, vt as test_flash_attention builds them (a spiky query row and a spiky key row, indices % ntok), pad rows / columns zero."""
    qkv = torch.randn((3, nimg, heads, ntok, 64), generator=g(ntok)) * 1.5
    qkv[0, 0, 0, 5 % ntok] *= 6.0
    qkv[1, 0, 0, 130 % ntok] *= 6.0
    q16, k16, v16 = (qkv[0] * 0.125 * LOG2E).to(dtype), qkv[1].to(dtype), qkv[2].to(dtype)
    q = torch.zeros((nimg, heads, pad, 64), dtype=dtype)
    k = torch.zeros_like(q)
    vt = torch.zeros((nimg, heads, 64, pad), dtype=dtype)
    q[:, :, :ntok], k[:, :, :ntok] = q16, k16
    cols = torch.tensor([vt_perm(t) for t in range(ntok)])
    vt[:, :, :, cols] = v16.transpose(-1, -2)
    return q16, k16, v16, q, k, vt


def _garbage_pads(q, k, ntok):
    """pad rows of q and k: alternating +-1e4, the first pad row the largest finite value of the type"""
    q, k = q.clone(), k.clone()
    alt = torch.tensor([1e4, -1e4]).repeat(32)
    for t in (q, k):
        t[:, :, ntok::2] = alt.to(t.dtype)
        t[:, :, ntok + 1::2] = (-alt).to(t.dtype)
        t[:, :, ntok] = torch.finfo(t.dtype).max
    return q, k


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("ntok", ATTN_NTOK)
def test_attention_edges(ntok, dtype):
    """Every 16-bit mode and the fp32 kernel at the tile edges (first tile == peeled masked tile, the half_tile boundary at
    ntok & 63 in {32, 33}, the one-sub-block tail wave at q0 + 32 == ntok, a one-block grid): element-wise against fp64, out inside
    guards and fully overwritten, modes 1 / 2 / 6 and 4 / 5 bit-identical, and nothing in the pad rows of q and k can reach an
    output (vt's pad columns stay zero, as mickey_hip.h requires)."""
    from mickey_amd import ops
    dev = _dev()
    c64 = (ntok + 63) // 64 * 64
    modes = (0,) if dtype == torch.float32 else (1, 2, 3, 4, 5, 6)
    for nimg, heads in ((1, 1), (2, 3)):
        for pad in (c64, c64 + 64) if ntok in (33, 65, 257) else (c64,):
            q16, k16, v16, q, k, vt = _attn_inputs(dtype, ntok, nimg, heads, pad, ops.LOG2E)
            s = q16.double() @ k16.double().transpose(-1, -2)                    # log2 domain
            ref = (torch.softmax(s * LN2, -1) @ v16.double()).permute(0, 2, 1, 3).reshape(nimg * ntok, heads * 64)
            if dtype == torch.float32:
                # per column d: the score error (gamma(64) sum_d |q||k|, both ways through exp2 and the normalisation: x 2 ln 2), the
                # row sum and the weighted sum (2 gamma(ntok + 8)), exp2f and the final scale (8u); all x max_j |v_jd|
                smax = (q16.double().abs() @ k16.double().abs().transpose(-1, -2)).amax((-1, -2))          # [nimg, heads]
                vmax = v16.double().abs().amax(-2)                                                          # [nimg, heads, 64]
                b = (2 * LN2 * gam(64) * smax[..., None] + 2 * gam(ntok + 8) + 8 * U) * vmax
                bound = b[:, None].expand(nimg, ntok, heads, 64).reshape(nimg * ntok, heads * 64)
            qd, kd, vd = q.to(dev), k.to(dev), vt.to(dev)
            outs = {}
            for mode in modes:
                ops.attn_set_mode(mode)
                what = "mode=%d ntok=%d pad=%d nimg=%d heads=%d" % (mode, ntok, pad, nimg, heads)
                out, check = guarded(nimg * ntok, heads * 64, dtype, dev, ld=heads * 64 + 8)
                ops.flash_attn(qd, kd, vd, out, nimg, heads, ntok, pad)
                check()
                assert _written(out), what + ": window elements left unwritten"
                o = out.cpu().double()
                assert bool(torch.isfinite(o).all()), what
                if dtype == torch.float32:
                    _within("attention f32", dtype, out, ref, bound, what)
                else:
                    emax = float((o - ref).abs().max())
                    key = ("attention max|err|/limit", _name(dtype))
                    WORST[key] = max(WORST.get(key, 0.0), emax / ATTN_EMAX[dtype])
                    assert emax < ATTN_EMAX[dtype], (what, emax)
                outs[mode] = out.clone()
                if pad > ntok:   # pad independence: garbage in the pad rows of q and k changes no output bit
                    qg, kg = _garbage_pads(q, k, ntok)
                    out2, check2 = guarded(nimg * ntok, heads * 64, dtype, dev, ld=heads * 64 + 8)
                    ops.flash_attn(qg.to(dev), kg.to(dev), vd, out2, nimg, heads, ntok, pad)
                    check2()
                    same = bits(out2) == bits(out)
                    if not bool(same.all()):
                        bad = torch.nonzero(~same)
                        raise AssertionError("%s: %d outputs depend on the pad rows of q / k, first at (row %d, column %d), token %d"
                                             % (what, bad.shape[0], int(bad[0, 0]), int(bad[0, 1]), int(bad[0, 0]) % ntok))
            if dtype != torch.float32:
                for a_, b_ in ((1, 2), (4, 5), (6, 2)):
                    assert torch.equal(bits(outs[a_]), bits(outs[b_])), "modes %d / %d differ at ntok=%d pad=%d nimg=%d heads=%d" % (a_, b_, ntok, pad, nimg, heads)
