"""-m gpu: the training path of the heads' transformer -- the 7 kernels of mk_train_layer.hip and the training half of mk_linattn.hip
(attn_train_kv_partial, attn_train_apply, attn_train_bwd_q, attn_train_bwd_kv and linattn_kv_reduce as they drive it) -- ELEMENT by
element against fp64 at every loop edge.  The entry points are called directly with the argument marshalling of ops.py (_mat, _wsplit,
_gplanes, _attn_rows); every output -- out, xhat, rstd, o1, o2, part, kv, gkv, work, gq, gk, gv, the tail's out -- sits in a
sentinel-filled guarded window (tests/helpers/guarded.py) with ld > cols where the entry point takes a stride.  After each call the
guards are checked, every wanted element is found overwritten and every output that was not asked for is found untouched.

  level 1  operands that are integers in [-4, 4]: the three GEMM forms, the tail and the kv block must give the fp64 result bit for bit;
  level 2  |got - ref64| <= bound on every element, references and bounds of tests/helpers/train_layer_refs.py, stated before any
           kernel ran (tests/test_train_layer_edges_cpu.py shows that a correct fp32 evaluation meets them in two summation orders
           and that seventeen subtly wrong ones do not).
Measured worst ratios: profiles/train_layer_edges_parity.txt."""
import time

import pytest
import torch

from tests.helpers import train_layer_refs as R
from tests.helpers.guarded import bits, guarded, sentinel_bits

pytestmark = pytest.mark.gpu

WORST = {}       # (kernel, output) -> largest |error| / bound seen in this process
EXACT = {}       # (kernel, output) -> number of bit-exact comparisons made
RAN = [0]
SLOWEST = [0.0, ""]
EXP = []
F32 = torch.float32


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _nv():
    from mickey_amd import _native
    return _native


def _ops():
    from mickey_amd import ops
    return ops


@pytest.fixture(scope="module", autouse=True)
def _report():
    t0 = time.perf_counter()
    yield
    for (kernel, what), r in sorted(WORST.items()):
        print("train layer edges worst |err| / bound: %-22s %-8s %.3f" % (kernel, what, r))
    for (kernel, what), n in sorted(EXACT.items()):
        print("train layer edges bit-exact comparisons: %-20s %-8s %d" % (kernel, what, n))
    for line in EXP:
        print(line)
    print("train layer edges: %d tests in %.1f s, slowest %.2f s (%s)" % (RAN[0], time.perf_counter() - t0, SLOWEST[0], SLOWEST[1]))


@pytest.fixture(autouse=True)
def _count(request):
    t0 = time.perf_counter()
    yield
    RAN[0] += 1
    dt = time.perf_counter() - t0
    if dt > SLOWEST[0]:
        SLOWEST[0], SLOWEST[1] = dt, request.node.name


def _written(t):
    return not bool((bits(t) == sentinel_bits(t.dtype)).any())


def _untouched(t):
    return bool((bits(t) == sentinel_bits(t.dtype)).all())


def _exact(kernel, what, got, want64, msg, skip_rows=()):
    """got (device, fp32) holds the bits of the fp64 integers want64; names the first element that does not"""
    want = want64.float().reshape(got.shape)
    assert bool((want.double() == want64.reshape(got.shape)).all()), "the reference is not representable in fp32"
    ne = bits(got.contiguous()).cpu() != bits(want)
    for r in skip_rows:
        ne[r] = False
    EXACT[(kernel, what)] = EXACT.get((kernel, what), 0) + 1
    if bool(ne.any()):
        i = int(torch.nonzero(ne.reshape(-1))[0])
        cols = got.shape[-1]
        raise AssertionError("%s %s, %s: %d of %d elements differ, first at (row %d, column %d) = (%d, %d) of its 64 x 64 tile: got %r, "
                             "fp64 %r" % (kernel, what, msg, int(ne.sum()), ne.numel(), i // cols, i % cols, (i // cols) % 64,
                                          (i % cols) % 64, float(got.reshape(-1)[i]), float(want64.reshape(-1)[i])))


def _within(kernel, what, got, ref, bound, msg):
    got = got.detach().double().cpu().reshape(ref.shape)
    worst, i = R.ratio(got, ref, bound)
    WORST[(kernel, what)] = max(WORST.get((kernel, what), 0.0), worst)
    if not worst <= 1.0:
        e = (got - ref).abs().reshape(-1)
        outside = int((e > bound.reshape(-1)).sum() + (~torch.isfinite(got)).sum())
        cols = ref.shape[-1]
        raise AssertionError("%s %s, %s: |err| / bound = %.3g at (row %d, column %d) = (%d, %d) of its 64 x 64 tile: got %r, fp64 %r, "
                             "bound %.3g; %d of %d elements outside" % (kernel, what, msg, worst, i // cols, i % cols, (i // cols) % 64,
                                                                        (i % cols) % 64, float(got.reshape(-1)[i]), float(ref.reshape(-1)[i]),
                                                                        float(bound.reshape(-1)[i]), outside, e.numel()))


def _check(kind, kernel, what, got, ref, bound, msg):
    if kind == "int":
        _exact(kernel, what, got, ref, msg)
    else:
        _within(kernel, what, got, ref, bound, msg)


def _strided(t, pad, dev):
    """t on the device as a [rows, cols] view of a [rows, cols + pad] buffer whose slack holds NaN: a read past a row shows"""
    if t is None:
        return None
    buf = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), device=dev, dtype=F32)
    buf[:, :t.shape[1]] = t.to(dev)
    return buf[:, :t.shape[1]]


def _w(w, dev):
    wd = [x.to(dev).contiguous() for x in w]
    return _ops()._wsplit(tuple(wd) if len(wd) == 3 else wd[0]) + (wd,)


def _grad_arg(G, gs, dev, pad=4):
    """the gradient as _gplanes wants it: [M, N] rows of stride N + pad, or 3 planes [M, gs] of row stride gs + pad that lie
    (M + 2) rows apart: gplane > M ldg.  -> (pointer, ldg, gplane, gsplit, M, N, the buffer that owns the memory)"""
    if not gs:
        gd = _strided(G, pad, dev)
        return _ops()._gplanes(gd) + (gd,)
    M = G.shape[0]
    buf = torch.full((3, M + 2, gs + pad), float("nan"), device=dev, dtype=F32)
    g3 = buf[:, :M, :gs]
    g3.copy_(G.to(dev).reshape(M, 3, gs).permute(1, 0, 2))
    args = _ops()._gplanes(g3)
    assert args[2] == (M + 2) * (gs + pad) > M * args[1] or M == 1
    return args + (buf,)


def _sync():
    torch.cuda.synchronize()


# ================================================================ mk_train_linear_fwd ===========================================
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("case", R.FWD_CASES, ids=str)
def test_linear_fwd(case, kind):
    dev, nv, ops = _dev(), _nv(), _ops()
    M, N, K1, K2, ws = case
    a1, a2, w = R.fwd_inputs(case, kind)
    pw, pw2, pw3, wsp, keep = _w(w, dev)
    assert wsp == ws
    for relu, pad in ((0, 0), (1, 4), (0, 4), (1, 0)):
        d1, d2 = _strided(a1, pad, dev), _strided(a2, 2 * pad, dev)
        out, chk = guarded(M, N, F32, dev, ld=N + pad)
        nv.call("mk_train_linear_fwd", *ops._mat(d1), K1, *ops._mat(d2), K2, pw, pw2, pw3, wsp, *ops._mat(out), M, N, relu, nv.stream())
        _sync()
        chk()
        msg = "%r relu %d pad %d" % (case, relu, pad)
        assert _written(out), "mk_train_linear_fwd left an element of out unwritten, " + msg
        _check(kind, "linear_fwd", "out", out, *R.fwd_ref(a1, a2, w, relu), msg)


def test_linear_fwd_relu_keeps_a_nan_and_gives_exact_zeros():
    dev, nv, ops = _dev(), _nv(), _ops()
    case = (65, 68, 32, 0, 0)
    a1, _, w = R.fwd_inputs(case, "int")
    a1 = a1.clone()
    a1[63, 5] = float("nan")
    pw, pw2, pw3, wsp, keep = _w(w, dev)
    d1 = _strided(a1, 4, dev)
    out, chk = guarded(65, 68, F32, dev, ld=72)
    nv.call("mk_train_linear_fwd", *ops._mat(d1), 32, None, 0, 0, pw, pw2, pw3, wsp, *ops._mat(out), 65, 68, 1, nv.stream())
    _sync()
    chk()
    ref, _ = R.fwd_ref(a1, None, w, 1)
    assert bool(torch.isnan(ref[63]).all()) and not bool(torch.isnan(ref[:63]).any()) and bool((ref[:63] == 0).any())
    assert bool(torch.isnan(out[63]).all()), "a NaN row did not stay NaN through the ReLU"
    ref[63] = 0
    _exact("linear_fwd", "out", out, ref, "a NaN in row 63", skip_rows=(63,))


# ================================================================ mk_train_linear_dgrad =========================================
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("case", R.DGRAD_CASES, ids=str)
def test_linear_dgrad(case, kind):
    dev, nv, ops = _dev(), _nv(), _ops()
    M, N, K1, K2, acc, mp, gs, ws = case
    G, w, old, mask = R.dgrad_inputs(case, kind)
    pg, ldg, gplane, gsplit, gm, gn, keep_g = _grad_arg(G, gs, dev)
    assert (gm, gn, gsplit) == (M, N, gs)
    pw, pw2, pw3, wsp, keep_w = _w(w, dev)
    md = _strided(mask, mp or 0, dev)
    o1, c1 = guarded(M, K1, F32, dev, ld=K1 + 4, fill=old[:, :K1].to(dev) if acc & 1 else None)
    o2, c2 = guarded(M, K2, F32, dev, ld=K2 + 8, fill=old[:, K1:].to(dev) if acc & 2 else None) if K2 else (None, lambda: None)
    nv.call("mk_train_linear_dgrad", pg, ldg, gplane, gsplit, pw, pw2, pw3, wsp, *ops._mat(md), *ops._mat(o1), K1, *ops._mat(o2), K2, acc,
            M, N, nv.stream())
    _sync()
    c1()
    c2()
    msg = repr(case)
    ref, bound = R.dgrad_ref(case, G, w, old, mask)
    assert _written(o1) and (o2 is None or _written(o2)), "mk_train_linear_dgrad left an element unwritten, " + msg
    _check(kind, "linear_dgrad", "o1", o1, ref[:, :K1], bound[:, :K1], msg)
    if K2:
        _check(kind, "linear_dgrad", "o2", o2, ref[:, K1:], bound[:, K1:], msg)
    if mask is not None:      # the header's promise: an exact (+)0 where mask <= 0 (and nothing accumulated), the gradient at a NaN
        zero = (mask <= 0) & ~R.dgrad_masks(case, mask)[1]
        got = torch.cat([o1, o2], 1).cpu() if K2 else o1.cpu()
        assert bool((bits(got)[zero] == 0).all()), "a masked element is not an exact +0.0, " + msg


# ================================================================ mk_train_linear_wgrad + mk_train_tail =========================
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("case", R.WGRAD_CASES, ids=str)
def test_linear_wgrad(case, kind):
    dev, nv, ops = _dev(), _nv(), _ops()
    M, N, K1, K2, rpc_arg, gs = case
    rpc, chunks = R.wgrad_plan(case)
    if not rpc_arg:
        assert ops.train_chunks(M) == (rpc, chunks)
    G, a1, a2 = R.wgrad_inputs(case, kind)
    nk = N * (K1 + K2)
    pg, ldg, gplane, gsplit, gm, gn, keep_g = _grad_arg(G, gs, dev)
    d1, d2 = _strided(a1, 4, dev), _strided(a2, 8, dev)
    for surplus, spad in R.WGRAD_VARIANTS:
        tot = chunks + surplus
        part, chk = guarded(tot, nk, F32, dev, ld=nk + spad)      # the gap between two chunks is row slack: it keeps the sentinel
        nv.call("mk_train_linear_wgrad", pg, ldg, gplane, gsplit, *ops._mat(d1), K1, *ops._mat(d2), K2, nv.ptr(part), nk + spad, rpc, tot,
                M, N, nv.stream())
        out, chk2 = guarded(1, nk, F32, dev)
        nv.call("mk_train_tail", nv.ptr(part), nk + spad, tot, nk, None, 0, 0, 0, nv.ptr(out), nv.stream())
        _sync()
        chk()
        chk2()
        msg = "%r, %d chunks of %d rows + %d, stride N K + %d" % (case, chunks, rpc, surplus, spad)
        assert _written(part) and _written(out), "a chunk or a gradient element was left unwritten, " + msg
        pref, pbound, dw, dbound = R.wgrad_ref(case, G, a1, a2, surplus)
        if surplus:
            assert bool((bits(part[chunks:]) == 0).all()), "a surplus chunk does not hold zeros, " + msg
        _check(kind, "linear_wgrad", "part", part, pref, pbound, msg)
        _check(kind, "wgrad + tail", "dw", out, dw[None], dbound[None], msg)


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("case", R.TAIL_CASES, ids=str)
def test_tail(case, kind):
    dev, nv = _dev(), _nv()
    nw, nl, wc, ls, pad = case
    wpart, lpart = R.tail_inputs(case, kind)
    wd, ld_ = _strided(wpart, pad, dev), _strided(lpart, pad, dev)
    out, chk = guarded(1, nw + nl, F32, dev)
    nv.call("mk_train_tail", nv.ptr(wd), nw + pad if nw else 0, wc if nw else 0, nw, nv.ptr(ld_), nl + pad if nl else 0, ls if nl else 0, nl,
            nv.ptr(out), nv.stream())
    _sync()
    chk()
    assert _written(out), "mk_train_tail left an element unwritten, %r" % (case,)
    ref, bound = R.tail_ref(wpart, lpart)
    _check(kind, "tail", "out", out, ref[None], bound[None], repr(case))


# ================================================================ LayerNorm(128) forward ==========================================
def _ln_outputs(nv, dev, M, saved):
    out, c0 = guarded(M, 128, F32, dev)
    xhat, c1 = guarded(M, 128, F32, dev)
    rstd, c2 = guarded(1, M, F32, dev)
    return out, xhat, rstd, (c0, c1, c2), (nv.ptr(xhat) if saved[0] else None, nv.ptr(rstd) if saved[1] else None)


def _ln_check(kernel, refs, out, xhat, rstd, checks, saved, msg):
    for c in checks:
        c()
    assert _written(out), "%s left an element of out unwritten, %s" % (kernel, msg)
    _within(kernel, "out", out, *refs["out"], msg)
    for name, t, want in (("xhat", xhat, saved[0]), ("rstd", rstd, saved[1])):
        if want:
            assert _written(t), "%s left an element of %s unwritten, %s" % (kernel, name, msg)
            _within(kernel, name, t.reshape(refs[name][0].shape), *refs[name], msg)
        else:
            assert _untouched(t), "%s wrote %s although it was not asked for, %s" % (kernel, name, msg)


@pytest.mark.parametrize("ldr", R.LN_RESID)
@pytest.mark.parametrize("M", R.LN_FWD_M)
def test_ln128_fwd(M, ldr):
    dev, nv, ops = _dev(), _nv(), _ops()
    u, gamma, beta, resid = R.ln_fwd_inputs(M)
    rs = None if ldr is None else resid
    refs = R.ln_fwd_ref(u.double(), 0.0, gamma, beta, rs)
    ud, gd, bd = u.to(dev), gamma.to(dev), beta.to(dev)
    rd = None if ldr is None else _strided(resid, ldr - 128, dev)
    for saved in R.LN_SAVED:
        out, xhat, rstd, checks, ptrs = _ln_outputs(nv, dev, M, saved)
        nv.call("mk_train_ln128_fwd", nv.ptr(ud), nv.ptr(gd), nv.ptr(bd), R.LN_EPS, *ops._mat(rd), nv.ptr(out), *ptrs, M, nv.stream())
        _sync()
        _ln_check("ln128_fwd", refs, out, xhat, rstd, checks, saved, "M %d ldr %s saved %r" % (M, ldr, saved))


@pytest.mark.parametrize("ldr", R.LN_RESID)
@pytest.mark.parametrize("case", R.LINLN_CASES, ids=str)
def test_linear_ln128_fwd(case, ldr):
    dev, nv, ops = _dev(), _nv(), _ops()
    M, K1, K2 = case
    a1, a2, w, gamma, beta, resid = R.linln_inputs(case)
    rs = None if ldr is None else resid
    refs = R.linln_ref(a1, a2, w, gamma, beta, rs)
    d1, d2, wd, gd, bd = _strided(a1, 4, dev), _strided(a2, 8, dev), w.to(dev), gamma.to(dev), beta.to(dev)
    rd = None if ldr is None else _strided(resid, ldr - 128, dev)
    for saved in R.LN_SAVED:
        out, xhat, rstd, checks, ptrs = _ln_outputs(nv, dev, M, saved)
        nv.call("mk_train_linear_ln128_fwd", *ops._mat(d1), K1, *ops._mat(d2), K2, nv.ptr(wd), nv.ptr(gd), nv.ptr(bd), R.LN_EPS,
                *ops._mat(rd), nv.ptr(out), *ptrs, M, nv.stream())
        _sync()
        _ln_check("linear_ln128_fwd", refs, out, xhat, rstd, checks, saved, "%r ldr %s saved %r" % (case, ldr, saved))


# ================================================================ LayerNorm(128) backward =========================================
@pytest.mark.parametrize("M", R.LN_BWD_M)
def test_ln128_bwd(M):
    dev, nv, ops = _dev(), _nv(), _ops()
    g, xhat, rstd, gamma = R.ln_bwd_inputs(M)
    refs = R.ln_bwd_ref(g, xhat, rstd, gamma)
    steps = ops.train_ln_steps(M)
    assert steps == R.ln_steps(M)
    gd, xd, rd, gmd = g.to(dev), xhat.to(dev), rstd.to(dev), gamma.to(dev)
    for want_gu, want_part, stride in R.LN_BWD_VARIANTS:
        gu, c0 = guarded(M, 128, F32, dev)
        part, c1 = guarded(steps, 256, F32, dev, ld=stride)
        nv.call("mk_train_ln128_bwd", nv.ptr(gd), nv.ptr(xd), nv.ptr(rd), nv.ptr(gmd), nv.ptr(gu) if want_gu else None,
                nv.ptr(part) if want_part else None, stride, M, nv.stream())
        _sync()
        c0()
        c1()
        msg = "M %d gu %d part %d stride %d" % (M, want_gu, want_part, stride)
        if want_gu:
            assert _written(gu), "mk_train_ln128_bwd left an element of gu unwritten, " + msg
            _within("ln128_bwd", "gu", gu, *refs["gu"], msg)
        else:
            assert _untouched(gu), "gu written although not asked for, " + msg
        if not want_part:
            assert _untouched(part), "part written although not asked for, " + msg
            continue
        assert _written(part), "mk_train_ln128_bwd left a column sum unwritten, " + msg
        _within("ln128_bwd", "part", part, *refs["part"], msg)
        out, c2 = guarded(1, 256, F32, dev)
        nv.call("mk_train_tail", None, 0, 0, 0, nv.ptr(part), stride, steps, 256, nv.ptr(out), nv.stream())
        _sync()
        c2()
        assert _written(out)
        _within("ln128_bwd + tail", "sums", out, refs["sums"][0][None], refs["sums"][1][None], msg)


# ================================================================ linear attention ===============================================
def _tokens(t, layout, col, dev):
    """[n, T, H, 16] on the device: dense, or plane `col` of a [n, T + 1, 3C] projection buffer (ld = 3C, an image stride that is
    not T ld, NaN everywhere else)"""
    if layout == "dense":
        return t.to(dev).contiguous(), None
    n, T, H, _ = t.shape
    buf = torch.full((n, T + 1, 3 * H, 16), float("nan"), device=dev, dtype=F32)
    view = buf[:, :T, col * H:(col + 1) * H]
    view.copy_(t.to(dev))
    return view, buf


def _attn_fwd(nv, ops, dev, q, k, v, layout, eps=R.LA_EPS):
    n, L, H, _ = q.shape
    S, C = k.shape[1], H * 16
    qd, kq = _tokens(q, layout, 0, dev)
    kd, kk = _tokens(k, layout, 1, dev)
    vd, kvv = _tokens(v, layout, 2, dev)
    out, c0 = guarded(n * L, C, F32, dev)
    kv, c1 = guarded(n * H, R.KVW, F32, dev)
    nwork = int(nv.query("mk_linattn_train_work_floats", n, L, S, C))
    work, c2 = guarded(1, nwork, F32, dev)
    nv.call("mk_linattn_train_fwd", *ops._attn_rows(qd), *ops._attn_rows(kd), *ops._attn_rows(vd), float(eps), nv.ptr(out), nv.ptr(kv),
            nv.ptr(work), n, L, S, C, nv.stream())
    _sync()
    for c in (c0, c1, c2):
        c()
    used = n * H * ((S + R.KV_CHUNK - 1) // R.KV_CHUNK) * R.KVW
    assert used <= nwork and _written(work[:, :used]) and _untouched(work[:, used:]), "work: the chunks of S, and nothing else, are written"
    assert _written(out) and _written(kv), "mk_linattn_train_fwd left an element unwritten"
    return out, kv, (qd, kd, vd)


@pytest.mark.parametrize("case", R.attn_cases(), ids=str)
def test_linattn_train(case):
    dev, nv, ops = _dev(), _nv(), _ops()
    C, L, S, n, layout, _ = case
    H = C // 16
    q, k, v, go = R.attn_inputs(case)
    msg = repr(case)
    f = R.attn_fwd_ref(q, k, v)
    out, kv, (qd, kd, vd) = _attn_fwd(nv, ops, dev, q, k, v, layout)
    _within("linattn_train_fwd", "kv", kv, f["kv"][0].reshape(n * H, R.KVW), f["kv"][1].reshape(n * H, R.KVW), msg)
    _within("linattn_train_fwd", "out", out, f["out"][0].reshape(n * L, C), f["out"][1].reshape(n * L, C), msg)
    kv32 = f["kv"][0].float()      # the backward is tested on its own: M | ks of the reference, rounded
    b = R.attn_bwd_ref(q, k, v, kv32, go)
    kvd, god = kv32.reshape(n * H, R.KVW).to(dev), go.to(dev).contiguous()
    nwork = int(nv.query("mk_linattn_train_work_floats", n, L, S, C))
    used = n * H * ((L + R.KV_CHUNK - 1) // R.KV_CHUNK) * R.KVW
    for need in R.ATTN_NEED:
        wins = dict(gq=guarded(n * L, C, F32, dev), gk=guarded(n * S, C, F32, dev), gv=guarded(n * S, C, F32, dev),
                    gkv=guarded(n * H, R.KVW, F32, dev), work=guarded(1, nwork, F32, dev))
        want = dict(gq=need[0], gk=need[1], gv=need[2], gkv=need[1] or need[2], work=need[1] or need[2])
        p = {name: (nv.ptr(wins[name][0]) if want[name] else None) for name in wins}
        nv.call("mk_linattn_train_bwd", *ops._attn_rows(qd), *ops._attn_rows(kd), *ops._attn_rows(vd), nv.ptr(kvd), nv.ptr(god),
                float(R.LA_EPS), p["work"], p["gkv"], p["gq"], p["gk"], p["gv"], n, L, S, C, nv.stream())
        _sync()
        m = "%s need %r" % (msg, need)
        for name, (t, chk) in wins.items():
            chk()
            if not want[name]:
                assert _untouched(t), "%s written although not asked for, %s" % (name, m)
            elif name == "work":
                assert used <= nwork and _written(t[:, :used]) and _untouched(t[:, used:]), "work: the chunks of L, and nothing else, " + m
            else:
                assert _written(t), "mk_linattn_train_bwd left an element of %s unwritten, %s" % (name, m)
                _within("linattn_train_bwd", name, t, b[name][0].reshape(t.shape), b[name][1].reshape(t.shape), m)


@pytest.mark.parametrize("S", R.ATTN_EXACT_S)
def test_kv_block_of_integers_is_exact(S):
    """phi(k) = k + 1 for a positive integer k and (S x integer) / S are exact (correctly rounded division: no fast-math flag in
    mickey_amd/build.py), so M | ks is a sum of integers whatever the chunking"""
    dev, nv, ops = _dev(), _nv(), _ops()
    case = (128, 7, S, 1, "dense", "exact")
    q, k, v, _ = R.attn_inputs(case)
    _, kv, _ = _attn_fwd(nv, ops, dev, q, k, v, "dense")
    _exact("linattn_train_fwd", "kv", kv, R.attn_fwd_ref(q, k, v)["kv"][0].reshape(8, R.KVW), repr(case))


def test_exp_pointwise_error():
    """E_EXP is a device constant: re-measured through these kernels at S = 1 with a large eps, where kv[256 + d] = phi(k[d]) = expf(k[d])"""
    dev, nv, ops = _dev(), _nv(), _ops()
    k = R.exp_probe_inputs()
    z = torch.zeros_like(k)
    _, kv, _ = _attn_fwd(nv, ops, dev, z, k, z, "dense", eps=1.0)
    got = kv.cpu().reshape(-1, 8, R.KVW)[..., 256:].double()
    x = k.reshape(-1, 8, 16).double()
    rel = (got - x.exp()).abs() / x.exp()
    worst, i = float(rel.max()), int(rel.argmax())
    EXP.append("train layer edges expf: max |expf(x) - exp(x)| / exp(x) = %.4g at x = %.6g over %d x in [-16, 0]; E_EXP %.4g, finding above %.4g"
               % (worst, float(x.reshape(-1)[i]), x.numel(), R.E_EXP, R.E_EXP_FINDING))
    print(EXP[-1])
    assert float(kv.cpu().reshape(-1, 8, R.KVW)[..., :256].abs().max()) == 0.0
    assert worst <= R.E_EXP_FINDING, EXP[-1]
    assert worst <= R.E_EXP, "the bounds of this module use E_EXP: " + EXP[-1]
