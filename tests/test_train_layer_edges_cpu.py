"""tests/helpers/train_layer_refs.py without a GPU: (1) every reference equals F.linear / F.layer_norm / linear_attention_formula under
fp64 autograd to 1e-12; (2) a correct fp32 evaluation meets every bound (and every integer comparison) at every listed case in two
summation orders; (3) seventeen subtly wrong evaluations each fail at a named case; (4) every case list reaches the edge it is named
for, derived from the library's host-side queries and the constexpr lines of the .hip sources."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from tests.helpers import train_layer_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D64 = torch.float64


@pytest.fixture(scope="module")
def nv():
    from mickey_amd import build, _native
    if not os.path.exists(build.lib_path()):
        build.build(verbose=False)
    _native.load()
    return _native


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _ok(kind, got32, ref, bound):
    """level 1: the same bits (as values: no -0.0 arises); level 2: within the bound everywhere"""
    if kind == "int":
        return bool((got32.double() == ref).all())
    return R.ratio(got32, ref, bound)[0] <= 1.0


# ================================================================ 1: the references equal torch =================================
def test_linear_references_equal_autograd():
    g = R.gen("cpu", "linear")
    a1, a2 = torch.randn((37, 36), generator=g), torch.randn((37, 32), generator=g)
    w = [torch.randn((16, 68), generator=g) for _ in range(3)]
    x = torch.cat([a1, a2], 1).double().requires_grad_()
    W = torch.cat(w).double().requires_grad_()
    for relu in (0, 1):
        y = F.relu(F.linear(x, W)) if relu else F.linear(x, W)
        assert _rel(R.fwd_ref(a1, a2, w, relu)[0], y.detach()) <= 1e-12
    G, old = torch.randn((37, 48), generator=g), torch.randn((37, 68), generator=g)
    h = torch.randn((37, 68), generator=g)
    h.view(-1)[::5] = 0.0
    xr = h.double().requires_grad_()
    gin, gw = torch.autograd.grad(F.linear(F.relu(xr), W), (xr, W), G.double())
    case = (37, 48, 36, 32, 2, 0, 0, 16)
    want = gin.clone()
    want[:, 36:] += old.double()[:, 36:]
    assert _rel(R.dgrad_ref(case, G, w, old, h)[0], want) <= 1e-12
    wcase = (37, 48, 36, 32, 16, 0)
    part, _, dw, _ = R.wgrad_ref(wcase, G, F.relu(h[:, :36]), F.relu(h[:, 36:]), surplus=2)
    assert part.shape == (5, 48 * 68) and float(part[3:].abs().max()) == 0.0
    assert _rel(dw.reshape(48, 68), gw) <= 1e-12
    assert _rel(R.tail_ref(part.float(), None)[0], part.float().double().sum(0)) <= 1e-12


def test_layernorm_references_equal_autograd():
    u, gamma, beta, resid = R.ln_fwd_inputs(33)
    x, gm, bt = u.double().requires_grad_(), gamma.double().requires_grad_(), beta.double().requires_grad_()
    y = F.layer_norm(x, (128,), gm, bt, R.LN_EPS)
    r = R.ln_fwd_ref(u.double(), 0.0, gamma, beta, resid)
    assert _rel(r["out"][0], y.detach() + resid.double()) <= 1e-12
    go = torch.randn((33, 128), generator=R.gen("cpu", "ln"))
    gx, ggm, gbt = torch.autograd.grad(y, (x, gm, bt), go.double())
    b = R.ln_bwd_ref(go, r["xhat"][0], r["rstd"][0], gamma)      # the fp64 xhat and rstd: the formula itself
    assert _rel(b["gu"][0], gx) <= 1e-12 and _rel(b["sums"][0], torch.cat([ggm, gbt])) <= 1e-12
    a1, a2, w, gamma, beta, resid = R.linln_inputs((17, 16, 16))
    y = F.layer_norm(F.linear(torch.cat([a1, a2], 1).double(), w.double()), (128,), gamma.double(), beta.double(), R.LN_EPS)
    assert _rel(R.linln_ref(a1, a2, w, gamma, beta, None)["out"][0], y) <= 1e-12


def test_attention_references_equal_autograd():
    from mickey_amd.train_attention import linear_attention_formula
    for case in [(48, 65, 63, 2, "dense", "normal"), (128, 5, 3, 1, "dense", "qzero"), (128, 33, 65, 2, "planes", "kneg")]:
        q, k, v, go = R.attn_inputs(case)
        qd, kd, vd = (t.double().requires_grad_() for t in (q, k, v))
        out = linear_attention_formula(qd, kd, vd, R.LA_EPS)
        f = R.attn_fwd_ref(q, k, v)
        assert _rel(f["out"][0], out.detach()) <= 1e-12
        b = R.attn_bwd_ref(q, k, v, f["kv"][0], go)
        for name, want in zip(("gq", "gk", "gv"), torch.autograd.grad(out, (qd, kd, vd), go.double())):
            assert _rel(b[name][0], want) <= 1e-12, (case, name)


# ================================================================ 2: a correct fp32 evaluation meets every bound ==================
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("kind", R.KINDS)
def test_fp32_gemm_forms_meet_the_bounds(kind, order):
    for case in R.FWD_CASES:
        a1, a2, w = R.fwd_inputs(case, kind)
        for relu in (0, 1):
            assert _ok(kind, R.fwd32(a1, a2, w, relu, order), *R.fwd_ref(a1, a2, w, relu)), ("fwd", case, relu)
    for case in R.DGRAD_CASES:
        ins = R.dgrad_inputs(case, kind)
        assert _ok(kind, R.dgrad32(case, *ins, order=order), *R.dgrad_ref(case, *ins)), ("dgrad", case)
    for case in R.WGRAD_CASES:
        ins = R.wgrad_inputs(case, kind)
        part, bpart, dw, bdw = R.wgrad_ref(case, *ins, surplus=2)
        p32, d32 = R.wgrad32(case, *ins, surplus=2, order=order)
        assert _ok(kind, p32, part, bpart) and _ok(kind, d32, dw, bdw), ("wgrad", case)
    for case in R.TAIL_CASES:
        ins = R.tail_inputs(case, kind)
        assert _ok(kind, R.tail32(*ins, order), *R.tail_ref(*ins)), ("tail", case)


def _all_within(got, refs, names, tag):
    for name, g in zip(names, got):
        worst, i = R.ratio(g, *refs[name])
        assert worst <= 1.0, (tag, name, worst, i)


@pytest.mark.parametrize("order", [0, 1])
def test_fp32_layernorms_meet_the_bounds(order):
    for M in R.LN_FWD_M:
        u, gamma, beta, resid = R.ln_fwd_inputs(M)
        for rs in (None, resid):
            _all_within(R.ln32(u, gamma, beta, rs, order=order), R.ln_fwd_ref(u.double(), 0.0, gamma, beta, rs), ("out", "xhat", "rstd"),
                        ("ln_fwd", M))
    for case in R.LINLN_CASES:
        a1, a2, w, gamma, beta, resid = R.linln_inputs(case)
        for rs in (None, resid):
            _all_within(R.linln32(a1, a2, w, gamma, beta, rs, order=order), R.linln_ref(a1, a2, w, gamma, beta, rs),
                        ("out", "xhat", "rstd"), ("linln", case))
    for M in R.LN_BWD_M:
        ins = R.ln_bwd_inputs(M)
        _all_within(R.ln_bwd32(*ins, order=order), R.ln_bwd_ref(*ins), ("gu", "part", "sums"), ("ln_bwd", M))


@pytest.mark.parametrize("order", [0, 1])
def test_fp32_attention_meets_the_bounds(order):
    for case in R.attn_cases():
        q, k, v, go = R.attn_inputs(case)
        f = R.attn_fwd_ref(q, k, v)
        kv32 = f["kv"][0].float()
        got = R.attn32(q, k, v, go, kv32, order=order)
        refs = dict(f, **R.attn_bwd_ref(q, k, v, kv32, go))
        _all_within([got[n] for n in refs], refs, list(refs), case)


@pytest.mark.parametrize("order", [0, 1])
def test_fp32_kv_block_of_integers_is_exact(order):
    for S in R.ATTN_EXACT_S:
        case = (128, 7, S, 1, "dense", "exact")
        q, k, v, go = R.attn_inputs(case)
        assert bool((R.attn32(q, k, v, go, order=order)["kv"].double() == R.attn_fwd_ref(q, k, v)["kv"][0]).all()), case


# ================================================================ 3: subtly wrong evaluations fail ================================
def _fwd_mutant(mutant, kind):
    def run():
        for case in R.FWD_CASES:
            a1, a2, w = R.fwd_inputs(case, kind)
            if (mutant == "seam" and a2 is None) or (mutant == "w3row" and len(w) == 1) or (mutant == "tile_row" and case[0] < R.BT):
                continue
            if not _ok(kind, R.fwd32(a1, a2, w, 0, 1, mutant), *R.fwd_ref(a1, a2, w, 0)):
                yield ("fwd", case)
    return run


def _dgrad_mutant(mutant, kind):
    def run():
        for case in R.DGRAD_CASES:
            ins = R.dgrad_inputs(case, kind)
            if not _ok(kind, R.dgrad32(case, *ins, order=1, mutant=mutant), *R.dgrad_ref(case, *ins)):
                yield ("dgrad", case)
    return run


def _wgrad_mutant(mutant, kind):
    def run():
        for case in R.WGRAD_CASES:
            ins = R.wgrad_inputs(case, kind)
            part, bpart, dw, bdw = R.wgrad_ref(case, *ins, surplus=2)
            p32, d32 = R.wgrad32(case, *ins, surplus=2, order=1, mutant=mutant)
            if not _ok(kind, p32, part, bpart):
                yield ("wgrad", case)
    return run


def _ln_mutant(mutant):
    def run():
        for M in R.LN_FWD_M:
            u, gamma, beta, resid = R.ln_fwd_inputs(M)
            refs = R.ln_fwd_ref(u.double(), 0.0, gamma, beta, None)
            got = R.ln32(u, gamma, beta, None, order=0, mutant=mutant)
            if any(R.ratio(g, *refs[n])[0] > 1.0 for n, g in zip(("out", "xhat", "rstd"), got)):
                yield ("ln_fwd", M)
    return run


def _ln_bwd_mutant(mutant):
    def run():
        for M in R.LN_BWD_M:
            ins = R.ln_bwd_inputs(M)
            if R.ratio(R.ln_bwd32(*ins, order=1, mutant=mutant)[0], *R.ln_bwd_ref(*ins)["gu"])[0] > 1.0:
                yield ("ln_bwd", M)
    return run


def _attn_mutant(mutant, outputs):
    def run():
        for case in R.attn_cases():
            C, L, S = case[:3]
            if (mutant in ("v_over_L", "scale_L") and L == S) or (mutant == "tok64" and S != 65) or (mutant == "head0" and C != 48):
                continue
            q, k, v, go = R.attn_inputs(case)
            f = R.attn_fwd_ref(q, k, v)
            kv32 = f["kv"][0].float()
            got = R.attn32(q, k, v, go, kv32, order=1, mutant=mutant)
            refs = dict(f, **R.attn_bwd_ref(q, k, v, kv32, go))
            if any(R.ratio(got[n], *refs[n])[0] > 1.0 for n in outputs):
                yield ("attn", case)
    return run


MUTANTS = {
    "last row of a 64-row tile dropped": [_fwd_mutant("tile_row", "int"), _fwd_mutant("tile_row", "normal")],
    "last quad of N dropped": [_fwd_mutant("last_quad", "int"), _fwd_mutant("last_quad", "normal")],
    "the contraction's last stage of 16 dropped": [_fwd_mutant("last_stage", "int"), _fwd_mutant("last_stage", "normal")],
    "A1 read where A2 belongs for the first quad after the seam": [_fwd_mutant("seam", "int"), _fwd_mutant("seam", "normal")],
    "w2 read for the first row of w3": [_fwd_mutant("w3row", "int"), _fwd_mutant("w3row", "normal")],
    "accumulate bit 1 ignored": [_dgrad_mutant("acc_bit1", "int"), _dgrad_mutant("acc_bit1", "normal")],
    "mask applied as < 0 instead of <= 0": [_dgrad_mutant("mask_lt", "int"), _dgrad_mutant("mask_lt", "normal")],
    "last chunk's last row dropped from a weight gradient": [_wgrad_mutant("last_row", "int"), _wgrad_mutant("last_row", "normal")],
    "a surplus chunk left unwritten": [_wgrad_mutant("surplus", "int"), _wgrad_mutant("surplus", "normal")],
    "variance taken as E[x^2] - mean^2 in fp32 on the offset rows": [_ln_mutant("var_e2")],
    "eps left out of rstd": [_ln_mutant("no_eps")],
    "mean(gamma g) taken over 127": [_ln_bwd_mutant("mean127")],
    "v / L instead of v / S with L != S": [_attn_mutant("v_over_L", ("kv",))],
    "scale of L / den instead of S / den": [_attn_mutant("scale_L", ("out",))],
    "phi' = 1 for x <= 0": [_attn_mutant("dphi1", ("gq",)), _attn_mutant("dphi1", ("gk",))],
    "token 64 of a 65-token sum dropped": [_attn_mutant("tok64", ("kv",))],
    "head H - 1 computed with head 0's block at H = 3": [_attn_mutant("head0", ("out",)), _attn_mutant("head0", ("gq",))],
}


@pytest.mark.parametrize("name", list(MUTANTS))
def test_mutant_fails(name):
    """every level it belongs to rejects the mutant: the integer comparison AND the bound, each at a named case"""
    for run in MUTANTS[name]:
        failed = list(run())
        print("%s: fails at %d cases, first %r" % (name, len(failed), failed[:1]))
        assert failed, "no listed case rejects the mutant '%s': the bound is too wide or the list misses the edge" % name


# ================================================================ 4: every case list reaches its edge =============================
def _constexpr(src, name):
    m = re.search(r"constexpr int %s = (\d+);" % name, src)
    assert m, name
    return int(m.group(1))


def _src(name):
    with open(os.path.join(ROOT, "mickey_amd", "csrc", name)) as f:
        return f.read()


def test_constants_are_the_sources():
    tl, la = _src("mk_train_layer.hip"), _src("mk_linattn.hip")
    for name, mine in (("BT", R.BT), ("KT", R.KT), ("STEP", R.STEP), ("MAXCHUNK", R.MAXCHUNK), ("DLN", R.DLN)):
        assert _constexpr(tl, name) == mine, name
    assert _constexpr(tl, "LNB_WAVES") == 16 and R.STEP % 16 == 0
    m = re.search(r"ln_fwd_kernel, dim3\(\(M \+ (\d+)\) / (\d+)\), dim3\((\d+)\)", tl)
    assert m and int(m.group(2)) == int(m.group(1)) + 1 == R.LN_BLOCK_ROWS and int(m.group(3)) == 4 * 64
    assert _constexpr(la, "KV_CHUNK") == R.KV_CHUNK and _constexpr(la, "KVW") == R.KVW
    from tests.helpers import heads_refs as H
    assert (H.KV_CHUNK, H.KVW) == (R.KV_CHUNK, R.KVW)


def test_gemm_lists_reach_their_edges():
    BT, KT = R.BT, R.KT
    for edge in (KT, 2 * KT, BT):
        assert {edge - 1, edge, edge + 1} <= set(R.M_EDGES)
    assert 1 in R.M_EDGES and max(R.M_EDGES) > 2 * BT
    assert all(N % 4 == 0 for N in R.FWD_N) and {BT - 4, BT, BT + 4} <= set(R.FWD_N) and min(R.FWD_N) == 4 and max(R.FWD_N) > 2 * BT
    assert (KT, 0) in R.FWD_K and any(K1 + K2 > 2 * KT for K1, K2 in R.FWD_K)            # the prefetch never / once / often taken
    assert any(K2 and K1 % BT and K1 + K2 <= BT for K1, K2 in R.FWD_K)                   # the seam inside a 64-wide tile
    assert all(ws % KT == 0 for ws in R.FWD_WSPLIT) and any(ws % BT and (2 * ws) % BT for ws in R.FWD_WSPLIT)
    assert {KT, 2 * KT} <= set(R.DGRAD_N) and max(R.DGRAD_N) > 2 * BT
    widths = [K1 + K2 for K1, K2 in R.DGRAD_K]
    assert {4, BT - 4, BT, BT + 4} <= set(widths) and max(widths) > 2 * BT and any(K2 and K1 % BT for K1, K2 in R.DGRAD_K)
    assert {c[4] for c in R.DGRAD_CASES} == {0, 1, 2, 3} and {c[5] for c in R.DGRAD_CASES} == {None, 0, 4}
    assert {c[6] for c in R.DGRAD_CASES} == {0, 16, 48} and {c[7] for c in R.DGRAD_CASES} == {0, 16, 48}
    assert {4, BT - 4, BT, BT + 4} == set(R.WGRAD_NK)
    assert {c[5] for c in R.WGRAD_CASES} == {0, 16, 48} and any(c[3] and c[2] % BT for c in R.WGRAD_CASES)
    assert {nw + nl for nw, nl in R.TAIL_SIZES} >= {1, 255, 256, 257} and any(nw == 0 for nw, _ in R.TAIL_SIZES)
    assert any(nl == 0 for _, nl in R.TAIL_SIZES) and {wc for wc, _ in R.TAIL_COUNTS} == {ls for _, ls in R.TAIL_COUNTS} == {1, 7, 8, 9, 32}
    for M in R.WGRAD_LIB_M + [4097]:      # the integer argument: every sum of |terms| stays below 2^24
        assert M * 16 < 2 ** 24


def test_chunk_and_step_lists_reach_their_edges(nv):
    for M in list(range(1, 700, 7)) + R.WGRAD_LIB_M + [8192, 8193, 124032]:
        assert int(nv.query("mk_train_rows_per_chunk", M)) == R.rows_per_chunk(M), M
        assert int(nv.query("mk_train_ln_steps", M)) == R.ln_steps(M), M
        rpc = R.rows_per_chunk(M)
        assert int(nv.query("mk_train_chunks", M)) == (M + rpc - 1) // rpc <= R.MAXCHUNK
    q = lambda M: (int(nv.query("mk_train_rows_per_chunk", M)), int(nv.query("mk_train_chunks", M)))   # noqa: E731
    assert q(4096) == (128, 32) and q(4097) == (256, 17) and 4097 - 16 * 256 == 1
    assert q(127) == (128, 1) and q(128) == (128, 1) and q(129) == (128, 2) and q(257) == (128, 3)
    assert {127, 128, 129, 257, 4096, 4097} == set(R.WGRAD_LIB_M)
    plans = {M: R.wgrad_plan((M, 8, 20, 0, 16, 0)) for M in R.WGRAD_SMALL_M}     # ragged and multiple chunks at 16 rows a chunk
    assert plans == {1: (16, 1), 15: (16, 1), 16: (16, 1), 17: (16, 2), 33: (16, 3)}
    two = [R.wgrad_plan((M, 8, 20, 0, 32, 0)) for M in R.WGRAD_TWO_STAGE_M]   # a prefetched stage that holds a single row
    assert two == [(32, 1), (32, 2), (32, 2)] and 17 == R.KT + 1 and 49 - 32 == R.KT + 1
    steps = {M: int(nv.query("mk_train_ln_steps", M)) for M in R.LN_BWD_M}
    assert steps == {1: 1, 15: 1, 16: 1, 17: 1, 127: 1, 128: 1, 129: 2, 257: 3}
    assert {3, 4, 5, R.LN_BLOCK_ROWS - 1, R.LN_BLOCK_ROWS, R.LN_BLOCK_ROWS + 1, 2 * R.LN_BLOCK_ROWS + 1} <= set(R.LN_FWD_M)
    assert {R.BT - 1, R.BT, R.BT + 1, 2 * R.BT + 1} <= set(R.LINLN_M) and (16, 0) in R.LINLN_K and (128, 128) in R.LINLN_K


def test_attention_lists_reach_their_edges(nv):
    chunks = lambda L, S: int(nv.query("mk_linattn_train_work_floats", 1, L, S, 16)) // R.KVW   # noqa: E731
    assert int(nv.query("mk_linattn_train_work_floats", 1, 1, 1, 16)) == R.KVW
    for T in R.ATTN_T:
        assert chunks(T, 7) == chunks(7, T) == (max(T, 7) + R.KV_CHUNK - 1) // R.KV_CHUNK
    assert [chunks(T, 1) for T in (63, 64, 65, 127, 128, 129)] == [1, 1, 2, 2, 2, 3]
    assert {1, 2, 3, 4, 5} <= set(R.ATTN_T)                                               # one to five tokens in a chunk
    cases = R.attn_cases()
    assert max(max(c[1], c[2]) for c in cases) <= 257
    for C in R.ATTN_C:
        H, t = C // 16, R.tokens_per_block(C)
        assert ((256 // H) * H < 256) == (H in (3, 5, 6, 7))
        for x in (t - 1, t, t + 1):
            assert any(c[0] == C and c[1] == x and c[2] == x for c in cases), (C, x)
        assert any(c[:3] == (C, 65, 63) for c in cases)
    assert {C // 16 for C in R.ATTN_C} == set(range(1, 9))
    assert {c[3] for c in cases} == {1, 2, 3} and {c[4] for c in cases} == {"dense", "planes"}
    for layout in ("dense", "planes"):                                                    # every C meets both layouts
        assert {c[0] for c in cases if c[4] == layout} == set(R.ATTN_C)
    assert {c[5] for c in cases} == {"normal", "kneg", "qzero"}
