"""References, input builders, bounds and the case lists of the trainable EncoderLayer's edge tests: all of mk_train_layer.hip and the
training half of mk_linattn.hip (tests/test_train_layer_edges_cpu.py checks them here on the CPU, tests/test_train_layer_edges_gpu.py
runs the kernels against them).  Pure torch on the CPU.

Level 1 (the three GEMM forms, the tail, the kv block of the attention): operands are integers in [-4, 4]; with a contraction of at
most 4097 terms every partial sum is an integer below 2^24, so an fp32 fma chain in ANY order gives the fp64 result bit for bit.

Level 2: every reference is fp64 on the fp32 inputs as passed, every bound is |got - ref64| <= bound element-wise, built from
  u = 2^-24 per fp32 operation on the magnitude of its result;  gam(n) sum |terms| for a length-n sum in any order (fused or not);
  SLACK = 1.01 for the second-order terms;  E_PHI = max(E_EXP, u) relative for phi(x) = x + 1 (x > 0) / expf(x);
errors are pushed through products and quotients to first order with running sums of |terms| (never norms): where two terms cancel
the bound is wide on its own account.  The derivations stand in the docstrings of the *_ref functions.

The *32 functions are correct fp32 evaluations in two summation orders (0: plain index order, one term after the other; 1: the
kernels' staged / chunked / strided order) and, with `mutant`, the subtly wrong evaluations that the bounds have to reject."""
import torch

from tests.helpers.guarded import sentinel_bits
from tests.helpers.heads_refs import E_EXP, E_EXP_FINDING, E_PHI, SLACK, U, gam, gen, phi64, ratio   # noqa: F401 (re-exported)

BT, KT, LN_BLOCK_ROWS, STEP, MAXCHUNK, DLN = 64, 16, 16, 128, 32, 128   # mk_train_layer.hip (asserted against the source / library)
KV_CHUNK, KVW = 64, 272                                                # mk_linattn.hip
LN_EPS = 1e-5
LA_EPS = float(torch.tensor(1e-6, dtype=torch.float32))
SENTINEL = float(torch.tensor([sentinel_bits(torch.float32)], dtype=torch.int32).view(torch.float32))

M_EDGES = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129]                 # MFMA tile 16, wave 32, block 64, two blocks
KINDS = ["int", "normal"]                                              # level 1, level 2


def draw(kind, shape, g):
    if kind == "int":
        return torch.randint(-4, 5, shape, generator=g).float()
    return torch.randn(shape, generator=g)


def cat(a1, a2):
    return a1 if a2 is None else torch.cat([a1, a2], 1)


def kperm(n):
    """the k order of mma_stage: stages of 16, MFMA e of a stage contracts k = e, 4 + e, 8 + e, 12 + e"""
    return [k0 + 4 * j + e for k0 in range(0, n, KT) for e in range(4) for j in range(4) if k0 + 4 * j + e < n]


def dot32(A, B, order):
    """fp32 [M, N] = sum_k A[m, k] B[n, k], one term after the other; order 0: k ascending, 1: kperm"""
    acc = torch.zeros((A.shape[0], B.shape[0]))
    for k in (range(A.shape[1]) if order == 0 else kperm(A.shape[1])):
        acc = acc + A[:, k, None] * B[None, :, k]
    return acc


def _relu_keep_nan(x):
    return torch.where(x > 0, x, torch.where(x != x, x, torch.zeros_like(x)))


# ================================================================ mk_train_linear_fwd ===========================================
# (M, N, K1, K2, wsplit)
FWD_K = [(16, 0), (32, 0), (144, 0), (16, 16), (16, 48), (48, 16)]     # one stage (no prefetch), two, nine; the seam inside a tile
FWD_N = [4, 28, 60, 64, 68, 132]
FWD_WSPLIT = [16, 48]
FWD_CASES = list(dict.fromkeys(
    [(M, 68, 32, 0, 0) for M in M_EDGES] + [(65, N, 32, 0, 0) for N in FWD_N] + [(65, 68, K1, K2, 0) for K1, K2 in FWD_K] +
    [(65, 3 * ws, K1, K2, ws) for ws in FWD_WSPLIT for K1, K2 in ((32, 0), (16, 16))]))


def fwd_inputs(case, kind):
    """-> a1 [M, K1], a2 [M, K2] or None, w: a list of one [N, K] or three [wsplit, K] matrices"""
    M, N, K1, K2, ws = case
    g = gen("fwd", case, kind)
    a1 = draw(kind, (M, K1), g)
    a2 = draw(kind, (M, K2), g) if K2 else None
    return a1, a2, [draw(kind, (ws or N, K1 + K2), g) for _ in range(3 if ws else 1)]


def fwd_ref(a1, a2, w, relu):
    """out = act([a1 | a2] . W^T): a chain of K fused multiply-adds from 0 -> gam(K) sum |terms|; the ReLU is 1-Lipschitz and exact.
    (+ 0.0: a sum of products that are all -0.0 is +0.0 in a chain that starts at +0.0)"""
    A, W = cat(a1, a2).double(), torch.cat(w).double()
    ref = A @ W.t() + 0.0
    return (_relu_keep_nan(ref) if relu else ref), gam(A.shape[1]) * (A.abs() @ W.abs().t()) * SLACK


def fwd32(a1, a2, w, relu, order=0, mutant=None):
    A, W, K1 = cat(a1, a2).clone(), torch.cat(w).clone(), a1.shape[1]
    if mutant == "seam":          # A1 read where A2 belongs for the first quad after the seam
        A[:, K1:K1 + 4] = a1[:, :4]
    if mutant == "w3row":         # w2 read for the first row of w3
        W[2 * w[0].shape[0]] = w[1][-1]
    if mutant == "last_stage":    # the contraction's last stage of 16 dropped
        A[:, -KT:] = 0
    out = dot32(A, W, order)
    if relu:
        out = _relu_keep_nan(out)
    if mutant == "tile_row":      # last row of a 64-row tile dropped
        out[BT - 1::BT] = 0
    if mutant == "last_quad":     # last quad of N dropped
        out[:, -4:] = 0
    return out


# ================================================================ mk_train_linear_dgrad =========================================
# (M, N, K1, K2, accumulate, mask pad (None: no mask; ldmask = K + pad), gsplit, wsplit)
DGRAD_N = [16, 32, 144]
DGRAD_K = [(4, 0), (60, 0), (64, 0), (68, 0), (132, 0), (4, 4), (60, 8), (36, 32)]
DGRAD_SPLITS = [(16, 0), (16, 16), (48, 0), (48, 48), (0, 16), (0, 48)]                # (gsplit, wsplit); N = 3 x the split
DGRAD_CASES = list(dict.fromkeys(
    [(M, 32, 68, 0, 0, None, 0, 0) for M in M_EDGES] + [(65, N, 68, 0, 0, None, 0, 0) for N in DGRAD_N] +
    [(65, 32, K1, K2, 0, None, 0, 0) for K1, K2 in DGRAD_K] +
    [(65, 32, 36, 32, acc, None, 0, 0) for acc in (1, 2, 3)] + [(65, 32, 60, 8, 3, None, 0, 0)] +
    [(65, 32, 36, 32, acc, mp, 0, 0) for mp in (0, 4) for acc in (0, 3)] +
    [(65, 3 * max(gs, ws), 68, 0, 0, None, gs, ws) for gs, ws in DGRAD_SPLITS] + [(33, 144, 36, 32, 3, 4, 48, 48)]))


def dgrad_inputs(case, kind):
    """-> g [M, N], w (list), old [M, K] (what the outputs hold before the call), mask [M, K] or None: positive values, zeros,
    -0.0, negatives and one NaN"""
    M, N, K1, K2, acc, mp, gs, ws = case
    K = K1 + K2
    g = gen("dgrad", case, kind)
    G = draw(kind, (M, N), g)
    w = [draw(kind, (ws or N, K), g) for _ in range(3 if ws else 1)]
    old = draw(kind, (M, K), g)
    mask = None
    if mp is not None:
        mask = torch.randn((M, K), generator=g)
        flat = mask.view(-1)
        flat[0::5] = 0.0
        flat[1::7] = -0.0
        flat[3] = float("nan")
    return G, w, old, mask


def dgrad_masks(case, mask, mutant=None):
    M, N, K1, K2, acc = case[:5]
    keep = torch.ones((M, K1 + K2), dtype=torch.bool) if mask is None else ~((mask < 0) if mutant == "mask_lt" else (mask <= 0))
    accm = torch.cat([torch.full((K1,), bool(acc & 1)), torch.full((K2,), bool(acc & 2) and mutant != "acc_bit1")])
    return keep, accm[None, :]


def dgrad_ref(case, G, w, old, mask):
    """[o1 | o2] = (G . W) where mask > 0 or NaN, an exact zero elsewhere, added to `old` where the column's accumulate bit is set:
    N fused multiply-adds and one addition -> gam(N + 1) (sum |terms| + |old|)"""
    keep, accm = dgrad_masks(case, mask)
    G, W = G.double(), torch.cat(w).double()
    zero = torch.zeros((), dtype=torch.float64)
    P = torch.where(keep, G @ W + 0.0, zero)
    Ab = torch.where(keep, G.abs() @ W.abs(), zero)
    o = torch.where(accm, old.double(), zero)
    return P + o, gam(G.shape[1] + 1) * (Ab + o.abs()) * SLACK


def dgrad32(case, G, w, old, mask, order=0, mutant=None):
    keep, accm = dgrad_masks(case, mask, mutant)
    P = torch.where(keep, dot32(G, torch.cat(w).t().contiguous(), order), torch.zeros(()))
    return torch.where(accm, P + old, P)


# ================================================================ mk_train_linear_wgrad =========================================
# (M, N, K1, K2, rows_per_chunk (0: the library's own chunking), gsplit)
WGRAD_SMALL_M, WGRAD_LIB_M, WGRAD_NK = [1, 15, 16, 17, 33], [127, 128, 129, 257, 4096, 4097], [4, 60, 64, 68]
WGRAD_TWO_STAGE_M = [17, 33, 49]        # at 32 rows a chunk: a chunk of two stages whose second holds one row (17; 49: its second chunk)
WGRAD_CASES = list(dict.fromkeys(
    [(M, 8, 20, 0, 16, 0) for M in WGRAD_SMALL_M] + [(M, 8, 20, 0, 0, 0) for M in WGRAD_LIB_M] +
    [(M, 8, 20, 0, 32, 0) for M in WGRAD_TWO_STAGE_M] +
    [(33, N, 20, 0, 16, 0) for N in WGRAD_NK] + [(33, 8, K, 0, 16, 0) for K in WGRAD_NK] + [(33, 8, 36, 32, 16, 0)] +
    [(33, 3 * gs, 20, 0, 16, gs) for gs in (16, 48)]))
WGRAD_VARIANTS = [(0, 0), (2, 8)]                                      # (surplus chunks, chunk_stride - N K)


def rows_per_chunk(M):
    """mk_train_rows_per_chunk, restated (asserted equal in tests/test_train_layer_edges_cpu.py)"""
    steps = (M + STEP - 1) // STEP
    return STEP * ((steps + MAXCHUNK - 1) // MAXCHUNK)


def wgrad_plan(case):
    """-> (rows per chunk, chunks that hold rows)"""
    rpc = case[4] or rows_per_chunk(case[0])
    return rpc, (case[0] + rpc - 1) // rpc


def wgrad_inputs(case, kind):
    M, N, K1, K2, _, _ = case
    g = gen("wgrad", case, kind)
    return draw(kind, (M, N), g), draw(kind, (M, K1), g), (draw(kind, (M, K2), g) if K2 else None)


def wgrad_ref(case, G, a1, a2, surplus=0):
    """-> (part64, bound of part, dw64, bound of dw): part[c] = G[rows of c]^T . [a1 | a2] flat, zeros for the surplus chunks; a chunk is
    a chain of at most rows_per_chunk fused multiply-adds: gam(rpc) sum |terms|; dw = the chunks added in order by mk_train_tail:
    gam(rpc + chunks) sum |terms|"""
    rpc, chunks = wgrad_plan(case)
    G, A = G.double(), cat(a1, a2).double()
    nk = G.shape[1] * A.shape[1]
    part, ab = torch.zeros((chunks + surplus, nk), dtype=torch.float64), torch.zeros((chunks + surplus, nk), dtype=torch.float64)
    for c in range(chunks):
        r = slice(c * rpc, min(G.shape[0], (c + 1) * rpc))
        part[c] = (G[r].t() @ A[r] + 0.0).reshape(-1)
        ab[c] = (G[r].abs().t() @ A[r].abs()).reshape(-1)
    return part, gam(rpc) * ab * SLACK, part.sum(0), gam(rpc + chunks + surplus) * ab.sum(0) * SLACK


def wgrad32(case, G, a1, a2, surplus=0, order=0, mutant=None):
    """-> (part32, dw32)"""
    rpc, chunks = wgrad_plan(case)
    A = cat(a1, a2)
    part = torch.zeros((chunks + surplus, G.shape[1] * A.shape[1]))
    for c in range(chunks):
        r1 = min(G.shape[0], (c + 1) * rpc)
        if mutant == "last_row" and c == chunks - 1:     # the last chunk's last row dropped
            r1 -= 1
        part[c] = dot32(G[c * rpc:r1].t().contiguous(), A[c * rpc:r1].t().contiguous(), order).reshape(-1)
    if mutant == "surplus" and surplus:                  # a surplus chunk left unwritten
        part[-1] = SENTINEL
    return part, tail32(part, None, order)


# ================================================================ mk_train_tail ==================================================
# (nw, nl, wchunks, lsteps, stride - count)
TAIL_SIZES = [(1, 0), (0, 1), (200, 55), (200, 56), (200, 57), (0, 256), (257, 0)]     # nw + nl = 1, 255, 256, 257; nw = 0; nl = 0
TAIL_COUNTS = [(1, 32), (7, 9), (8, 8), (9, 7), (32, 1)]                               # the loop is unrolled by 8
TAIL_CASES = [(nw, nl, 3, 2, 0) for nw, nl in TAIL_SIZES] + [(200, 57, wc, ls, 3) for wc, ls in TAIL_COUNTS]


def tail_inputs(case, kind):
    nw, nl, wc, ls, _ = case
    g = gen("tail", case, kind)
    return (draw(kind, (wc, nw), g) if nw else None), (draw(kind, (ls, nl), g) if nl else None)


def tail_ref(wpart, lpart):
    """out = [sum_c wpart[c] | sum_s lpart[s]]: n additions from 0 -> gam(n) sum |terms|"""
    refs = [(p.double().sum(0) + 0.0, gam(p.shape[0]) * p.double().abs().sum(0) * SLACK) for p in (wpart, lpart) if p is not None]
    return torch.cat([r for r, _ in refs]), torch.cat([b for _, b in refs])


def tail32(wpart, lpart, order=0):
    def total(p):
        if order:
            return p.flip(0).sum(0)
        acc = torch.zeros(p.shape[1])
        for c in range(p.shape[0]):
            acc = acc + p[c]
        return acc
    return torch.cat([total(p) for p in (wpart, lpart) if p is not None])


# ================================================================ LayerNorm(128) forward ==========================================
LN_FWD_M = [1, 3, 4, 5, 15, 16, 17, 33]                                # 4 waves, 16 rows per block
LN_RESID = [None, 128, 132]                                            # ldr
LN_SAVED = [(1, 1), (1, 0), (0, 1), (0, 0)]                            # (xhat, rstd) wanted
LINLN_M = [1, 15, 16, 17, 63, 64, 65, 129]
LINLN_K = [(16, 0), (128, 0), (256, 0), (16, 16), (128, 128)]
LINLN_CASES = list(dict.fromkeys([(M, 128, 0) for M in LINLN_M] + [(65, K1, K2) for K1, K2 in LINLN_K]))   # (M, K1, K2)


def ln_fwd_inputs(M):
    """-> u, gamma, beta, resid: rows as heads_refs.ln_inputs builds them (even rows centred, odd rows with a mean of 6 sd)"""
    from tests.helpers.heads_refs import ln_inputs
    u, w, b, resid = ln_inputs(M, DLN, case="train_ln")
    return u, w[0], b[0], resid


def linln_inputs(case):
    M, K1, K2 = case
    g = gen("linln", case)
    a1 = torch.randn((M, K1), generator=g)
    a2 = torch.randn((M, K2), generator=g) if K2 else None
    w = torch.randn((DLN, K1 + K2), generator=g) / (K1 + K2) ** 0.5
    gamma, beta = 1 + 0.5 * torch.randn(DLN, generator=g), torch.randn(DLN, generator=g)
    return a1, a2, w, gamma, beta, torch.randn((M, DLN), generator=g)


def ln_fwd_ref(u64, e_in, gamma, beta, resid, eps=LN_EPS):
    """fp64 LayerNorm of rows u64 that the kernel holds with an error of at most e_in (0, or the bound of the linear in front of it)
    -> {out, xhat, rstd: (ref64, bound)} for  mean = sum / D; d = u - mean; rstd = 1 / sqrt(sum d^2 / D + eps); xh = d rstd;
    out = xh gamma + beta (+ resid):
      mean:  |dmean| <= mean(e_in) + gam(D + 1) sum (|u| + e_in) / D                                            =: mu
      d:     computed d_i = d_i + s + p_i, s the common shift (|s| <= mu), |p_i| <= e_in_i + u (|d_i| + e_in_i + mu)
      var:   sum (d_i + s + p_i)^2 = sum (d_i + p_i)^2 + 2 s sum p_i + D s^2 (sum d_i = 0 exactly):
             |dvar| <= 2 mean(|d| p) + mean(p^2) + 2 mu mean(p) + mu^2, + gam(D + 5) (var + that) for squares, sum, / D and + eps
      rstd:  relative error rho = dvar / (2 (var + eps)) + 4 u (sqrt, reciprocal)
      xh:    rstd (mu + p) + |xh| (rho + u);   out: |gamma| dxh + u |xh gamma| + u |xh gamma + beta| (+ u |out| with resid)"""
    D = u64.shape[1]
    gamma, beta = gamma.double(), beta.double()
    mean = u64.mean(1, keepdim=True)
    d = u64 - mean
    var = (d * d).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = d * rstd
    y = xh * gamma + beta
    e_in = e_in if torch.is_tensor(e_in) else torch.full_like(u64, float(e_in))
    mu = e_in.mean(1, keepdim=True) + gam(D + 1) * (u64.abs() + e_in).sum(1, keepdim=True) / D
    p = e_in + U * (d.abs() + e_in + mu)
    dvar = 2 * (d.abs() * p).mean(1, keepdim=True) + (p * p).mean(1, keepdim=True) + 2 * mu * p.mean(1, keepdim=True) + mu * mu
    dvar = dvar + gam(D + 5) * (var + dvar)
    rho = dvar / (2 * (var + eps)) + 4 * U
    dxh = (rstd * (mu + p) + xh.abs() * (rho + U)) * SLACK
    out, dout = y, gamma.abs() * dxh + U * (xh * gamma).abs() + U * y.abs()
    if resid is not None:
        out = y + resid.double()
        dout = dout + U * (out.abs() + dout)
    return dict(out=(out, dout * SLACK), xhat=(xh, dxh), rstd=(rstd.reshape(-1), (rstd * rho * SLACK).reshape(-1)))


def _rowsum32(t, order):
    """[M, 128] -> [M, 1]; order 0: one column after the other, 1: a lane's two columns, then a binary tree over the 64 lanes"""
    if order == 0:
        acc = torch.zeros((t.shape[0], 1))
        for c in range(t.shape[1]):
            acc = acc + t[:, c:c + 1]
        return acc
    t = t[:, 0::2] + t[:, 1::2]
    while t.shape[1] > 1:
        t = t[:, :t.shape[1] // 2] + t[:, t.shape[1] // 2:]
    return t


def ln32(u, gamma, beta, resid, eps=LN_EPS, order=0, mutant=None):
    """-> (out, xhat, rstd) in fp32"""
    mean = _rowsum32(u, order) * (1.0 / DLN)
    d = u - mean
    var = _rowsum32(d * d, order) * (1.0 / DLN)
    if mutant == "var_e2":        # variance taken as E[x^2] - mean^2
        var = _rowsum32(u * u, order) * (1.0 / DLN) - mean * mean
    rstd = 1.0 / torch.sqrt(var + (0.0 if mutant == "no_eps" else torch.tensor(eps, dtype=torch.float32)))
    xh = d * rstd
    out = xh * gamma + beta
    return (out if resid is None else out + resid), xh, rstd.reshape(-1)


def linln_ref(a1, a2, w, gamma, beta, resid, eps=LN_EPS):
    """the fp64 linear followed by the fp64 LayerNorm; the linear's bound gam(K) sum |terms| is the LayerNorm's e_in"""
    A, W = cat(a1, a2).double(), w.double()
    return ln_fwd_ref(A @ W.t(), gam(A.shape[1]) * (A.abs() @ W.abs().t()) * SLACK, gamma, beta, resid, eps)


def linln32(a1, a2, w, gamma, beta, resid, eps=LN_EPS, order=0, mutant=None):
    return ln32(dot32(cat(a1, a2), w, order), gamma, beta, resid, eps, order, mutant)


# ================================================================ LayerNorm(128) backward =========================================
LN_BWD_M = [1, 15, 16, 17, 127, 128, 129, 257]                         # 16 waves, a step of 128 rows
LN_BWD_VARIANTS = [(1, 0, 256), (0, 1, 256), (1, 1, 256), (1, 1, 264), (0, 1, 264)]   # (gu, part wanted, part_stride)


def ln_steps(M):
    return (M + STEP - 1) // STEP


def ln_bwd_inputs(M):
    """-> g, xhat32, rstd32 (the fp64 reference's, rounded: the kernel is tested on its own), gamma"""
    u, gamma, beta, _ = ln_fwd_inputs(M)
    r = ln_fwd_ref(u.double(), 0.0, gamma, beta, None)
    return torch.randn((M, DLN), generator=gen("ln_bwd", M)), r["xhat"][0].float(), r["rstd"][0].float(), gamma


def ln_bwd_ref(g, xhat, rstd, gamma):
    """a = g gamma (u |a|); c1 = mean(a): e1 = gam(D + 1) mean |a|; c2 = mean(a xh): e2 = gam(D + 2) mean |a xh|;
    gu = rstd (a - c1 - xh c2): rstd (3 u |a| + e1 + 2 u |c1| + |xh| e2 + 3 u |xh c2|) + u |gu|  (product, two subtractions).
    part[step] = column sums over the step's rows of g xh | g: at most 128 terms and the products -> gam(STEP + 1) sum |terms|;
    sums = the steps added in order by mk_train_tail: gam(STEP + 1 + steps).  -> {gu, part, sums: (ref64, bound)}"""
    M, D = g.shape
    g, xh, rs, gm = g.double(), xhat.double(), rstd.double()[:, None], gamma.double()
    a = g * gm
    c1, c2 = a.mean(1, keepdim=True), (a * xh).mean(1, keepdim=True)
    gu = rs * (a - c1 - xh * c2)
    e1, e2 = gam(D + 1) * a.abs().mean(1, keepdim=True), gam(D + 2) * (a * xh).abs().mean(1, keepdim=True)
    bgu = (rs * (3 * U * a.abs() + e1 + 2 * U * c1.abs() + xh.abs() * e2 + 3 * U * (xh * c2).abs()) + U * gu.abs()) * SLACK
    t = torch.cat([g * xh, g], 1)
    steps = ln_steps(M)
    part = torch.stack([t[s * STEP:(s + 1) * STEP].sum(0) for s in range(steps)])
    ab = torch.stack([t[s * STEP:(s + 1) * STEP].abs().sum(0) for s in range(steps)])
    return dict(gu=(gu, bgu), part=(part, gam(STEP + 1) * ab * SLACK), sums=(part.sum(0), gam(STEP + 1 + steps) * ab.sum(0) * SLACK))


def ln_bwd32(g, xhat, rstd, gamma, order=0, mutant=None):
    """-> (gu, part, sums) in fp32; order 1: wave w of 16 sums rows w, w + 16, ... of a step, the waves are added in order"""
    a = g * gamma
    c1 = _rowsum32(a, order) * (1.0 / (DLN - 1 if mutant == "mean127" else DLN))
    c2 = _rowsum32(a * xhat, order) * (1.0 / DLN)
    gu = rstd[:, None] * (a - c1 - xhat * c2)
    t = torch.cat([g * xhat, g], 1)
    part = []
    for s in range(ln_steps(g.shape[0])):
        blk = t[s * STEP:(s + 1) * STEP]
        rows = [blk[w::16] for w in range(16)] if order else [blk]
        acc = torch.zeros(2 * DLN)
        for r in rows:
            wacc = torch.zeros(2 * DLN)
            for i in range(r.shape[0]):
                wacc = wacc + r[i]
            acc = acc + wacc
        part.append(acc)
    part = torch.stack(part)
    return gu, part, tail32(None, part, 0)


# ================================================================ linear attention, forward and backward ==========================
ATTN_T = [1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 127, 128, 129]       # waves take every 4th token; tokens per block at H = 8; KV_CHUNK
ATTN_C = [16, 32, 48, 64, 80, 96, 112, 128]
ATTN_NEED = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)]
ATTN_SPECIAL = [(128, 33, 65, 2, "planes", "kneg"), (128, 5, 3, 1, "dense", "qzero"), (48, 65, 65, 1, "dense", "qzero")]
ATTN_EXACT_S = sorted(set(ATTN_T))


def tokens_per_block(C):
    return 256 // (C // 16)


def attn_cases():
    """(C, L, S, nimg, layout, inputs): nimg in {1, 3} and the two layouts alternate so that every edge meets both"""
    shapes = [(128, T, 7) for T in ATTN_T] + [(128, 7, T) for T in ATTN_T]
    for C in ATTN_C:
        t = tokens_per_block(C)
        shapes += [(C, t - 1, t - 1), (C, t, t), (C, t + 1, t + 1), (C, 65, 63)]
    out = [(C, L, S, (1, 3)[(i // 2) % 2], ("dense", "planes")[i % 2], "normal") for i, (C, L, S) in enumerate(dict.fromkeys(shapes))]
    return out + ATTN_SPECIAL


def attn_inputs(case):
    """-> q [n, L, H, 16], k, v [n, S, H, 16], go [n, L, H, 16], fp32"""
    C, L, S, nimg, _, kind = case
    H = C // 16
    g = gen("attn", case)
    q, go = torch.randn((nimg, L, H, 16), generator=g), torch.randn((nimg, L, H, 16), generator=g)
    k, v = torch.randn((nimg, S, H, 16), generator=g), torch.randn((nimg, S, H, 16), generator=g)
    if kind == "kneg":            # phi underflows towards 0, den tends to eps
        k = -4 - 8 * torch.rand((nimg, S, H, 16), generator=g)
    if kind == "qzero":           # phi' = phi = 1 at x = +-0.0
        q[:, L // 2, :, 0::2] = 0.0
        q[:, L // 2, :, 1::2] = -0.0
    if kind == "exact":           # phi(k) = k + 1 and v / S are exact: the kv block is a sum of integers
        k = torch.randint(1, 5, (nimg, S, H, 16), generator=g).float()
        v = torch.randint(-4, 5, (nimg, S, H, 16), generator=g).float() * S
    return q, k, v, go


def _kvsplit(kv, n, H):
    kv = kv.reshape(n, H, KVW)
    return kv[..., :256].reshape(n, H, 16, 16), kv[..., 256:]


def attn_fwd_ref(q, k, v, eps=LA_EPS):
    """-> {kv [n, H, 272], out [n, L, H, 16]: (ref64, bound)}, E = E_PHI:
      M = sum_s phi(k) (v / S): phi E, v / S and the product 2 u, the sum gam(S) -> eM = (gam(S + 2) + E) sum |terms|; eks = (gam(S) + E) ks
      z = Q . ks (positive terms): ez = Q . eks + (gam(16) + E) z;  den = z + eps: rden = (ez + u den) / den;  scale = S / den: + u
      s = Q . M[:, v]: es = Q . eM + (gam(16) + E) Q . |M|;  out = s scale: es scale + |out| (rden + 2 u)"""
    q, k, v = q.double(), k.double(), v.double()
    n, L, H, _ = q.shape
    S = k.shape[1]
    Q, K, V = phi64(q), phi64(k), v / S
    M, aM = torch.einsum("nshd,nshv->nhdv", K, V), torch.einsum("nshd,nshv->nhdv", K, V.abs())
    ks = K.sum(1)
    eM, eks = (gam(S + 2) + E_PHI) * aM * SLACK, (gam(S) + E_PHI) * ks * SLACK
    z = torch.einsum("nlhd,nhd->nlh", Q, ks)
    den = z + eps
    rden = (torch.einsum("nlhd,nhd->nlh", Q, eks) + (gam(16) + E_PHI) * z + U * den) / den
    scale = (S / den)[..., None]
    out = torch.einsum("nlhd,nhdv->nlhv", Q, M) * scale
    es = torch.einsum("nlhd,nhdv->nlhv", Q, eM) + (gam(16) + E_PHI) * torch.einsum("nlhd,nhdv->nlhv", Q, M.abs())
    eout = (es * scale + out.abs() * (rden[..., None] + 2 * U)) * SLACK
    return dict(kv=(torch.cat([M.reshape(n, H, 256), ks], -1), torch.cat([eM.reshape(n, H, 256), eks], -1)), out=(out, eout))


def attn_bwd_ref(q, k, v, kv32, go, eps=LA_EPS):
    """the backward on M | ks AS PASSED (kv32, fp32) -> {gq, gk, gv, gkv: (ref64, bound)}, E = E_PHI, all first order x SLACK:
      den: rden = (gam(16) + E) z / den + u;  out recomputed: eo = (gam(16) + E) (Q . |M|) scale + |out| (rden + 2 u)
      dot = gO . out: edot = |gO| . eo + gam(16) sum |gO out|;  gnum = gO S / den: egn = |gnum| (rden + 2 u)
      gden = -dot / den: egden = edot / den + |gden| (rden + u)
      gQ = (gden ks + gnum . M) phi': ea = egden ks + egn . |M| + gam(17) (|gden| ks + |gnum| . |M|);  egq = ea phi' + |gQ| (E + u)
      gM = sum_l Q gnum: Q . egn + (gam(L + 2) + E) sum |Q gnum|;  gks = sum_l Q gden: Q . egden + (gam(L + 2) + E) sum |Q gden|
      gK = (gks + V . gM) phi': eb = egks + |V| . egM + (gam(17) + u) (|gks| + |V| . |gM|);  egk = eb phi' + |gK| (E + u)
      gV = (K . gM) / S: (K . egM + (gam(16) + E) K . |gM|) / S + u |gV|"""
    q, k, v, go = q.double(), k.double(), v.double(), go.double()
    n, L, H, _ = q.shape
    S = k.shape[1]
    M, ks = _kvsplit(kv32.double(), n, H)
    Q, K, V = phi64(q), phi64(k), v / S
    ksb = ks[:, None]
    z = torch.einsum("nlhd,nhd->nlh", Q, ks)
    den = z + eps
    rden = (gam(16) + E_PHI) * z / den + U
    scale = (S / den)[..., None]
    out = torch.einsum("nlhd,nhdv->nlhv", Q, M) * scale
    eo = (gam(16) + E_PHI) * torch.einsum("nlhd,nhdv->nlhv", Q, M.abs()) * scale + out.abs() * (rden[..., None] + 2 * U)
    dot = (go * out).sum(-1)
    edot = (go.abs() * eo).sum(-1) + gam(16) * (go * out).abs().sum(-1)
    gn = go * scale
    egn = gn.abs() * (rden[..., None] + 2 * U)
    gden = -dot / den
    egden = edot / den + gden.abs() * (rden + U)
    a = torch.einsum("nlhv,nhdv->nlhd", gn, M) + gden[..., None] * ksb
    ea = (egden[..., None] * ksb + torch.einsum("nlhv,nhdv->nlhd", egn, M.abs()) +
          gam(17) * (gden.abs()[..., None] * ksb + torch.einsum("nlhv,nhdv->nlhd", gn.abs(), M.abs())))
    dq = torch.where(q > 0, torch.ones_like(Q), Q)
    gq = a * dq
    egq = (ea * dq + gq.abs() * (E_PHI + U)) * SLACK
    gM = torch.einsum("nlhd,nlhv->nhdv", Q, gn)
    egM = (torch.einsum("nlhd,nlhv->nhdv", Q, egn) + (gam(L + 2) + E_PHI) * torch.einsum("nlhd,nlhv->nhdv", Q, gn.abs())) * SLACK
    gks = torch.einsum("nlhd,nlh->nhd", Q, gden)
    egks = (torch.einsum("nlhd,nlh->nhd", Q, egden) + (gam(L + 2) + E_PHI) * torch.einsum("nlhd,nlh->nhd", Q, gden.abs())) * SLACK
    b = torch.einsum("nshv,nhdv->nshd", V, gM) + gks[:, None]
    eb = (torch.einsum("nshv,nhdv->nshd", V.abs(), egM) + egks[:, None] +
          (gam(17) + U) * (torch.einsum("nshv,nhdv->nshd", V.abs(), gM.abs()) + gks.abs()[:, None]))
    dk = torch.where(k > 0, torch.ones_like(K), K)
    gk = b * dk
    egk = (eb * dk + gk.abs() * (E_PHI + U)) * SLACK
    gv = torch.einsum("nshd,nhdv->nshv", K, gM) / S
    egv = ((torch.einsum("nshd,nhdv->nshv", K, egM) + (gam(16) + E_PHI) * torch.einsum("nshd,nhdv->nshv", K, gM.abs())) / S +
           U * gv.abs()) * SLACK
    return dict(gq=(gq, egq), gk=(gk, egk), gv=(gv, egv),
                gkv=(torch.cat([gM.reshape(n, H, 256), gks], -1), torch.cat([egM.reshape(n, H, 256), egks], -1)))


def toksum32(t, order, skip=None):
    """[n, T, ...] -> the sum over the tokens in fp32; order 0: one token after the other; 1: chunks of KV_CHUNK, within a chunk
    wave b sums tokens b, b + 4, ..., the four partials added as ((0 + 1) + 2) + 3, the chunks in order.  skip: a token left out."""
    def chain(x):
        acc = torch.zeros(x.shape[:1] + x.shape[2:])
        for i in range(x.shape[1]):
            acc = acc + x[:, i]
        return acc
    if skip is not None:
        t = torch.cat([t[:, :skip], t[:, skip + 1:]], 1)
    if order == 0:
        return chain(t)
    total = torch.zeros(t.shape[:1] + t.shape[2:])
    for c0 in range(0, t.shape[1], KV_CHUNK):
        ch = t[:, c0:c0 + KV_CHUNK]
        w = [chain(ch[:, b::4]) for b in range(4)]
        total = total + (((w[0] + w[1]) + w[2]) + w[3])
    return total


def phi32(x):
    return torch.where(x > 0, x + 1.0, x.clamp_max(0.0).exp())


def attn32(q, k, v, go, kv32=None, eps=LA_EPS, order=0, mutant=None):
    """-> dict(kv, out, gq, gk, gv, gkv) in fp32; the backward on kv32 when given (as the kernel gets it), else on its own kv"""
    n, L, H, _ = q.shape
    S = k.shape[1]
    eps = torch.tensor(eps, dtype=torch.float32)
    Q, K = phi32(q), phi32(k)
    V = v / float(L if mutant == "v_over_L" else S)
    skip = 64 if mutant == "tok64" and S == 65 else None
    M = toksum32(K[..., :, None] * V[..., None, :], order, skip)           # [n, H, 16, 16]
    ks = toksum32(K, order, skip)
    kv = torch.cat([M.reshape(n, H, 256), ks], -1)

    def apply(M, ks, num):
        if mutant == "head0" and H == 3:      # head H - 1 computed with head 0's block
            M, ks = M.clone(), ks.clone()
            M[:, 2], ks[:, 2] = M[:, 0], ks[:, 0]
        den = torch.einsum("nlhd,nhd->nlh", Q, ks) + eps
        return torch.einsum("nlhd,nhdv->nlhv", Q, M) * (float(num) / den)[..., None], den

    out, _ = apply(M, ks, L if mutant == "scale_L" else S)
    if kv32 is not None:
        M, ks = _kvsplit(kv32, n, H)
    o2, den = apply(M, ks, S)
    gn = go * (float(S) / den)[..., None]
    gden = -(go * o2).sum(-1) / den
    dq = torch.ones_like(Q) if mutant == "dphi1" else torch.where(q > 0, torch.ones_like(Q), Q)
    gq = (torch.einsum("nlhv,nhdv->nlhd", gn, M) + gden[..., None] * ks[:, None]) * dq
    gM = toksum32(Q[..., :, None] * gn[..., None, :], order)
    gks = toksum32(Q * gden[..., None], order)
    dk = torch.ones_like(K) if mutant == "dphi1" else torch.where(k > 0, torch.ones_like(K), K)
    gk = (torch.einsum("nshv,nhdv->nshd", V, gM) + gks[:, None]) * dk
    gv = torch.einsum("nshd,nhdv->nshv", K, gM) / float(S)
    return dict(kv=kv, out=out, gq=gq, gk=gk, gv=gv, gkv=torch.cat([gM.reshape(n, H, 256), gks], -1))


def exp_probe_inputs(nimg=512):
    """k [nimg, 1, 8, 16] in [-16, 0] for the S = 1 shape at which kv[256 + d] = phi(k[d]) = expf(k[d])"""
    g = gen("exp_probe", nimg)
    k = -16.0 * torch.rand((nimg, 1, 8, 16), generator=g)
    k.view(-1)[:4096] = torch.linspace(-16.0, 0.0, 4096)
    return k
