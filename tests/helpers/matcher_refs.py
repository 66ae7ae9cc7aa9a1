"""References, input builders and the case lists of the matcher edge tests (tests/test_matcher_edges_cpu.py checks them here on
the CPU, tests/test_matcher_edges_gpu.py runs the kernels against them; for the backward, at the end of the file,
tests/test_matcher_grad_edges_cpu.py and tests/test_matcher_grad_edges_gpu.py).  Pure torch on the CPU.

The references are the project's oracle on .double() inputs; the error scale of a case is the SAME oracle run in fp32 against that
(floor32), i.e. a property of the reference and the inputs alone."""
import functools
import zlib

import torch
import torch.nn.functional as F

from oracle import mickey_oracle as O

TINY = 1e-30          # elements of the fp64 reference below this are compared absolutely (<= 2 TINY), everything else relatively
TEMPERATURE = 0.1
SPACING = 2.0 ** -20  # the spacing of a logit v2 in [8, 16): keeps degenerate cases (1 x 1) from demanding exactness
FACTOR = 4.0          # tolerance = FACTOR * max(floor32, SPACING)

# ---- the case lists (shared, so that the CPU tests cover exactly what the GPU tests run) --------------------------------------
DS_SHAPES = [(1, 1), (1, 40), (40, 1), (31, 33), (32, 32), (33, 31), (64, 96), (127, 130), (129, 65), (130, 257), (257, 132)]
DS_B9_SHAPES = [(33, 31), (129, 65)]
DS_SMALL_C = [2, 64, 126]
DS_HOT_SHAPES = [(64, 96), (127, 130), (130, 257), (257, 132)]
DS_MISALIGNED_SHAPES = [(32, 32), (129, 64)]
DUSTBINS = [None, 0.7, 8.0]
SK_SHAPES = [(1, 1), (1, 40), (40, 1), (6, 2), (7, 3), (8, 4), (62, 63), (63, 64), (64, 65), (254, 130), (255, 131), (256, 66), (300, 513)]
SK_C32_SHAPES = [(7, 3), (63, 64)]   # (at C = 32 cosines spread twice as far: larger shapes of the wide family fall below TINY)
SK_PARAMS = [(1.3, 10), (1.0, 0), (-2.0, 3), (6.0, 10)]   # (alpha, iters)
MNN_SHAPES = [(2, 2), (2, 70), (5, 3), (16, 16), (65, 66), (130, 257), (257, 130), (1024, 40), (1025, 40), (2049, 17)]
MNN_BATCHES = [1, 3, 9]
MNN_LIMIT_CASES = [(2, 8200, 3), (1, 16384, 3)]           # (B, n0, n1): past 64 KiB of sort keys, and the documented maximum
HOT_KEYPOINTS = (0, 31, 32)                                # + m - 1: first / last lane of a 32-tile, the first of the next
HOT_SCALE = 3.2                                            # S = 10.24 on a duplicate: v2 = 10.24 / T * log2(e) = 147.7 at T = 0.1
MNN_LEVELS = (1.25, 1.5, 1.75, 2.0, 2.25)


def gen(case, B, n0, n1, extra=0):
    """A generator seeded from (case, B, n0, n1)."""
    return torch.Generator().manual_seed(zlib.crc32(repr((case, B, n0, n1, extra)).encode()))


# ---- descriptors ---------------------------------------------------------------------------------------------------------------
def unit_descriptors(B, C, n0, n1, pull=2.0, case="unit"):
    """L2-normalised [B, C, n0], [B, C, n1]; keypoint k < min(n0, n1) of image 1 is a near-duplicate of keypoint k of image 0."""
    g = gen(case, B, n0, n1, C)
    m = min(n0, n1)
    d0 = F.normalize(torch.randn((B, C, n0), generator=g), dim=1)
    d1 = torch.randn((B, C, n1), generator=g)
    d1[:, :, :m] += pull * d0[:, :, :m]
    return d0, F.normalize(d1, dim=1)


def hot_keypoints(n0, n1):
    m = min(n0, n1)
    return sorted({k for k in HOT_KEYPOINTS + (m - 1,) if 0 <= k < m})


def hot_descriptors(B, C, n0, n1):
    """The unit set with a few keypoints made EXACT duplicates across the two images and scaled by 3.2 in both: their logit is
    10.24 / T, past what a sum of 2^v2 without a running maximum can hold at T = 0.1."""
    d0, d1 = unit_descriptors(B, C, n0, n1)
    for k in hot_keypoints(n0, n1):
        d1[:, :, k] = d0[:, :, k]
        d0[:, :, k] *= HOT_SCALE
        d1[:, :, k] *= HOT_SCALE
    return d0, d1


def wide_descriptors(B, C, n0, n1):
    """The unit set (pull 1) scaled so that S / sqrt(C) = 64 cos: Sinkhorn outputs over many decades instead of flat to 7 %."""
    d0, d1 = unit_descriptors(B, C, n0, n1, pull=1.0, case="wide")
    s = 8.0 * C ** 0.25
    return d0 * s, d1 * s


def descriptors(family, B, C, n0, n1):
    return {"unit": unit_descriptors, "hot": hot_descriptors, "wide": wide_descriptors}[family](B, C, n0, n1)


def keypoint_scores(B, n0, n1):
    """scr0 [B, 1, n0], scr1 [B, 1, n1] in [0.25, 1)"""
    g = gen("scr", B, n0, n1)
    return 0.25 + 0.75 * torch.rand((B, 1, n0), generator=g), 0.25 + 0.75 * torch.rand((B, 1, n1), generator=g)


# ---- references ----------------------------------------------------------------------------------------------------------------
def dual_softmax64(d0, d1, dustbin, temperature=TEMPERATURE):
    return O.dual_softmax(d0.double(), d1.double(), dustbin, temperature)


def sinkhorn64(d0, d1, alpha, iters):
    return O.sinkhorn(d0.double(), d1.double(), alpha, iters, descriptor_dim=d0.shape[1])


def sinkhorn_uv64(d0, d1, alpha, iters):
    """The iterates u [B, n0 + 1], v [B, n1 + 1] (natural log) that O.sinkhorn ends with, and its result from them
    (test_matcher_edges_cpu.py asserts that this equals O.sinkhorn bit for bit)."""
    d0, d1 = d0.double(), d1.double()
    S = torch.einsum("bdn,bdm->bnm", d0, d1) / d0.shape[1] ** 0.5
    b, m, n = S.shape
    a = torch.as_tensor(alpha, dtype=S.dtype)
    Z = torch.cat([torch.cat([S, a.expand(b, m, 1)], -1), torch.cat([a.expand(b, 1, n), a.expand(b, 1, 1)], -1)], 1)
    ms, ns = torch.tensor(float(m)), torch.tensor(float(n))
    norm = -(ms + ns).log()
    log_mu = torch.cat([norm.expand(m), ns.log()[None] + norm])[None].expand(b, -1).double()
    log_nu = torch.cat([norm.expand(n), ms.log()[None] + norm])[None].expand(b, -1).double()
    u, v = torch.zeros_like(log_mu), torch.zeros_like(log_nu)
    for _ in range(iters):
        u = log_mu - torch.logsumexp(Z + v.unsqueeze(1), dim=2)
        v = log_nu - torch.logsumexp(Z + u.unsqueeze(2), dim=1)
    return u, v, (Z + u.unsqueeze(2) + v.unsqueeze(1) - norm).exp()[:, :-1, :-1]


def floor32(p32, p64):
    """The fp32 oracle's own error: max |p32 - p64| / p64 over the elements that are compared relatively (p64 >= TINY)."""
    big = p64 >= TINY
    if not bool(big.any()):
        return 0.0
    return float(((p32.double() - p64).abs() / p64.clamp_min(TINY))[big].max())


def tolerance(floor):
    return FACTOR * max(floor, SPACING)


@functools.lru_cache(maxsize=None)
def dual_softmax_case(family, B, C, n0, n1, dustbin):
    """-> dict: d0, d1, s0, s1 (fp32), P64, kp32 (what the kernels must return bit for bit), F64 = P64 * kp64, floor (scores),
    floor_final.  Cached: treat as read-only."""
    d0, d1 = descriptors(family, B, C, n0, n1)
    s0, s1 = keypoint_scores(B, n0, n1)
    P64 = dual_softmax64(d0, d1, dustbin)
    P32 = O.dual_softmax(d0, d1, dustbin, TEMPERATURE)
    kp32 = torch.matmul(s0.transpose(2, 1), s1)
    kp64 = torch.matmul(s0.double().transpose(2, 1), s1.double())
    F64 = P64 * kp64
    v2max = float((torch.matmul(d0.double().transpose(1, 2), d1.double()) / TEMPERATURE).max()) * 1.4426950408889634
    return dict(d0=d0, d1=d1, s0=s0, s1=s1, P64=P64, P32=P32, kp32=kp32, F64=F64, floor=floor32(P32, P64),
                floor_final=floor32(P32 * kp32, F64), v2max=v2max)


@functools.lru_cache(maxsize=None)
def sinkhorn_case(family, B, C, n0, n1, alpha, iters):
    """-> dict as dual_softmax_case, plus the fp64 iterates u64 [B, n0 + 1], v64 [B, n1 + 1] (natural log)."""
    d0, d1 = descriptors(family, B, C, n0, n1)
    s0, s1 = keypoint_scores(B, n0, n1)
    u64, v64, P64 = sinkhorn_uv64(d0, d1, alpha, iters)
    P32 = O.sinkhorn(d0, d1, alpha, iters, descriptor_dim=C)
    kp32 = torch.matmul(s0.transpose(2, 1), s1)
    kp64 = torch.matmul(s0.double().transpose(2, 1), s1.double())
    F64 = P64 * kp64
    return dict(d0=d0, d1=d1, s0=s0, s1=s1, P64=P64, P32=P32, kp32=kp32, F64=F64, u64=u64, v64=v64, floor=floor32(P32, P64),
                floor_final=floor32(P32 * kp32, F64))


def dual_softmax_cases():
    """Every (family, B, C, n0, n1, dustbin, split) the GPU tests run through the element-wise metric."""
    out = []
    for split in (False, True):
        for n0, n1 in DS_SHAPES:
            for db in DUSTBINS:
                out.append(("unit", 2, 128, n0, n1, db, split))
        for n0, n1 in DS_B9_SHAPES:
            out.append(("unit", 9, 128, n0, n1, 0.7, split))
    for n0, n1 in DS_HOT_SHAPES:
        for db in DUSTBINS:
            out.append(("hot", 2, 128, n0, n1, db, False))
    for C in DS_SMALL_C:
        for n0, n1 in DS_B9_SHAPES:
            out.append(("unit", 2, C, n0, n1, 8.0, False))
    return out


def sinkhorn_cases():
    """Every (family, B, C, n0, n1, alpha, iters) the GPU tests run."""
    out = []
    for n0, n1 in SK_SHAPES:
        for C in (128, 32) if (n0, n1) in SK_C32_SHAPES else (128,):
            for family in ("unit", "wide"):
                for alpha, iters in SK_PARAMS:
                    out.append((family, 2, C, n0, n1, alpha, iters))
    return out


# ---- mutual nearest neighbours -----------------------------------------------------------------------------------------------
def mutual_nn_ref(scores):
    """Batched, deterministic get_matches_list on scores[b, :-1, :-1] (min_conf = 0): the FIRST maximal index wins either arg-max
    (torch.max on the CPU: asserted in test_matcher_edges_cpu.py), a row is kept when carg[rarg[i]] == i and exp(v) > 0, matches
    are ordered by score, descending, equal scores by ascending row.  -> list of int64 [m_b, 2]."""
    out = []
    for b in range(scores.shape[0]):
        sub = scores[b, :-1, :-1]
        if sub.numel() == 0:
            out.append(torch.zeros((0, 2), dtype=torch.int64))
            continue
        rval, rarg = sub.max(1)
        carg = sub.max(0).indices
        rows = torch.arange(sub.shape[0])
        keep = (carg[rarg] == rows) & (rval.exp() > 0)
        i0, i1, v = rows[keep], rarg[keep], rval[keep]
        order = torch.sort(v, descending=True, stable=True).indices
        out.append(torch.stack([i0, i1], 1)[order])
    return out


def mutual_nn_scores(B, n0, n1, plants=True):
    """Continuous random scores in (0, 1) and, with `plants`, everything that makes mutual-NN go wrong (see the module docstring
    of test_matcher_edges_gpu.py): -> (scores [B, n0, n1], info per pair).  info[b]: planted [(row, column)], dup_cols
    [(row, column, later column)], dup_rows [(row, later row, column)], inf_row, lastcol_row, lastrow_col (None where the shape
    has no room)."""
    g = gen("mnn", B, n0, n1)
    sc = torch.rand((B, n0, n1), generator=g).clamp_min(1e-6)
    info = []
    m = min(n0, n1)
    k = m // 2 if (plants and m >= 4) else 0          # half of the min(n0, n1) - 1 usable rows, rounded up
    for b in range(B):
        rows = torch.randperm(n0 - 1, generator=g)[:k].tolist()
        cols = torch.randperm(n1 - 1, generator=g)[:k].tolist()
        lev = torch.randint(0, len(MNN_LEVELS), (k,), generator=g).tolist()
        for r, c, l in zip(rows, cols, lev):
            sc[b, r, c] = MNN_LEVELS[l]
        d = dict(planted=list(zip(rows, cols)), dup_cols=[], dup_rows=[], inf_row=None, lastcol_row=None, lastrow_col=None)
        info.append(d)
        if m < 16 or not plants:
            continue
        free_r = [r for r in range(n0 - 1) if r not in set(rows)]
        free_c = [c for c in range(n1 - 1) if c not in set(cols)]
        used = set()
        # a later column that repeats column c in the row of its maximum (and in a few more rows): the row maximum is attained twice
        for r, c in zip(rows, cols):
            later = [x for x in free_c if x > c]
            if len(d["dup_cols"]) == 3 or not later:
                continue
            c2 = later[int(torch.randint(0, len(later), (1,), generator=g))]
            free_c.remove(c2)
            more = torch.randperm(n0 - 1, generator=g)[:4].tolist()
            for rr in set(more + [r]):
                if rr == r or rr in free_r:
                    sc[b, rr, c2] = sc[b, rr, c]
            d["dup_cols"].append((r, c, c2))
            used.add(r)
        # the same for rows: the column maximum is attained twice
        for r, c in zip(rows, cols):
            later = [x for x in free_r if x > r]
            if len(d["dup_rows"]) == 3 or not later or r in used:
                continue
            r2 = later[int(torch.randint(0, len(later), (1,), generator=g))]
            free_r.remove(r2)
            more = torch.randperm(n1 - 1, generator=g)[:4].tolist()
            for cc in set(more + [c]):
                if cc == c or cc in free_c:
                    sc[b, r2, cc] = sc[b, r, cc]
            d["dup_rows"].append((r, r2, c))
            used.add(r)
        rest = [(r, c) for r, c in zip(rows, cols) if r not in used]
        if free_r:
            d["inf_row"] = free_r[-1]
            sc[b, free_r[-1], :] = float("-inf")        # no match: the row arg-max finds nothing
        if len(rest) >= 1:
            d["lastcol_row"] = rest[0][0]
            sc[b, rest[0][0], n1 - 1] = 3.0            # the row's global maximum sits in the excluded last column
        if len(rest) >= 2:
            d["lastrow_col"] = rest[1][1]
            sc[b, n0 - 1, rest[1][1]] = 3.0            # the column's maximum sits in the excluded last row
    return sc, info


# ---- the matcher's backward (tests/test_matcher_grad_edges_cpu.py, tests/test_matcher_grad_edges_gpu.py) ------------------------
LOG2E = 1.4426950408889634
GRAD_KINDS = ("dsc0", "dsc1", "scr0", "scr1", "dustbin")
GRAD_SHAPES = [(1, 1), (1, 40), (40, 1), (31, 33), (32, 32), (33, 31), (64, 96), (128, 128), (127, 130), (129, 65), (65, 129),
               (130, 257), (257, 132), (96, 545), (545, 96)]
GRAD_SPARSE_SHAPES = [(33, 31), (129, 65), (130, 257)]
GRAD_CHAIN_SHAPES = [(33, 31), (129, 65), (257, 132)]
GRAD_DIRTY_SHAPES = [(129, 65), (65, 129)]
GRAD_BATCHES = [1, 8, 9]
GRAD_SUBSETS = [(True, False, False, False, False), (False, True, False, False, False), (False, False, True, True, False),
                (False, False, False, False, True)]   # which of GRAD_KINDS a call asks for
ZERO_SCORE_KEYPOINTS = (0, 31, 32)                   # + n - 1: border keypoints, whose score is exactly 0


def grad_scores(B, n0, n1):
    """keypoint_scores as [B, n0], [B, n1] with exact zeros at indices 0, 31, 32 and n - 1 of either side where they exist (border
    keypoints: their score gradient is not zero).  A side of fewer than 3 keypoints keeps its scores: planted there, no score of
    the side would be left, the other side's score gradient and its magnitude sum would vanish and the comparison say nothing."""
    s0, s1 = keypoint_scores(B, n0, n1)
    out = []
    for s, n in ((s0, n0), (s1, n1)):
        s = s.reshape(B, n).clone()
        if n >= 3:
            for k in ZERO_SCORE_KEYPOINTS + (n - 1,):
                if k < n:
                    s[:, k] = 0.0
        out.append(s)
    return out


def ref_final(d0, d1, s0, s1, dustbin, temperature=TEMPERATURE):
    """the reference formula, dualSoftmax x kp_matrix_scores, in the dtype it is given; s0 [B, n0], s1 [B, n1] or None"""
    S = torch.matmul(d0.transpose(1, 2), d1) / temperature
    if dustbin is not None:
        B, m, n = S.shape
        a = dustbin.reshape(())
        Z = torch.cat([torch.cat([S, a.expand(B, m, 1)], -1), torch.cat([a.expand(B, 1, n), a.expand(B, 1, 1)], -1)], 1)
        P = (torch.softmax(Z, 1) * torch.softmax(Z, 2))[:, :-1, :-1]
    else:
        P = torch.softmax(S, 1) * torch.softmax(S, 2)
    return P if s0 is None else P * (s0[:, :, None] * s1[:, None, :])


def formula_grads(d0, d1, s0, s1, dustbin, temperature, G):
    """What mk_dual_softmax_bwd computes (its header comment), written out in torch in the dtype of the inputs: two sweeps over G,
    no division by s.  s0 / s1: [B, n0] / [B, n1] (or [B, 1, n]) or None; dustbin: a one-element tensor or None.
    -> dict  g: [g_dsc0 [B, C, n0], g_dsc1 [B, C, n1], g_scr0, g_scr1 (shaped as s0 / s1; None without scores), g_dustbin [B] PER
                PAIR (None without a dustbin)]
             M: the same five expressions with every term replaced by its absolute value -- the scale an fp32 evaluation errs on:
                Mu = sum_j |G P| s1, Mv = sum_i |G P| s0, MdS = |2 G s0 s1 P| + A s0 Mu + Bm s1 Mv, M0 = |dsc1| MdS^T / T,
                M1 = |dsc0| MdS / T, Ma = sum_i exp(a - lr_i) s0 Mu + sum_j exp(a - lc_j) s1 Mv
             lse2: [B, 2, max(n0, n1)], the row (side 0) and column (side 1) log-sums of the augmented matrix times log2(e): the
                layout of ops.dual_softmax_train_fwd; slots [side, n ..) are 0."""
    B, _, n0 = d0.shape
    n1 = d1.shape[2]
    S = torch.matmul(d0.transpose(1, 2), d1) / temperature
    if dustbin is not None:
        a = dustbin.reshape(())
        Z = torch.cat([torch.cat([S, a.expand(B, n0, 1)], -1), torch.cat([a.expand(B, 1, n1), a.expand(B, 1, 1)], -1)], 1)
        lr, lc = torch.logsumexp(Z, 2)[:, :-1], torch.logsumexp(Z, 1)[:, :-1]
    else:
        lr, lc = torch.logsumexp(S, 2), torch.logsumexp(S, 1)
    A, Bm = torch.exp(S - lr[:, :, None]), torch.exp(S - lc[:, None, :])
    P = A * Bm
    s0v = s0.reshape(B, n0) if s0 is not None else torch.ones((B, n0), dtype=d0.dtype)
    s1v = s1.reshape(B, n1) if s1 is not None else torch.ones((B, n1), dtype=d0.dtype)
    W = G * P
    u, v = (W * s1v[:, None, :]).sum(2), (W * s0v[:, :, None]).sum(1)   # sweep 1
    r, c = s0v * u, s1v * v
    kp = s0v[:, :, None] * s1v[:, None, :]
    dS = 2 * G * kp * P - A * r[:, :, None] - Bm * c[:, None, :]   # sweep 2
    g0, g1 = torch.matmul(d1, dS.transpose(1, 2)) / temperature, torch.matmul(d0, dS) / temperature
    aW, a0, a1 = W.abs(), s0v.abs(), s1v.abs()
    Mu, Mv = (aW * a1[:, None, :]).sum(2), (aW * a0[:, :, None]).sum(1)
    Mr, Mc = a0 * Mu, a1 * Mv
    MdS = (2 * G * kp * P).abs() + A * Mr[:, :, None] + Bm * Mc[:, None, :]
    M0, M1 = torch.matmul(d1.abs(), MdS.transpose(1, 2)) / temperature, torch.matmul(d0.abs(), MdS) / temperature
    ga = Ma = None
    if dustbin is not None:
        er, ec = torch.exp(a - lr), torch.exp(a - lc)
        ga = -(er * r).sum(1) - (ec * c).sum(1)
        Ma = (er * Mr).sum(1) + (ec * Mc).sum(1)
    lse2 = torch.zeros((B, 2, max(n0, n1)), dtype=d0.dtype)
    lse2[:, 0, :n0], lse2[:, 1, :n1] = lr * LOG2E, lc * LOG2E
    has = s0 is not None
    return dict(g=[g0, g1, u.reshape(s0.shape) if has else None, v.reshape(s1.shape) if has else None, ga],
                M=[M0, M1, Mu.reshape(s0.shape) if has else None, Mv.reshape(s1.shape) if has else None, Ma], lse2=lse2)


def floor32g(g32, g64, M):
    """The fp32 formula's own error in the backward's metric: max |g32 - g64| / M over the elements with M >= TINY.  Below that
    (the hot family: the score gradient of a planted duplicate whose partner's score is 0 sums terms of 1e-43, denormal in fp32)
    an element is compared absolutely, by the 2 TINY of the pass criterion |got - g64| <= tol M + 2 TINY, as the forward's floor32
    leaves elements below TINY to its absolute bound."""
    pos = M >= TINY
    if not bool(pos.any()):
        return 0.0
    return float(((g32.double() - g64).abs()[pos] / M[pos]).max())


def lse_term(d):
    """What a backward that is fed log-sums off by at most d (log2 domain; d = max |lse - lse64| of the lse it is given, measured
    against the fp64 reference: a property of the backward's INPUT) may add to the relative tolerance: a shift d of a log-sum
    scales A = 2^(v - lr) or Bm = 2^(v - lc) by 2^+-d = 1 +- ln2 d, and every term of u, v, dS and the dustbin sum holds at most one
    A and one Bm: 2 ln2 d of M.  Used where the backward is given the forward kernel's own lse: test_chain_forward_lse, and the
    hot family.  The hot family cannot be fed the fp64 log-sums rounded to fp32: its planted duplicates have log2-domain logits
    v = 147.7, where fp32 values are 2^-16 = 1.5e-5 apart and the 128-term fp32 dot product behind v is off by a few of those;
    P = 2^((v - lc) + (v - lr)) is then off by ln2 x twice that, 1e-4 (measured on g_scr0 / g_scr1 at keypoint min(n0, n1) - 1, the
    one planted duplicate whose partner's score is not 0: tile positions 31, 1 and 3 at the three shapes; 56 x the fp32 formula's
    floor, which does not see it because its log-sums come from its own logits).  The forward kernel's log-sums come from the same
    correlation as the backward's v, the rounding cancels as it does in the fp32 formula and in training, and their own distance
    from the fp64 log-sums is what this term covers."""
    return 2.0 * 0.6931471805599453 * d


def grad_G(kind, B, n0, n1, F64):
    """G = dL / d final_scores, fp32 [B, n0, n1].  dense: randn.  sparse: about 5 % of the cells non-zero, divided by
    F64 + 1e-16 as the trainer's REINFORCE gradient is (backward of log(final + 1e-16))."""
    g = gen("G", B, n0, n1, kind)
    G = torch.randn((B, n0, n1), generator=g, dtype=torch.float64)
    if kind == "sparse":
        G = G * (torch.rand((B, n0, n1), generator=g) < 0.05) / (F64 + 1e-16)
    return G.float()


@functools.lru_cache(maxsize=None)
def grad_case(family, B, n0, n1, dustbin, gkind, scores=True):
    """One case of the backward's tests at C = 128, T = TEMPERATURE.  -> dict: d0, d1 [B, 128, n], s0, s1 [B, n] (None without
    scores), G [B, n0, n1], db (one-element fp32 tensor or None) -- the fp32 inputs of the kernels; g64, M: formula_grads on their
    .double(); lse64 [B, 2, nmax] (log2 domain, fp64); floor: per output kind floor32g of formula_grads run in fp32 on the same
    inputs (None where the output does not exist); floor_lse: max |fp32 torch.logsumexp x log2(e), rounded to fp32, - lse64| over
    the slots in use.  Cached: treat as read-only."""
    d0, d1 = descriptors(family, B, 128, n0, n1)
    s0, s1 = grad_scores(B, n0, n1) if scores else (None, None)
    db = torch.tensor([dustbin], dtype=torch.float32) if dustbin is not None else None
    dd = [t.double() if t is not None else None for t in (d0, d1, s0, s1, db)]
    F64 = ref_final(*dd, TEMPERATURE)
    G = grad_G(gkind, B, n0, n1, F64)
    r64 = formula_grads(*dd, TEMPERATURE, G.double())
    r32 = formula_grads(d0, d1, s0, s1, db, TEMPERATURE, G)
    floor = [None if g is None else floor32g(h, g, M) for h, g, M in zip(r32["g"], r64["g"], r64["M"])]
    used = torch.zeros((B, 2, max(n0, n1)), dtype=torch.bool)
    used[:, 0, :n0], used[:, 1, :n1] = True, True
    floor_lse = float((r32["lse2"].double() - r64["lse2"]).abs()[used].max())
    return dict(d0=d0, d1=d1, s0=s0, s1=s1, G=G, db=db, g64=r64["g"], M=r64["M"], lse64=r64["lse2"], floor=floor,
                floor_lse=floor_lse, used=used)


def grad_cases():
    """test name of tests/test_matcher_grad_edges_gpu.py -> the list that test is parametrised over."""
    paths = (False, True)
    return {
        # (n0, n1, split, dustbin): B = 2, unit family, dense G, with scores (and once more without)
        "test_backward_elementwise": [(n0, n1, sp, db) for n0, n1 in GRAD_SHAPES for sp in paths for db in DUSTBINS],
        # (family, gkind, n0, n1, split): every dustbin of DUSTBINS inside the test
        "test_backward_sparse_G_and_hot": [("unit", "sparse", n0, n1, sp) for n0, n1 in GRAD_SPARSE_SHAPES for sp in paths]
        + [("hot", "dense", n0, n1, False) for n0, n1 in DS_HOT_SHAPES],
        "test_lse_elementwise": [(n0, n1, sp, db) for n0, n1 in GRAD_SHAPES for sp in paths for db in DUSTBINS],
        "test_chain_forward_lse": [(n0, n1, sp) for n0, n1 in GRAD_CHAIN_SHAPES for sp in paths],
        "test_unused_lse_slots_and_dirty_work": [(n0, n1, sp) for n0, n1 in GRAD_DIRTY_SHAPES for sp in paths],
        "test_batches": [(B, n0, n1, sp) for B in GRAD_BATCHES for n0, n1 in DS_B9_SHAPES for sp in paths],
        "test_pair_isolation": [(3, 65, 129, sp) for sp in paths],
        "test_output_subsets": [(129, 65, sp) for sp in paths],
        "test_misaligned_outputs": [(n0, n1, sp) for n0, n1 in DS_MISALIGNED_SHAPES for sp in paths],
    }
