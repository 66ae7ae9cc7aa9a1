"""References, input builders, case tables, metrics and bounds of the pose-solver edge tests (tests/test_solver_edges_cpu.py checks
them on the CPU, tests/test_solver_edges_gpu.py runs the kernels of mk_solver.hip against them).  Pure torch on the CPU.

The references are the project's oracle (oracle/mickey_oracle.py, oracle/train_oracle.py) evaluated in fp64; the error scale of a
case (`floor32`) is the SAME oracle evaluated in fp32 on the same inputs, measured against that -- a property of the reference and
the inputs alone, never of a kernel.

Three levels of comparison:
  exact        indices, copies, masks, round counts, arg-max winners, REINFORCE sums, flags: compared as integers / bits.  A mask or
               a round count can only be exact when no residual sits on the threshold, so every refinement case keeps, in fp64, every
               residual of every round at least MARGIN = 16 x (the fp32 oracle's largest residual error on that case) away from it.
               The cases are chosen by seed (first_seed) so that this holds with NO element exempt.
  element-wise |got - ref64| / scale <= FACTOR x max(floor32, 2^-23) on every element, with `scale` per output:
                   R entries 1;  t max(1, |abar|, |bbar|);  X / Y  d (|Ki_a0 u| + |Ki_a1 v| + |Ki_a2|);
                   scores / confidences: the sum of their (positive) terms;  gather gradients: the fp64 sum of the absolute
                   contributions to that keypoint.
  conditioning every triple / masked set that is fitted has fp64 singular values s2 / s1 >= 0.1 (and s3 / s2 >= 0.1 where the fit has
               full rank): a property of the inputs, asserted on the CPU; no result is filtered afterwards.

FACTOR is 4 (the fp32 oracle and a kernel round in different places; two independent evaluations of that accuracy are within a small
multiple of each other) except for the back-projection, where the count is made below (BACKPROJECT_FACTOR)."""
import contextlib
import functools
import math
import zlib

import torch

from oracle import mickey_oracle as O
from oracle import train_oracle as TO

EPS32 = 2.0 ** -23
FACTOR = 4.0
# mk_gather_backproject inverts K by cofactors in fp32 and evaluates d (Ki_a0 u + Ki_a1 v + Ki_a2).  Roundings of half an ulp each,
# relative to the scale above (K upper triangular with positive focal lengths: no cancellation in det or in the cofactors beyond the
# 1.01 of the skew term): cofactor 2 products + 1 difference (3), det 3 cofactor products + 2 sums on top of their cofactors (3 + 5),
# the reciprocal (1), cofactor x reciprocal (1); then 2 products, 2 sums and the product with d (5): 18 half-ulps = 9 x 2^-23 when
# every rounding goes the same way.  The fp32 oracle (LAPACK inverse, matmul) measures 1 - 2 x 2^-23 here, so 4 x floor32 would ask a
# correct kernel for less than its worst case.
BACKPROJECT_FACTOR = 9.0
MARGIN_FACTOR = 16.0
COND = 0.1
TH_INLIER, TH_SOFT = 0.15, 0.3
CENTRE = (0.2, -0.1, 4.0)
SPREAD = (1.5, 1.0, 0.7)


def f32(x):
    """x rounded to fp32, as a Python float (what a kernel receives for a `float` argument)"""
    return float(torch.tensor(x, dtype=torch.float32))


@contextlib.contextmanager
def default_dtype(dtype):
    """The oracle allocates its constants (eye, ones) in the default dtype: fp64 references run under this."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


# ---- metric ------------------------------------------------------------------------------------------------------------------
def rel_err(x, ref, scale):
    """|x - ref| / scale per element in fp64 (inf where x is not finite)"""
    x = x.double().reshape(ref.shape)
    e = (x - ref).abs() / scale
    return torch.where(torch.isfinite(x), e, torch.full_like(e, float("inf")))


def floor32(x32, ref, scale):
    return float(rel_err(x32, ref, scale).max())


def bound(floor, factor=FACTOR):
    return factor * max(floor, EPS32)


def ratio(got, ref, scale, floor, factor=FACTOR):
    """-> (largest |got - ref| / scale / bound, flat index of that element)"""
    r = (rel_err(got, ref, scale) / bound(floor, factor)).reshape(-1)
    i = int(torch.argmax(r))
    return float(r[i]), i


def lane_slot(j):
    return "match %d (lane %d, slot %d; element %d of 256-block %d, of 512-block %d)" % (j, j % 64, j // 64, j % 256, j // 256, j // 512)


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def points(g, *shape):
    """[..., 3] fp32 of unit scale in front of a camera"""
    return torch.tensor(CENTRE) + torch.randn(shape + (3,), generator=g) * torch.tensor(SPREAD)


def rotation(g, size=0.3, mirror=False):
    """fp64 rotation of a few tenths of a radian (times diag(1, 1, -1) when mirrored)"""
    a = (torch.rand(3, generator=g, dtype=torch.float64) - 0.5) * 2 * size
    th = float(a.norm())
    k = a / th
    Kx = torch.tensor([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]], dtype=torch.float64)
    R = torch.eye(3, dtype=torch.float64) + math.sin(th) * Kx + (1 - math.cos(th)) * (Kx @ Kx)
    return R @ torch.diag(torch.tensor([1.0, 1.0, -1.0], dtype=torch.float64)) if mirror else R


def planted_set(g, k, outliers=0.3, noise=(0.005, 0.07)):
    """-> X, Y [k, 3] fp32, R [3, 3], t [3] fp64: Y = R X + t + graded noise (sigma noise[0] + noise[1] u^2 per match), a fraction
    `outliers` of the matches moved by N(0, 0.8); the order of the matches is random, so inliers sit in every lane and slot"""
    X = points(g, k)
    R = rotation(g)
    t = (torch.rand(3, generator=g, dtype=torch.float64) - 0.5) * 0.6
    sig = noise[0] + noise[1] * torch.rand(k, 1, generator=g, dtype=torch.float64) ** 2
    Y = X.double() @ R.T + t + sig * torch.randn(k, 3, generator=g, dtype=torch.float64)
    out = torch.rand(k, generator=g) < outliers
    Y[out] += 0.8 * torch.randn(int(out.sum()), 3, generator=g, dtype=torch.float64)
    return X, Y.float(), R, t


def perturbed(g, R, t, rot=0.03, trans=0.05):
    """a start pose near (R, t), rounded to fp32"""
    dR = rotation(g, rot)
    return (dR @ R).float(), (t + (torch.rand(3, generator=g, dtype=torch.float64) - 0.5) * 2 * trans).float()


# ---- rigid fits in a chosen precision: the oracle's arithmetic ----------------------------------------------------------------
def kabsch(A, B, w=None, dtype=torch.float64, reflection=True, centroid_by_count=False):
    """oracle kabsch on [M, n, 3] sets in `dtype` -> R [M, 3, 3], t [M, 1, 3], H.  The two switches make the subtly wrong variants the
    CPU tests must catch: the reflection fix left out; centroids divided by the number of matches instead of sum |w|."""
    with default_dtype(dtype):
        A, B = A.to(dtype), B.to(dtype)
        if w is not None:
            w = w.to(dtype)
        if reflection and not centroid_by_count:
            return O.kabsch(A, B, w, masked=w is not None)
        if w is None:
            am, bm = A.mean(1, keepdim=True), B.mean(1, keepdim=True)
            H = (A - am).transpose(1, 2) @ (B - bm)
        else:
            den = float(A.shape[1]) if centroid_by_count else (w.abs().sum(1, keepdim=True) + 1e-16)
            wn = (w / den).unsqueeze(-1)
            am, bm = (wn * A).sum(1, keepdim=True), (wn * B).sum(1, keepdim=True)
            H = (A - am).transpose(1, 2) @ (w.unsqueeze(-1) * (B - bm))
        U, S, V = torch.svd(H)
        Z = torch.eye(3).repeat(A.shape[0], 1, 1)
        if reflection:
            Z[:, 2, 2] = torch.sign(torch.linalg.det(U @ V.transpose(1, 2)))
        R = V @ Z @ U.transpose(1, 2)
        return R, bm - am @ R.transpose(1, 2), H


def dist(X, Y, R, t, dtype=torch.float64):
    with default_dtype(dtype):
        return O.point_dist(X.to(dtype), Y.to(dtype), R.to(dtype), t.to(dtype))


def sing_ratios(H):
    """s2 / s1, s3 / s2 of [M, 3, 3] in fp64"""
    S = torch.linalg.svdvals(H.double())
    return S[:, 1] / S[:, 0], S[:, 2] / S[:, 1].clamp_min(1e-300)


# ============================================================ mk_gather_backproject (+ _kf, _bwd) ==============================
# (name, B, rows_per_pair, k, n0, n1, keyframes K or None)
GATHER_CASES = [
    ("k 1", 1, 1, 1, 7, 13, None),
    ("k 255", 3, 3, 255, 13, 7, None),
    ("k 256", 1, 3, 256, 7, 13, None),
    ("k 257", 3, 1, 257, 7, 13, None),
    ("one row of image 0", 3, 3, 5, 1, 5, None),
    ("tall", 3, 3, 257, 13, 7, None),
    ("keyframes", 3, 3, 257, 7, 13, 2),
    ("keyframes, one out of range", 3, 1, 256, 13, 7, 2),
]
GATHER_BWD_MODES = ["random", "one keypoint of image 1", "no repeats"]


def intrinsics(g, B):
    """[B, 3, 3] fp32 with different focal lengths and a skew term"""
    K = torch.zeros(B, 3, 3)
    K[:, 0, 0] = 580.0 + 40.0 * torch.rand(B, generator=g)
    K[:, 1, 1] = 610.0 + 40.0 * torch.rand(B, generator=g)
    K[:, 0, 1] = 1.5 * (torch.rand(B, generator=g) - 0.5)
    K[:, 0, 2] = 270.0 + 10.0 * torch.rand(B, generator=g)
    K[:, 1, 2] = 360.0 + 10.0 * torch.rand(B, generator=g)
    K[:, 2, 2] = 1.0
    return K


def edge_cells(n0, n1):
    """the cells whose (i, j) split goes wrong when n0 is taken for n1: 0, n1 - 1, n1, n0 * n1 - 1"""
    return sorted({c for c in (0, n1 - 1, n1, n0 * n1 - 1) if c < n0 * n1})


@functools.lru_cache(maxsize=None)
def gather_case(name, B, rpp, k, n0, n1, K, mode="random"):
    """-> dict of fp32 / int32 inputs and the fp64 references (cached: read-only)"""
    g = gen("gather", name, mode)
    rows, ncell = B * rpp, n0 * n1
    nk = B if K is None else K
    if mode == "one keypoint of image 1":     # every cell of every row is (i, 3): column 3 of the score matrix
        idx = torch.randint(0, n0, (rows, k), generator=g) * n1 + 3
    elif mode == "no repeats":                 # k <= ncell cells without replacement, rows of different pairs only
        assert k <= min(n0, n1) and rpp == 1
        idx = torch.stack([torch.randperm(n0, generator=g)[:k] * n1 + torch.randperm(n1, generator=g)[:k] for _ in range(rows)])
    else:
        idx = torch.randint(0, ncell, (rows, k), generator=g)
        e = edge_cells(n0, n1)
        for r in range(rows):                  # the edge cells in every row, at both ends of it where there is room
            for q, c in enumerate(e[:k]):
                idx[r, q if q % 2 == 0 else k - 1 - q] = c
    kf = None
    if K is not None:
        kf = torch.tensor([1, 0, 1][:B])       # rows repeated and out of order
        if "out of range" in name:
            kf[1] = K
    c = dict(idx=idx.int(), fs=torch.rand(B, n0, n1, generator=g),
             kps0=torch.rand(nk, 2, n0, generator=g) * torch.tensor([540.0, 720.0]).view(1, 2, 1),
             kps1=torch.rand(B, 2, n1, generator=g) * torch.tensor([540.0, 720.0]).view(1, 2, 1),
             dep0=1.0 + 4.0 * torch.rand(nk, 1, n0, generator=g), dep1=1.0 + 4.0 * torch.rand(B, 1, n1, generator=g),
             K0=intrinsics(g, B), K1=intrinsics(g, B), kf=kf, gX=torch.randn(rows, k, 3, generator=g),
             gY=torch.randn(rows, k, 3, generator=g))
    c["valid_pair"] = torch.ones(B, dtype=torch.bool) if kf is None else (kf < K)
    c.update(gather_ref(c, B, rpp, n0, n1))
    return c


def gather_ref(c, B, rpp, n0, n1, split_n=None):
    """fp64 and fp32 evaluations of the gather + back-projection by the oracle's backproject; split_n: the divisor of the cell split
    (n1; passing n0 gives the wrong reference the CPU test must catch).  Pairs whose keyframe is out of range are computed with
    keyframe 0 and masked by the caller (`valid_pair`)."""
    split_n = n1 if split_n is None else split_n
    idx = c["idx"].long()
    rows, k = idx.shape
    pair = torch.arange(B).repeat_interleave(rpp)
    src0 = pair if c["kf"] is None else torch.where(c["valid_pair"], c["kf"], torch.zeros_like(c["kf"]))[pair]
    i0 = (torch.div(idx, split_n, rounding_mode="trunc")).clamp_max(n0 - 1)
    i1 = (idx - torch.div(idx, split_n, rounding_mode="trunc") * split_n).clamp_max(n1 - 1)
    r0, r1 = src0.view(-1, 1).expand(rows, k), pair.view(-1, 1).expand(rows, k)
    uv0, uv1 = c["kps0"][r0, :, i0], c["kps1"][r1, :, i1]           # [rows, k, 2]
    d0, d1 = c["dep0"][r0, :, i0], c["dep1"][r1, :, i1]             # [rows, k, 1]
    out = dict(wts=c["fs"].reshape(B, -1)[r1, idx], corr=torch.cat([uv0, uv1, d0, d1], -1), i0=i0, i1=i1, pair=pair)
    for nm, uv, d, Km in (("X", uv0, d0, c["K0"]), ("Y", uv1, d1, c["K1"])):
        with default_dtype(torch.float64):
            ref = O.backproject(uv.double(), d.double(), Km.double()[pair])
            Ki = torch.linalg.inv(Km.double())[pair]                # [rows, 3, 3]
        scale = d.double() * (Ki[:, None, :, 0].abs() * uv[..., 0:1].double().abs() + Ki[:, None, :, 1].abs() * uv[..., 1:2].double().abs()
                              + Ki[:, None, :, 2].abs())
        x32 = O.backproject(uv, d, Km[pair])
        out[nm] = ref
        out[nm + "_scale"] = scale
        out[nm + "_floor"] = floor32(x32, ref, scale)
    return out


def gather_bwd_ref(c, B, rpp, n0, n1, dtype=torch.float64):
    """autograd through the oracle's gather + backproject in `dtype` (-> gkps0 [B, 2, n0], gdep0 [B, 1, n0], gkps1, gdep1) and, in
    fp64, the sum of the absolute contributions to every keypoint (the scale of its error)"""
    idx = c["idx"].long()
    rows, k = idx.shape
    pair = c["pair"]
    r = pair.view(-1, 1).expand(rows, k)
    leaves = [c[n].to(dtype).clone().requires_grad_() for n in ("kps0", "dep0", "kps1", "dep1")]
    with default_dtype(dtype):
        X = O.backproject(leaves[0][r, :, c["i0"]], leaves[1][r, :, c["i0"]], c["K0"].to(dtype)[pair])
        Y = O.backproject(leaves[2][r, :, c["i1"]], leaves[3][r, :, c["i1"]], c["K1"].to(dtype)[pair])
        ((X * c["gX"].to(dtype)).sum() + (Y * c["gY"].to(dtype)).sum()).backward()
    grads = [l.grad for l in leaves]
    if dtype != torch.float64:
        return grads
    scales = []
    for uvn, dn, Kn, gn, ii, n in (("kps0", "dep0", "K0", "gX", c["i0"], n0), ("kps1", "dep1", "K1", "gY", c["i1"], n1)):
        Ki = torch.linalg.inv(c[Kn].double())[pair][:, None]        # [rows, 1, 3, 3]
        g = c[gn].double().abs()                                     # [rows, k, 3]
        uv, d = c[uvn].double()[r, :, ii], c[dn].double()[r, 0, ii]
        cu = d * (g * Ki[..., 0].abs()).sum(-1)
        cv = d * (g * Ki[..., 1].abs()).sum(-1)
        cd = (g * (Ki[..., 0].abs() * uv[..., 0:1].abs() + Ki[..., 1].abs() * uv[..., 1:2].abs() + Ki[..., 2].abs())).sum(-1)
        flat = (r * n + ii).reshape(-1)
        su, sv, sd = (torch.zeros(B * n, dtype=torch.float64).index_add_(0, flat, x.reshape(-1)) for x in (cu, cv, cd))
        scales += [torch.stack([su.view(B, n), sv.view(B, n)], 1), sd.view(B, 1, n)]
    return grads, scales


# ============================================================ mk_ransac_hypotheses ==============================================
HYP_K = [3, 4, 5, 63, 64, 65, 255, 256, 257, 2016, 2017, 4768]
HYP_IT = [1, 15, 16, 17, 33, 100, 129, 132]
HYP_PASS = 8        # hypotheses a wave parks per pass (mk_solver.hip)


def nsplit_rule(cus, nsets, it_ransac):
    """blocks per correspondence set, as mk_ransac_hypotheses states it"""
    if it_ransac < 16:
        return 1
    return max(4, min((it_ransac + 3) // 4, (2 * cus + nsets - 1) // nsets))


def split_parts(cus, nsets, it_ransac):
    """-> (nsplit, per, number of empty parts, the largest number of passes a wave makes)"""
    ns = nsplit_rule(cus, nsets, it_ransac)
    per = (it_ransac + ns - 1) // ns
    empty = sum(1 for p in range(ns) if p * per >= it_ransac)
    passes = max(((min(it_ransac, p * per + per) - p * per) + 4 * HYP_PASS - 1) // (4 * HYP_PASS) for p in range(ns) if p * per < it_ransac)
    return ns, per, empty, passes


def sets_with_empty_parts(cus, it_ransac=100):
    """the smallest set count whose launch has parts with no hypotheses (23 on 256 CUs: nsplit 23, per 5, three empty)"""
    for nsets in range(1, 2 * cus + 1):
        if split_parts(cus, nsets, it_ransac)[2] > 0:
            return nsets
    return None


def regime_cases(cus):
    """(regime, nsets, it_ransac, k) from the device's CU count: the four launch regimes of the nsplit rule, and it_ransac = 132 with four
    blocks per set (33 hypotheses each: every wave of every part makes a second pass)"""
    return [("nsplit 1", 3, 15, 65),
            ("nsplit 4, second pass of one hypothesis", (cus + 1) // 2, 129, 9),
            ("nsplit ceil(it / 4)", 1, 100, 65),
            ("empty parts", sets_with_empty_parts(cus), 100, 9),
            ("nsplit 4, second pass in every part", (cus + 1) // 2, 132, 9)]


def hyp_sets(g, nsets, k, noise=0.02):
    """-> X, Y [nsets, k, 3] fp32: Y a rigid image of X per set plus N(0, noise) -- every match is a soft inlier of a good triple
    to a degree, so every match's term counts in a score"""
    X = points(g, nsets, k)
    Y = torch.empty_like(X)
    for s in range(nsets):
        R = rotation(g)
        t = (torch.rand(3, generator=g, dtype=torch.float64) - 0.5) * 0.6
        Y[s] = (X[s].double() @ R.T + t + noise * torch.randn(k, 3, generator=g, dtype=torch.float64)).float()
    return X, Y


def conditioned_triples(g, X, Y, it_ransac, must=()):
    """[nsets * it_ransac, 3] int64: three distinct matches per hypothesis, redrawn until the fp64 cross-covariance of the triple has
    s2 / s1 >= 2 COND (built in, not filtered afterwards); `must`: indices that the first hypotheses of every set contain"""
    nsets, k, _ = X.shape
    nh = nsets * it_ransac
    gsel = torch.arange(nsets).repeat_interleave(it_ransac)
    hloc = torch.arange(nh) % it_ransac
    out = torch.zeros(nh, 3, dtype=torch.int64)
    todo = torch.ones(nh, dtype=torch.bool)
    for attempt in range(200):
        rows = torch.nonzero(todo).view(-1)
        if rows.numel() == 0:
            return out
        tri = torch.multinomial(torch.ones(rows.numel(), k), 3, generator=g)
        if attempt < 100:
            for q, j in enumerate(must):
                sel = hloc[rows] == q
                tri[sel, q % 3] = j
        distinct = (tri[:, 0] != tri[:, 1]) & (tri[:, 0] != tri[:, 2]) & (tri[:, 1] != tri[:, 2])
        s = gsel[rows][:, None]
        _, _, H = kabsch(X[s, tri], Y[s, tri])
        ok = distinct & (sing_ratios(H)[0] >= 2 * COND)
        out[rows[ok]] = tri[ok]
        todo[rows[ok]] = False
    raise AssertionError("no well-conditioned triple for %d hypotheses" % int(todo.sum()))


def hypotheses_ref(X, Y, idx3, it_ransac, th=TH_SOFT, dtype=torch.float64, drop_last=False, reflection=True):
    """oracle kabsch + soft_inliers in `dtype` -> R [nh, 9], t [nh, 3], score [nh], and the fp64-only extras (H, centroid norms).
    drop_last / reflection=False: the wrong references of the CPU test."""
    nsets, k, _ = X.shape
    gsel = torch.arange(nsets).repeat_interleave(it_ransac)
    A, B = X[gsel[:, None], idx3], Y[gsel[:, None], idx3]
    R, t, H = kabsch(A, B, dtype=dtype, reflection=reflection)
    kk = k - 1 if drop_last else k
    with default_dtype(dtype):
        score = torch.cat([O.soft_inliers(X[gsel[i:i + 512], :kk].to(dtype), Y[gsel[i:i + 512], :kk].to(dtype), R[i:i + 512], t[i:i + 512], f32(th))
                           for i in range(0, len(gsel), 512)])
    cn = torch.maximum(A.double().mean(1).norm(dim=-1), B.double().mean(1).norm(dim=-1)).clamp_min(1.0)
    return dict(R=R.reshape(-1, 9), t=t.reshape(-1, 3), score=score.reshape(-1), H=H, t_scale=cn[:, None])


def hypotheses_case_from(X, Y, idx3, it_ransac):
    """fp64 reference, scales and floors of one launch"""
    r64 = hypotheses_ref(X, Y, idx3, it_ransac)
    r32 = hypotheses_ref(X, Y, idx3, it_ransac, dtype=torch.float32)
    one = torch.ones(())
    c = dict(X=X, Y=Y, idx3=idx3, it_ransac=it_ransac, ref=r64, cond=float(sing_ratios(r64["H"])[0].min()),
             scale=dict(R=one.double(), t=r64["t_scale"], score=r64["score"]))
    c["floor"] = {n: floor32(r32[n], r64[n], c["scale"][n]) for n in ("R", "t", "score")}
    return c


@functools.lru_cache(maxsize=None)
def hypotheses_case(nsets, it_ransac, k):
    g = gen("hyp", nsets, it_ransac, k)
    X, Y = hyp_sets(g, nsets, k)
    must = sorted({j for j in (0, 63, 64, 255, 256, k - 1) if j < k})[-min(it_ransac, 6):]
    return hypotheses_case_from(X, Y, conditioned_triples(g, X, Y, it_ransac, must), it_ransac)


def hyp_where(c, i, width):
    h = i // width
    tri = c["idx3"][h].tolist()
    it = c["it_ransac"]
    return "set %d, hypothesis %d (number %d of its set), component %d, triple %s" % (h // it, h, h % it, i % width, tri)


# ---- injected noise: the exponential race ---------------------------------------------------------------------------------------
RACE_K = [3, 4, 5, 255, 256, 257, 513]


def topk_lowest_index(keys, n, reverse_ties=False):
    """top-n of every row of `keys`, descending, EXACT ties to the lowest index (reverse_ties: to the highest -- the wrong rule)"""
    if reverse_ties:
        k = keys.shape[1]
        return (k - 1) - torch.sort(keys.flip(1), dim=1, descending=True, stable=True).indices[:, :n]
    return torch.sort(keys, dim=1, descending=True, stable=True).indices[:, :n]


@functools.lru_cache(maxsize=None)
def race_case(k, kind):
    """-> w [nsets, k], noise [nsets * it, k], the wanted idx3.  kind: 'dense' (a fifth of the weights zero), 'two' / 'one' positive
    weights, 'tie lanes' (an exact maximal key in matches 5 and 9: two lanes), 'tie stride' (in matches 6 and 262: one lane's
    consecutive strides)"""
    g = gen("race", k, kind)
    nsets, it = 2, 5
    w = torch.rand(nsets, k, generator=g) + 0.05
    w[torch.rand(nsets, k, generator=g) < 0.2] = 0.0
    w[:, k - 1] = 0.9
    noise = torch.empty(nsets * it, k).exponential_(1.0, generator=g).clamp_min(2.0 ** -9)     # keys <= 1.05 x 512
    if kind in ("two", "one"):
        keep = [k - 1, k // 2][: 2 if kind == "two" else 1]
        z = torch.zeros_like(w)
        z[:, keep] = w[:, keep] + 0.1
        w = z
    elif kind.startswith("tie"):
        a, b = (5, 9) if kind == "tie lanes" else (6, 262)
        assert b < k
        w[:, a] = w[:, b] = 0.75
        noise[:, a] = noise[:, b] = 2.0 ** -10         # key 768 twice: above every other key
    keys = w.repeat_interleave(it, 0) / noise
    return dict(w=w, noise=noise, it=it, nsets=nsets, keys=keys, idx3=topk_lowest_index(keys, 3))


def race_cases():
    out = []
    for k in RACE_K:
        out.append((k, "dense"))
        out += [(k, "two"), (k, "one")] if k in (3, 5, 257) else []
        if k >= 255:
            out.append((k, "tie lanes"))
        if k >= 263:
            out.append((k, "tie stride"))
    return out


# ---- on-device draws: weights positive on exactly three matches -----------------------------------------------------------------
def draw_cases():
    """(k, the three matches with a positive weight): {0, 255, k - 1} and {0, 256, k - 1}; at k = 257 the second has two members only"""
    out = [(3, (0, 1, 2))]
    for k in (257, 513, 2017):
        out += [(k, s) for s in ((0, 255, k - 1), (0, 256, k - 1)) if len(set(s)) == 3]
    return out


DRAW_WEIGHTS = (0.5, 0.3, 0.2)


def draw_law_violations(idx3, support, weights=DRAW_WEIGHTS, nsig=5.0):
    """first-pick frequencies against w_i / sum w and second-pick frequencies given the first against w_j / (sum w - w_i), each within
    nsig binomial standard deviations -> list of violations (empty: the law holds)"""
    bad = []
    n = idx3.shape[0]
    pos = {s: i for i, s in enumerate(support)}
    W = sum(weights)
    for i, si in enumerate(support):
        first = idx3[:, 0] == si
        n1 = int(first.sum())
        p = weights[i] / W
        if abs(n1 - n * p) > nsig * math.sqrt(n * p * (1 - p)):
            bad.append("first pick %d: %d of %d, expected %.1f" % (si, n1, n, n * p))
        for j, sj in enumerate(support):
            if j == i:
                continue
            n2 = int((first & (idx3[:, 1] == sj)).sum())
            q = weights[j] / (W - weights[i])
            if abs(n2 - n1 * q) > nsig * math.sqrt(max(n1 * q * (1 - q), 1e-9)):
                bad.append("second pick %d after %d: %d of %d, expected %.1f" % (sj, si, n2, n1, n1 * q))
    assert set(pos) == set(support)
    return bad


# ============================================================ refinement state machines ==========================================
def refine_machine(X, Y, R0, t0, th, num_ref, min_inl, dtype=torch.float64, tie_rule=None):
    """mk_refine_pose after its arg-max, for ONE pair, by the oracle's hard_inliers / kabsch / soft_inliers in `dtype`:
    best = min_inl; up to num_ref times: refit on the inliers of the current pose iff their count >= min_inl and > best.
    -> dict(R [3, 3], t [1, 3], conf, mask [k] bool, rounds, dists: the residuals [k] of every evaluation, Hs: the H of every refit,
    counts)"""
    th = f32(th)
    Xb, Yb = X[None].to(dtype), Y[None].to(dtype)
    R, t = R0[None].to(dtype), t0.reshape(1, 1, 3).to(dtype)
    best, rounds, dists, Hs, counts = float(min_inl), 0, [], [], []
    for _ in range(num_ref):
        d = dist(Xb, Yb, R, t, dtype)[0]
        inl = (th - d) >= 0
        c = int(inl.sum())
        dists.append(d)
        counts.append(c)
        if not (c >= min_inl and c > best):
            break
        best = c
        rounds += 1
        R, t, H = kabsch(Xb, Yb, inl[None].to(dtype), dtype=dtype)
        Hs.append(H[0])
    d = dist(Xb, Yb, R, t, dtype)[0]
    dists.append(d)
    with default_dtype(dtype):
        conf = O.soft_inliers(Xb, Yb, R, t, th)[0, 0]
    return dict(R=R[0], t=t[0], conf=conf, mask=(th - d) >= 0, rounds=rounds, dists=dists, Hs=Hs, counts=counts)


def train_machine(X, Y, sample, th, num_ref, dtype=torch.float64, drop=None, centroid_by_count=False):
    """mk_train_ransac_masks' state machine for ONE hypothesis (train_oracle.refine_masks, which the CPU test holds this against):
    cur = fin = sample, pre = |sample|; up to num_ref times: fit cur, ref = inliers, stop unless |ref| > pre; pre = |ref|, fin = cur,
    cur = ref.  -> dict(mask [S] float, rounds, dists, Hs).  drop: a match left out of every fit (the wrong reference)."""
    th = f32(th)
    S = X.shape[0]
    cur = torch.zeros(S, dtype=torch.bool)
    cur[sample] = True
    fin, pre, rounds, dists, Hs = cur.clone(), len(sample), 0, [], []
    Xb, Yb = X[None].to(dtype), Y[None].to(dtype)
    for _ in range(num_ref):
        w = cur.clone()
        if drop is not None:
            w[drop] = False
        R, t, H = kabsch(Xb, Yb, w[None].to(dtype), dtype=dtype, centroid_by_count=centroid_by_count)
        Hs.append(H[0])
        d = dist(Xb, Yb, R, t, dtype)[0]
        dists.append(d)
        ref = (th - d) >= 0
        if not int(ref.sum()) > pre:
            break
        pre, fin, cur = int(ref.sum()), cur, ref
        rounds += 1
    return dict(mask=fin.float(), rounds=rounds, dists=dists, Hs=Hs)


def machine_margin(m64, m32, th):
    """-> (margin: the smallest |residual - th| over every evaluation of the fp64 machine, err32: the fp32 oracle's largest residual
    error over the same evaluations, same: whether the fp32 machine took the same path).  The case is usable when
    margin >= MARGIN_FACTOR x err32."""
    th = f32(th)
    if len(m64["dists"]) != len(m32["dists"]) or m64["rounds"] != m32["rounds"]:
        return 0.0, float("inf"), False
    margin = min(float((d - th).abs().min()) for d in m64["dists"])
    err = max(float((a.double() - b).abs().max()) for a, b in zip(m32["dists"], m64["dists"]))
    return margin, err, True


def well_conditioned(Hs, full_rank):
    for H in Hs:
        r21, r32 = sing_ratios(H[None])
        if float(r21) < COND or (full_rank and float(r32) < COND):
            return False
    return True


# ---- mk_refine_pose ---------------------------------------------------------------------------------------------------------------
# (name, k, B, it_matches, it_ransac, num_ref, min_inliers rule, wanted rounds of the first pair (None: whatever it is),
#  tie pattern: where a second, equal maximum is planted)
#   min_inliers rule: int = that value; "first" = the first count (no refit); "first-1" = one below it (refit)
REFINE_CASES = [
    ("k 3", 3, 2, 1, 1, 4, "first-1", 1, None),
    ("k 3, min = count", 3, 2, 3, 1, 4, "first", 0, None),
    ("k 5", 5, 2, 7, 73, 4, "first-1", None, None),
    ("k 511", 511, 2, 7, 73, 4, 3, 2, "lanes"),
    ("k 512", 512, 2, 8, 64, 4, 3, 3, "waves"),
    ("k 513", 513, 2, 27, 19, 4, 3, 4, "stride"),
    ("k 513, one refinement", 513, 2, 27, 19, 1, 3, 1, "waves"),
    ("k 513, no refinement", 513, 2, 27, 19, 0, 3, 0, "stride"),
    ("k 1025", 1025, 2, 25, 41, 4, 3, None, "stride"),
    ("k 1025, min = count", 1025, 2, 25, 41, 4, "first", 0, "waves"),
    ("k 1025, min = count - 1", 1025, 2, 25, 41, 4, "first-1", None, "lanes"),
]
REFINE_HP = {1, 511, 512, 513, 1025}


def tie_pair(pattern, HP, g):
    """-> (winner, later index with the same score): in one thread's stride (i, i + 512), in two lanes of a wave, in two waves"""
    if pattern == "stride":
        i = int(torch.randint(0, HP - 512, (1,), generator=g))
        return i, i + 512
    if pattern == "lanes":
        w = int(torch.randint(1, min(HP, 512) // 64, (1,), generator=g))
        return w * 64 + 3, w * 64 + 41
    if pattern == "waves":
        return 64 + 17, 3 * 64 + 2
    raise AssertionError(pattern)


def first_seed(build, limit=400):
    """the first seed for which build(seed) returns a case (it returns None when the margin, the conditioning or the wanted round
    count is missed): the case table is closed under this deterministic search"""
    for seed in range(limit):
        c = build(seed)
        if c is not None:
            c["seed"] = seed
            return c
    raise AssertionError("no seed below %d gives a usable case" % limit)


@functools.lru_cache(maxsize=None)
def refine_case(name, k, B, it_m, it_r, num_ref, min_rule, want_rounds, tie):
    HP = it_m * it_r

    def build(seed):
        g = gen("refine", name, seed)
        X, Y = torch.empty(B * it_m, k, 3), torch.empty(B * it_m, k, 3)
        Rh, th_, score = torch.empty(B * HP, 3, 3), torch.empty(B * HP, 3), torch.rand(B * HP, generator=g)
        pairs, margin, err32 = [], float("inf"), 0.0
        for b in range(B):
            if tie is None or HP < 128:
                win = int(torch.randint(HP // 2, HP, (1,), generator=g)) if HP > 1 else 0
                later = None
            else:
                win, later = tie_pair(tie, HP, g)
                if b == 1 and later + 1 < HP:      # the second pair: shifted by one lane, so that it is not the same threads again
                    win, later = win + 1, later + 1
            truth = []
            for m in range(it_m):
                Xs, Ys, R, t = planted_set(g, k, outliers=0.3 if k > 8 else 0.0)
                X[b * it_m + m], Y[b * it_m + m] = Xs, Ys
                truth.append((R, t))
            for h in range(HP):
                R, t = truth[h // it_r]
                Rh[b * HP + h], th_[b * HP + h] = perturbed(g, R, t)
            score[b * HP + win] = 2.0
            if later is not None:
                score[b * HP + later] = 2.0
            s = b * it_m + win // it_r
            R0, t0 = Rh[b * HP + win], th_[b * HP + win]
            if isinstance(min_rule, str) and b > 0:
                min_inl = pairs[0]["min_inl"]      # one min_inliers per launch: the rule is stated for the first pair
            elif isinstance(min_rule, str):
                c0 = int(((f32(TH_INLIER) - dist(X[s][None], Y[s][None], R0[None], t0.reshape(1, 1, 3))[0]) >= 0).sum())
                min_inl = c0 if min_rule == "first" else c0 - 1
                if min_inl < 1:
                    return None
            else:
                min_inl = min_rule
            m64 = refine_machine(X[s], Y[s], R0, t0, TH_INLIER, num_ref, min_inl)
            m32 = refine_machine(X[s], Y[s], R0, t0, TH_INLIER, num_ref, min_inl, dtype=torch.float32)
            mg, er, same = machine_margin(m64, m32, TH_INLIER)
            if not same or not well_conditioned(m64["Hs"], full_rank=k > 3):
                return None
            if b == 0 and want_rounds is not None and m64["rounds"] != want_rounds:
                return None
            margin, err32 = min(margin, mg), max(err32, er)
            pairs.append(dict(win=win, later=later, set=s, min_inl=min_inl, m64=m64, m32=m32))
        if not margin >= MARGIN_FACTOR * err32:
            return None
        ref = dict(R=torch.stack([p["m64"]["R"] for p in pairs]).reshape(B, 9), t=torch.stack([p["m64"]["t"] for p in pairs]).reshape(B, 3),
                   conf=torch.stack([p["m64"]["conf"] for p in pairs]).reshape(B, 1))
        r32 = dict(R=torch.stack([p["m32"]["R"] for p in pairs]).reshape(B, 9), t=torch.stack([p["m32"]["t"] for p in pairs]).reshape(B, 3),
                   conf=torch.stack([p["m32"]["conf"] for p in pairs]).reshape(B, 1))
        tsc = []
        for p in pairs:
            w = p["m64"]["mask"].double() if p["m64"]["rounds"] else None
            Xs, Ys = X[p["set"]].double(), Y[p["set"]].double()
            tsc.append(1.0 if w is None else max(1.0, float((w[:, None] * Xs).sum(0).norm() / w.sum()), float((w[:, None] * Ys).sum(0).norm() / w.sum())))
        scale = dict(R=torch.ones((), dtype=torch.float64), t=torch.tensor(tsc, dtype=torch.float64)[:, None], conf=ref["conf"])
        return dict(X=X, Y=Y, Rh=Rh.reshape(-1, 9), th=th_, score=score, pairs=pairs, min_inl=pairs[0]["min_inl"], margin=margin, err32=err32,
                    ref=ref, scale=scale, floor={n: floor32(r32[n], ref[n], scale[n]) for n in ref},
                    mask=torch.stack([p["m64"]["mask"] for p in pairs]), rounds=[p["m64"]["rounds"] for p in pairs],
                    best=[p["win"] for p in pairs])

    return first_seed(build)


# ---- mk_train_ransac_masks -----------------------------------------------------------------------------------------------------
TRAIN_S = [8, 63, 64, 65, 255, 256, 257, 512, 513, 1023, 1024]
# (S, num_corr, it_ransac, num_ref): every S; num_corr in {3, 8, S}; it_ransac in {1, 4, 5}; num_ref in {0, 4}
TRAIN_CASES = [(8, 3, 5, 4), (8, 8, 1, 4), (63, 8, 4, 4), (64, 8, 5, 4), (65, 8, 5, 4), (65, 65, 1, 4), (255, 8, 4, 4), (256, 8, 5, 4),
               (257, 3, 5, 4), (512, 8, 1, 4), (513, 8, 5, 4), (1023, 8, 4, 4), (1024, 8, 5, 4), (1024, 8, 5, 0), (1024, 1024, 1, 4)]
TRAIN_NSETS = 2


@functools.lru_cache(maxsize=None)
def train_case(S, nc, it_r, num_ref):
    """injected indices: samples of `nc` inliers-by-construction; the first hypotheses contain the matches 63, 64 and S - 1"""
    def build(seed):
        g = gen("train", S, nc, it_r, num_ref, seed)
        X, Y = torch.empty(TRAIN_NSETS, S, 3), torch.empty(TRAIN_NSETS, S, 3)
        idx = torch.empty(TRAIN_NSETS * it_r, nc, dtype=torch.int64)
        hyps, margin, err32 = [], float("inf"), 0.0
        for s in range(TRAIN_NSETS):
            X[s], Y[s], _, _ = planted_set(g, S, outliers=0.3 if S > 8 else 0.0)
            must = [j for j in (63, 64, S - 1) if j < S]
            for h in range(it_r):
                smp = torch.randperm(S, generator=g)[:nc]
                if nc < S:
                    for q, j in enumerate(must[:nc]):
                        if j not in smp.tolist():
                            smp[q] = j
                    if len(set(smp.tolist())) < nc:
                        return None
                idx[s * it_r + h] = smp
                m64 = train_machine(X[s], Y[s], smp, TH_INLIER, num_ref)
                m32 = train_machine(X[s], Y[s], smp, TH_INLIER, num_ref, dtype=torch.float32)
                if num_ref:
                    mg, er, same = machine_margin(m64, m32, TH_INLIER)
                    if not same or not well_conditioned(m64["Hs"], full_rank=nc > 3):
                        return None
                    margin, err32 = min(margin, mg), max(err32, er)
                hyps.append(m64)
        if num_ref and not margin >= MARGIN_FACTOR * err32:
            return None
        return dict(X=X, Y=Y, idx=idx, hyps=hyps, margin=margin, err32=err32, mask=torch.stack([h["mask"] for h in hyps]),
                    rounds=torch.tensor([h["rounds"] for h in hyps], dtype=torch.int32))

    return first_seed(build)


TRAIN_RACE_CASES = [(8, 3, "dense"), (63, 8, "dense"), (64, 8, "dense"), (65, 8, "dense"), (257, 8, "dense"), (1023, 8, "dense"),
                    (1024, 8, "dense"), (1024, 8, "few"), (65, 65, "dense"), (513, 8, "tie")]


@functools.lru_cache(maxsize=None)
def train_race_case(S, nc, kind):
    """injected noise: -> w [2, S], noise [2 * 5, S], wanted indices = the stable top-nc of w / noise.  'few': five positive weights
    for nc = 8 (the rest are the lowest free indices); 'tie': an exact maximal key in matches 70 and 70 + 256 (one lane, slots 1, 5)"""
    g = gen("train race", S, nc, kind)
    it = 5
    w = torch.rand(2, S, generator=g) + 0.05
    w[torch.rand(2, S, generator=g) < 0.2] = 0.0
    w[:, S - 1] = 0.9
    noise = torch.empty(2 * it, S).exponential_(1.0, generator=g).clamp_min(2.0 ** -9)
    if kind == "few":
        z = torch.zeros_like(w)
        keep = [S - 1, 64, 63, 700, 2]
        z[:, keep] = w[:, keep] + 0.1
        w = z
    if kind == "tie":
        w[:, 70] = w[:, 326] = 0.75
        noise[:, 70] = noise[:, 326] = 2.0 ** -10
    keys = w.repeat_interleave(it, 0) / noise
    return dict(w=w, noise=noise, it=it, idx=topk_lowest_index(keys, nc), keys=keys)


# ---- mk_reinforce_scatter ------------------------------------------------------------------------------------------------------
SCATTER_CASES = [(S, it_m) for S in (1, 511, 512, 513) for it_m in (1, 3)]
SCATTER_NCELL = 600


@functools.lru_cache(maxsize=None)
def scatter_case(S, it_m, B=2):
    g = gen("scatter", S, it_m)
    idx = torch.stack([torch.randperm(SCATTER_NCELL, generator=g)[:S] for _ in range(B * it_m)])
    lv = torch.rand(B * it_m, generator=g)
    pre, pre_b = torch.randn(B, SCATTER_NCELL, generator=g), torch.randint(0, 5, (B, SCATTER_NCELL), generator=g).float()
    want, want_b = pre.clone(), pre_b.clone()
    for r in range(B * it_m):                  # row after row, fp32, as the reference's loop
        want[r // it_m, idx[r]] += lv[r]
        want_b[r // it_m, idx[r]] += 1.0
    drawn = torch.zeros(B, SCATTER_NCELL, dtype=torch.bool)
    for r in range(B * it_m):
        drawn[r // it_m, idx[r]] = True
    return dict(idx=idx.int(), lv=lv, pre=pre, pre_b=pre_b, want=want, want_b=want_b, drawn=drawn, B=B)


_ = TO   # train_oracle: held against train_machine in tests/test_solver_edges_cpu.py


# ============================================================ mk_train_aggregate_fwd / _bwd =======================================
# (B, it_matches, it_ransac, null hypothesis, temperature): it_ransac in {1, 63, 64, 65, 129} (the lane-strided loops make a second
# and a third trip), it_matches in {1, 4, 5, 64} (one wave takes 1, 2 and 16 sets), temperature 0.05 (the max subtraction at 1e4)
AGG_CASES = [(1, 1, 1, 0, 20.0), (3, 4, 63, 1, 20.0), (1, 5, 64, 0, 20.0), (3, 5, 65, 1, 20.0), (1, 64, 129, 1, 20.0), (3, 4, 129, 0, 20.0),
             (3, 5, 65, 1, 0.05), (1, 64, 1, 1, 20.0)]
AGG_BWD_CASES = [(1, 1, 255), (1, 4, 64), (1, 1, 257), (3, 5, 65)]     # 255, 256, 257 hypotheses: the 256-thread blocks; several pairs
NULL_LOSS, NULL_SCORE = 0.8, 0.35 * 512
AGG_TINY = 1e-30      # softmax weights below this (fp32 holds nothing under 1e-45) are compared absolutely


def aggregate_ref(out, it_m, it_r, add_null, temp, dtype=torch.float64, drop_last=False):
    """loss_class.py:229-246 / 263-268 as train_oracle.single_iteration states them, in `dtype`, with autograd for coef.
    -> loss_value [rows], per_pair [B, 3], coef [nhyp, 2], and in fp64 the scales (sums of the absolute terms).
    drop_last: the last hypothesis of every set left out of the softmax (the wrong reference)."""
    o = out.to(dtype).reshape(-1, it_r, 4)
    rows = o.shape[0]
    lv_in, score = o[..., 0].clone().requires_grad_(), o[..., 3].clone().requires_grad_()
    lr, lt = o[..., 1], o[..., 2]
    keep = it_r - 1 if drop_last and it_r > 1 else it_r
    sm = torch.softmax(score[:, :keep] / temp, -1)
    loss_rot, loss_trans = (lr[:, :keep] * sm).sum(-1), (lt[:, :keep] * sm).sum(-1)
    lv, sc = lv_in[:, :keep], score[:, :keep]
    if add_null:
        lv = torch.cat([lv, torch.full((rows, 1), NULL_LOSS, dtype=dtype)], -1)
        sc = torch.cat([sc, torch.full((rows, 1), f32(NULL_SCORE), dtype=dtype)], -1)
    w = torch.softmax(sc / temp, -1)
    loss_value = (lv * w).sum(-1)
    loss_value.sum().backward()
    coef = torch.stack([lv_in.grad, score.grad], -1).reshape(-1, 2)
    per_pair = torch.stack([loss_value.detach().reshape(-1, it_m).sum(-1), loss_rot.detach().reshape(-1, it_m).sum(-1),
                            loss_trans.detach().reshape(-1, it_m).sum(-1)], -1)
    res = dict(loss_value=loss_value.detach(), per_pair=per_pair, coef=coef)
    if dtype == torch.float64 and not drop_last:
        wd = w.detach()
        lv_abs = (lv.detach().abs() * wd).sum(-1)
        smd = wd[:, :it_r]
        res["scale"] = dict(loss_value=lv_abs.clamp_min(AGG_TINY),
                            per_pair=torch.stack([lv_abs.reshape(-1, it_m).sum(-1), loss_rot.detach().reshape(-1, it_m).sum(-1),
                                                  loss_trans.detach().reshape(-1, it_m).sum(-1)], -1).clamp_min(AGG_TINY),
                            coef=torch.stack([smd, smd * (o[..., 0].abs() + lv_abs[:, None]) / temp], -1).reshape(-1, 2).clamp_min(AGG_TINY))
    return res


@functools.lru_cache(maxsize=None)
def aggregate_case(B, it_m, it_r, add_null, temp):
    """out [nhyp, 4] = (loss in [0, 1), rotation error, translation error, score up to 512), Rt finite, singular values (3, 2, 1)
    except the planted rank-one hypotheses (1, 0, 0): the first and the last hypothesis of every third set, over waves and pairs"""
    g = gen("aggregate", B, it_m, it_r, add_null, temp)
    nh = B * it_m * it_r
    out = torch.rand(nh, 4, generator=g) * torch.tensor([1.0, 0.5, 1.0, 512.0])
    out[nh // 2, 3] = 512.0
    Rt = torch.randn(nh, 12, generator=g)
    saved = torch.zeros(nh, 32)
    saved[:, 18:21] = torch.tensor([3.0, 2.0, 1.0])
    rank1 = sorted({r * it_r + h for r in range(0, B * it_m, 3) for h in (0, it_r - 1)})
    saved[rank1, 18:21] = torch.tensor([1.0, 0.0, 0.0])
    saved[rank1[-1], 18:21] = torch.tensor([0.0, 0.0, 1.5])          # the one large value need not come first
    r64 = aggregate_ref(out, it_m, it_r, add_null, temp)
    r32 = aggregate_ref(out, it_m, it_r, add_null, temp, dtype=torch.float32)
    floor = {n: floor32(r32[n], r64[n], r64["scale"][n]) for n in ("loss_value", "per_pair", "coef")}
    return dict(out=out, Rt=Rt, saved=saved, rank1=len(rank1), ref=r64, floor=floor)


# ============================================================ mk_train_tail_fwd / _bwd ============================================
# (S, it_ransac, loss, soft clipping); B = 2 pairs x it_matches = 3 sets (the pair of a set is r / it_matches).  Even sets are proper,
# odd sets MIRRORED (Y ~ R diag(1, 1, -1) X + t: the fit's reflection branch, d = -1, forward and backward).  The mask of
# hypothesis h of set r is kind (r + h) % 3: all ones | the matches {63, 64, S - 1} plus five others | three matches (rank two).
TAIL_CASES = [(8, 5, "POSE_ERR", 1), (63, 4, "VCRE", 1), (64, 1, "POSE_ERR", 0), (65, 5, "VCRE", 0), (255, 4, "POSE_ERR", 1),
              (256, 5, "VCRE", 1), (257, 1, "POSE_ERR", 0), (1024, 5, "VCRE", 1)]
TAIL_B, TAIL_ITM = 2, 3
MASK_KINDS = ("all", "eight", "three")


@contextlib.contextmanager
def oracle_in(dtype):
    """default dtype `dtype` for the oracle's constants, and its eye grid (built .float()) cast to it"""
    eye = TO.eye_grid
    TO.eye_grid = lambda: eye().to(dtype)
    try:
        with default_dtype(dtype):
            yield
    finally:
        TO.eye_grid = eye


def tail_ref(c, dtype=torch.float64, grad_out=None, reflection=True, centroid_by_count=False):
    """the oracle's differentiable tail in `dtype`: masked kabsch -> soft_inliers -> train_oracle.pose_loss, and with grad_out
    [nh, 2] = dL / d(loss, score) the gradients w.r.t. X, Y by autograd through the SVD"""
    it_r, it_m = c["it_r"], TAIL_ITM
    X, Y = c["X"].to(dtype).clone(), c["Y"].to(dtype).clone()
    if grad_out is not None:
        X.requires_grad_()
        Y.requires_grad_()
    Xv, Yv = X.repeat_interleave(it_r, 0), Y.repeat_interleave(it_r, 0)
    pair = torch.arange(TAIL_B).repeat_interleave(it_m * it_r)
    with oracle_in(dtype):
        R, t, H = kabsch(Xv, Yv, c["mask"], dtype=dtype, reflection=reflection, centroid_by_count=centroid_by_count)
        score = O.soft_inliers(Xv, Yv, R, t, f32(TH_SOFT))
        K = c["K"].to(dtype)[pair]
        lv, lr, lt = TO.pose_loss(c["kind"], R, t, c["Rgt"].to(dtype)[pair], c["tgt"].to(dtype)[pair].reshape(-1, 1, 3), K, K, bool(c["soft"]))
    res = dict(out=torch.cat([lv.reshape(-1, 1), lr.reshape(-1, 1), lt.reshape(-1, 1), score.reshape(-1, 1)], 1).detach(),
               Rt=torch.cat([R.reshape(-1, 9), t.reshape(-1, 3)], 1).detach(), H=H.detach())
    if grad_out is not None:
        g = grad_out.to(dtype)
        ((lv.reshape(-1) * g[:, 0]).sum() + (score.reshape(-1) * g[:, 1]).sum()).backward()
        res["gX"], res["gY"] = X.grad, Y.grad
    return res


@functools.lru_cache(maxsize=None)
def tail_case(S, it_r, kind, soft):
    def build(seed):
        g = gen("tail", S, it_r, kind, soft, seed)
        nsets = TAIL_B * TAIL_ITM
        X = points(g, nsets, S)
        Y = torch.empty_like(X)
        Rgt, tgt = torch.empty(TAIL_B, 3, 3), torch.empty(TAIL_B, 3)
        mask = torch.zeros(nsets * it_r, S)
        kinds = []
        for r in range(nsets):
            Rm = rotation(g, mirror=r % 2 == 1)
            t = (torch.rand(3, generator=g, dtype=torch.float64) - 0.5) * 0.6
            Y[r] = (X[r].double() @ Rm.T + t + 0.02 * torch.randn(S, 3, generator=g, dtype=torch.float64)).float()
            if r % TAIL_ITM == 0:
                Rgt[r // TAIL_ITM], tgt[r // TAIL_ITM] = perturbed(g, rotation(g), t)
            for h in range(it_r):
                mk = MASK_KINDS[(r + h) % 3]
                if mk == "all":
                    sel = torch.arange(S)
                elif mk == "eight":
                    must = sorted({j for j in (63, 64, S - 1) if j < S})
                    rest = [j for j in torch.randperm(S, generator=g).tolist() if j not in must][:5]
                    sel = torch.tensor(must + rest)
                else:
                    sel = conditioned_triples(g, X[r:r + 1], Y[r:r + 1], 1)[0]
                mask[r * it_r + h, sel] = 1.0
                kinds.append(mk)
        K = intrinsics(g, TAIL_B)
        c = dict(X=X, Y=Y, mask=mask, Rgt=Rgt, tgt=tgt, K=K, it_r=it_r, kind=kind, soft=soft, kinds=kinds,
                 grad_out=torch.randn(nsets * it_r, 2, generator=g) * torch.tensor([1.0, 0.05]))
        r64 = tail_ref(c, grad_out=c["grad_out"])
        r21, r32_ = sing_ratios(r64["H"])
        full = torch.tensor([k != "three" for k in kinds])
        if float(r21.min()) < COND or float(r32_[full].min()) < COND:
            return None
        r32 = tail_ref(c, dtype=torch.float32, grad_out=c["grad_out"])
        w = mask.double()
        sw = w.sum(1, keepdim=True)
        Xv, Yv = X.double().repeat_interleave(it_r, 0), Y.double().repeat_interleave(it_r, 0)
        am, bm = (w[..., None] * Xv).sum(1) / sw, (w[..., None] * Yv).sum(1) / sw
        Rm = r64["Rt"][:, :9].reshape(-1, 3, 3)
        d = torch.sign(torch.linalg.det(Rm @ torch.linalg.svd(r64["H"])[0] @ torch.linalg.svd(r64["H"])[2]))   # = Z_33: R = V Z U^T
        tsc = torch.maximum(am.norm(dim=1), bm.norm(dim=1)).clamp_min(1.0)[:, None]
        one = torch.ones((), dtype=torch.float64)
        scale = dict(out=torch.cat([r64["out"][:, :3].abs().clamp_min(1.0), r64["out"][:, 3:]], 1),
                     Rt=torch.cat([one.expand(len(kinds), 9), tsc.expand(-1, 3)], 1),
                     gX=r64["gX"].abs().amax(dim=(1, 2), keepdim=True), gY=r64["gY"].abs().amax(dim=(1, 2), keepdim=True))
        floor = {n: floor32(r32[n], r64[n], scale[n]) for n in scale}
        c.update(ref=r64, scale=scale, floor=floor, am=am, bm=bm, sw=sw[:, 0], full=full, cond=(float(r21.min()), float(r32_[full].min())))
        return c

    return first_seed(build, 50)


# ---- the isotropic set: H with three equal singular values --------------------------------------------------------------------------
# R(H) (the polar factor) is smooth there and the closed-form Kabsch adjoint of mk_train_tail.hip's header stays finite; torch's SVD
# backward does not (its 1 / (s_i^2 - s_j^2) poles).  So the reference is central differences of the whole fp64 tail, and the error
# scale of the case is the header's closed form evaluated in fp32 with torch (tail_closed_form) against that.
def tail_closed_form(c, dtype=torch.float64):
    """gX, gY of the tail by the closed-form adjoint of the Kabsch map (d = +/-1), everything else by autograd with R, t as leaves:
        Q = V^T (dL/dR) U;  C_ij = -(Q_ij - Q_ji) / (s_i + s_j)  [z_i = z_j],  (Q_ij + Q_ji) / (s_o - s_3)  [z_i != z_j, o the other index];
        dL/dH = U C V^T;  H = sum w (x - abar)(y - bbar)^T,  t = bbar - R abar"""
    it_r, it_m = c["it_r"], TAIL_ITM
    X, Y = c["X"].to(dtype), c["Y"].to(dtype)
    Xv, Yv = X.repeat_interleave(it_r, 0), Y.repeat_interleave(it_r, 0)
    w = c["mask"].to(dtype)
    sw = w.sum(1, keepdim=True)
    am, bm = (w[..., None] * Xv).sum(1) / sw, (w[..., None] * Yv).sum(1) / sw
    xc, yc = Xv - am[:, None], Yv - bm[:, None]
    H = xc.transpose(1, 2) @ (w[..., None] * yc)
    U, S, Vh = torch.linalg.svd(H)
    V = Vh.transpose(1, 2)
    d = torch.sign(torch.linalg.det(U @ Vh))
    z = torch.stack([torch.ones_like(d), torch.ones_like(d), d], 1)
    R = ((V * z[:, None]) @ U.transpose(1, 2)).detach().requires_grad_()
    t = (bm[:, None] - am[:, None] @ R.detach().transpose(1, 2)).detach().requires_grad_()
    Xl, Yl = Xv.detach().clone().requires_grad_(), Yv.detach().clone().requires_grad_()
    pair = torch.arange(TAIL_B).repeat_interleave(it_m * it_r)
    g = c["grad_out"].to(dtype)
    with oracle_in(dtype):
        score = O.soft_inliers(Xl, Yl, R, t, f32(TH_SOFT))
        K = c["K"].to(dtype)[pair]
        lv, _, _ = TO.pose_loss(c["kind"], R, t, c["Rgt"].to(dtype)[pair], c["tgt"].to(dtype)[pair].reshape(-1, 1, 3), K, K, bool(c["soft"]))
    ((lv.reshape(-1) * g[:, 0]).sum() + (score.reshape(-1) * g[:, 1]).sum()).backward()
    Gt = t.grad[:, 0]                                               # [nh, 3]
    GR = R.grad - Gt[:, :, None] * am[:, None, :]
    da, db = -(R.detach().transpose(1, 2) @ Gt[..., None])[..., 0], Gt
    Q = V.transpose(1, 2) @ GR @ U
    C = torch.zeros_like(Q)
    for i in range(3):
        for j in range(3):
            if i == j:
                continue
            same = z[:, i] == z[:, j]
            o = j if i == 2 else i
            C[:, i, j] = torch.where(same, -(Q[:, i, j] - Q[:, j, i]) / (S[:, i] + S[:, j]), (Q[:, i, j] + Q[:, j, i]) / (S[:, o] - S[:, 2]))
    GH = U @ C @ V.transpose(1, 2)
    wn = (w / sw)[..., None]
    gXv = Xl.grad + w[..., None] * (yc @ GH.transpose(1, 2)) + wn * da[:, None]
    gYv = Yl.grad + w[..., None] * (xc @ GH) + wn * db[:, None]
    nsets = X.shape[0]
    return dict(gX=gXv.reshape(nsets, it_r, -1, 3).sum(1), gY=gYv.reshape(nsets, it_r, -1, 3).sum(1), S=S)


def tail_central_differences(c, eps=1e-6):
    """gX, gY by central differences of the fp64 tail (it_ransac = 1: a set is a hypothesis, so one pair of evaluations moves the
    same coordinate of every set)"""
    assert c["it_r"] == 1
    g = c["grad_out"].double()
    out = {}
    for name in ("X", "Y"):
        base = c[name].double()
        grad = torch.zeros_like(base)
        for j in range(base.shape[1]):
            for a in range(3):
                vals = []
                for s in (1.0, -1.0):
                    d = dict(c)
                    d[name] = base.clone()
                    d[name][:, j, a] += s * eps
                    o = tail_ref(d)["out"]
                    vals.append(o[:, 0] * g[:, 0] + o[:, 3] * g[:, 1])
                grad[:, j, a] = (vals[0] - vals[1]) / (2 * eps)
        out["g" + name] = grad
    return out


@functools.lru_cache(maxsize=None)
def isotropic_case():
    """six sets of S = 8: an octahedron c +/- e_i (six matches in the mask) and two matches outside every mask, Y = R X + t.  Even
    sets: R a quarter turn about an axis, everything exact in fp32 -- the three singular values of H are EXACTLY 2; odd sets: a generic
    rotation, equal to rounding.  POSE_ERR without clipping, it_ransac = 1."""
    g = gen("isotropic")
    nsets, S = TAIL_B * TAIL_ITM, 8
    ctr = torch.tensor([0.25, -0.125, 4.0], dtype=torch.float64)
    e = torch.eye(3, dtype=torch.float64)
    X = torch.empty(nsets, S, 3, dtype=torch.float64)
    Y = torch.empty_like(X)
    quarter = [torch.tensor([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]]), torch.tensor([[1.0, 0, 0], [0, 0, -1], [0, 1, 0]]),
               torch.tensor([[0.0, 0, 1], [0, 1, 0], [-1, 0, 0]])]
    for r in range(nsets):
        X[r, :6] = torch.cat([ctr + e, ctr - e])
        X[r, 6:] = points(g, 2).double()
        Rm = quarter[r // 2].double() if r % 2 == 0 else rotation(g)
        t = torch.tensor([0.5, 0.25, -0.125], dtype=torch.float64)
        Y[r] = X[r] @ Rm.T + t
        Y[r, 6:] += 0.05 * torch.randn(2, 3, generator=g, dtype=torch.float64)
    mask = torch.zeros(nsets, S)
    mask[:, :6] = 1.0
    Rgt, tgt = torch.stack([rotation(g), rotation(g)]).float(), (torch.rand(TAIL_B, 3, generator=g) - 0.5)
    c = dict(X=X.float(), Y=Y.float(), mask=mask, Rgt=Rgt, tgt=tgt, K=intrinsics(g, TAIL_B), it_r=1, kind="POSE_ERR", soft=0,
             kinds=["octahedron"] * nsets, grad_out=torch.randn(nsets, 2, generator=g) * torch.tensor([1.0, 0.05]))
    fd = tail_central_differences(c)
    cf64, cf32 = tail_closed_form(c), tail_closed_form(c, torch.float32)
    scale = {n: fd[n].abs().amax(dim=(1, 2), keepdim=True) for n in fd}
    c.update(ref=fd, closed64=cf64, closed32=cf32, scale=scale, floor={n: floor32(cf32[n], fd[n], scale[n]) for n in fd},
             sing=torch.linalg.svdvals(tail_ref(c)["H"]))
    return c


# ============================================================ guarded windows for integer outputs ================================
# tests/helpers/guarded.py holds floating-point windows; the solver's indices, counts and flags are int32 and its inlier mask is
# uint8.  Same geometry (256-byte aligned window, at least four rows and 256 bytes of sentinel on either side), same report.
INT_SENTINEL = {torch.int32: 0x7B57A3C5, torch.uint8: 0xA5}     # no index, count or flag; neither 0 nor 1


def guarded_int(rows, cols, dtype, device, fill=None):
    """-> (view [rows, cols] of `dtype`, check): as tests.helpers.guarded.guarded with ld = cols, for int32 and uint8"""
    s = INT_SENTINEL[dtype]
    esz = torch.empty((), dtype=dtype).element_size()
    guard = max(4 * cols, 256 // esz)
    flat = torch.full((256 // esz + guard + rows * cols + guard,), s, dtype=dtype, device=device)
    off = guard + (-(flat.data_ptr() + guard * esz) % 256) // esz
    assert (flat.data_ptr() + off * esz) % 256 == 0 and off >= guard and off + rows * cols + guard <= flat.numel()
    view = flat[off:off + rows * cols].view(rows, cols)
    outside = torch.ones(flat.numel(), dtype=torch.bool, device=device)
    outside[off:off + rows * cols] = False
    if fill is not None:
        view.fill_(fill)

    def check():
        bad = outside & (flat != s)
        if bool(bad.any()):
            rel = int(torch.nonzero(bad)[0]) - off
            raise AssertionError("guard overwritten at (row %d, column %d) of a [%d, %d] %s window: %d of %d guard elements changed"
                                 % (rel // cols, rel % cols, rows, cols, dtype, int(bad.sum()), int(outside.sum())))

    return view, check
