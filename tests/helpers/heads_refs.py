"""References, input builders, bounds and the case lists of the heads' stage-kernel edge tests (tests/test_heads_edges_cpu.py
checks them here on the CPU, tests/test_heads_edges_gpu.py runs the kernels against them).  Pure torch on the CPU.

Every reference is fp64 on the fp32 / 16-bit inputs as passed.  Every bound is |got - ref64| <= bound element-wise, and every part
of a bound is one of
  * an a-priori rounding bound: u = 2^-24; a length-n fp32 sum or dot product in ANY order (fused multiply-adds or not) is within
    gamma(n) * sum |terms| of the exact one, gamma(n) = n u / (1 - n u); a few more u for the single roundings around it; x 1.01
    for the second-order terms;
  * one rounding to the output type (U_OUT) plus its underflow term (UNDERFLOW);
  * a pointwise constant of the device's expf / sigmoid, measured THROUGH the kernels at a one-term shape by
    tests/test_heads_edges_gpu.py on every run (E_EXP, E_SIG below: 2 x the measured maximum)."""
import functools
import zlib

import torch
import torch.nn.functional as F

from oracle import mickey_oracle as O

U = 2.0 ** -24
U_OUT = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
UNDERFLOW = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25}
SLACK = 1.01                     # second-order terms
PLANE_SCALE = 64.0               # ops.SPLIT_ACT_SCALE (asserted equal in the GPU module)

# ---- pointwise constants (measured on an MI355X through the kernels; see test_exp_pointwise_error / test_sigmoid_pointwise_error) ----
E_EXP_MEASURED = 8.21e-8         # (8.205e-8 at x = -7.5816) max |expf(x) - exp(x)| / exp(x), x in [-16, 0]: ks of mk_linattn_kv at L = 1
E_SIG_MEASURED = 8.74e-8         # (8.739e-8 at x = 4.0027) max |1 / (1 + expf(-x)) - sigmoid(x)|, x in [-100, 100]: mk_head_tails with one non-zero weight
E_EXP, E_SIG = 2 * E_EXP_MEASURED, 2 * E_SIG_MEASURED
E_EXP_FINDING, E_SIG_FINDING = 2.4e-7, 2.4e-7   # (2 ulp at 1.0) a larger measured error is a finding about the kernel
E_PHI = max(E_EXP, U)            # phi(x) = x + 1 (one rounding) for x > 0, expf(x) else

LN_EPS = 1e-5
LA_EPS = float(torch.tensor(1e-6, dtype=torch.float32))   # the kernels' 1e-6f
KVW, KV_CHUNK = 272, 64


def gam(n):
    return n * U / (1 - n * U)


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def ratio(got, ref, bound):
    """-> (worst |got - ref| / bound, flat index of it); a non-finite element or an error where the bound is 0 counts as inf."""
    got, ref, bound = got.double().reshape(-1), ref.double().reshape(-1), bound.double().reshape(-1)
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    err = (got - ref).abs()
    inf = torch.full_like(err, float("inf"))
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, inf, torch.zeros_like(err)))
    r = torch.where(torch.isfinite(got), r, inf)
    return float(r.max()), int(r.argmax())


def b_out(e, ref, dtype):
    """the bound of a value within e of ref after its rounding to dtype"""
    if dtype == torch.float32:
        return e
    return (e + U_OUT[dtype] * (ref.abs() + e)) * SLACK + UNDERFLOW[dtype]


# ================================================================ LayerNorm ====================================================
LN_NARROW_D, LN_NARROW_ROWS = [4, 64, 100, 128], [1, 7, 8, 9, 31, 32, 33]            # 8 rows per wave, 32 per block
LN_WIDE_D, LN_WIDE_ROWS = [132, 384, 1024, 1028, 2048], [1, 3, 4, 5, 15, 16, 17]     # 4 rows per wave, 16 per block; MAXV = 8 past 1024
LN_OUT_FORMS = ["f32", "bf16", "f16", "planes", "hi", "resid_only"]
LN_LAYOUT_D = [4, 100, 128, 132, 1028]
# name -> dict(rows_out, rows_per_img, skip, wgroup_rows, bordered (nimg, H, W) or None, groups)
LN_LAYOUTS = {
    "skip": dict(rows_out=3 * 5, rows_per_img=6, skip=1, wgroup_rows=0, bordered=None, groups=1),       # 5 rows an image: no multiple of 4 or 8
    "groups": dict(rows_out=3 * 5, rows_per_img=15, skip=0, wgroup_rows=5, bordered=None, groups=3),    # a wave's rows straddle two (w, b)
    "bordered": dict(rows_out=2 * 30, rows_per_img=60, skip=0, wgroup_rows=30, bordered=(2, 3, 5), groups=2),   # two buffers, W < 8
}


def ln_rows(D):
    return LN_NARROW_ROWS if D <= 128 else LN_WIDE_ROWS


def ln_cases():
    return [(D, rows) for D in LN_NARROW_D + LN_WIDE_D for rows in ln_rows(D)]


def ln_inputs(rows_in, D, groups=1, case="ln"):
    """x fp32 [rows_in, D]: even rows centred, odd rows with a mean of 6 of their standard deviations; w, b [groups, D]; resid"""
    g = gen(case, rows_in, D, groups)
    sd = 0.5 + 2 * torch.rand((rows_in, 1), generator=g)
    x = torch.randn((rows_in, D), generator=g) * sd
    odd = (torch.arange(rows_in) % 2 == 1).float()[:, None]
    sign = torch.where(torch.arange(rows_in) % 4 == 1, 1.0, -1.0)[:, None]
    x = x + odd * sign * 6.0 * sd
    w = torch.randn((groups, D), generator=g)
    b = torch.randn((groups, D), generator=g)
    resid = torch.randn((rows_in, D), generator=g)
    return x, w, b, resid


def ln_row_in(rows_out, rows_per_img, skip):
    """input row of every output row (mickey_hip.h: mk_layernorm)"""
    r = torch.arange(rows_out)
    rpo = rows_per_img - skip
    return (r // rpo) * rows_per_img + skip + r % rpo


def bordered_rows(nimg, H, W):
    return (nimg * (H + 1) + 1) * (W + 1) + 1


def bordered_index(nimg, H, W):
    """row of pixel (b, y, x) in a bordered feature map (asserted equal to ops.bordered_index in test_heads_edges_cpu.py)"""
    m = torch.arange(nimg * H * W)
    q = m // W
    return m + q + (q // H + 1) * (W + 1) + 1


def ln_row_out(rows_out, bordered):
    """output row of every row; bordered = (nimg, H, W): buffers of nimg * H * W pixels, one behind the other"""
    r = torch.arange(rows_out)
    if not bordered:
        return r
    nimg, H, W = bordered
    m = nimg * H * W
    return (r // m) * bordered_rows(nimg, H, W) + bordered_index(nimg, H, W)[r % m]


def ln_group(rows_out, wgroup_rows):
    r = torch.arange(rows_out)
    return r // wgroup_rows if wgroup_rows > 0 else torch.zeros_like(r)


def ln_ref(x, w, b, eps, wgroup_rows=0):
    """fp64 LayerNorm of the rows of x (already selected) with (w, b)[row // wgroup_rows] -> (y64, e32): the a-priori bound of an fp32
    evaluation  mean = sum / D;  d = x - mean;  rstd = 1 / sqrt(sum d^2 / D + eps);  y = d rstd w + b:
      mean:  |dmean| <= gamma(D + 1) sum |x| / D                                                   =: mu
      d:     |dd| <= mu + u (|d| + mu)
      var:   sum (d - dmean)^2 = D var + D dmean^2 exactly (sum d = 0), squares and sum gamma(D + 3), / D and + eps 2 u
      rstd:  relative error <= (gamma(D + 5) var + mu^2) / (2 (var + eps)) + 4 u  (sqrt, reciprocal: <= 2 u each)   =: rho
      y:     rstd |w| |dd| + |d rstd w| (rho + 3 u) + u |y|"""
    rows, D = x.shape
    x64 = x.double()
    grp = ln_group(rows, wgroup_rows)
    w64, b64 = w.double().reshape(-1, D)[grp], b.double().reshape(-1, D)[grp]
    mean = x64.mean(1, keepdim=True)
    d = x64 - mean
    var = (d * d).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = d * rstd * w64 + b64
    mu = gam(D + 1) * x64.abs().sum(1, keepdim=True) / D
    dd = mu + U * (d.abs() + mu)
    rho = (gam(D + 5) * var + mu * mu) / (2 * (var + eps)) + 4 * U
    e = (rstd * w64.abs() * dd + (d * rstd * w64).abs() * (rho + 3 * U) + U * y.abs()) * SLACK
    return y, e


def ln_oracle(x, w, b, eps, wgroup_rows=0):
    """the project's oracle (F.layer_norm) on .double() inputs, group by group"""
    rows, D = x.shape
    wg = wgroup_rows if wgroup_rows > 0 else rows
    w, b = w.double().reshape(-1, D), b.double().reshape(-1, D)
    return torch.cat([F.layer_norm(x[i * wg:(i + 1) * wg].double(), (D,), w[i], b[i], eps) for i in range((rows + wg - 1) // wg)])


def ln_expected(x, w, b, resid, eps, wgroup_rows=0):
    """-> (ref of `out` and of the updated resid (the same number), bound of the fp32 value): resid None = plain LayerNorm"""
    y, e = ln_ref(x, w, b, eps, wgroup_rows)
    if resid is None:
        return y, e
    ref = y + resid.double()
    return ref, (e + U * (ref.abs() + e)) * SLACK


def planes_bounds(ref, e32, scale=PLANE_SCALE):
    """(bound of hi, bound of hi + lo) against scale * ref"""
    s = scale
    sy = (s * ref).abs()
    return 2.0 ** -11 * sy + s * e32, s * e32 + 2.0 ** -22 * sy + 2.0 ** -25


def planes_of(y32, scale=PLANE_SCALE):
    """what a correct fp32 implementation stores: hi = fp16(s y), lo = fp16(s y - hi)"""
    sv = y32.float() * scale
    hi = sv.half()
    return hi, (sv - hi.float()).half()


def ln_fp32(x, w, b, eps, wgroup_rows=0, order=0, cols=None):
    """A correct fp32 implementation; order 0: torch's own sums, 1: columns reversed and summed by an explicit running sum in
    blocks of 7.  cols: the number of columns the statistics run over (a MUTANT when != D: x then has to hold them)."""
    rows = x.shape[0]
    D = w.shape[-1]
    n = D if cols is None else cols
    xs = x[:, :n].float()
    grp = ln_group(rows, wgroup_rows)
    ww, bb = w.reshape(-1, D)[grp], b.reshape(-1, D)[grp]

    def total(t):
        if order == 0:
            return t.sum(1, keepdim=True)
        t = t.flip(1)
        acc = torch.zeros((rows, 1))
        for i in range(0, t.shape[1], 7):
            acc = acc + t[:, i:i + 7].sum(1, keepdim=True)
        return acc

    mean = total(xs) / n
    d = xs - mean
    rstd = 1.0 / torch.sqrt(total(d * d) / n + eps)
    return d[:, :D] * rstd * ww + bb


# ================================================================ linear attention ==============================================
LA_KV_C, LA_KV_L = [16, 64, 96, 128], [1, 3, 4, 5, 63, 64, 65, 129]
LA_KV_LONG = (128, 1938)                               # 31 chunks
LA_G, LA_NIMG = 2, 3
LA_APPLY = [(128, L) for L in (31, 32, 33, 63, 64, 65)] + [(64, L) for L in (63, 64, 65)] + [(96, L) for L in (41, 42, 43)] + [(16, 5)]
LA_OUT_TYPES = [torch.float32, torch.bfloat16, torch.float16]


def la_kv_cases():
    return [(C, L) for C in LA_KV_C for L in LA_KV_L] + [LA_KV_LONG]


@functools.lru_cache(maxsize=None)
def la_inputs(C, L, G=LA_G, nimg=LA_NIMG):
    """qkv fp32 [G, nimg * L, 3C], every image its own data.  Treat as read-only."""
    return torch.randn((G, nimg * L, 3 * C), generator=gen("la", C, L, G, nimg)) * 1.5


def phi64(x):
    return torch.where(x > 0, x + 1.0, x.clamp_max(0.0).exp())


def la_split(qkv, L, C):
    """-> q, k, v [G * nimg, L, H, 16] (views of qkv, its dtype)"""
    x = qkv.reshape(-1, L, 3, C // 16, 16)
    return x[:, :, 0], x[:, :, 1], x[:, :, 2]


def la_chunks(L):
    return (L + KV_CHUNK - 1) // KV_CHUNK


def _kv_block(K, vv):
    """M | ks of tokens [n, s, H, 16] -> [n, H, 272] (the formula at the head of mk_linattn.hip)"""
    n, _, H, _ = K.shape
    M = torch.einsum("nshd,nshv->nhdv", K, vv).reshape(n, H, 256)
    return torch.cat([M, K.sum(1)], -1)


def la_work64(qkv, L, C, drop_last_of_ragged=False, inv_len=None):
    """-> (work64, abs64) [G * nimg, H, nchunk, 272]: the chunk partials and the sums of the |terms|.  The two switches are the
    MUTANTS of test_heads_edges_cpu.py."""
    _, k, v = la_split(qkv.double(), L, C)
    K, vv = phi64(k), v * ((1.0 / L) if inv_len is None else inv_len)
    w, a = [], []
    for c in range(la_chunks(L)):
        s0, s1 = c * KV_CHUNK, min(L, (c + 1) * KV_CHUNK)
        if drop_last_of_ragged and s1 - s0 < KV_CHUNK and s1 - s0 > 1:
            s1 -= 1
        w.append(_kv_block(K[:, s0:s1], vv[:, s0:s1]))
        a.append(_kv_block(K[:, s0:s1], vv[:, s0:s1].abs()))
    return torch.stack(w, 2), torch.stack(a, 2)


def la_work_bound(abs64, L):
    """chunk partial: <= 64 terms, each phi (E_PHI) x (v x fl(1 / L): 2 u) x 1 rounding, summed: gamma(ntok); ks: E_PHI + gamma"""
    ntok = min(L, KV_CHUNK)
    return (gam(ntok + 3) + E_PHI) * abs64 * SLACK


def la_kv_bound(abs64, L):
    """kv = all L terms in some order"""
    return (gam(L + 3) + E_PHI) * abs64.sum(2) * SLACK


def la_apply64(qkv, kv, L, C, eps=LA_EPS):
    """msg from the given kv [G * nimg * H, 272] (fp32 as a kernel left it, or fp64) -> (out64, e32) [G, nimg * L, C]:
      Q = phi(q): E_PHI;  z = Q . ks (16 positive terms): gamma(16) + E_PHI;  den = z + eps, scale = L / den: 2 u
      s = Q . KV[:, v]: (gamma(16) + E_PHI) sum |Q KV|;  out = s scale: u"""
    G = qkv.shape[0]
    H = C // 16
    q, _, _ = la_split(qkv.double(), L, C)
    Q = phi64(q)
    kv = kv.double().reshape(-1, H, KVW)
    M, ks = kv[..., :256].reshape(-1, H, 16, 16), kv[..., 256:]
    den = torch.einsum("nlhd,nhd->nlh", Q, ks) + eps
    scale = (L / den)[..., None]
    out = torch.einsum("nlhd,nhdv->nlhv", Q, M) * scale
    absn = torch.einsum("nlhd,nhdv->nlhv", Q, M.abs()) * scale
    e = ((gam(16) + E_PHI) * absn + out.abs() * (gam(16) + E_PHI + 3 * U)) * SLACK
    return out.reshape(G, -1, C), e.reshape(G, -1, C), den


def phi32(x):
    return torch.where(x > 0, x + 1.0, x.clamp_max(0.0).exp())


def la_work32(qkv, L, C, order=0):
    """chunk partials in torch fp32; order 1: tokens reversed"""
    _, k, v = la_split(qkv, L, C)
    K, vv = phi32(k), v * torch.tensor(1.0 / L, dtype=torch.float32)
    out = []
    for c in range(la_chunks(L)):
        s0, s1 = c * KV_CHUNK, min(L, (c + 1) * KV_CHUNK)
        Kc, vc = K[:, s0:s1], vv[:, s0:s1]
        if order:
            Kc, vc = Kc.flip(1), vc.flip(1)
            blk = torch.zeros((Kc.shape[0], C // 16, KVW))
            for s in range(Kc.shape[1]):
                blk = blk + _kv_block(Kc[:, s:s + 1], vc[:, s:s + 1])
        else:
            blk = _kv_block(Kc, vc)
        out.append(blk)
    return torch.stack(out, 2)


def la_apply32(qkv, kv32, L, C, order=0):
    G = qkv.shape[0]
    H = C // 16
    q, _, _ = la_split(qkv, L, C)
    Q = phi32(q)
    kv = kv32.float().reshape(-1, H, KVW)
    M, ks = kv[..., :256].reshape(-1, H, 16, 16), kv[..., 256:]
    if order:
        Q, M, ks = Q.flip(-1), M.flip(-2), ks.flip(-1)
    den = torch.einsum("nlhd,nhd->nlh", Q, ks) + torch.tensor(1e-6)
    return (torch.einsum("nlhd,nhdv->nlhv", Q, M) * (float(L) / den)[..., None]).reshape(G, -1, C)


# ================================================================ positional encoding ===========================================
PE_TYPES = [torch.float32, torch.float16, torch.bfloat16]
PE_G, PE_NIMG, PE_HW = 3, 2, (3, 5)
PE_BIG = dict(G=3, nimg=2, hw=(127, 87), C=128)        # 3 * 2 * 11049 * 128 / 4 = 2121408 > 8192 * 256: the grid-stride loop's second trip


def pe_cases():
    return [(dt, has_pe, C, wide) for dt in PE_TYPES for has_pe in (True, False) for C in (8, 128) for wide in (False, True)]


def pe_table(C, h, w):
    """fp32 [h * w, C]"""
    return O.sine_pos_encoding(C, h, w).reshape(C, h * w).t().contiguous()


def pe_inputs(dtype, G, nimg, npix, C):
    return (torch.randn((G, nimg * npix, C), generator=gen("pe", G, nimg, npix, C)) * 2).to(dtype)


def pe_ref(x, pe, nimg, shift=0):
    """-> (xs32: the fp32 sum, bit for bit; ref64: the exact sum).  shift = 1: the MUTANT that takes the pe row of pixel p + 1."""
    if pe is None:
        return x.float(), x.double()
    t = pe.roll(-shift, 0).repeat(nimg, 1)[None]
    return x.float() + t, x.double() + t.double()


def pe_cat_bound(ref64, dtype):
    return (U_OUT[dtype] + U) * ref64.abs() + UNDERFLOW[dtype]


# ================================================================ head tails ====================================================
HT_C, HT_CD = [32, 64, 96, 128], [64, 128, 192]
HT_HW = [(5, 5), (7, 7), (11, 9), (33, 32), (51, 38)]
HT_NIMG, HT_DOWN, HT_MAX_DEPTH = 2, 14.0, 60.0
HT_LDS = [dict(nimg=1, h=129, w=127, C=32, Cd=64), dict(nimg=2, h=5, w=13, C=32, Cd=256)]   # 65660 B and 66560 B of dynamic LDS


def ht_cases():
    """(h, w, border, use_softmax, use_depth_sigmoid, norm_dsc, C, Cd): every (h, w) x border x use_softmax, the rest cycling so that
    every value of every switch and width meets every other"""
    out, i = [], 0
    for h, w in HT_HW:
        for border in (0, 3):
            for sm in (1, 0):
                out.append((h, w, border, sm, (i // 2) % 2, (i + i // 4) % 2, HT_C[i % 4], HT_CD[(i + i // 4) % 3]))
                i += 1
    return out


@functools.lru_cache(maxsize=None)
def ht_inputs(nimg, h, w, C, Cd):
    g = gen("ht", nimg, h, w, C, Cd)
    n = h * w
    fd, fo, fz = (torch.randn((nimg * n, C), generator=g) for _ in range(3))
    fdsc = torch.randn((nimg * n, Cd), generator=g)
    ws, wxy, wd = torch.randn((C,), generator=g) * 4, torch.randn((2, C), generator=g) * 0.3, torch.randn((C,), generator=g)
    return dict(fd=fd, fo=fo, fz=fz, fdsc=fdsc, ws=ws, wxy=wxy, wd=wd)


def _interior(h, w, border):
    m = torch.zeros((h, w), dtype=torch.bool)
    m[border:h - border, border:w - border] = True
    return m.reshape(-1)


def _dot(f, wt, nimg, n):
    """-> (logits64 [nimg, n], gamma(C) sum |terms|)"""
    C = f.shape[1]
    f, wt = f.double(), wt.double()
    return (f @ wt).reshape(nimg, n), (gam(C) * (f.abs() @ wt.abs())).reshape(nimg, n)


def ht_ref(c, nimg, h, w, border, use_softmax, use_depth_sigmoid, norm_dsc, down=HT_DOWN, max_depth=HT_MAX_DEPTH, leak=None):
    """fp64 references (through the oracle) and bounds -> dict name -> (ref64, bound), shapes [nimg, 1 | 2 | Cd, n].
    leak: a flat pixel index whose border mask is NOT applied (the MUTANT of test_heads_edges_cpu.py)."""
    n = h * w
    C, Cd = c["fd"].shape[1], c["fdsc"].shape[1]

    def nchw(f, ch):
        return f.double().reshape(nimg, h, w, ch).permute(0, 3, 1, 2)

    inside = _interior(h, w, border)
    a, ea = _dot(c["fd"], c["ws"], nimg, n)
    logit = F.conv2d(nchw(c["fd"], C), c["ws"].double().view(1, C, 1, 1))
    if use_softmax:
        scr = O.border_softmax(logit, border).reshape(nimg, 1, n) if leak is None else None
        if leak is not None:
            m = inside.clone()
            m[leak] = True
            e = torch.exp((a - (a.mean(1, keepdim=True) + 1e-16)) / 100.0) * m
            scr = (e / (e.sum(1, keepdim=True) + 1e-16))[:, None]
        # mean: the logits' own error + gamma(n + 1) sum |a| / n; argument of exp: that + 2 u |a - mean|, / 100 (u);
        # e: relative (argument error + E_EXP); sum of positive e: gamma(n); 1 / (sum + eps): 2 u; e * inv: u
        emean = ea.mean(1, keepdim=True) + gam(n + 1) * a.abs().mean(1, keepdim=True)
        darg = (ea + emean + 3 * U * (a - a.mean(1, keepdim=True)).abs()) / 100.0
        rel = darg + darg.max(1, keepdim=True).values + 2 * E_EXP + gam(n) + 3 * U
        bscr = (scr[:, 0] * rel * SLACK)[:, None]
    else:
        m = inside.double() if leak is None else (inside | (torch.arange(n) == leak)).double()
        scr = (torch.sigmoid(logit).reshape(nimg, 1, n) * m)
        bscr = ((0.25 * ea + E_SIG) * SLACK * inside.double())[:, None]
    ax, eax = _dot(c["fo"], c["wxy"][0], nimg, n)
    ay, eay = _dot(c["fo"], c["wxy"][1], nimg, n)
    kps = O.abs_keypoints(torch.sigmoid(F.conv2d(nchw(c["fo"], C), c["wxy"].double().view(2, C, 1, 1))), down).reshape(nimg, 2, n)
    bk = (torch.stack([eax, eay], 1) * 0.25 + E_SIG) * down * SLACK + 2 * U * kps.abs()
    d, ed = _dot(c["fz"], c["wd"], nimg, n)
    if use_depth_sigmoid:
        depth = (max_depth * torch.sigmoid(d))[:, None]
        bd = ((0.25 * ed + E_SIG) * max_depth * SLACK + U * depth[:, 0].abs())[:, None]
    else:
        depth, bd = d[:, None], ed[:, None] * SLACK
    x = nchw(c["fdsc"], Cd)
    if norm_dsc:
        dsc = (x / x.pow(2).sum(1, keepdim=True).add(1e-10).pow(0.5)).reshape(nimg, Cd, n)
        bdsc = (0.5 * gam(Cd + 1) + 5 * U) * dsc.abs() * SLACK   # sum of squares gamma(Cd) (halved by the root), sqrt, 1 / x, product
    else:
        dsc = x.reshape(nimg, Cd, n)
        bdsc = torch.zeros_like(dsc)
    out = dict(scr=(scr, bscr), kps=(kps, bk), depth=(depth, bd), dsc=(dsc, bdsc))
    out = {k: (r.contiguous(), e.contiguous()) for k, (r, e) in out.items()}
    out["inside"] = inside
    return out


def ht_fp32(c, nimg, h, w, border, use_softmax, use_depth_sigmoid, norm_dsc, order=0, down=HT_DOWN, max_depth=HT_MAX_DEPTH):
    """the tails in torch fp32; order 1: channels and pixels reversed in every sum"""
    n = h * w

    def dot(f, wt):
        if order:
            f, wt = f.flip(1), wt.flip(0)
            acc = torch.zeros(f.shape[0])
            for i in range(0, f.shape[1], 5):
                acc = acc + (f[:, i:i + 5] * wt[i:i + 5]).sum(1)
            return acc.reshape(nimg, n)
        return (f @ wt).reshape(nimg, n)

    def tot(t):
        return (t.flip(1) if order else t).sum(1, keepdim=True)

    inside = _interior(h, w, border).float()
    a = dot(c["fd"], c["ws"])
    if use_softmax:
        e = torch.exp((a - (tot(a) / n + 1e-16)) / 100.0) * inside
        scr = e * (1.0 / (tot(e) + 1e-16))
    else:
        scr = torch.sigmoid(a) * inside
    p = torch.arange(n)
    cell = torch.stack([(p % w).float(), (p // w).float()])[None]
    kps = (torch.sigmoid(torch.stack([dot(c["fo"], c["wxy"][0]), dot(c["fo"], c["wxy"][1])], 1)) + cell) * down
    d = dot(c["fz"], c["wd"])
    depth = max_depth * torch.sigmoid(d) if use_depth_sigmoid else d
    f = c["fdsc"]
    sc = 1.0 / torch.sqrt(tot(f * f) + 1e-10) if norm_dsc else torch.ones((f.shape[0], 1))
    dsc = (f * sc).reshape(nimg, n, -1).permute(0, 2, 1)
    return dict(scr=scr[:, None], kps=kps, depth=depth[:, None], dsc=dsc)
