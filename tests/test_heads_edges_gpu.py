"""-m gpu: the heads' own stage kernels -- LayerNorm (mk_norm.hip: narrow and wide kernel, MAXV = 4 and 8, every output form), the
unfused linear attention (mk_linattn.hip: chunk partials, kv, apply), mk_posenc_add and mk_head_tails (mk_heads.hip) -- ELEMENT by
element against fp64, at the smallest shapes where a ragged wave, a chunk boundary, a block-stride loop or a row map can go wrong.
Every output sits inside guard rows (tests/helpers/guarded.py) and is found fully overwritten, every input is a view into a NaN
buffer, a failure names the element and where in its wave, chunk or block it sits.

Bounds (tests/helpers/heads_refs.py states them term by term; tests/test_heads_edges_cpu.py shows that a correct fp32
implementation meets them in two summation orders and that subtly wrong ones do not): |got - ref64| <= bound, each part of a bound
being an a-priori rounding bound (u = 2^-24, gamma(n) sum |terms| for a length-n fp32 sum in any order), one rounding to the output
type plus its underflow term, or one of two pointwise constants of the device's expf, measured through the kernels themselves at
a one-term shape and re-measured on every run:
  E_EXP = 2 x 8.21e-8  relative error of expf(x), x in [-16, 0]: Ksum of mk_linattn_kv at L = 1 (measured on an MI355X: 8.205e-8
                       at x = -7.5816 over 2^18 values; finding threshold 2.4e-7)
  E_SIG = 2 x 8.74e-8  absolute error of 1 / (1 + expf(-x)), x in [-100, 100]: scr / depth of mk_head_tails with one non-zero weight
                       (measured: 8.739e-8 at x = 4.0027 over 2^16 values; finding threshold 2.4e-7)
det_norm_kernel's expf((a - mean) / 100) cannot be isolated at any shape (the normalisation divides it out at one pixel); it is
the same device function at |argument| < 2, of either sign, and takes E_EXP -- the one part of a bound that is carried over from a
neighbouring range rather than measured on its own (the softmax scores use 1.4 % of their bound).
Plane outputs at s = SPLIT_ACT_SCALE: |hi - s y64| <= 2^-11 |s y64| + s e32, |hi + lo - s y64| <= s e32 + 2^-22 |s y64| + 2^-25.
kv equals its chunk partials added in chunk order bit for bit; xs of mk_posenc_add equals the fp32 sum bit for bit; border scores
are exactly 0.  Measured worst ratios: profiles/heads_edges_parity.txt."""
import pytest
import torch

from tests.helpers import heads_refs as R
from tests.helpers.guarded import bits, guarded, sentinel_bits

pytestmark = pytest.mark.gpu

WORST = {}     # (kernel, output / type) -> largest |error| / bound seen in this process
MEASURED = {}  # pointwise constant -> value measured in this process


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _nv():
    from mickey_amd import _native
    return _native


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    for (kernel, what), r in sorted(WORST.items()):
        print("heads edges worst |err| / bound: %-24s %-14s %.3f" % (kernel, what, r))
    for name, v in sorted(MEASURED.items()):
        print("heads edges pointwise constant: %s measured %.4g" % (name, v))


def _name(dtype):
    return str(dtype).replace("torch.", "")


def _poisoned(t, dev, extra_cols=8, extra_rows=4):
    """Device copy of t (its last dimension = a row) as a view into a NaN buffer with `extra_cols` more columns per row and
    `extra_rows` more rows: whatever a kernel reads past a row's end or past the last row shows in its outputs."""
    t2 = t.reshape(-1, t.shape[-1])
    r, c = t2.shape
    buf = torch.full((r + extra_rows, c + extra_cols), float("nan"), dtype=t.dtype, device=dev)
    buf[:r, :c] = t2.to(dev)
    return buf[:r, :c]


def _written(t):
    return not bool((bits(t) == sentinel_bits(t.dtype)).any())


def _untouched(t):
    return bool((bits(t) == sentinel_bits(t.dtype)).all())


def _within(kernel, kind, got, ref, bound, what, where):
    """|got - ref| <= bound element-wise; on failure the worst ratio and where(flat index) -> the element and its place."""
    got = got.detach().double().cpu().reshape(ref.shape)
    worst, i = R.ratio(got, ref, bound)
    key = (kernel, kind)
    WORST[key] = max(WORST.get(key, 0.0), worst)
    if not worst <= 1.0:
        e = (got - ref).abs().reshape(-1)
        outside = int((e > bound.reshape(-1)).sum() + (~torch.isfinite(got)).sum())
        raise AssertionError("%s %s, %s: |err| / bound = %.3g at %s: got %r, fp64 %r, bound %.3g; %d of %d elements outside"
                             % (kernel, kind, what, worst, where(i), float(got.reshape(-1)[i]), float(ref.reshape(-1)[i]),
                                float(bound.reshape(-1)[i]), outside, e.numel()))


# ================================================================ LayerNorm ====================================================
def _ln_where(D):
    def where(i):
        r, c = i // D, i % D
        if D <= 128:
            return ("row %d, column %d = block %d, wave %d, row pair %d, half %d, lane %d"
                    % (r, c, r // 32, (r // 8) % 4, (r % 8) // 2, r % 2, 32 * (r % 2) + c // 4))
        return "row %d, column %d = block %d, wave %d, row %d of the wave, lane %d, vector %d" % (r, c, r // 16, (r // 4) % 4, r % 4, (c // 4) % 64, c // 256)
    return where


def _ln_run(form, x, w, b, resid0, D, rows_out, rows_per_img, skip, wgroup_rows, bordered, half, dev, what):
    """One ops.layernorm call in output form `form` (R.LN_OUT_FORMS) on the CPU inputs; x [rows_in, D], resid0 [rows_out, D] or None.
    half: the output is the second column half of 2 D-wide rows.  Checks guards, coverage and values."""
    from mickey_amd import ops
    row_in, row_out = R.ln_row_in(rows_out, rows_per_img, skip), R.ln_row_out(rows_out, bordered)
    ref, e = R.ln_expected(x[row_in], w, b, resid0, R.LN_EPS, wgroup_rows)
    nbuf = rows_out if not bordered else rows_out // (bordered[0] * bordered[1] * bordered[2]) * R.bordered_rows(*bordered)
    xd = _poisoned(x, dev)
    wd, bd = _poisoned(w, dev, extra_cols=0)[:w.shape[0]], _poisoned(b, dev, extra_cols=0)[:b.shape[0]]
    checks, resid = [], None
    if resid0 is not None:
        resid, chk = guarded(rows_out, D, torch.float32, dev, ld=D + 8, fill=resid0)
        checks.append(chk)
    odt = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "planes": torch.float16, "hi": torch.float16}.get(form)
    outs, full = [], []
    for _ in range(0 if odt is None else (2 if form == "planes" else 1)):
        win, chk = guarded(nbuf, 2 * D if half else D, odt, dev, ld=(2 * D if half else D) + 8)
        checks.append(chk)
        full.append(win)
        outs.append(win[:, D:] if half else win)
    kw = dict(resid=resid, rows_out=rows_out, rows_per_img=rows_per_img, skip=skip, wgroup_rows=wgroup_rows, bordered=bordered)
    if form in ("planes", "hi"):
        ops.layernorm(xd, wd, bd, R.LN_EPS, out=(outs[0], outs[1] if form == "planes" else None), **kw)
    elif form == "resid_only":
        assert ops.layernorm(xd, wd, bd, R.LN_EPS, out=None, out_dtype=None, **kw) is None
    else:
        ops.layernorm(xd, wd, bd, R.LN_EPS, out=outs[0], **kw)
    torch.cuda.synchronize()
    for chk in checks:
        chk()
    where = _ln_where(D)
    rest = torch.ones(nbuf, dtype=torch.bool)
    rest[row_out] = False
    for o, f in zip(outs, full):
        assert _written(o[row_out.to(dev)]), what + ": output elements left unwritten"
        assert _untouched(o[rest.to(dev)]) if bool(rest.any()) else True, what + ": a border row was written"
        assert not half or _untouched(f[:, :D]), what + ": the first column half was written"
    kernel = "layernorm narrow" if D <= 128 else ("layernorm wide" if D <= 1024 else "layernorm wide MAXV=8")
    if resid is not None:
        _within(kernel, "resid", resid, ref, e, what, where)
    if form in ("f32", "bf16", "f16"):
        _within(kernel, _name(odt), outs[0][row_out.to(dev)], ref, R.b_out(e, ref, odt), what, where)
        if resid is not None and form == "f32":
            assert torch.equal(outs[0][row_out.to(dev)], resid), what + ": out is not the updated resid"
    elif form in ("planes", "hi"):
        bh, bs = R.planes_bounds(ref, e)
        hi = outs[0][row_out.to(dev)].double().cpu()
        _within(kernel, "hi plane", hi, R.PLANE_SCALE * ref, bh, what, where)
        if form == "planes":
            _within(kernel, "hi + lo", hi + outs[1][row_out.to(dev)].double().cpu(), R.PLANE_SCALE * ref, bs, what, where)


@pytest.mark.parametrize("D", R.LN_NARROW_D + R.LN_WIDE_D)
def test_layernorm_elementwise(D):
    """Every row count around the rows a wave and a block own, every output form, with and without the residual (ldx = ldo = ldr =
    D + 8)."""
    from mickey_amd import ops
    dev = _dev()
    assert ops.SPLIT_ACT_SCALE == R.PLANE_SCALE
    for rows in R.ln_rows(D):
        x, w, b, resid = R.ln_inputs(rows, D)
        for form in R.LN_OUT_FORMS:
            for with_resid in ((True,) if form == "resid_only" else (False, True)):
                what = "D=%d rows=%d %s resid=%d" % (D, rows, form, with_resid)
                _ln_run(form, x, w, b, resid if with_resid else None, D, rows, rows, 0, 0, None, False, dev, what)


@pytest.mark.parametrize("D", R.LN_LAYOUT_D)
@pytest.mark.parametrize("layout", sorted(R.LN_LAYOUTS))
def test_layernorm_row_maps(layout, D):
    """skip = 1 with 5 rows an image, (w, b) groups of 5 rows, two bordered buffers of 2 x 3 x 5 pixels; the output is the second
    half of 2 D-wide rows, ldx, ldo, ldr all larger than D."""
    dev = _dev()
    lay = R.LN_LAYOUTS[layout]
    rows_in = lay["rows_out"] // (lay["rows_per_img"] - lay["skip"]) * lay["rows_per_img"]
    x, w, b, _ = R.ln_inputs(rows_in, D, lay["groups"], case=layout)
    resid = R.ln_inputs(lay["rows_out"], D, 1, case=layout + " resid")[3]
    for form in ("f32", "bf16", "f16", "planes", "hi"):
        for with_resid in (False, True):
            what = "%s D=%d %s resid=%d" % (layout, D, form, with_resid)
            _ln_run(form, x, w, b, resid if with_resid else None, D, lay["rows_out"], lay["rows_per_img"], lay["skip"], lay["wgroup_rows"],
                    lay["bordered"], True, dev, what)


# ================================================================ linear attention ==============================================
def _kv_where(H, nchunk):
    def where(i):
        e = i % R.KVW
        chunk = (i // R.KVW) % nchunk if nchunk else 0
        rest = i // R.KVW // max(nchunk, 1)
        what = "KV[d=%d][v=%d]" % (e // 16, e % 16) if e < 256 else "Ksum[d=%d]" % (e - 256)
        return "image %d, head %d, %s%s" % (rest // H, rest % H, "chunk %d of %d, " % (chunk, nchunk) if nchunk else "", what)
    return where


def _linattn_kv(qkv, L, C, dev, G=R.LA_G, nimg=R.LA_NIMG):
    """ops.linattn_kv on guarded kv / work, the rows past qkv's last poisoned -> (kv [G nimg H, 272], work [G nimg, H, nchunk, 272])"""
    from mickey_amd import ops
    H, nchunk = C // 16, R.la_chunks(L)
    qd = _poisoned(qkv, dev, extra_cols=0)
    kv, ck = guarded(G * nimg * H, R.KVW, torch.float32, dev)
    nwork = ops.linattn_work_floats(G, nimg, L, C)
    assert nwork == G * nimg * H * nchunk * R.KVW
    work, cw = guarded(1, nwork, torch.float32, dev)
    ops.linattn_kv(qd, kv, work, G, nimg, L, C)
    torch.cuda.synchronize()
    ck()
    cw()
    assert _written(kv) and _written(work), "kv or work: elements left unwritten"
    return qd, kv, work.view(G * nimg, H, nchunk, R.KVW)


@pytest.mark.parametrize("C,L", R.la_kv_cases())
def test_linattn_kv_elementwise(C, L):
    """G x nimg = 2 x 3, every image its own data: the chunk partials and kv element-wise, kv = its partials added in chunk order."""
    dev = _dev()
    qkv = R.la_inputs(C, L)
    work64, abs64 = R.la_work64(qkv, L, C)
    _, kv, work = _linattn_kv(qkv, L, C, dev)
    H, nchunk = C // 16, R.la_chunks(L)
    what = "C=%d L=%d" % (C, L)
    _within("linattn_kv", "work", work, work64, R.la_work_bound(abs64, L), what, _kv_where(H, nchunk))
    _within("linattn_kv", "kv", kv, work64.sum(2), R.la_kv_bound(abs64, L), what, _kv_where(H, 0))
    w = work.cpu()
    s = torch.zeros_like(w[:, :, 0])
    for c in range(nchunk):
        s = s + w[:, :, c]
    assert torch.equal(s.reshape(-1, R.KVW), kv.cpu()), what + ": kv is not its chunk partials added in chunk order"


@pytest.mark.parametrize("C,L", R.LA_APPLY)
def test_linattn_apply_elementwise(C, L):
    """fp32, bf16 and fp16 output with ldo = C + 8, against fp64 on the kernel's own kv."""
    from mickey_amd import ops
    dev = _dev()
    qkv = R.la_inputs(C, L)
    qd, kv, _ = _linattn_kv(qkv, L, C, dev)
    ref, e, _ = R.la_apply64(qkv, kv.cpu(), L, C)
    H = C // 16
    tpb = 256 // H

    def where(i):
        row, c = i // C, i % C
        s = row % L
        return ("group %d, image %d, token %d, channel %d = block %d, thread %d (token %d of %d in the block, head %d, v = %d)"
                % (row // (R.LA_NIMG * L), (row // L) % R.LA_NIMG, s, c, s // tpb, (s % tpb) * H + c // 16, s % tpb, tpb, c // 16, c % 16))

    for dt in R.LA_OUT_TYPES:
        out, check = guarded(R.LA_G * R.LA_NIMG * L, C, dt, dev, ld=C + 8)
        ops.linattn_apply(qd, kv, out, C + 8, R.LA_G, R.LA_NIMG, L, C)
        torch.cuda.synchronize()
        check()
        what = "C=%d L=%d %s" % (C, L, _name(dt))
        assert _written(out), what + ": output elements left unwritten"
        _within("linattn_apply", _name(dt), out, ref.reshape(-1, C), R.b_out(e, ref, dt).reshape(-1, C), what, where)


def test_exp_pointwise_error():
    """E_EXP: at L = 1 and v = 1, Ksum[d] of mk_linattn_kv is phi(k[d]) itself (one term, three zero partials, 1 / L = 1) and
    KV[d][v] the same number: 2^18 values of k in [-16, 0] (every input of the tests above lies inside), against fp64 exp."""
    dev = _dev()
    C, n = 128, 2048
    k = torch.cat([torch.linspace(-16.0, 0.0, n * C - 4), torch.tensor([-0.0, -2.0 ** -126, -2.0 ** -24, -1.0])])
    qkv = torch.zeros((1, n, 3 * C))
    qkv[0, :, C:2 * C] = k.reshape(n, C)
    qkv[0, :, 2 * C:] = 1.0
    _, kv, work = _linattn_kv(qkv, 1, C, dev, G=1, nimg=n)
    ks = kv.cpu().reshape(n, C // 16, R.KVW)[..., 256:].reshape(-1).double()
    assert torch.equal(kv.cpu(), work.cpu().reshape(-1, R.KVW))
    M = kv.cpu().reshape(n, C // 16, R.KVW)[..., :256].reshape(n, C // 16, 16, 16)
    assert torch.equal(M, kv.cpu().reshape(n, C // 16, R.KVW)[..., 256:, None].expand(-1, -1, -1, 16)), "KV[d][v] != phi(k[d]) * 1"
    ref = k.double().exp()
    rel = (ks - ref).abs() / ref
    worst, i = float(rel.max()), int(rel.argmax())
    MEASURED["E_EXP (relative, expf on [-16, 0])"] = worst
    print("expf through mk_linattn_kv: max relative error %.4g at x = %r over %d values (constant: %.4g measured, E_EXP = %.4g)"
          % (worst, float(k[i]), k.numel(), R.E_EXP_MEASURED, R.E_EXP))
    assert worst <= R.E_EXP_FINDING, worst
    assert worst <= R.E_EXP_MEASURED * 1.0001, "E_EXP_MEASURED is stale: %.6g measured" % worst


# ================================================================ positional encoding ===========================================
def _posenc(dtype, has_pe, G, nimg, h, w, C, wide, dev):
    from mickey_amd import ops
    npix = h * w
    rows = G * nimg * npix
    x = R.pe_inputs(dtype, G, nimg, npix, C)
    pe = R.pe_table(C, h, w) if has_pe else None
    xs32, ref = R.pe_ref(x, pe, nimg)
    xs, cx = guarded(rows, C, torch.float32, dev)
    cat, cc = guarded(rows, C, dtype, dev, ld=2 * C if wide else C)
    ops.posenc_add(_poisoned(x, dev, extra_cols=0), _poisoned(pe, dev, extra_cols=0) if has_pe else None, xs, cat, G, nimg, npix, C)
    torch.cuda.synchronize()
    cx()
    cc()     # with ld_cat = 2 C the second column half is row slack: still the sentinel
    what = "%s pe=%d C=%d ld_cat=%d npix=%d" % (_name(dtype), has_pe, C, 2 * C if wide else C, npix)
    assert _written(xs) and _written(cat), what + ": output elements left unwritten"

    def where(i):
        r, c = i // C, i % C
        return "group %d, image %d, pixel %d, channel %d = vector %d: block %d (mod the grid), thread %d" % (
            r // (nimg * npix), (r // npix) % nimg, r % npix, c, i // 4, (i // 4 // 256) % 8192, (i // 4) % 256)

    got = xs.cpu().reshape(xs32.shape)
    if not torch.equal(got, xs32):
        i = int(torch.nonzero((got != xs32).reshape(-1))[0])
        raise AssertionError("posenc_add %s: xs is not the fp32 sum at %s: got %r, expected %r"
                             % (what, where(i), float(got.reshape(-1)[i]), float(xs32.reshape(-1)[i])))
    _within("posenc_add", "cat " + _name(dtype), cat, ref.reshape(-1, C), R.pe_cat_bound(ref, dtype).reshape(-1, C), what, where)


@pytest.mark.parametrize("dtype,has_pe,C,wide", R.pe_cases())
def test_posenc_add_elementwise(dtype, has_pe, C, wide):
    """G = 3, nimg = 2, 3 x 5 pixels: pix wraps per image and per group."""
    h, w = R.PE_HW
    _posenc(dtype, has_pe, R.PE_G, R.PE_NIMG, h, w, C, wide, _dev())


def test_posenc_add_past_the_grid_cap():
    """more float4 than 8192 blocks x 256 threads: the grid-stride loop takes a second trip"""
    b = R.PE_BIG
    _posenc(torch.bfloat16, True, b["G"], b["nimg"], b["hw"][0], b["hw"][1], b["C"], False, _dev())


# ================================================================ head tails ====================================================
def _head_tails(c, nimg, h, w, border, sm, dsig, nd, dev, down=R.HT_DOWN, max_depth=R.HT_MAX_DEPTH):
    """mk_head_tails as ops.head_tails calls it, outputs in guarded windows -> dict of CPU tensors [nimg, 1 | 2 | Cd, n]"""
    nv = _nv()
    n = h * w
    C, Cd = c["fd"].shape[1], c["fdsc"].shape[1]
    ins = [_poisoned(c[k], dev, extra_cols=0) for k in ("fd", "ws", "fo", "wxy", "fz", "wd", "fdsc")]
    outs = {name: guarded(nimg * ch, n, torch.float32, dev) for name, ch in (("scr", 1), ("kps", 2), ("depth", 1), ("dsc", Cd))}
    nv.call("mk_head_tails", *[nv.ptr(t) for t in ins], *[nv.ptr(outs[k][0]) for k in ("scr", "kps", "depth", "dsc")], nimg, h, w, C, Cd,
            border, int(sm), int(dsig), float(max_depth), int(nd), float(down), nv.stream())
    torch.cuda.synchronize()
    for name, (o, chk) in outs.items():
        chk()
        assert _written(o), name + ": output elements left unwritten"
    return {name: o.cpu().reshape(nimg, -1, n) for name, (o, _) in outs.items()}


def _ht_check(c, nimg, h, w, border, sm, dsig, nd, dev):
    n = h * w
    C, Cd = c["fd"].shape[1], c["fdsc"].shape[1]
    what = "h=%d w=%d border=%d softmax=%d depth_sigmoid=%d norm_dsc=%d C=%d Cd=%d" % (h, w, border, sm, dsig, nd, C, Cd)
    got = _head_tails(c, nimg, h, w, border, sm, dsig, nd, dev)
    r = R.ht_ref(c, nimg, h, w, border, sm, dsig, nd)

    def where_of(ch):
        def where(i):
            p = i % n
            return ("image %d, channel %d, pixel %d = (y %d, x %d): det_norm thread %d trip %d; dsc block %d, pixel %d of its 64; tail wave %d"
                    % (i // (ch * n), (i // n) % ch, p, p // w, p % w, p % 1024, p // 1024, p // 64, p % 64, (i // (ch * n)) * n + p))
        return where

    inside = r["inside"]
    edge = got["scr"][:, 0, ~inside]
    assert bool((edge == 0).all()), what + ": %d border scores are not exactly 0" % int((edge != 0).sum())
    _within("head_tails", "scr softmax" if sm else "scr sigmoid", got["scr"], r["scr"][0], r["scr"][1], what, where_of(1))
    if sm and bool(inside.any()):
        tot = got["scr"].double().sum((1, 2))
        assert bool(((tot - r["scr"][0].sum((1, 2))).abs() <= r["scr"][1].sum((1, 2))).all()), what + ": scores sum to %r" % tot.tolist()
    _within("head_tails", "kps", got["kps"], r["kps"][0], r["kps"][1], what, where_of(2))
    _within("head_tails", "depth sigmoid" if dsig else "depth", got["depth"], r["depth"][0], r["depth"][1], what, where_of(1))
    if nd:
        _within("head_tails", "dsc", got["dsc"], r["dsc"][0], r["dsc"][1], what, where_of(Cd))
    else:
        assert torch.equal(got["dsc"], c["fdsc"].reshape(nimg, n, Cd).permute(0, 2, 1)), what + ": dsc is not the transposed input"


@pytest.mark.parametrize("h,w,border,sm,dsig,nd,C,Cd", R.ht_cases())
def test_head_tails_elementwise(h, w, border, sm, dsig, nd, C, Cd):
    """2 images (n odd at 5 x 5, 7 x 7, 11 x 9: dsc's transposed [Cd, n] rows start unaligned); 5 x 5 with border 3 is all border,
    7 x 7 has one interior pixel (score 1 within the bound), 33 x 32 gives det_norm_kernel's 1024 threads a second trip."""
    _ht_check(R.ht_inputs(R.HT_NIMG, h, w, C, Cd), R.HT_NIMG, h, w, border, sm, dsig, nd, _dev())


@pytest.mark.parametrize("k", range(len(R.HT_LDS)))
def test_head_tails_past_64_kib_of_lds(k):
    """det_norm_kernel at 129 x 127 pixels and dsc_tail_kernel at Cd = 256 take more than 64 KiB of dynamic LDS (mk_head_tails
    reserves up to the 160 KiB its argument check admits)."""
    d = R.HT_LDS[k]
    c = R.ht_inputs(d["nimg"], d["h"], d["w"], d["C"], d["Cd"])
    for sm in (1, 0):
        _ht_check(c, d["nimg"], d["h"], d["w"], 3, sm, 0, 1, _dev())


def test_sigmoid_pointwise_error():
    """E_SIG: with one non-zero weight (1.0) the logit IS the feature value (products with 0, a sum of one term), so scr without
    softmax and border, and depth with max_depth = 1, are 1 / (1 + expf(-x)) of it: 2^16 values in [-100, 100] against fp64."""
    dev = _dev()
    nimg, h, w, C, Cd = 16, 64, 64, 32, 64
    n = h * w
    g = R.gen("sigmoid sweep")
    v = torch.cat([torch.linspace(-100.0, 100.0, nimg * n - 4), torch.tensor([0.0, -0.0, 2.0 ** -126, -88.5])])
    c = dict(fd=torch.randn((nimg * n, C), generator=g), fo=torch.zeros((nimg * n, C)), fz=torch.randn((nimg * n, C), generator=g),
             fdsc=torch.ones((nimg * n, Cd)), ws=torch.zeros(C), wxy=torch.zeros((2, C)), wd=torch.zeros(C))
    c["fd"][:, 5], c["fz"][:, 31] = v, v
    c["ws"][5], c["wd"][31] = 1.0, 1.0
    got = _head_tails(c, nimg, h, w, 0, 0, 1, 1, dev, max_depth=1.0)
    ref = torch.sigmoid(v.double())
    worst = 0.0
    for name in ("scr", "depth"):
        err = (got[name].double().reshape(-1) - ref).abs()
        assert bool(torch.isfinite(got[name]).all())
        print("sigmoid through mk_head_tails %s: max |err| %.4g at x = %r over %d values" % (name, float(err.max()), float(v[int(err.argmax())]), v.numel()))
        worst = max(worst, float(err.max()))
    assert torch.equal(got["kps"][:, 0].reshape(nimg, h, w), ((0.5 + torch.arange(w).float()) * R.HT_DOWN).expand(nimg, h, w))
    MEASURED["E_SIG (absolute, 1 / (1 + expf(-x)) on [-100, 100])"] = worst
    print("sigmoid: measured %.4g (constant: %.4g measured, E_SIG = %.4g)" % (worst, R.E_SIG_MEASURED, R.E_SIG))
    assert worst <= R.E_SIG_FINDING, worst
    assert worst <= R.E_SIG_MEASURED * 1.0001, "E_SIG_MEASURED is stale: %.6g measured" % worst
