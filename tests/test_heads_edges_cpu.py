"""No GPU: the references, bounds and input builders of tests/test_heads_edges_gpu.py (tests/helpers/heads_refs.py) are what that
file takes them for -- each fp64 reference is the project's oracle on .double() inputs, every bound admits a correct fp32
implementation in two summation orders and rejects a subtly wrong one on at least one case of the lists, the inputs exercise what
they are meant to -- and the host-side argument checks of the heads' entry points refuse what they promise to refuse before
anything is launched."""
import os

import pytest
import torch
import torch.nn.functional as F

from oracle import mickey_oracle as O
from tests.helpers import heads_refs as R


def _close(a, b, rtol=1e-12):
    return bool(((a - b).abs() <= rtol * (b.abs() + b.abs().max())).all())     # (sums that cancel: relative to the largest element)


def _ok(got, ref, bound):
    return R.ratio(got, ref, bound)[0] <= 1.0


# ---- references = the oracle on .double() inputs ------------------------------------------------------------------------------
def test_layernorm_reference_is_the_oracle():
    for D, rows in R.ln_cases():
        x, w, b, _ = R.ln_inputs(rows, D)
        y, e = R.ln_ref(x, w, b, R.LN_EPS)
        assert _close(y, F.layer_norm(x.double(), (D,), w[0].double(), b[0].double(), R.LN_EPS), 1e-11), (D, rows)
        assert bool((e > 0).all()) and bool(torch.isfinite(e).all())
    for name, lay in R.LN_LAYOUTS.items():
        for D in R.LN_LAYOUT_D:
            rows_in = lay["rows_out"] // (lay["rows_per_img"] - lay["skip"]) * lay["rows_per_img"]
            x, w, b, _ = R.ln_inputs(rows_in, D, lay["groups"], case=name)
            xs = x[R.ln_row_in(lay["rows_out"], lay["rows_per_img"], lay["skip"])]
            y, _ = R.ln_ref(xs, w, b, R.LN_EPS, lay["wgroup_rows"])
            assert _close(y, R.ln_oracle(xs, w, b, R.LN_EPS, lay["wgroup_rows"]), 1e-11), (name, D)
    # the row maps: skip = 1 drops row 0 of every image; a wave's rows straddle two groups
    assert R.ln_row_in(15, 6, 1).tolist() == [1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 13, 14, 15, 16, 17]
    assert R.ln_group(15, 5).tolist()[3:6] == [0, 0, 1] and R.ln_group(15, 5).tolist()[7:11] == [1, 1, 1, 2]


def test_bordered_row_map_is_ops_bordered_index():
    from mickey_amd import ops
    for nimg, H, W in ((2, 3, 5), (1, 1, 1), (3, 7, 2), (2, 5, 9)):
        assert torch.equal(R.bordered_index(nimg, H, W), ops.bordered_index(nimg, H, W, torch.device("cpu")))
        assert R.bordered_rows(nimg, H, W) == (nimg * (H + 1) + 1) * (W + 1) + 1
    ro = R.ln_row_out(60, (2, 3, 5))
    assert torch.equal(ro[:30], R.bordered_index(2, 3, 5)) and torch.equal(ro[30:], R.bordered_rows(2, 3, 5) + R.bordered_index(2, 3, 5))
    assert int(ro.max()) < 2 * R.bordered_rows(2, 3, 5) and ro.unique().numel() == 60


def test_linear_attention_references_are_the_oracle_and_the_formula():
    for C, L in R.la_kv_cases():
        qkv = R.la_inputs(C, L)
        q, k, v = R.la_split(qkv.double(), L, C)
        work, absw = R.la_work64(qkv, L, C)
        n, H = q.shape[0], C // 16
        assert work.shape == (n, H, R.la_chunks(L), R.KVW) and n == R.LA_G * R.LA_NIMG
        # kv and work from the formula at the head of mk_linattn.hip, as explicit einsums
        K = F.elu(k) + 1.0
        M = torch.einsum("nshd,nshv->nhdv", K, v / L).reshape(n, H, 256)
        assert bool(((work.sum(2)[..., :256] - M).abs() <= 1e-12 * absw.sum(2)[..., :256]).all())
        assert _close(work.sum(2)[..., 256:], K.sum(1))
        for c in range(R.la_chunks(L)):
            s = slice(c * 64, min(L, c * 64 + 64))
            assert _close(work[:, :, c, 256:], K[:, s].sum(1))
            Mc = torch.einsum("nshd,nshv->nhdv", K[:, s], v[:, s] / L).reshape(n, H, 256)
            assert bool(((work[:, :, c, :256] - Mc).abs() <= 1e-12 * absw[:, :, c, :256]).all())
        out, e, den = R.la_apply64(qkv, work.sum(2).reshape(-1, R.KVW), L, C)
        ref = O.linear_attention(q, k, v).reshape(out.shape)
        assert bool(((out - ref).abs() <= 1e-6 * e).all()), (C, L)        # (e is ~1e-6 of the terms: fp64 agreement to ~1e-12)
        # den bounded away from eps; both branches of phi well populated
        assert float(den.min()) > 1e4 * R.LA_EPS, (C, L, float(den.min()))
        if L * C >= 256:
            for t in (q, k):
                assert 0.3 <= float((t > 0).double().mean()) <= 0.7, (C, L)
    assert all(float((R.la_split(R.la_inputs(C, L), L, C)[1] > 0).float().mean()) >= 0.3 for C, L in R.LA_APPLY)


def test_posenc_and_tail_references_are_the_oracle():
    h, w = R.PE_HW
    for C in (8, 128):
        pe = R.pe_table(C, h, w)
        assert torch.equal(pe.t().reshape(C, h, w), O.sine_pos_encoding(C, h, w))
        x = R.pe_inputs(torch.float16, R.PE_G, R.PE_NIMG, h * w, C)
        xs32, ref = R.pe_ref(x, pe, R.PE_NIMG)
        feats = x.double().reshape(R.PE_G * R.PE_NIMG, h, w, C).permute(0, 3, 1, 2) + O.sine_pos_encoding(C, h, w).double()[None]
        assert torch.equal(ref, feats.permute(0, 2, 3, 1).reshape(ref.shape))
        assert _ok(xs32, ref, R.U * ref.abs())
        assert torch.equal(R.pe_ref(x, None, R.PE_NIMG)[0], x.float())
    b = R.PE_BIG
    assert b["G"] * b["nimg"] * b["hw"][0] * b["hw"][1] * b["C"] // 4 > 8192 * 256
    for hh, ww, border, sm, dsig, nd, C, Cd in R.ht_cases():
        c = R.ht_inputs(R.HT_NIMG, hh, ww, C, Cd)
        r = R.ht_ref(c, R.HT_NIMG, hh, ww, border, sm, dsig, nd)
        n = hh * ww
        nchw = lambda f, ch: f.double().reshape(R.HT_NIMG, hh, ww, ch).permute(0, 3, 1, 2)   # noqa: E731
        logit = F.conv2d(nchw(c["fd"], C), c["ws"].double().view(1, C, 1, 1))
        if sm:
            assert torch.equal(r["scr"][0], O.border_softmax(logit, border).reshape(R.HT_NIMG, 1, n))
            tot = r["scr"][0].sum(2)
            assert bool((((tot - 1).abs() < 1e-12) | (tot == 0)).all())
        k = torch.sigmoid(F.conv2d(nchw(c["fo"], C), c["wxy"].double().view(2, C, 1, 1)))
        assert torch.equal(r["kps"][0], O.abs_keypoints(k, R.HT_DOWN).reshape(R.HT_NIMG, 2, n))
        inside = r["inside"]
        assert bool((r["scr"][0][:, 0, ~inside] == 0).all()) and bool((r["scr"][1][:, 0, ~inside] == 0).all())
        if (hh, ww, border) == (5, 5, 3):
            assert not bool(inside.any()) and bool((r["scr"][0] == 0).all())
        if (hh, ww, border) == (7, 7, 3):
            assert int(inside.sum()) == 1
            if sm:
                assert bool(((r["scr"][0][:, 0, inside] - 1).abs() < 1e-15).all())
    shapes = {(h_, w_) for h_, w_, *_ in R.ht_cases()}
    assert shapes == set(R.HT_HW) and (11 * 9) % 64 == 35 and (R.HT_NIMG * 99) % 4 != 0 and 33 * 32 > 1024
    for k_, vals in ((3, (0, 1)), (4, (0, 1)), (5, (0, 1)), (6, R.HT_C), (7, R.HT_CD), (2, (0, 3))):
        assert {cs[k_] for cs in R.ht_cases()} == set(vals), k_
    for d in R.HT_LDS:
        assert max((d["h"] * d["w"] + 32) * 4, d["Cd"] * 65 * 4) > 64 * 1024 and max((d["h"] * d["w"] + 32) * 4, d["Cd"] * 65 * 4) <= 160 * 1024


# ---- the inputs are what they are meant to be ----------------------------------------------------------------------------------
def test_layernorm_inputs_have_centred_rows_and_rows_far_from_zero():
    for D, rows in R.ln_cases():
        if rows < 3 or D < 64:
            continue
        x, _, _, _ = R.ln_inputs(rows, D)
        z = (x.double().mean(1) / x.double().std(1)).abs()
        assert float(z[1::2].min()) > 4.0 and float(z[0::2].max()) < 1.0, (D, rows, z)


def test_no_designed_case_leaves_an_element_out():
    """every bound is positive wherever the reference is not an exact zero by construction (border scores, norm_dsc = 0)"""
    for C, L in R.la_kv_cases():
        work, absw = R.la_work64(R.la_inputs(C, L), L, C)
        assert bool((R.la_work_bound(absw, L) > 0).all()) and bool((R.la_kv_bound(absw, L) > 0).all())
    for hh, ww, border, sm, dsig, nd, C, Cd in R.ht_cases():
        r = R.ht_ref(R.ht_inputs(R.HT_NIMG, hh, ww, C, Cd), R.HT_NIMG, hh, ww, border, sm, dsig, nd)
        assert bool((r["scr"][1][:, 0, r["inside"]] > 0).all()) and bool((r["kps"][1] > 0).all()) and bool((r["depth"][1] > 0).all())
        assert bool((r["dsc"][1] > 0).all()) == bool(nd)


# ---- every bound admits a correct fp32 implementation, in two summation orders ------------------------------------------------------
def _ln_forms_ok(y32, ref, e):
    ok = _ok(y32, ref, e)
    for dt in (torch.bfloat16, torch.float16):
        ok = ok and _ok(y32.to(dt), ref, R.b_out(e, ref, dt))
    hi, lo = R.planes_of(y32)
    bh, bs = R.planes_bounds(ref, e)
    return ok and _ok(hi, R.PLANE_SCALE * ref, bh) and _ok(hi.double() + lo.double(), R.PLANE_SCALE * ref, bs)


@pytest.mark.parametrize("order", [0, 1])
def test_layernorm_bounds_admit_fp32(order):
    for D, rows in R.ln_cases():
        x, w, b, resid = R.ln_inputs(rows, D)
        ref, e = R.ln_expected(x, w, b, None, R.LN_EPS)
        assert _ln_forms_ok(R.ln_fp32(x, w, b, R.LN_EPS, order=order), ref, e), (D, rows)
        ref, e = R.ln_expected(x, w, b, resid, R.LN_EPS)
        assert _ln_forms_ok(R.ln_fp32(x, w, b, R.LN_EPS, order=order) + resid, ref, e), (D, rows, "resid")
        assert float((R.PLANE_SCALE * ref).abs().max()) < 60000.0           # no plane saturates
    for name, lay in R.LN_LAYOUTS.items():
        for D in R.LN_LAYOUT_D:
            rows_in = lay["rows_out"] // (lay["rows_per_img"] - lay["skip"]) * lay["rows_per_img"]
            x, w, b, _ = R.ln_inputs(rows_in, D, lay["groups"], case=name)
            xs = x[R.ln_row_in(lay["rows_out"], lay["rows_per_img"], lay["skip"])]
            ref, e = R.ln_expected(xs, w, b, None, R.LN_EPS, lay["wgroup_rows"])
            assert _ln_forms_ok(R.ln_fp32(xs, w, b, R.LN_EPS, lay["wgroup_rows"], order=order), ref, e), (name, D)


@pytest.mark.parametrize("order", [0, 1])
def test_linear_attention_bounds_admit_fp32(order):
    for C, L in R.la_kv_cases():
        if order and L > 200:
            continue                                     # (the token-by-token order at L = 1938 is the same code path, 31 times)
        qkv = R.la_inputs(C, L)
        work, absw = R.la_work64(qkv, L, C)
        w32 = R.la_work32(qkv, L, C, order)
        assert _ok(w32, work, R.la_work_bound(absw, L)), (C, L)
        kv32 = w32[:, :, 0].clone()
        for c in range(1, w32.shape[2]):
            kv32 = kv32 + w32[:, :, c]
        assert _ok(kv32, work.sum(2), R.la_kv_bound(absw, L)), (C, L)
    for C, L in R.LA_APPLY:
        qkv = R.la_inputs(C, L)
        kv32 = R.la_work32(qkv, L, C).sum(2).reshape(-1, R.KVW)
        out, e, _ = R.la_apply64(qkv, kv32, L, C)
        o32 = R.la_apply32(qkv, kv32, L, C, order)
        assert _ok(o32, out, e), (C, L)
        for dt in (torch.bfloat16, torch.float16):
            assert _ok(o32.to(dt), out, R.b_out(e, out, dt)), (C, L, dt)


def test_posenc_bounds_admit_fp32():
    h, w = R.PE_HW
    for dt, has_pe, C, _ in R.pe_cases():
        x = R.pe_inputs(dt, R.PE_G, R.PE_NIMG, h * w, C)
        xs32, ref = R.pe_ref(x, R.pe_table(C, h, w) if has_pe else None, R.PE_NIMG)
        assert _ok(xs32.to(dt), ref, R.pe_cat_bound(ref, dt)), (dt, has_pe, C)


@pytest.mark.parametrize("order", [0, 1])
def test_head_tail_bounds_admit_fp32(order):
    for hh, ww, border, sm, dsig, nd, C, Cd in R.ht_cases():
        c = R.ht_inputs(R.HT_NIMG, hh, ww, C, Cd)
        r = R.ht_ref(c, R.HT_NIMG, hh, ww, border, sm, dsig, nd)
        got = R.ht_fp32(c, R.HT_NIMG, hh, ww, border, sm, dsig, nd, order)
        for name in ("scr", "kps", "depth", "dsc"):
            worst, i = R.ratio(got[name], r[name][0], r[name][1])
            assert worst <= 1.0, (name, hh, ww, border, sm, dsig, nd, C, Cd, worst, i)


# ---- every metric rejects a subtly wrong implementation -----------------------------------------------------------------------
def test_one_element_off_by_twice_its_bound_is_rejected():
    D, rows = 100, 9
    x, w, b, _ = R.ln_inputs(rows, D)
    ref, e = R.ln_expected(x, w, b, None, R.LN_EPS)
    for i in (0, rows * D - 1, 4 * D + 99):
        bad = ref.clone()
        bad.reshape(-1)[i] += 2 * e.reshape(-1)[i]
        assert _ok(ref, ref, e) and not _ok(bad, ref, e) and R.ratio(bad, ref, e)[1] == i
    qkv = R.la_inputs(96, 65)
    work, absw = R.la_work64(qkv, 65, 96)
    bw = R.la_work_bound(absw, 65)
    bad = work.clone()
    bad[3, 2, 1, 271] -= 2 * bw[3, 2, 1, 271]
    assert not _ok(bad, work, bw)
    out, e, _ = R.la_apply64(qkv, work.sum(2).reshape(-1, R.KVW), 65, 96)
    for dt in R.LA_OUT_TYPES:
        bb = R.b_out(e, out, dt)
        bad = out.clone()
        bad[1, 64, 95] += 2 * bb[1, 64, 95]
        assert _ok(out, out, bb) and not _ok(bad, out, bb)
    h, w_ = R.PE_HW
    x = R.pe_inputs(torch.bfloat16, R.PE_G, R.PE_NIMG, h * w_, 8)
    _, ref = R.pe_ref(x, R.pe_table(8, h, w_), R.PE_NIMG)
    bad = ref.clone()
    bad[2, 29, 7] += 2 * R.pe_cat_bound(ref, torch.bfloat16)[2, 29, 7]
    assert not _ok(bad, ref, R.pe_cat_bound(ref, torch.bfloat16))
    hh, ww, border, sm, dsig, nd, C, Cd = [cs for cs in R.ht_cases() if cs[:3] == (11, 9, 3) and cs[3] == 1][0]
    r = R.ht_ref(R.ht_inputs(R.HT_NIMG, hh, ww, C, Cd), R.HT_NIMG, hh, ww, border, sm, dsig, nd)
    for name in ("scr", "kps", "depth"):
        ref, bnd = r[name]
        i = int(bnd.reshape(-1).argmax())
        bad = ref.clone()
        bad.reshape(-1)[i] += 2 * bnd.reshape(-1)[i]
        assert not _ok(bad, ref, bnd), name


def _rejected_somewhere(results):
    return any(not ok for ok in results)


def test_mutants_of_the_kv_sum_are_rejected():
    dropped, wrong_len = [], []
    for C, L in R.la_kv_cases():
        qkv = R.la_inputs(C, L)
        work, absw = R.la_work64(qkv, L, C)
        bw, bk = R.la_work_bound(absw, L), R.la_kv_bound(absw, L)
        m1, _ = R.la_work64(qkv, L, C, drop_last_of_ragged=True)
        m2, _ = R.la_work64(qkv, L, C, inv_len=1.0 / (L + 1))
        dropped.append(_ok(m1, work, bw) and _ok(m1.sum(2), work.sum(2), bk))
        wrong_len.append(_ok(m2, work, bw) and _ok(m2.sum(2), work.sum(2), bk))
        if L % 64 > 1:
            assert not dropped[-1], (C, L)               # every ragged chunk shows its last token
        if L <= 129:
            assert not wrong_len[-1], (C, L)
    assert _rejected_somewhere(dropped) and _rejected_somewhere(wrong_len)


def test_mutants_of_layernorm_are_rejected():
    wide_mean, neighbour = [], []
    for D, rows in R.ln_cases():
        x, w, b, _ = R.ln_inputs(rows, D)
        xw = torch.cat([x, R.ln_inputs(rows, 4, case="slack")[0]], 1)     # the columns a kernel reading past D would find (ldx > D)
        ref, e = R.ln_expected(x, w, b, None, R.LN_EPS)
        wide_mean.append(_ok(R.ln_fp32(xw, w, b, R.LN_EPS, cols=D + 4), ref, e))
        assert not wide_mean[-1], (D, rows)
    lay = R.LN_LAYOUTS["groups"]
    for D in R.LN_LAYOUT_D:
        x, w, b, _ = R.ln_inputs(lay["rows_out"], D, lay["groups"], case="groups")
        ref, e = R.ln_expected(x, w, b, None, R.LN_EPS, lay["wgroup_rows"])
        # a wave that takes (w, b) once for all its rows: rows 4 .. 7 (wide) / 0 .. 7 (narrow) use the group of the wave's first row
        per = 8 if D <= 128 else 4
        grp = R.ln_group(lay["rows_out"], lay["wgroup_rows"])[torch.arange(lay["rows_out"]) // per * per]
        y = torch.cat([R.ln_fp32(x[i:i + 1], w[grp[i]], b[grp[i]], R.LN_EPS) for i in range(lay["rows_out"])])
        neighbour.append(_ok(y, ref, e))
        assert not neighbour[-1], D
    assert _rejected_somewhere(wide_mean) and _rejected_somewhere(neighbour)


def test_mutants_of_the_tails_and_the_posenc_are_rejected():
    leaks = []
    for hh, ww, border, sm, dsig, nd, C, Cd in R.ht_cases():
        if border == 0:
            continue
        c = R.ht_inputs(R.HT_NIMG, hh, ww, C, Cd)
        r = R.ht_ref(c, R.HT_NIMG, hh, ww, border, sm, dsig, nd)
        bad = R.ht_ref(c, R.HT_NIMG, hh, ww, border, sm, dsig, nd, leak=hh * ww - 1)["scr"][0]     # the last pixel keeps its score
        leaks.append(_ok(bad, r["scr"][0], r["scr"][1]))
        assert not leaks[-1], (hh, ww, sm)
    assert _rejected_somewhere(leaks)
    h, w = R.PE_HW
    shifted = []
    for dt, has_pe, C, _ in R.pe_cases():
        if not has_pe:
            continue
        x = R.pe_inputs(dt, R.PE_G, R.PE_NIMG, h * w, C)
        pe = R.pe_table(C, h, w)
        xs32, ref = R.pe_ref(x, pe, R.PE_NIMG)
        bad32, _ = R.pe_ref(x, pe, R.PE_NIMG, shift=1)
        shifted.append(torch.equal(bad32, xs32) or _ok(bad32.to(dt), ref, R.pe_cat_bound(ref, dt)))
        assert not shifted[-1], (dt, C)
    assert _rejected_somewhere(shifted)


# ---- the entry points' argument checks ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from mickey_amd import build, _native
    if not os.path.exists(build.lib_path()):
        build.build(verbose=False)
    return _native.load()


def _refused(lib, rc, *words):
    """MK_ERR_INVALID_ARGUMENT (1; a launch error is 2: nothing was launched) and an error text that says why"""
    msg = lib.mk_last_error()
    assert rc == 1, (rc, msg)
    assert all(w in msg for w in words), msg


def test_layernorm_rejects_short_leading_dimensions_without_a_device(lib):
    p = 0x100000   # never dereferenced: every call below fails its argument checks before any launch
    ok = dict(ldx=128, ldo=128, ldr=128, out=p, resid=p, D=128)

    def call(planes=False, **kw):
        a = dict(ok, **kw)
        if planes:
            return lib.mk_layernorm_planes(p, a["ldx"], p, p, 1e-5, a["out"], p, a["ldo"], 64.0, a["resid"], a["ldr"], 8, a["D"], 8, 0, 0,
                                           0, 0, 0, None, None)
        return lib.mk_layernorm(p, a["ldx"], p, p, 1e-5, a["out"], a["ldo"], 1, a["resid"], a["ldr"], 8, a["D"], 8, 0, 0, 0, 0, 0, 2, None)

    for planes in (False, True):
        for D in (128, 384):
            for name in ("ldx", "ldo", "ldr"):
                _refused(lib, call(planes, D=D, **{n: (D - 4 if n == name else D) for n in ("ldx", "ldo", "ldr")}), b"mk_layernorm", b">= D")
        _refused(lib, call(planes, ldx=130), b"mk_layernorm")
        _refused(lib, call(planes, D=130), b"mk_layernorm", b"D=130")
    # the leading dimension of an operand that is not there is not looked at
    _refused(lib, call(out=None, resid=None), b"null")


def test_linattn_apply_rejects_more_than_128_channels_without_a_device(lib):
    p = 0x100000
    for C in (144, 256, 1024, 0, 24):
        _refused(lib, lib.mk_linattn_apply(p, p, p, max(C, 8), 1, 1, 8, C, 2, None), b"mk_linattn_apply", b"128")
        if C > 128:
            _refused(lib, lib.mk_linattn_kv(p, p, p, 1, 1, 8, C, None), b"mk_linattn_kv", b"128")
    _refused(lib, lib.mk_linattn_apply(p, p, p, 64, 1, 1, 8, 128, 2, None), b"mk_linattn_apply")     # ldo < C
    _refused(lib, lib.mk_linattn_apply(p, p, None, 128, 1, 1, 8, 128, 2, None), b"mk_linattn_apply")


def test_head_tails_rejects_more_lds_than_it_reserves_without_a_device(lib):
    p = 0x100000

    def call(h, w, Cd, nimg=1):
        return lib.mk_head_tails(p, p, p, p, p, p, p, p, p, p, p, nimg, h, w, 32, Cd, 3, 1, 0, 60.0, 1, 14.0, None)

    _refused(lib, call(203, 202, 64), b"mk_head_tails")          # (h w + 32) * 4 > 160 KiB
    _refused(lib, call(5, 5, 631), b"mk_head_tails")             # Cd * 65 * 4 > 160 KiB
    _refused(lib, call(5, 5, 64, nimg=0), b"mk_head_tails")
    _refused(lib, call(0, 5, 64), b"mk_head_tails")
